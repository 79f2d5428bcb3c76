"""The properties of the registration host layer (cusift_amd/csrc/sift_register.hip) that cannot be seen from outside:
one synchronisation per blocking call and nothing else that blocks, the order in which a call enqueues its work, no
launches in loops, and the arguments of score_splits that tests/test_ransac_sizes.py plans with.  Everything is asserted
on the bodies of functions, found by name, and on a call's path: its body plus the bodies of every function of the file
that it reaches, each once.  No GPU."""
import functools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cusift_amd", "csrc")

BLOCKING = ("hipDeviceSynchronize", "hipMemcpy(", "hipMemcpyDtoH(", "hipEventSynchronize", "hipMalloc(", "hipFree(",
            "cusift_ctx_synchronize", "cusift_memcpy")
# (per_cu, tile, round_to_tile) of the four call sites of score_splits, in the order they stand in sift_register.hip;
# tests/test_ransac_sizes.py and tests/test_pnp_sizes.py plan their sizes with these
PLANAR, RIGID, EPI = (8, 64, True), (4, 256, False), (8, 64, True)
PNP = (8, 64, True)
LAUNCH_BANNED = ("for (", "while (", "hipMemcpy", "hipMemset", "Synchronize", "grow_scratch")
DEFINITION = r'^(?:static|extern "C") [^\n(;={]*?\b(\w+)\('


@functools.lru_cache(maxsize=None)
def code():
    """sift_register.hip without its comments."""
    text = open(os.path.join(CSRC, "sift_register.hip")).read()
    return "\n".join(line.split("//")[0] for line in text.splitlines()) + "\n"


def body(name):
    """The function `name` of the file, from its signature to the closing brace at the start of a line."""
    found = [m for m in re.finditer(DEFINITION, code(), flags=re.M) if m.group(1) == name]
    assert len(found) == 1, (name, len(found))
    begin = found[0].start()
    line = code()[begin:code().index("\n", begin)]
    return line if line.rstrip().endswith("}") else code()[begin:code().index("\n}\n", begin)]  # a one-line function


def path(name, without=()):
    """The body of `name` and of every function of the file that it reaches, each once; `without`: calls not followed."""
    defined = set(re.findall(DEFINITION, code(), flags=re.M))
    seen, todo = [], [name]
    while todo:
        f = todo.pop()
        if f in seen or f in without:
            continue
        seen.append(f)
        todo += [g for g in defined if re.search(r"\b%s\(" % g, body(f).split("{", 1)[1])]
    return "\n".join(body(f) for f in seen)


def in_order(text, *keys):
    at = [text.index(k) for k in keys]
    return at == sorted(at)


def one_sync_nothing_else(name, without=()):
    """The uniform rule of a blocking call: one hipStreamSynchronize on its path and nothing else that blocks."""
    p = path(name, without)
    assert p.count("hipStreamSynchronize(") == 1, (name, p.count("hipStreamSynchronize("))
    assert not [b for b in BLOCKING if b in p], name
    return p


def check_four_launches(name, kernels):
    """planar_launch / epipolar_launch / pnp_launch: the four launches behind the marking, in their order, none in a loop, and nothing
    that copies or waits."""
    launch = body(name)
    assert launch.count("hipLaunchKernelGGL(") == 4
    assert in_order(launch, *("hipLaunchKernelGGL(" + k for k in kernels))
    for banned in LAUNCH_BANNED:
        assert banned not in launch, (name, banned)


def check_planar_launch():
    check_four_launches("planar_launch", ("planar_compact_kernel", "homography_solve_kernel", "planar_score_kernel",
                                          "planar_select_kernel"))


def check_matcher_of_a_fused_call(fused, run):
    """The fused call enqueues the mutual matcher or the plain one, once, before the run; nothing in that helper blocks.
    Replaces `reg.index("cusift_match_mutual(") < reg.index("cusift_match(ctx") < reg.index("..._run(")`."""
    assert fused.count("match_enqueue(") == 1 and fused.count(run) == 1 and in_order(fused, "match_enqueue(", run)
    helper = body("match_enqueue")
    assert in_order(helper, "ctx->cross_check", "cusift_match_mutual(", "cusift_match(ctx")
    reached = path("match_enqueue")
    assert "Synchronize" not in reached and not [b for b in BLOCKING if b in reached]
    assert "match_mutual_kernel<" in reached and "match_kernel<" in reached  # it does reach both matchers' launches


def model_field(descriptor, field):
    """What the RansacModel `descriptor` (kHomography, kFundamental, kPnP) carries in `field`, as text."""
    struct = code()[code().index("struct RansacModel {"):]
    members = struct[struct.index("{") + 1:struct.index("\n};\n")]
    names = [re.sub(r"^.*[ *]", "", n.strip()) for decl in members.split(";") if decl.strip() for n in decl.split(",")]
    found = re.findall(r"static const RansacModel %s\{([^}]*)\};" % descriptor, code())
    assert len(found) == 1, descriptor
    values = [v.strip() for v in found[0].split(",")]
    assert len(values) == len(names) and names.count(field) == 1, (descriptor, names, values)
    return values[names.index(field)]


LAUNCHES = ("planar_launch(", "epipolar_launch(", "pnp_launch(")


def check_dispatch(run, launch):
    """The model's four launches in a runner: `launch` once, under its branch of the three-way choice by m.launch.  Each
    launch function is named three times in the file: its definition and one call in either runner."""
    assert run.count(launch) == 1 and [run.count(f) for f in LAUNCHES] == [1, 1, 1]
    assert in_order(run, "if (m.launch == kPlanarLaunch)", "planar_launch(", "else if (m.launch == kEpipolarLaunch)",
                    "epipolar_launch(", "\n  else\n", "pnp_launch(")
    assert [code().count(f) for f in LAUNCHES] == [3, 3, 3]


def check_pose_launch():
    """pose_launch, the pose stage of a pair and of a pair list: the head(s) zeroed, the vote, the write; the grid carries
    the pairs, nothing loops over them, nothing copies or waits."""
    stage = body("pose_launch")
    assert in_order(stage, "hipMemsetAsync(", "hipLaunchKernelGGL(pose_vote_kernel", "hipLaunchKernelGGL(pose_write_kernel")
    assert stage.count("hipLaunchKernelGGL(") == 2 and stage.count("hipMemsetAsync(") == 1
    assert "kPoseHeadBytes * (size_t)n_pairs" in stage
    assert "const dim3 grid(std::max(idiv_up(num_pts, 256), 1), 1, n_pairs);" in stage
    for banned in ("for (", "while (", "hipMemcpy", "Synchronize", "grow_scratch"):
        assert banned not in stage, banned
    for name in ("pose_vote_kernel", "pose_write_kernel"):
        assert code().count("hipLaunchKernelGGL(" + name) == 1, name  # no second copy of the stage
    assert code().count("pose_launch(") == 3  # the definition, pose_enqueue, ransac_batch_run


def check_batch_call(name, launch, pose=False):
    """A pair-list call: one hipStreamSynchronize on its path and nothing else that blocks; nothing of its own in the
    entry point; in ransac_batch_run one read-back, the order matcher -> marking -> model launches -> (pose stage) ->
    read-back -> wait, one marking launch statement and no launch in a loop over the pairs."""
    one_sync_nothing_else(name)
    entry = body(name)
    assert "Synchronize" not in entry and "hipMemcpy" not in entry and "hipLaunchKernelGGL(" not in entry
    assert entry.count("ransac_batch_run(") == 1 and entry.count("batch_check(") == 1
    assert in_order(entry, "batch_check(", "if (n_pairs == 0) return CUSIFT_OK;", "ransac_batch_run(")
    assert ("pose_stage(" in entry) == pose and ("&st.cams" in entry) == pose
    run = body("ransac_batch_run")
    assert run.count("hipStreamSynchronize(") == 1 and not [b for b in BLOCKING if b in run]
    assert in_order(run, "match_batch_launch(", "sequence_mark_kernel", launch, "pose_launch(", "hipMemcpyAsync(",
                    "hipStreamSynchronize(", "pose_report(")
    check_dispatch(run, launch)
    assert run.count("hipMemcpyAsync(") == 1  # one read-back; the pair list is uploaded by the matcher's launcher
    # the marking here, compact / solve / score / select in the model's launch function, the pose stage's two in pose_launch
    assert run.count("hipLaunchKernelGGL(") == 1 and run.count("pose_launch(") == 1
    assert "hipLaunchKernelGGL(m.launch == kPnPLaunch ? sequence_pnp_mark_kernel : sequence_mark_kernel" in run
    assert re.search(r"if \(pose\)\s*\n\s*TRY\(pose_launch\(", run)
    launches = run[run.index("match_batch_launch("):run.index("hipMemcpyAsync(")]
    assert "for (" not in launches and "while (" not in launches
    return entry


def check_chain_run(launch):
    """ransac_run, the run of the three chains: mark -> four launches -> (pose enqueue) -> the one read-back -> the one
    wait -> (pose report); the staged pose route of fewer records than the model can fit leaves before anything is
    enqueued."""
    run = body("ransac_run")
    # was: order of ("planar_mark_kernel", "planar_launch(" / "epipolar_launch(", "hipMemcpyAsync(", "hipStreamSynchronize(")
    # in planar_run / epipolar_run, and of ("epipolar_launch(", "pose_enqueue(", "hipMemcpyAsync(", "hipStreamSynchronize(",
    # "pose_report(") in epipolar_run
    assert in_order(run, "mark_launch(", launch, "pose_enqueue(", "hipMemcpyAsync(", "hipStreamSynchronize(", "pose_report(")
    # was: run.count("hipMemcpyAsync(") == 1 -- one read-back, nothing uploaded
    assert run.count("hipMemcpyAsync(") == 1
    # was: epi.count("hipStreamSynchronize(") == 1 and epi.count("pose_enqueue(") == 1
    assert run.count("hipStreamSynchronize(") == 1 and run.count("pose_enqueue(") == 1
    # was: run.count("hipLaunchKernelGGL(") == 1 and run.count("planar_launch(") == 1 -- the marking, then the shared four
    assert run.count("hipLaunchKernelGGL(") == 0 and run.count("mark_launch(") == 1 and run.count(launch) == 1
    check_dispatch(run, launch)
    # was: one launch in mark_launch, planar_mark_kernel.  Now one per branch: the PnP model's marking, else the planar one
    mark = body("mark_launch")
    assert mark.count("hipLaunchKernelGGL(") == 2 and mark.count("hipLaunchKernelGGL(planar_mark_kernel") == 1
    assert mark.count("hipLaunchKernelGGL(pnp_mark_kernel") == 1
    assert re.search(r"if \([^\n]*\)[^\n;]*\n\s*hipLaunchKernelGGL\(pnp_mark_kernel[^;]*;\n\s*else\n\s*hipLaunchKernelGGL\(planar_mark_kernel", mark)
    for banned in LAUNCH_BANNED:
        assert banned not in mark, banned
    # the other way out: the answer that needs no device work, and from there the staged pose route, which has its own wait
    # was: "if (num_pts < 8) {" -- now the model's minimum, which is 8 for H and F as before and 6 for PnP
    assert run.count("pose_run(") == 1 and in_order(run, "if (num_pts < m.min_pts) {", "pose_run(", "\n  }\n", "grow_scratch(")
    assert [model_field(d, "min_pts") for d in ("kHomography", "kFundamental", "kPnP")] == ["8", "8", "6"]
    assert re.search(r"return pose \? pose_run\([^;]*\) : CUSIFT_OK;", run)


# was tests/test_planar.py::test_one_synchronisation_in_the_planar_entry_points
def test_one_synchronisation_in_the_planar_entry_points():
    for name in ("cusift_estimate_homography", "cusift_register_planar"):
        # was: one hipStreamSynchronize( and no blocking call in the planar section; planar_run( counted 3 times, the
        # definition and its two callers.  The section held no pose route: neither call hands the run a stage
        one_sync_nothing_else(name, without=("pose_run",))
        assert body(name).count("ransac_run(") == 1 and "&st" not in body(name)
    check_chain_run("planar_launch(")
    check_planar_launch()


# was tests/test_planar_batch.py::test_one_synchronisation_in_the_batch_entry_point
def test_one_synchronisation_in_the_batch_entry_point():
    # was: one hipStreamSynchronize( and no blocking call, the order match_batch_launch( -> sequence_mark_kernel ->
    # planar_launch( -> hipMemcpyAsync( -> hipStreamSynchronize(, one hipMemcpyAsync(, one hipLaunchKernelGGL( (the
    # marking) and no loop in front of the read-back, all in the entry point's own text.  The body is ransac_batch_run
    # now: the same on the call's path and on the runner (check_batch_call)
    entry = check_batch_call("cusift_register_planar_batch", "planar_launch(")
    assert "ransac_batch_run(ctx, kHomography," in entry
    assert model_field("kHomography", "launch") == "kPlanarLaunch"
    check_planar_launch()
    # five launches on the path -- the marking, compact / solve / score / select -- and no pose stage
    p = path("cusift_register_planar_batch", without=("epipolar_launch", "pnp_launch", "pose_launch", "match_batch_launch"))
    assert p.count("hipLaunchKernelGGL(") == 5


def test_one_synchronisation_in_the_other_pair_list_entry_points():
    """The rule of the planar pair-list call on its three siblings, which no test held to it."""
    for name, model, launch, pose in (("cusift_register_epipolar_batch", "kFundamental", "epipolar_launch(", False),
                                      ("cusift_register_pose_batch", "kFundamental", "epipolar_launch(", True),
                                      ("cusift_register_pnp_batch", "kPnP", "pnp_launch(", False)):
        entry = check_batch_call(name, launch, pose)
        assert "ransac_batch_run(ctx, %s," % model in entry
    assert model_field("kFundamental", "launch") == "kEpipolarLaunch" and model_field("kPnP", "launch") == "kPnPLaunch"
    check_pose_launch()
    assert code().count("ransac_batch_run(") == 5  # the definition and the four calls


# was tests/test_epipolar.py::test_one_synchronisation_in_the_epipolar_entry_points
def test_one_synchronisation_in_the_epipolar_entry_points():
    for name in ("cusift_estimate_fundamental", "cusift_register_epipolar"):
        # was: one hipStreamSynchronize( and no blocking call in the epipolar section (which did not hold pose_run);
        # epipolar_run( counted 3 times, the definition and its two callers
        one_sync_nothing_else(name, without=("pose_run",))
        assert body(name).count("ransac_run(") == 1 and "&st" not in body(name)
    check_chain_run("epipolar_launch(")
    # was: the four launches of epipolar_launch in their order, and its banned list
    check_four_launches("epipolar_launch", ("planar_compact_kernel", "epipolar_solve_kernel", "epipolar_score_kernel",
                                            "epipolar_select_kernel"))
    reg = body("cusift_register_epipolar")
    check_matcher_of_a_fused_call(reg, "ransac_run(")
    assert "Synchronize" not in reg and "hipMemcpy" not in reg  # nothing of its own


# was tests/test_pose.py::test_one_synchronisation_in_the_pose_entry_points
def test_one_synchronisation_in_the_pose_entry_points():
    # the staged call.  was: one hipStreamSynchronize( and no blocking call between `struct PoseOut {` and
    # `struct EpipolarOut {`; pose_run( counted twice, the definition and the caller
    one_sync_nothing_else("cusift_estimate_pose")
    assert body("cusift_estimate_pose").count("pose_run(") == 1
    run = body("pose_run")
    # was: order of ("planar_mark_kernel", "pose_enqueue(", "hipStreamSynchronize(", "pose_report(") in pose_run
    assert in_order(run, "mark_launch(", "pose_enqueue(", "hipStreamSynchronize(", "pose_report(")
    assert run.count("hipMemcpyAsync(") == 1 and run.count("hipStreamSynchronize(") == 1  # F goes up; the head's copy is the stage's
    # was: order of (hipMemsetAsync(, pose_vote_kernel, pose_write_kernel, hipMemcpyAsync() and two launches in
    # pose_enqueue; the first three stand in pose_launch now, which the pair-list runner shares
    enq = body("pose_enqueue")
    assert in_order(enq, "pose_launch(", "hipMemcpyAsync(")
    assert enq.count("pose_launch(") == 1 and enq.count("hipMemcpyAsync(") == 1 and "hipLaunchKernelGGL(" not in enq
    assert "nullptr, 1, PlanarBatch{})" in enq  # one pair, into the records
    for banned in ("for (", "while (", "Synchronize", "grow_scratch"):
        assert banned not in enq, banned
    check_pose_launch()
    # one pose_report serves the pair calls and the runner's loop, on the head it is handed
    assert body("pose_report").startswith("static void pose_report(const char *head, const PoseOut &o, size_t p = 0)")
    assert code().count("pose_report(") == 4 and code().count("kPoseHeadRt") == 1
    # the fused call: the epipolar run with the stage behind its launches, in front of its one read-back and wait
    fused = body("cusift_register_pose")
    assert "Synchronize" not in fused and "hipMemcpy" not in fused and not [b for b in BLOCKING if b in fused]
    check_matcher_of_a_fused_call(fused, "ransac_run(")
    assert fused.count("ransac_run(") == 1 and "&st)" in fused
    check_chain_run("epipolar_launch(")
    # either way through the run there is one wait: the run's own, or -- fewer than 8 records -- the staged route's
    one_sync_nothing_else("cusift_register_pose", without=("pose_run",))
    staged = path("pose_run")
    assert staged.count("hipStreamSynchronize(") == 1 and not [b for b in BLOCKING if b in staged]


def test_one_synchronisation_in_the_pnp_entry_points():
    for name in ("cusift_estimate_pnp", "cusift_register_pnp"):
        one_sync_nothing_else(name, without=("pose_run",))
        assert body(name).count("ransac_run(") == 1 and "&st" not in body(name) and "pose_stage(" not in body(name)
    check_chain_run("pnp_launch(")
    check_four_launches("pnp_launch", ("planar_compact_kernel", "pnp_solve_kernel", "pnp_score_kernel",
                                       "pnp_select_kernel"))
    reg = body("cusift_register_pnp")
    check_matcher_of_a_fused_call(reg, "ransac_run(")
    assert "Synchronize" not in reg and "hipMemcpy" not in reg  # nothing of its own
    # the chain's copies are gone
    for gone in ("pnp_run", "pnp_splits", "PnPBlock", "PnPOut", "pnp_nothing"):
        assert gone not in open(os.path.join(CSRC, "sift_register.hip")).read(), gone


# the same rule on the blocking calls that no test held to it before
def test_one_synchronisation_in_the_other_blocking_entry_points():
    for name in ("cusift_find_homography", "cusift_estimate_rigid", "cusift_register_rgbd_batch"):
        one_sync_nothing_else(name)
    # cusift_register_rgbd waits in two places that exclude each other: where a frame is empty, and at the read-back
    rgbd = path("cusift_register_rgbd")
    assert not [b for b in BLOCKING if b in rgbd]
    entry = body("cusift_register_rgbd")
    assert rgbd.count("hipStreamSynchronize(") == 2 and entry.count("hipStreamSynchronize(") == 2
    empty = entry[entry.index("if (n1 == 0 || num_pts2 == 0) {"):]
    empty = empty[:empty.index("\n  }\n")]
    assert empty.count("hipStreamSynchronize(") == 1 and "return CUSIFT_OK;" in empty
    check_matcher_of_a_fused_call(entry, "rigid_launch(")
    check_matcher_of_a_fused_call(body("cusift_register_planar"), "ransac_run(")


# was tests/test_ransac_sizes.py::test_call_sites_of_score_splits_pass_what_the_plans_here_assume
def test_call_sites_of_score_splits_pass_what_the_plans_here_assume():
    """Whoever changes the planner or a call site learns here that the sizes of tests/test_ransac_sizes.py and tests/test_pnp_sizes.py
    need another look."""
    calls = re.findall(r"score_splits\(ctx, num_pts, \(long\)loop_blocks \* n_pairs, (\d+), (\d+), (true|false), &\w+\)", code())
    want = [(str(p), str(t), "true" if r else "false") for p, t, r in (PLANAR, RIGID, EPI, PNP)]
    assert calls == want and code().count("score_splits(") == 5, calls  # the definition and the four call sites
    assert in_order(code(), "static int score_splits(", "static void planar_launch(", "8, 64, true, &pts_per_split",
                    "static void rigid_launch(", "4, 256, false, &pts_per_split", "static void epipolar_launch(",
                    "8, 64, true, &per_split", "static void pnp_launch(", "8, 64, true, &cand_per_split")
    for blocks in ("loop_blocks = idiv_up(num_loops, 64)", "loop_blocks = idiv_up(num_loops, 256)"):
        assert blocks in code(), blocks
    planner = body("score_splits")  # was: from its signature to `struct PlanarOut {`
    for line in ("const long target = ((long)per_cu * ctx->num_cus + wgs - 1) / wgs;",
                 "std::max(1L, std::min(std::min(target, (long)idiv_up(num_pts, tile)), 65535L))",
                 "round_to_tile ? idiv_up(idiv_up(num_pts, splits), tile) * tile : idiv_up(num_pts, splits)",
                 "return idiv_up(num_pts, per_split);"):
        assert line in planner, line
    context = open(os.path.join(CSRC, "sift_context.hip")).read()
    assert "hipDeviceGetAttribute(&ctx->num_cus, hipDeviceAttributeMultiprocessorCount, device)" in context
    for src, const in (("sift_epipolar.hip", "constexpr int kEpiTile = 64;"), ("sift_rigid.hip", "constexpr int kRigidTile = 256;"),
                       ("sift_rigid.hip", "constexpr int kRigidThreads = 256;"), ("sift_planar.hip", "constexpr int kPlanarTile = 64;"),
                       ("sift_planar.hip", "constexpr int kPlanarThreads = 256;"), ("sift_rgbd.hip", "constexpr int kSelectThreads = 256;"),
                       ("sift_pose.hip", "constexpr int kPoseThreads = 256;"),
                       ("sift_pnp.hip", "constexpr int kPnPTile = 64;"),
                       ("sift_ransac_chain.h", "constexpr int kRansacTile = 64;"),
                       # each unit's tile is the one of the scoring body it shares
                       ("sift_epipolar.hip", "static_assert(kEpiTile == kRansacTile &&"),
                       ("sift_planar.hip", "static_assert(kPlanarTile == kRansacTile &&"),
                       ("sift_pnp.hip", "static_assert(kPnPTile == kRansacTile &&")):
        assert const in open(os.path.join(CSRC, src)).read(), const
    # the walks test_ransac_sizes.py is about stand as its plans restate them: one for the planar, epipolar and PnP
    # scoring kernels (ransac_score), which each unit's kernel calls
    for src, walk in (("sift_ransac_chain.h", "for (int tile = begin; tile < end; tile += kRansacTile) {"),
                      ("sift_epipolar.hip", "ransac_score(EpipolarScore{"),
                      ("sift_planar.hip", "ransac_score(PlanarScore{"),
                      ("sift_pnp.hip", "ransac_score(PnPScore{"),
                      ("sift_rigid.hip", "for (int tile = begin; tile < end; tile += kRigidTile) {"),
                      ("sift_planar.hip", "for (int b = tx; b < (int)blockIdx.x; b += kPlanarThreads) before += block_counts[b];"),
                      ("sift_rgbd.hip", "for (int b = tx; b < (int)blockIdx.x; b += kSelectThreads) before += block_counts[b];")):
        assert walk in open(os.path.join(CSRC, src)).read(), walk
