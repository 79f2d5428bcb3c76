"""Cross-checked registration: cusift_ctx_set_cross_check and what it does to cusift_register_planar, cusift_register_rgbd,
cusift_register_planar_batch and cusift_register_rgbd_batch (cusift_amd/csrc/sift_register.hip; the marking and selection
kernels of sift_planar.hip and sift_sequence.hip).

THE RULE.  Record i of frame 1 is mutual iff its match m lies in [0, n2) and the column side's best for record m of frame
2 is i, the column side being test_match_mutual.column_model: the lowest record of frame 1 wins an exactly tied best.

YARDSTICKS, none fitted to what the kernels return:
  * counts: a numpy model of the rule (mutual_model) on planted many-to-one frames.  Frame 1 holds N records with one
    partner each in frame 2 and, at higher indices, K exact copies of K of them.  A copy's row of the score matrix is its
    original's bit for bit, so both tie for the best of the partner's column and the original, the lower record, keeps
    it.  The descriptors are unit-norm random vectors, a partner's is the record's plus 1 % noise: a true pair scores
    about 1e-4 (L2) against about 0.7 for any other pair, so every threshold used here is passed or missed by orders of
    magnitude and the model's counts do not depend on the last bits of a score (asserted on the CPU).
  * everything else: the staged routes (cusift_match_mutual, then the host applies the rule, then
    cusift_estimate_homography; cusift_match_mutual + cusift_select_mutual + cusift_estimate_rigid) and the pair calls,
    byte for byte -- the routes are deterministic.
No tolerance appears in this file except the end-to-end test's, which is test_planar.test_end_to_end_on_a_warped_frame's.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import test_planar
from oracle_binding import SIFT_POINT_DTYPE
from test_match_mutual import column_model, expected_selection
from test_matching_exact import HUGE, ambiguity, exact_pair, match_model, score_matrix
from test_planar import candidates, corner_distance, fit_set, improve, r32_of, sample4, warp
from test_planar_batch import unit_descriptors
from test_rgbd import H, THRESH2, W, camera
from test_rgbd_batch import encode_depth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_cross_check")
BIN = os.path.join(CPP, "cross_check_dropin")
MAX_PTS = 1024
MASK64 = 0xFFFFFFFFFFFFFFFF
LOOPS = 1008
# distance -> the planar rule that fits it and the thresholds of both registrations
PLANAR = {1: dict(rule=1, lo=999.0, hi=0.8), 0: dict(rule=0, lo=0.0, hi=0.8)}
SELECT = dict(score_threshold=999.0, ambiguity_threshold=0.8)
SHIFT = (7, -4)  # frame 2's pixel = frame 1's + SHIFT: a translation in the plane and, at one depth, in space
DEPTH_MM = 2000
ONE_RECORD = np.zeros(1, SIFT_POINT_DTYPE)  # what an empty frame's buffer holds


# ------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------
def row_model(S, l2):
    """(best, second, idx) of every row of S: FindMinCorr / FindMaxCorr's result wherever a row's best is unique."""
    order = np.argsort(S if l2 else -S, axis=1, kind="stable")
    rows = np.arange(len(S))
    return S[rows, order[:, 0]], S[rows, order[:, 1]], order[:, 0].astype(np.int32)


def mutual_model(S, l2, row_idx=None):
    """bool [n1]: record i's match m lies in [0, n2) and column_model's best for column m is i."""
    n1, n2 = S.shape
    m = row_model(S, l2)[2] if row_idx is None else np.asarray(row_idx)
    back = column_model(S, l2)[2]
    ok = (m >= 0) & (m < n2)
    return ok & (back[np.where(ok, m, 0)] == np.arange(n1))


def model_counts(f1, f2, distance):
    """(candidates without the cross-check, with it, the mutual mask) of a planted pair by the numpy model alone, for the
    planar rule and -- the same numbers -- for the RGB-D selection at SELECT."""
    S = score_matrix(f1["data"], f2["data"], distance, exact=False)
    best, second, idx = row_model(S, distance)
    amb = ambiguity(best, second, distance)
    args = PLANAR[distance]
    if args["rule"] == 0:
        keep = (best > np.float32(args["lo"])) & (amb < np.float32(args["hi"]))
    else:
        keep = (best < np.float32(args["lo"]) ** 2) & (amb < np.float32(args["hi"]) ** 2)
    sel = (best < np.float32(999.0) ** 2) & (amb < np.float32(0.8) ** 2) if distance else keep
    mutual = mutual_model(S, distance, idx)
    # the margins that make these counts independent of a score's last bits: ambiguities far from the threshold
    edge = np.abs(amb.astype(np.float64) - (0.64 if args["rule"] == 1 else 0.8))
    return int(keep.sum()), int((keep & mutual).sum()), mutual, float(edge[keep].min()), int(sel.sum())


# ------------------------------------------------------------------------------------------------------------------
# the frames
# ------------------------------------------------------------------------------------------------------------------
def noisy(r, d):
    out = d + r.normal(0, 0.01 / np.sqrt(128), d.shape).astype(np.float32)
    return (out / np.linalg.norm(out.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)


def pixels(r, n, taken=()):
    """n distinct integer pixels at least 40 from the border, none of them in `taken` (flat indices)."""
    free = np.setdiff1d(np.arange((W - 80) * (H - 80)), np.asarray(taken, np.int64))
    flat = r.choice(free, n, replace=False)
    return flat, np.c_[40 + flat % (W - 80), 40 + flat // (W - 80)]


def flat_of(px):
    return (px[:, 1] - 40) * (W - 80) + (px[:, 0] - 40)


def records_at(px, data):
    p = np.zeros(len(px), SIFT_POINT_DTYPE)
    p["coords2D"], p["data"] = px.astype(np.float32), data
    p["score"], p["ambiguity"], p["match"] = 0.25, 0.5, -5
    p["match_xpos"], p["match_ypos"], p["match_error"] = -3.0, -4.0, 7.0
    p["coords3D"] = 7.0
    return p


def depth_image(px, mm):
    d = np.zeros((H, W), np.uint16)
    d[px[:, 1], px[:, 0]] = encode_depth(mm)
    return d


def many_to_one(n_true, n_extra, n2, seed, frame2=None):
    """(frame 1, frame 2, depth 1, depth 2): frame 1 = n_true records whose partners are distinct records of frame 2, SHIFT
    away at DEPTH_MM, then n_extra exact descriptor copies of the true records 0, 3, 6, ... at pixels and depths of their
    own.  frame2 = (records, depth) reuses a frame 2."""
    r = np.random.default_rng(seed)
    if frame2 is None:
        _, px2 = pixels(r, n2)
        f2 = records_at(px2, unit_descriptors(r, n2))
        d2 = depth_image(px2, np.full(n2, DEPTH_MM))
    else:
        f2, d2 = frame2
        px2 = f2["coords2D"].astype(np.int64)
    partner = r.permutation(n2)[:n_true]
    px_true = px2[partner] - np.array(SHIFT)
    data = noisy(r, f2["data"][partner])
    src = 3 * np.arange(n_extra)
    assert src.max() < n_true
    # a copy is a gross outlier of the planted motion: at least 50 px from where its original stands
    pool = list(pixels(r, 4 * n_extra, flat_of(px_true))[1])
    px_extra = np.array([pool.pop(next(k for k, q in enumerate(pool) if np.abs(q - px_true[i]).max() >= 50)) for i in src])
    assert np.abs(px_extra - px_true[src]).max(axis=1).min() >= 50 and len(np.unique(flat_of(px_extra))) == n_extra
    f1 = records_at(np.r_[px_true, px_extra], np.r_[data, data[src]])
    d1 = depth_image(np.r_[px_true, px_extra], np.r_[np.full(n_true, DEPTH_MM), r.integers(900, 2800, n_extra)])
    return f1, f2, d1, d2, partner


# (records of frame 1 = true + copies, copies, records of frame 2): 300, 900 and 1024 cross a 64-row block and a
# 256-record block, n2 != n1
PLANTED = {0: (250, 50, 280), 2: (800, 100, 1000), 4: (900, 124, 950)}


class Frames:
    """Eight frames in 1024 slots: three planted pairs (0, 1), (2, 3), (4, 5); 6 is empty; 7 holds 5 records.  The first
    280 records of frame 3 are frame 1's with noise, 3 px right and 5 px down, so (1, 3) is a pair without copies and
    frame 1 stands on both sides.  Records past a count are live-looking copies with valid pixels."""

    def __init__(self):
        sets, self.partner = {}, {}
        f1a, f2a, d1a, d2a, self.partner[0] = many_to_one(*PLANTED[0], seed=21)
        r = np.random.default_rng(5)
        px3 = np.r_[f2a["coords2D"].astype(np.int64) + np.array((3, 5)),
                    pixels(r, 1000 - 280, flat_of(f2a["coords2D"].astype(np.int64) + np.array((3, 5))))[1]]
        f2b = records_at(px3, np.r_[noisy(r, f2a["data"]), unit_descriptors(r, 1000 - 280)])
        d2b = depth_image(px3, np.full(1000, DEPTH_MM))
        f1b, _, d1b, _, self.partner[2] = many_to_one(*PLANTED[2], seed=22, frame2=(f2b, d2b))
        f1c, f2c, d1c, d2c, self.partner[4] = many_to_one(*PLANTED[4], seed=23)
        frames = [f1a, f2a, f1b, f2b, f1c, f2c, f2a[:0], f2c[:5]]
        depth = [d1a, d2a, d1b, d2b, d1c, d2c, np.zeros_like(d1a), d2c]
        self.points = np.zeros((8, MAX_PTS), SIFT_POINT_DTYPE)
        self.points[:] = np.resize(f2b, MAX_PTS)
        for k, f in enumerate(frames):
            self.points[k, :len(f)] = f
        self.n = np.array([len(f) for f in frames])
        self.counters = self.n.astype(np.uint32)
        self.counters[4] = 3000  # a full frame whose counter says more
        self.depth = np.stack(depth)

    def frame(self, k):
        return self.points[k, :self.n[k]].copy()


@pytest.fixture(scope="module")
def frames():
    return Frames()


# every planted pair, a frame on both sides, an empty frame on either side, fewer than 8 records, a self pair, a pair of
# unrelated frames (few candidates)
PAIRS = np.array([(0, 1), (2, 3), (4, 5), (1, 3), (6, 1), (0, 6), (7, 5), (3, 3), (2, 5)], np.int32)


# ------------------------------------------------------------------------------------------------------------------
# without a GPU
# ------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_recipes_agree():
    from cusift_amd import batch, capi
    import inspect

    extras = open(os.path.join(ROOT, "include", "cusift_amd_extras.h")).read()
    assert "int cusift_ctx_set_cross_check(cusift_ctx *ctx, int on);" in extras
    handle = C.CDLL(capi.LIB_PATH)
    assert hasattr(handle, "cusift_ctx_set_cross_check")
    res, args = capi.SIGNATURES["cusift_ctx_set_cross_check"]
    assert res is C.c_int and len(args) == 2
    assert capi.lib().cusift_ctx_set_cross_check(None, 1) == -1  # CUSIFT_ERR_INVALID: no context
    assert callable(capi.Context.set_cross_check)
    for bad in (2, -1, 0.5, "on", None):
        with pytest.raises(ValueError):
            capi.check_cross_check(bad)
    assert [capi.check_cross_check(v) for v in (False, True, 0, 1, np.int32(1))] == [0, 1, 0, 1, 1]
    assert inspect.signature(batch.BatchExtractor.__init__).parameters["cross_check"].default is False
    # the existing entry points keep their argument counts
    for name, nargs in (("cusift_register_planar", 24), ("cusift_register_rgbd", 23), ("cusift_register_rgbd_batch", 25),
                        ("cusift_register_planar_batch", 24)):
        assert len(capi.SIGNATURES[name][1]) == nargs, name
    assert "cpp_cross_check" in open(os.path.join(ROOT, "Makefile")).read()
    assert "tests/cpp_cross_check/cross_check_dropin.cpp" in open(os.path.join(ROOT, "CMakeLists.txt")).read()
    assert "tests/cpp_cross_check/cross_check_dropin" in open(os.path.join(ROOT, ".gitignore")).read()
    head = open(os.path.join(ROOT, "include", "matching.h")).read()
    assert "inline void SetCrossCheck(bool on)" in head and "cusift_ctx_set_cross_check(" in head
    assert "written" in extras.split("int cusift_register_planar(")[0].rsplit("/*", 1)[1]  # the const caveat


@pytest.mark.parametrize("n1,n2", [(70, 95), (129, 160)])
def test_mutual_model_on_exact_ties_exercises_the_lowest_row_rule(n1, n2):
    """On the exact 'ties' family some record of frame 1 scores exactly its partner's best and still is not mutual: a
    lower record of frame 1 holds the same score.  Such a record would be mutual under any other tie rule."""
    s1, s2 = exact_pair(n1, n2, "ties")
    for l2 in (1, 0):
        S = score_matrix(s1["data"], s2["data"], l2)
        idx = match_model(S, l2, HUGE)[2]
        best, _, back = column_model(S, l2)
        mutual = mutual_model(S, l2, idx)
        ok = (idx >= 0) & (idx < n2)
        m = np.where(ok, idx, 0)
        rows = np.arange(n1)
        losers = ok & ~mutual & (S[rows, m] == best[m]) & (back[m] < rows)
        print("(%d, %d) l2=%d: %d mutual of %d, %d lose a tie to a lower record" % (n1, n2, l2, mutual.sum(), n1,
                                                                                      losers.sum()))
        # by brute force: a mutual record is the FIRST row attaining its column's extreme, and the records that attain
        # it without being the first are the losers counted above
        lost = 0
        for i in np.flatnonzero(ok):
            col = [float(v) for v in S[:, idx[i]]]
            top = min(col) if l2 else max(col)
            assert mutual[i] == (col.index(top) == i), i
            lost += col[i] == top and col.index(top) != i
        assert losers.sum() == lost >= 1


def test_planted_frames_give_the_counts_by_the_model_alone(frames):
    for a, (n_true, n_extra, n2) in PLANTED.items():
        f1, f2 = frames.frame(a), frames.frame(a + 1)
        assert (len(f1), len(f2)) == (n_true + n_extra, n2) and len(f1) != len(f2)
        for distance in (1, 0):
            off, on, mutual, edge, sel = model_counts(f1, f2, distance)
            print("pair (%d, %d) d%d: %d candidates, %d mutual; nearest ambiguity %.3f from its threshold" %
                  (a, a + 1, distance, off, on, edge))
            assert (off, on, sel) == (n_true + n_extra, n_true, n_true + n_extra)
            assert mutual[:n_true].all() and not mutual[n_true:].any()
            assert edge > 0.5
            # a copy's row IS its original's: the tie is exact in any arithmetic
            assert f1["data"][n_true:].tobytes() == f1["data"][3 * np.arange(n_extra)].tobytes()
    # (1, 3): no copies, every record mutual; the self pair: every record its own match
    S = score_matrix(frames.frame(1)["data"], frames.frame(3)["data"], 1, exact=False)
    assert mutual_model(S, 1).all()
    f3 = frames.frame(3)
    S = score_matrix(f3["data"], f3["data"], 1, exact=False)
    assert np.array_equal(row_model(S, 1)[2], np.arange(len(f3))) and mutual_model(S, 1).all()


def test_cpp_program_compiles_and_links_with_plain_gxx():
    if os.path.exists(BIN):
        os.remove(BIN)
    subprocess.check_call(["make", "-C", CPP, "all"], stdout=subprocess.DEVNULL)
    assert os.path.exists(BIN)
    recipe = open(os.path.join(CPP, "Makefile")).read()
    assert "hipcc" not in recipe and "/opt/rocm" not in recipe
    assert "#include <hip" not in open(os.path.join(ROOT, "include", "matching.h")).read()


def test_touched_kernels_compile_for_gfx950_without_scratch_or_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs

    found = set()
    for src, wanted in (("sift_planar.hip", ("planar_mark_kernel",)),
                        ("sift_sequence.hip", ("sequence_mark_kernel", "sequence_select_kernel"))):
        asm = kernel_regs.assembly(src)
        assert "gfx950" in asm
        for k in kernel_regs.kernels(asm):
            hit = [w for w in wanted if w in k["name"]]
            if not hit:
                continue
            found.update(hit)
            assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
            assert k["name"].endswith(("PK12cusift_point", "S2_", "S9_")), k["name"]  # the cross-check pointer is last
    assert len(found) == 3, sorted(found)


# ------------------------------------------------------------------------------------------------------------------
# on the GPU
# ------------------------------------------------------------------------------------------------------------------
def upload(ctx, arr):
    from cusift_amd.capi import DeviceBuffer

    return DeviceBuffer.from_numpy(ctx, arr)


@pytest.fixture()
def own():
    """A context of this test's own, cross-check off: the session's shared context is never switched."""
    from cusift_amd import capi

    if capi.device_count() < 1:
        pytest.fail("gpu test selected but no HIP device is visible")
    c = capi.Context(0)
    yield c
    c.close()


def planar_pair(ctx, f1, f2, seed, distance, **kw):
    """register_planar on fresh uploads; returns (PlanarResult, frame 1 afterwards, frame 2 afterwards)."""
    b1, b2 = upload(ctx, f1 if len(f1) else ONE_RECORD), upload(ctx, f2 if len(f2) else ONE_RECORD)
    args = dict(loops=LOOPS, thresh=5.0, refine_loops=5, refine_thresh=3.0, want_all=True)
    args.update(PLANAR[distance])
    args.update(kw)
    res = ctx.register_planar(b1.ptr, len(f1), b2.ptr, len(f2), distance=distance, seed=seed & MASK64, **args)
    out = res, b1.to_numpy(SIFT_POINT_DTYPE, (max(len(f1), 1),))[:len(f1)], b2.to_numpy(SIFT_POINT_DTYPE,
                                                                                       (max(len(f2), 1),))[:len(f2)]
    b1.free()
    b2.free()
    return out


def rgbd_pair(ctx, f1, d1, f2, d2, seed, distance, kind="3d"):
    """register_rgbd on fresh uploads; returns ((Rt, pairs, flags, inliers), frame 1 afterwards, frame 2 afterwards)."""
    b1, b2 = upload(ctx, f1 if len(f1) else ONE_RECORD), upload(ctx, f2 if len(f2) else ONE_RECORD)
    e1, e2 = upload(ctx, d1), upload(ctx, d2)
    res = ctx.register_rgbd(b1.ptr, len(f1), e1.ptr, b2.ptr, len(f2), e2.ptr, W, H, camera(), distance=distance, loops=1024,
                            thresh2=THRESH2, kind=kind, seed=seed & MASK64, **SELECT)
    out = res, b1.to_numpy(SIFT_POINT_DTYPE, (max(len(f1), 1),))[:len(f1)], b2.to_numpy(SIFT_POINT_DTYPE,
                                                                                       (max(len(f2), 1),))[:len(f2)]
    for b in (b1, b2, e1, e2):
        b.free()
    return out


def planar_batch(ctx, fr, seed, distance, pairs=PAIRS):
    pts, cnt = upload(ctx, fr.points), upload(ctx, fr.counters)
    res = ctx.register_planar_batch(pts.ptr, cnt.ptr, 8, MAX_PTS, pairs, distance=distance, loops=LOOPS, thresh=5.0,
                                    refine_loops=5, refine_thresh=3.0, seed=seed, want_inliers=True, want_errors=True,
                                    **PLANAR[distance])
    after = pts.to_numpy(SIFT_POINT_DTYPE, (8, MAX_PTS))
    pts.free()
    cnt.free()
    return res, after


def rgbd_batch(ctx, fr, seed, distance, pairs=PAIRS):
    pts, cnt, dep = upload(ctx, fr.points), upload(ctx, fr.counters), upload(ctx, fr.depth)
    res = ctx.register_rgbd_batch(pts.ptr, cnt.ptr, 8, MAX_PTS, dep.ptr, W, H, camera(), pairs, distance=distance,
                                  loops=1024, thresh2=THRESH2, kind="3d", seed=seed, **SELECT)
    after = pts.to_numpy(SIFT_POINT_DTYPE, (8, MAX_PTS))
    for b in (pts, cnt, dep):
        b.free()
    return res, after


def same_planar(x, y):
    return all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(x, y))


def same_planar_batch(x, y):
    if any(np.asarray(u).tobytes() != np.asarray(v).tobytes() for u, v in zip(x[:7], y[:7])):
        return False
    return all(a.tobytes() == b.tobytes() for a, b in zip(x.inliers, y.inliers)) and all(
        a.tobytes() == b.tobytes() for a, b in zip(x.match_error, y.match_error))


def same_rgbd(x, y):
    return all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(x, y))


def same_rgbd_batch(x, y):
    return all(u.tobytes() == v.tobytes() for u, v in zip(x[:3], y[:3])) and all(
        a.tobytes() == b.tobytes() for a, b in zip(x[3] + x[4], y[3] + y[4]))


# ---- 1. planted many-to-one: fails without the feature ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
@pytest.mark.parametrize("a", sorted(PLANTED))
def test_planted_many_to_one_pair_calls(own, frames, a, distance):
    n_true, n_extra, n2 = PLANTED[a]
    f1, f2 = frames.frame(a), frames.frame(a + 1)
    off, off_after, _ = planar_pair(own, f1, f2, 3, distance)
    r_off, _, _ = rgbd_pair(own, f1, frames.depth[a], f2, frames.depth[a + 1], 3, distance)
    own.set_cross_check(True)
    on, _, _ = planar_pair(own, f1, f2, 3, distance)
    r_on, _, _ = rgbd_pair(own, f1, frames.depth[a], f2, frames.depth[a + 1], 3, distance)
    print("pair (%d, %d) d%d: planar %d -> %d candidates, %d -> %d inliers; RGB-D %d -> %d matches, %d -> %d inliers" %
          (a, a + 1, distance, off.num_candidates, on.num_candidates, off.num_matches, on.num_matches, len(r_off[1]),
           len(r_on[1]), r_off[3], r_on[3]))
    assert off.num_candidates == n_true + n_extra and len(r_off[1]) == n_true + n_extra
    assert on.num_candidates == n_true and len(r_on[1]) == n_true
    assert on.drawn.max() < n_true and np.array_equal(on.drawn, sample4(3, n_true, LOOPS))  # candidates 0 .. n_true - 1
    assert not on.inliers[n_true:].any() and on.inliers[:n_true].all() and on.num_matches == n_true
    assert on.num_fit == n_true  # the refit saw no copy: every true record lies on the translation
    assert np.array_equal(r_on[1], np.c_[np.arange(n_true), frames.partner[a]]) and r_on[2].all() and r_on[3] == n_true
    shift = np.array([1, 0, SHIFT[0], 0, 1, SHIFT[1], 0, 0], np.float64)
    # on: exact integer correspondences and no copy in the refit set, so the refit is the translation up to fp32
    assert corner_distance(on.homography[:8], shift) < 1e-2
    # off: the copies are in the refit set and bend the eight coefficients (the perspective terms most, and the corners
    # lie outside the 640 x 480 the records cover), by an amount no short argument bounds.  What can be held is what
    # test_planar holds every refit to: the float64 restatement of ImproveHomography over the same set from the same
    # winner, within max(64 d_order, r32), match_error and num_fit included.
    matched = off_after.copy()
    matched["match_error"] = f1["match_error"]
    test_planar.check_refit(matched, off, off_after, PLANAR[distance], 5, 3.0, n2)
    assert off.num_matches >= n_true


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
def test_planted_many_to_one_batch_calls(own, frames, distance):
    off, _ = planar_batch(own, frames, 3, distance)
    r_off, _ = rgbd_batch(own, frames, 3, distance)
    own.set_cross_check(True)
    on, recs = planar_batch(own, frames, 3, distance)
    r_on, _ = rgbd_batch(own, frames, 3, distance)
    assert recs.tobytes() == frames.points.tobytes()  # the records: never written
    for p, (a, b) in enumerate(PAIRS[:3]):
        n_true, n_extra, _ = PLANTED[a]
        assert off.num_candidates[p] == n_true + n_extra and r_off[1][p] == n_true + n_extra, p
        assert on.num_candidates[p] == n_true and r_on[1][p] == n_true, p
        assert on.inliers[p][:n_true].all() and not on.inliers[p][n_true:].any() and on.num_fit[p] == n_true, p
        assert np.array_equal(r_on[3][p], np.c_[np.arange(n_true), frames.partner[a]]), p
    # no copies: nothing to remove; the self pair: every record is its own mutual match
    assert on.num_candidates[3] == off.num_candidates[3] == 280 and r_on[1][3] == r_off[1][3] == 280
    assert on.num_candidates[7] == off.num_candidates[7] == 1000 and r_on[1][7] == r_off[1][7] == 1000
    # an empty frame on either side, fewer than 8 records: no candidate, as before
    for p in (4, 5, 6):
        assert on.num_candidates[p] == 0 and on.num_matches[p] == 0, p
    assert r_on[1][4] == 0 and r_on[1][5] == 0


# ---- 2. planar pair, on, equals the staged route -----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
@pytest.mark.parametrize("a,b", [(0, 1), (4, 5), (2, 5)])
def test_planar_pair_equals_the_staged_route(own, frames, a, b, distance):
    f1, f2 = frames.frame(a), frames.frame(b)
    args = PLANAR[distance]
    if (a, b) == (2, 5):  # unrelated frames: thresholds that keep a strict subset with non-mutual records in it
        args = dict(rule=1, lo=999.0, hi=0.999) if distance else dict(rule=0, lo=0.0, hi=0.999)
    # staged: match_mutual, the host applies the rule, estimate_homography
    c1, c2 = upload(own, f1), upload(own, f2)
    own.match_mutual(c1.ptr, len(f1), c2.ptr, len(f2), distance)
    own.synchronize()
    m1, m2 = c1.to_numpy(SIFT_POINT_DTYPE, (len(f1),)), c2.to_numpy(SIFT_POINT_DTYPE, (len(f2),))
    ok = (m1["match"] >= 0) & (m1["match"] < len(f2))
    mutual = ok & (m2["match"][np.where(ok, m1["match"], 0)] == np.arange(len(f1)))
    out = m1.copy()
    out["score"][~mutual] = -2.0 if args["rule"] == 0 else 1e30  # fails `cand` and `fit` under the rule in use
    assert len(candidates(out, args["rule"], args["lo"], args["hi"], len(f2))) == len(
        fit_set(out, args["rule"], args["lo"], args["hi"], len(f2)))
    plain = candidates(m1, args["rule"], args["lo"], args["hi"], len(f2))
    kept = candidates(out, args["rule"], args["lo"], args["hi"], len(f2))
    if (a, b) == (2, 5):
        assert 8 <= len(kept) < len(plain)  # the rule bites on records the thresholds let through
    d = upload(own, out)
    staged = own.estimate_homography(d.ptr, len(f1), len(f2), loops=LOOPS, thresh=5.0, refine_loops=5, refine_thresh=3.0,
                                     seed=9, want_all=True, **args)
    after = d.to_numpy(SIFT_POINT_DTYPE, (len(f1),))
    after["score"] = m1["score"]
    own.set_cross_check(True)
    fused, g1, g2 = planar_pair(own, f1, f2, 9, distance, **args)
    print("pair (%d, %d) d%d: %d candidates by the thresholds, %d mutual; %d inliers, %d fit" %
          (a, b, distance, len(plain), len(kept), fused.num_matches, fused.num_fit))
    assert fused.num_candidates == len(kept)
    assert same_planar(fused, staged)
    assert np.array_equal(fused.drawn, kept[sample4(9, len(kept), LOOPS)])
    assert g1.tobytes() == after.tobytes()
    assert g2.tobytes() == m2.tobytes()  # d_sift2's match fields: match_mutual's
    for buf in (c1, c2, d):
        buf.free()


# ---- 3. RGB-D pair, on, equals its staged route ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
@pytest.mark.parametrize("a,b", [(0, 1), (4, 5)])
def test_rgbd_pair_equals_the_staged_route(own, frames, a, b, distance):
    f1, f2 = frames.frame(a), frames.frame(b)
    n1, n2 = len(f1), len(f2)
    c1, c2 = upload(own, f1), upload(own, f2)
    e1, e2 = upload(own, frames.depth[a]), upload(own, frames.depth[b])
    own.lift_depth(c1.ptr, n1, e1.ptr, W, H, camera())
    own.lift_depth(c2.ptr, n2, e2.ptr, W, H, camera())
    own.match_mutual(c1.ptr, n1, c2.ptr, n2, distance)
    d_pairs = upload(own, np.full((n1, 2), -9, np.int32))
    d_coord = upload(own, np.full((n1, 6), -9.0, np.float32))
    d_count = upload(own, np.full(1, -9, np.int32))
    own.select_mutual(c1.ptr, n1, c2.ptr, n2, d_pairs.ptr, d_coord.ptr, d_count.ptr, kind="3d", **SELECT)
    own.synchronize()
    count = int(d_count.to_numpy(np.int32, (1,))[0])
    pairs, coord = d_pairs.to_numpy(np.int32, (n1, 2))[:count], d_coord.to_numpy(np.float32, (n1, 6))[:count]
    m1, m2 = c1.to_numpy(SIFT_POINT_DTYPE, (n1,)), c2.to_numpy(SIFT_POINT_DTYPE, (n2,))
    want_p, want_c = expected_selection(m1, m2, SELECT["score_threshold"], SELECT["ambiguity_threshold"], True, True)
    assert pairs.tobytes() == want_p.tobytes() and coord.tobytes() == want_c.tobytes()
    rt, n_in, _, flags = own.estimate_rigid(coord, loops=1024, thresh2=THRESH2, kind="3d", seed=9)
    own.set_cross_check(True)
    (g_rt, g_pairs, g_flags, g_in), g1, g2 = rgbd_pair(own, f1, frames.depth[a], f2, frames.depth[b], 9, distance)
    assert count == PLANTED[a][0] == len(g_pairs)
    assert g_rt.tobytes() == rt.tobytes() and g_in == n_in and g_pairs.tobytes() == pairs.tobytes()
    assert np.array_equal(g_flags, flags)
    assert g1.tobytes() == m1.tobytes() and g2.tobytes() == m2.tobytes()
    for buf in (c1, c2, e1, e2, d_pairs, d_coord, d_count):
        buf.free()


# ---- 4. both batch forms, on, equal the pair calls ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
def test_batch_forms_equal_the_pair_calls(own, frames, distance):
    seed = 0xC0FFEE
    own.set_cross_check(True)
    res, _ = planar_batch(own, frames, seed, distance)
    rgbd, _ = rgbd_batch(own, frames, seed, distance)
    ident = np.eye(3, dtype=np.float32).ravel()
    for p, (a, b) in enumerate(PAIRS):
        # the self pair against a copy: the pair call refuses overlapping ranges
        f1, f2 = frames.frame(a), frames.frame(b)
        one, after, _ = planar_pair(own, f1, f2, seed + p, distance, want_all=False)
        what = "pair %d (%d, %d) d%d" % (p, a, b, distance)
        print("%s: %d candidates, %d inliers, %d fit; RGB-D %d matches, %d inliers" %
              (what, one.num_candidates, one.num_matches, one.num_fit, rgbd[1][p], rgbd[2][p]))
        assert res.homography[p].tobytes() == one.homography.tobytes(), what
        assert res.ransac[p].tobytes() == one.ransac.tobytes(), what
        got = (res.num_candidates[p], res.num_matches[p], res.num_fit[p], res.best_loop[p])
        assert got == (one.num_candidates, one.num_matches, one.num_fit, one.best_loop), (what, got)
        assert res.counts[p] == len(f1) and np.array_equal(res.inliers[p], one.inliers[:len(f1)]), what
        if one.num_candidates >= 8:
            assert res.match_error[p].tobytes() == after["match_error"].tobytes(), what
        else:
            assert np.isnan(res.match_error[p]).all() and np.array_equal(res.homography[p], ident), what
        (rt, sel, flags, n_in), _, _ = rgbd_pair(own, f1, frames.depth[a], f2, frames.depth[b], seed + p, distance)
        assert rgbd[0][p].tobytes() == rt.tobytes() and rgbd[1][p] == len(sel) and rgbd[2][p] == n_in, what
        assert rgbd[3][p].tobytes() == sel.tobytes() and np.array_equal(rgbd[4][p], flags), what
    assert res.num_candidates[8] < 8 or res.num_candidates[8] < len(frames.frame(2))  # unrelated frames


# ---- 5. off is off ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_off_is_off_after_on(own, frames):
    from cusift_amd import capi

    f1, f2 = frames.frame(2), frames.frame(3)

    def everything(ctx):
        out = [planar_pair(ctx, f1, f2, 5, 1), rgbd_pair(ctx, f1, frames.depth[2], f2, frames.depth[3], 5, 1),
               planar_batch(ctx, frames, 5, 1), rgbd_batch(ctx, frames, 5, 1)]
        return out

    own.set_cross_check(True)
    with_it = everything(own)
    own.set_cross_check(False)
    # the calls that share register_scratch, in between: a rigid call and a selection on matched records
    coord = np.random.default_rng(1).uniform(-1, 1, (500, 6)).astype(np.float32)
    rigid = own.estimate_rigid(coord, loops=256, kind="3d", seed=2)
    c1, c2 = upload(own, f1), upload(own, f2)
    own.match(c1.ptr, len(f1), c2.ptr, len(f2), 1)
    sel = [upload(own, np.full((len(f1), 2), -9, np.int32)), upload(own, np.full((len(f1), 6), -9.0, np.float32)),
           upload(own, np.full(1, -9, np.int32))]
    own.select_matches(c1.ptr, len(f1), c2.ptr, len(f2), sel[0].ptr, sel[1].ptr, sel[2].ptr, kind="2d", **SELECT)
    own.synchronize()
    selected = [sel[0].to_numpy(np.int32, (len(f1), 2)), sel[1].to_numpy(np.float32, (len(f1), 6)),
                sel[2].to_numpy(np.int32, (1,))]
    again = everything(own)
    fresh = capi.Context(0)
    try:
        want = everything(fresh)
        want_rigid = fresh.estimate_rigid(coord, loops=256, kind="3d", seed=2)
        d1, d2 = upload(fresh, f1), upload(fresh, f2)
        fresh.match(d1.ptr, len(f1), d2.ptr, len(f2), 1)
        sel2 = [upload(fresh, np.full((len(f1), 2), -9, np.int32)), upload(fresh, np.full((len(f1), 6), -9.0, np.float32)),
                upload(fresh, np.full(1, -9, np.int32))]
        fresh.select_matches(d1.ptr, len(f1), d2.ptr, len(f2), sel2[0].ptr, sel2[1].ptr, sel2[2].ptr, kind="2d", **SELECT)
        fresh.synchronize()
        want_selected = [sel2[0].to_numpy(np.int32, (len(f1), 2)), sel2[1].to_numpy(np.float32, (len(f1), 6)),
                         sel2[2].to_numpy(np.int32, (1,))]
    finally:
        fresh.close()
    assert all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(rigid, want_rigid))
    assert selected[2][0] == len(f1) and all(u.tobytes() == v.tobytes() for u, v in zip(selected, want_selected))
    assert same_planar(again[0][0], want[0][0]) and same_rgbd(again[1][0], want[1][0])
    assert same_planar_batch(again[2][0], want[2][0]) and same_rgbd_batch(again[3][0], want[3][0])
    for k in range(4):  # every device record the calls wrote or left alone
        for u, v in zip(again[k][1:], want[k][1:]):
            assert u.tobytes() == v.tobytes(), k
    assert again[0][2].tobytes() == f2.tobytes()  # off: frame 2 of the planar pair call is not written
    # and the setting did something while it was on
    assert with_it[0][0].num_candidates == 800 and again[0][0].num_candidates == 900
    assert not same_planar_batch(with_it[2][0], again[2][0]) and not same_rgbd_batch(with_it[3][0], again[3][0])


# ---- 6. refusals write nothing -----------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals_write_nothing(own, frames):
    from cusift_amd import capi

    lib, INVALID = capi.lib(), -1
    both = np.concatenate([frames.frame(0), frames.frame(1)])
    n1, n2 = int(frames.n[0]), int(frames.n[1])
    d = upload(own, both)
    hom, ran = np.full(9, 9.0, np.float32), np.full(9, 9.0, np.float32)
    ints = [C.c_int(-7) for _ in range(4)]
    flags = np.full(n1, 9, np.int8)

    def planar(p1, c1, p2, c2):
        return lib.cusift_register_planar(own.handle, p1, c1, p2, c2, 1, 1, 999.0, 0.8, 64, 5.0, 5, 3.0, 1, hom.ctypes.data,
                                          ran.ctypes.data, *[C.byref(v) for v in ints], flags.ctypes.data, None, None, None)

    def untouched():
        own.synchronize()
        return ((hom == 9.0).all() and (ran == 9.0).all() and all(v.value == -7 for v in ints) and (flags == 9).all() and
                d.to_numpy(SIFT_POINT_DTYPE, both.shape).tobytes() == both.tobytes())

    # a bad value: refused, the setting stays what it was (off: overlapping ranges are still accepted)
    for bad in (2, -1, 7):
        assert lib.cusift_ctx_set_cross_check(own.handle, bad) == INVALID
    assert untouched()
    assert lib.cusift_ctx_set_cross_check(own.handle, 1) == 0
    for bad in (2, -1):
        assert lib.cusift_ctx_set_cross_check(own.handle, bad) == INVALID  # stays on: the refusals below show it
    rec = SIFT_POINT_DTYPE.itemsize
    assert planar(d.ptr, n1, d.ptr, n1) == INVALID and untouched()  # the same set
    assert planar(d.ptr, n1, d.ptr + (n1 - 1) * rec, n2) == INVALID and untouched()  # one record shared
    assert planar(d.ptr + 10 * rec, n1, d.ptr, 11) == INVALID and untouched()  # the second set ends inside the first
    assert planar(d.ptr, n1, d.ptr + n1 * rec, n2) == 0 and ints[0].value == PLANTED[0][0]  # adjacent ranges: accepted
    own.set_cross_check(False)
    d2 = upload(own, both)
    d, both_d = d2, d
    hom[:], ran[:], flags[:] = 9.0, 9.0, 9
    assert planar(d.ptr, n1, d.ptr, n1) == 0 and ints[0].value > 0  # off: a set against itself is today's behaviour
    both_d.free()
    d2.free()


# ---- 7. end to end -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_end_to_end_on_a_warped_frame_on_and_off(oracle, gray1, record_property):
    """gray1.pgm against itself warped by test_planar's homography, extracted by two BatchExtractors (cross_check off and
    on) and registered with register_planar(0, 1).  Each run is held to test_end_to_end_on_a_warped_frame's bound: the
    corner error against the known homography is at most 1.5 x that of the all-CPU route (oracle extraction and matcher,
    oracle RANSAC on the samples this run drew, numpy refit over this run's candidate rule) plus r32."""
    import torch
    from cusift_amd.batch import BatchExtractor

    Hm = np.array([[0.98, -0.03, 9.0], [0.025, 1.01, -6.0], [1.5e-5, -2.0e-5, 1.0]])
    h, w = gray1.shape
    imgs = np.stack([gray1, warp(gray1, Hm)])
    prm = dict(num_octaves=4, init_blur=0.0, peak_thresh=1.0, max_pts=4096)
    kw = dict(distance=1, rule=1, lo=999.0, hi=0.8, loops=2000, thresh=5.0, refine_loops=5, refine_thresh=3.0, seed=21,
              want_all=True)
    truth = Hm.ravel()[:8] / Hm[2, 2]
    o1, o2 = oracle.extract(imgs[0], **prm).copy(), oracle.extract(imgs[1], **prm).copy()
    back = o2.copy()
    oracle.match(o1, o2, 1)
    oracle.match(back, o1, 1)
    cand = {False: candidates(o1, 1, 999.0, 0.8, len(o2))}
    ok = np.isin(np.arange(len(o1)), cand[False])
    cand[True] = np.flatnonzero(ok & (back["match"][np.clip(o1["match"], 0, len(o2) - 1)] == np.arange(len(o1))))
    saved = test_planar.CORNERS
    test_planar.CORNERS = np.array([[0, 0], [w, 0], [0, h], [w, h]], dtype=np.float64)
    got = {}
    try:
        for on in (False, True):
            ex = BatchExtractor(2, w, h, cross_check=on, **prm)
            try:
                ex.extract(ex.images_from_numpy(imgs))
                torch.cuda.synchronize()
                dev1 = ex.to_host()[0].copy()
                res = ex.register_planar(0, 1, **kw)
            finally:
                ex.close()
            used = np.unique(res.drawn)
            key = lambda r: np.c_[r["coords2D"], r["scale"]].astype(np.float64)  # noqa: E731
            dist = np.abs(key(dev1[used])[:, None, :] - key(o1)[None, :, :]).max(axis=2)
            to_oracle = np.zeros(len(dev1), dtype=np.int32)
            to_oracle[used] = dist.argmin(axis=1)
            hom, _, _, _, _ = oracle.find_homography(o1, to_oracle[res.drawn], thresh=5.0)
            cpu = improve(o1, hom, 5, 3.0, cand[on]).astype(np.float32)
            d_dev, d_cpu, r32 = corner_distance(res.homography[:8], truth), corner_distance(cpu, truth), r32_of(cpu)
            ratio = res.num_matches / max(res.num_candidates, 1)
            print("cross-check %s: %d candidates (%d on the CPU), %d inliers (ratio %.3f), corner error %.4f px, all-CPU "
                  "%.4f px, r32 %.3g" % ("on" if on else "off", res.num_candidates, len(cand[on]), res.num_matches, ratio,
                                         d_dev, d_cpu, r32))
            record_property("inlier_ratio_cross_check_%s" % ("on" if on else "off"), ratio)
            assert res.num_matches >= 50
            assert d_dev <= 1.5 * d_cpu + r32, (on, d_dev, d_cpu, r32)
            got[on] = res
    finally:
        test_planar.CORNERS = saved
    assert got[True].num_candidates <= got[False].num_candidates


# ---- 8. the C++ program ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cpp_program_passes_on_gpu():
    subprocess.check_call(["make", "-C", CPP, "all"], stdout=subprocess.DEVNULL)
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout
