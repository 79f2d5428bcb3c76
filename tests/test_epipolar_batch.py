"""The pair-list forms of the fundamental matrix and of the calibrated pose: cusift_register_epipolar_batch and
cusift_register_pose_batch (cusift_amd/csrc/sift_register.hip: ransac_batch_run; sift_sequence.hip: the marking;
sift_epipolar.hip / sift_pose.hip with one grid layer per pair), capi.Context.register_epipolar_batch /
register_pose_batch and BatchExtractor.register_epipolar_sequence / register_pose_sequence.  tests/test_pnp_batch.py holds
the same for cusift_register_pnp_batch and shares this file's frames.

The defining equality is bit for bit: every output of pair p = (a, b) is what the staged route gives -- pair p's row of
cusift_match_batch scattered into a copy of frame a's records, cusift_estimate_fundamental with seed + p and then
cusift_estimate_pose on that F at refine_thresh -- and, where the rows equal cusift_match's fields (asserted for every
pair), what cusift_register_epipolar / cusift_register_pose give on copies of the two frames.

THE FRAMES.  One planted 3-D scene, 1024 points of tests/test_pnp.py's 2-to-6 frustum that three views see: view 0, view
1 = its geometry `sideways`, view 2 = its geometry `rot20` (both with its camera CAM).  A record carries its point's
pixel in its view (0.3 px of noise; every fifth record of a frame a gross outlier), the point in its view's camera
coordinates in coords3D, and the point's unit descriptor with 1 % of noise of the frame's own, so that the matcher
finds the planted partner and no two scores tie.  Frame 0 holds 25 of its points twice (other noise): both records
find the same partner and pass the thresholds, and only the cross-check tells them apart.  Eight frames in 1024 slots:
    0  view 0, 1024 records          1  view 1, 900 records          2  view 2, 700 records, every coords3D zero
    3  empty                         4  view 1, 5 records, x = NaN   5  view 1, 6 planted records
    6  view 2, 7 planted records     7  view 2, 1024 records, every coords3D the same point; its counter says 3000
The 13 points of frames 5 and 6 carry no pixel noise in any frame: six noisy pixels make a poor minimal pose.
The restatements (tests/test_pose.py's pose_model, tests/test_epipolar.py's pinned Sampson test) recount every integer
from the returned doubles and reproduce [R | t] within test_pose.py's 1e-9; the truth errors stay inside test_pose.py's
ROT_BOUND / DIR_BOUND on the pairs (0, 1) and (0, 2).  No tolerance is new.
"""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from oracle_binding import SIFT_POINT_DTYPE
from test_epipolar import coords, inliers, match_error as sampson_error, refit as epi_refit
from test_planar import candidates, upload
from test_planar_batch import RULES, match_rows
from test_pnp import CAM, GEOMETRIES, H, W, frustum, project
from test_pose import DIR_BOUND, ROT_BOUND, camera, dir_err, pose_model, rot_err
from test_rgbd_batch import MASK64, SENTINEL, tie_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("cusift_register_epipolar_batch", "cusift_register_pose_batch", "cusift_register_pnp_batch")
MAX_PTS, N_FRAMES, LOOPS = 1024, 8, 1008  # 15.75 blocks of 64 loops: the last one is ragged
N_POINTS = 1024
THRESH, REFINE_THRESH, REFINE_LOOPS = 1.0, 1.0, 5
SEEDS = (1, 0xC0FFEE, MASK64 - 1)  # the last one wraps in seed + p
# repeats, both directions, a self pair, a full frame whose counter says 3000; then every degenerate kind: frame a
# empty, frame b empty, fewer records than the model fits (5, 6 and 7 < 8), every match rejected (a NaN partner)
PAIRS = np.array([(0, 1), (1, 0), (0, 2), (0, 1), (2, 0), (1, 1), (1, 2), (7, 0), (3, 1), (1, 3), (4, 0), (0, 4), (5, 0),
                  (6, 0)], np.int32)
DEGENERATE_AT = (8, 9, 10, 11, 12, 13)
PLANTED_PAIRS = {0: (0, 1), 2: (0, 2)}  # position in PAIRS: the views of tests/test_pnp.py's `sideways` and `rot20`
VIEW_OF = {0: 0, 1: 1, 2: 2, 4: 1, 5: 1, 6: 2, 7: 2}


# ------------------------------------------------------------------------------------------------------------------
# the frames
# ------------------------------------------------------------------------------------------------------------------
def view_pose(v):
    """(R, t) with X_v = R X_0 + t."""
    if v == 0:
        return np.eye(3), np.zeros(3)
    R, centre = GEOMETRIES["sideways" if v == 1 else "rot20"][:2]
    return R, -R @ np.array(centre)


def unit_rows(d):
    return (d / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)


class Frames:
    def __init__(self, n_points=N_POINTS, max_pts=MAX_PTS, counts=(1024, 900, 700, 0, 5, 6, 7, 1024), seed=31,
                 outliers=5):
        rng = np.random.default_rng(seed)
        X = np.zeros((0, 3))
        while len(X) < n_points:
            Y = frustum(rng, 4 * n_points, (2.0, 6.0))
            ok = np.ones(len(Y), bool)
            for v in (1, 2):
                R, t = view_pose(v)
                Z = Y @ R.T + t
                b = project(Z, CAM)
                ok &= (Z[:, 2] > 0.1) & ((b >= 0) & (b < [W, H])).all(axis=1)
            X = np.r_[X, Y[ok]]
        self.world = X[:n_points]
        self.desc = unit_rows(np.abs(rng.normal(size=(n_points, 128))).astype(np.float32))
        self.max_pts = max_pts
        self.points = np.zeros((len(counts), max_pts), SIFT_POINT_DTYPE)
        self.ids = []
        self.planted = []
        # the points of the frames of 6 and of 7 records: planted and without pixel noise in every frame, once in frame 0 --
        # a minimal sample of noisy pixels is a poor pose, and these frames are to be fitted
        self.quiet = rng.permutation(n_points)[:13] if len(counts) == N_FRAMES else np.zeros(0, int)
        for k, n in enumerate(counts):
            ids = rng.permutation(n_points)[:n]
            if k == 0:  # 25 points twice, with noise of their own: both records match one partner, one of them is mutual
                others = ids[~np.isin(ids, self.quiet)]
                ids = np.r_[others[:len(others) - 25], self.quiet, others[:25]]
            if len(self.quiet) and n in (6, 7):
                ids = self.quiet[:6] if n == 6 else self.quiet[6:]
            rec, planted = self.records(rng, VIEW_OF.get(k, 0), ids, 0 if n < 8 else outliers)
            if k == 0:  # the second copy's descriptor lies five times as far from the point's: no score ties with the first's
                rec["data"][-25:] = unit_rows(self.desc[ids[-25:]] +
                                              rng.normal(0, 0.05 / np.sqrt(128), (25, 128)).astype(np.float32))
            self.points[k, :n] = rec
            self.ids.append(ids)
            self.planted.append(planted)
            # slots past the count: live-looking copies with valid pixels, so that a stage that ignores a count shows
            tail, _ = self.records(rng, 0, rng.permutation(n_points)[:max_pts - n], 0)
            tail["coords2D"] = 17.0
            self.points[k, n:] = tail
        if len(counts) == N_FRAMES:
            self.points["coords3D"][2] = 0.0                 # PnP: all depths zero
            self.points["coords2D"][4, :, 0] = np.nan        # every match into it, and out of it, is rejected
            self.points["coords3D"][7] = (0.1, -0.2, 3.0)    # PnP: no solvable hypothesis, a winner without support
        # the match fields carry values no stage produces
        self.points["score"], self.points["ambiguity"], self.points["match"] = 0.25, 0.5, -5
        self.points["match_xpos"], self.points["match_ypos"], self.points["match_error"] = -3.0, -4.0, 7.0
        self.n = np.array(counts)
        self.counters = self.n.astype(np.uint32)
        if len(counts) == N_FRAMES:
            self.counters[7] = 3000
        self.points.setflags(write=False)

    def records(self, rng, view, ids, outliers):
        R, t = view_pose(view)
        Xv = self.world[ids] @ R.T + t
        quiet = np.isin(ids, self.quiet)
        px = project(Xv, CAM) + np.where(quiet[:, None], 0.0, rng.normal(0, 0.3, size=(len(ids), 2)))
        planted = np.ones(len(ids), bool)
        if outliers:
            planted[::outliers] = False
            planted[quiet] = True
            px[~planted] = rng.uniform([0, 0], [W, H], size=((~planted).sum(), 2))
        rec = np.zeros(len(ids), SIFT_POINT_DTYPE)
        rec["coords2D"], rec["coords3D"] = px.astype(np.float32), Xv.astype(np.float32)
        rec["data"] = unit_rows(self.desc[ids] + rng.normal(0, 0.01 / np.sqrt(128), (len(ids), 128)).astype(np.float32))
        rec["scale"] = 2.0
        return rec, planted

    def upload(self, ctx, counters="own"):
        cnt = None if counters is None else upload(ctx, self.counters if isinstance(counters, str) else counters)
        return upload(ctx, self.points), cnt

    def pose_of(self, a, b):
        """The planted (R, t) of pair (a, b) in the calls' direction: X_a = R X_b + t."""
        Ra, ta = view_pose(VIEW_OF[a])
        Rb, tb = view_pose(VIEW_OF[b])
        R = Ra @ Rb.T
        return R, ta - R @ tb


@functools.lru_cache(maxsize=None)
def the_frames():
    return Frames()


@pytest.fixture(scope="module")
def frames():
    return the_frames()


def scatter(fb, rows_p, a, b, counts=None, mutual=None, rule=0):
    """The staged route's records of pair (a, b): its match rows in a copy of frame a's records (the scatter of
    tests/test_planar_batch.py's `staged`).  mutual (bool [na]): a record that is not gets a score no rule accepts."""
    counts = fb.n if counts is None else counts
    na, nb = int(counts[a]), int(counts[b])
    copy = fb.points[a, :max(na, 1)].copy()
    if na > 0 and nb > 0:  # a pair whose frame b is empty has no row
        row = rows_p[:na]
        copy["score"][:na], copy["ambiguity"][:na], copy["match"][:na] = row["score"], row["ambiguity"], row["match"]
        partner = np.where((row["match"] >= 0) & (row["match"] < nb), row["match"], 0)
        copy["match_xpos"][:na] = fb.points[b, partner]["coords2D"][:, 0]
        copy["match_ypos"][:na] = fb.points[b, partner]["coords2D"][:, 1]
        if mutual is not None:
            copy["score"][:na][~mutual] = -2.0 if rule == 0 else 1e30
    return copy, na, nb


def batch_args(distance, loops=LOOPS, refine_loops=REFINE_LOOPS, **kw):
    args = dict(distance=distance, loops=loops, thresh=THRESH, refine_loops=refine_loops, refine_thresh=REFINE_THRESH,
                want_inliers=True, want_errors=True)
    args.update(RULES[distance])
    args.update(kw)
    return args


def pose_batch(ctx, fb, seed, distance=1, pairs=PAIRS, counters="own", **kw):
    """register_pose_batch on a fresh upload; returns (PoseBatchResult, the records afterwards)."""
    pts, cnt = fb.upload(ctx, counters)
    n_frames, max_pts = fb.points.shape
    res = ctx.register_pose_batch(pts.ptr, cnt.ptr if cnt is not None else None, n_frames, max_pts, pairs, camera(CAM),
                                  None, seed=seed, want_points=True, **batch_args(distance, **kw))
    after = pts.to_numpy(SIFT_POINT_DTYPE, (n_frames, max_pts))
    pts.free()
    if cnt is not None:
        cnt.free()
    return res, after


def epi_batch(ctx, fb, seed, distance=1, pairs=PAIRS, **kw):
    pts, cnt = fb.upload(ctx)
    n_frames, max_pts = fb.points.shape
    res = ctx.register_epipolar_batch(pts.ptr, cnt.ptr, n_frames, max_pts, pairs, seed=seed, **batch_args(distance, **kw))
    after = pts.to_numpy(SIFT_POINT_DTYPE, (n_frames, max_pts))
    pts.free()
    cnt.free()
    return res, after


def staged(ctx, copy, na, nb, seed, distance, loops=LOOPS, refine_loops=REFINE_LOOPS):
    """cusift_estimate_fundamental, then cusift_estimate_pose on its F at refine_thresh, over one upload of `copy`.
    Returns (EpipolarResult, PoseResult, the records afterwards)."""
    buf = upload(ctx, copy)
    epi = ctx.estimate_fundamental(buf.ptr, na, nb, loops=loops, thresh=THRESH, refine_loops=refine_loops,
                                   refine_thresh=REFINE_THRESH, seed=seed & MASK64, **RULES[distance])
    pose = ctx.estimate_pose(buf.ptr, na, epi.fundamental, camera(CAM), None, nb, thresh=REFINE_THRESH, **RULES[distance])
    after = buf.to_numpy(SIFT_POINT_DTYPE, (max(na, 1),))[:na]
    buf.free()
    return epi, pose, after


def same_epipolar(res, p, one, after, na, what):
    """Pair p of an EpipolarBatchResult / PoseBatchResult against an EpipolarResult and the records its call left."""
    assert res.fundamental[p].tobytes() == one.fundamental.tobytes(), (what, p)
    assert res.ransac[p].tobytes() == one.ransac.tobytes(), (what, p)
    got = (res.num_candidates[p], res.num_matches[p], res.num_fit[p], res.best_loop[p])
    assert got == (one.num_candidates, one.num_matches, one.num_fit, one.best_loop), (what, p, got)
    assert res.counts[p] == na and len(res.inliers[p]) == na and len(res.match_error[p]) == na, (what, p)
    assert np.array_equal(res.inliers[p], one.inliers[:na]), (what, p)
    if one.num_candidates >= 8:
        assert res.match_error[p].tobytes() == after["match_error"][:na].tobytes(), (what, p)
    else:  # no fit: the pair routes leave match_error alone and the batch writes none
        assert np.isnan(res.match_error[p]).all() and (after["match_error"][:na] == 7.0).all(), (what, p)


def same_pose(res, p, pose, after, na, what):
    """The pose outputs of pair p against a PoseResult (or RegisterPoseResult) and the records its call left."""
    assert res.rt[p].tobytes() == pose.rt.tobytes(), (what, p)
    assert res.num_front[p] == pose.num_front and np.array_equal(res.votes[p], pose.votes), (what, p)
    assert res.sigma[p].tobytes() == pose.sigma.tobytes(), (what, p)
    assert res.points3d[p].shape == (na, 3), (what, p)
    assert res.points3d[p].tobytes() == np.ascontiguousarray(after["coords3D"][:na]).tobytes(), (what, p)


def same_results(x, y, pairs=None):
    """Every field of two batch results, arrays and lists alike, for the pairs named (None: all)."""
    pairs = range(len(x.counts)) if pairs is None else pairs
    return all(np.asarray(u[p]).tobytes() == np.asarray(v[p]).tobytes() for p in pairs for u, v in zip(x, y))


def fill_extractor(ex, fb, k_frames=3):
    """Frames 0 .. k_frames - 1 of `fb` into the extractor's own slot, as tests/test_pose.py's last test fills it."""
    import torch

    for k in range(k_frames):
        raw = torch.from_numpy(fb.points[k].view(np.uint8).reshape(fb.max_pts, -1).copy()).to(ex.device)
        ex.points[k] = raw
    ex.counts[:] = torch.from_numpy(fb.counters[:k_frames].astype(np.int32)).to(ex.device)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------
# without a GPU
# ------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_recipes_agree_on_the_three_pair_list_calls():
    from cusift_amd import batch, capi

    extras = open(os.path.join(ROOT, "include", "cusift_amd_extras.h")).read()
    front = open(os.path.join(ROOT, "include", "cusift_amd.h")).read()
    handle = C.CDLL(capi.LIB_PATH)
    for name, nargs, seed_at, cams in zip(NAMES, (24, 31, 25), (15, 15, 16), (0, 2, 1)):
        assert "int %s(cusift_ctx *ctx, const cusift_point *d_points" % name in extras, name
        assert "int %s(" % name not in front, name
        assert hasattr(handle, name), name
        res, args = capi.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs, (name, len(args))
        assert args[seed_at] is C.c_uint64 and args.count(C.c_uint64) == 1, name  # the seed, where the header has it
        assert args.count(C.POINTER(capi.Camera)) == cams, name
    for m in ("register_epipolar_batch", "register_pose_batch", "register_pnp_batch"):
        assert callable(getattr(capi.Context, m)), m
    for m in ("register_epipolar_sequence", "register_pose_sequence", "register_pnp_sequence"):
        assert callable(getattr(batch.BatchExtractor, m)), m
    assert capi.EpipolarBatchResult._fields[:6] == capi.EpipolarResult._fields[:6]
    assert capi.EpipolarBatchResult._fields[6:] == capi.PlanarBatchResult._fields[6:]
    assert capi.PoseBatchResult._fields == capi.EpipolarBatchResult._fields + capi.PoseResult._fields + ("points3d",)
    assert capi.PnPBatchResult._fields[:6] == capi.PnPResult._fields[:6]
    assert capi.PnPBatchResult._fields[6:] == capi.PlanarBatchResult._fields[6:]
    for head, wrapper in (("epipolar.h", "RegisterEpipolarSequence(std::vector<SiftData *> &frames"),
                          ("pose.h", "RegisterPoseSequence(std::vector<SiftData *> &frames"),
                          ("pnp.h", "RegisterPnPSequence(std::vector<SiftData *> &frames")):
        text = open(os.path.join(ROOT, "include", head)).read()
        assert wrapper in text and "#include <hip" not in text, head
    make = open(os.path.join(ROOT, "Makefile")).read()
    assert "cpp_sequence_pose" in make
    assert "tests/cpp_sequence_pose/sequence_pose_dropin.cpp" in open(os.path.join(ROOT, "CMakeLists.txt")).read()
    assert "tests/cpp_sequence_pose/sequence_pose_dropin" in open(os.path.join(ROOT, ".gitignore")).read()
    host = open(os.path.join(ROOT, "cusift_amd", "csrc", "sift_register.hip")).read()
    assert "has no batch form" not in host


def test_new_and_changed_kernels_compile_for_gfx950_without_scratch_or_spills():
    """pnp_solve / pnp_score / pnp_select with the pair dimension, the PnP marking of a pair list, pose_write with its
    output array and pose_vote: no scratch, no spills; the solve kernel's LDS stays at 70,656 bytes."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs

    found = set()
    for src, wanted in (("sift_pnp.hip", ("pnp_solve_kernel", "pnp_score_kernel", "pnp_select_kernel")),
                        ("sift_sequence.hip", ("sequence_pnp_mark_kernel", "sequence_mark_kernel")),
                        ("sift_pose.hip", ("pose_write_kernel", "pose_vote_kernel")),
                        ("sift_planar.hip", ("planar_compact_kernel",))):
        asm = kernel_regs.assembly(src)
        assert "gfx950" in asm
        for k in kernel_regs.kernels(asm):
            hit = [w for w in wanted if w in k["name"]]
            if not hit:
                continue
            found.update(hit)
            print("%s: %d VGPRs, %d AGPRs, %d bytes of scratch, %d bytes of LDS" %
                  (k["name"][:48], k["vgpr_count"], k["agpr_count"], k["private_segment_fixed_size"],
                   k["group_segment_fixed_size"]))
            assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
            if "pnp_solve_kernel" in k["name"]:
                assert k["group_segment_fixed_size"] == 70656, k["group_segment_fixed_size"]
    assert len(found) == 8, sorted(found)


def test_frames_hold_what_the_tests_rely_on(frames):
    assert frames.n.tolist() == [1024, 900, 700, 0, 5, 6, 7, 1024] and frames.counters[7] == 3000
    assert frames.planted[5].all() and frames.planted[6].all() and len(frames.planted[5]) == 6
    assert np.isnan(frames.points["coords2D"][4, :, 0]).all() and not frames.points["coords3D"][2].any()
    assert len(np.unique(frames.points["coords3D"][7], axis=0)) == 1
    # the descriptors make the match: a record's own point is by far its nearest in any other frame
    d0, d1 = frames.points["data"][0, :1024].astype(np.float64), frames.points["data"][1, :900].astype(np.float64)
    best = (d0 @ d1.T).argmax(axis=1)
    there = np.isin(frames.ids[0], frames.ids[1])
    assert np.array_equal(frames.ids[1][best[there]], frames.ids[0][there])
    # the planted poses are those of tests/test_pnp.py's geometries
    R, t = frames.pose_of(0, 1)
    assert np.allclose(R, GEOMETRIES["sideways"][0].T) and np.allclose(t, GEOMETRIES["sideways"][1])


# ------------------------------------------------------------------------------------------------------------------
# on the GPU
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
@pytest.mark.parametrize("seed", SEEDS)
def test_batches_equal_the_staged_route_bit_for_bit(ctx, frames, seed, distance):
    res, recs = pose_batch(ctx, frames, seed, distance)
    assert recs.tobytes() == frames.points.tobytes()  # the records: untouched
    epi, recs = epi_batch(ctx, frames, seed, distance)
    assert recs.tobytes() == frames.points.tobytes()
    assert same_results(epi, type(epi)(*res[:9]))  # the pose batch's F part is the F batch's
    rows = match_rows(ctx, frames, PAIRS, distance)
    for p, (a, b) in enumerate(PAIRS):
        copy, na, nb = scatter(frames, rows[p], a, b)
        one, pose, after = staged(ctx, copy, na, nb, seed + p, distance)
        print("distance %d seed %#x pair %d (%d, %d): %d candidates, %d inliers, %d fit, loop %d, %d in front" %
              (distance, seed, p, a, b, one.num_candidates, one.num_matches, one.num_fit, one.best_loop, pose.num_front))
        same_epipolar(res, p, one, after, na, "staged")
        same_pose(res, p, pose, after, na, "staged")
        if p not in DEGENERATE_AT:
            assert one.num_candidates >= 8 and one.num_matches >= 8, p
    for p in PLANTED_PAIRS:
        assert res.num_fit[p] >= 0.6 * 0.9 * min(frames.n[PAIRS[p][0]], frames.n[PAIRS[p][1]]), p
    # the same pair twice in one list draws from its own seed each
    assert res.best_loop[0] != res.best_loop[3] or res.ransac[0].tobytes() != res.ransac[3].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
def test_batches_equal_the_fused_pair_calls_bit_for_bit(ctx, frames, distance):
    """First the condition -- the batch rows ARE the pair matcher's fields, for every pair of the list, with no tied row
    among them -- then the equality of every output with cusift_register_pose (whose F part is cusift_register_epipolar's)."""
    seed = 77
    rows = match_rows(ctx, frames, PAIRS, distance)
    res, _ = pose_batch(ctx, frames, seed, distance)
    kw = dict(distance=distance, loops=LOOPS, thresh=THRESH, refine_loops=REFINE_LOOPS, refine_thresh=REFINE_THRESH)
    kw.update(RULES[distance])
    for p, (a, b) in enumerate(PAIRS):
        na, nb = int(frames.n[a]), int(frames.n[b])
        f1, f2 = frames.points[a, :max(na, 1)].copy(), frames.points[b, :max(nb, 1)].copy()
        if na > 0 and nb > 0:
            b1, b2 = upload(ctx, f1), upload(ctx, f2)
            ctx.match(b1.ptr, na, b2.ptr, nb, distance)
            ctx.synchronize()
            m = b1.to_numpy(SIFT_POINT_DTYPE, (na,))
            tie = tie_rows(m["score"], m["ambiguity"], distance) & (m["ambiguity"] != 0)
            assert not tie.any(), (p, np.nonzero(tie)[0][:10])
            for f in ("score", "ambiguity", "match"):
                assert rows[p, :na][f].tobytes() == m[f].tobytes(), (p, f)
        d1, d2 = upload(ctx, f1), upload(ctx, f2)
        one = ctx.register_pose(d1.ptr, na, d2.ptr, nb, camera(CAM), None, seed=(seed + p) & MASK64, **kw)
        after = d1.to_numpy(SIFT_POINT_DTYPE, (max(na, 1),))[:na]
        same_epipolar(res, p, one, after, na, "register_pose")
        same_pose(res, p, one, after, na, "register_pose")
        e1, e2 = upload(ctx, f1), upload(ctx, f2)
        two = ctx.register_epipolar(e1.ptr, na, e2.ptr, nb, seed=(seed + p) & MASK64, **kw)
        same_epipolar(res, p, two, e1.to_numpy(SIFT_POINT_DTYPE, (max(na, 1),))[:na], na, "register_epipolar")


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
def test_cross_check_on_equals_the_staged_route_over_mutual_rows(frames, distance):
    """A context of this test's own with the cross-check on: the records stay untouched, every pair equals the staged
    route over the rows of cusift_match_batch_mutual with the records that are not mutual taken out by their score, and
    the fused pair call with the setting on."""
    from cusift_amd import capi

    if capi.device_count() < 1:
        pytest.fail("gpu test selected but no HIP device is visible")
    seed = 0xC0FFEE
    rule = RULES[distance]["rule"]
    with capi.Context(0) as own:
        pts, cnt = frames.upload(own)
        rows_d = upload(own, np.full((len(PAIRS), MAX_PTS, 16), SENTINEL, np.uint8))
        back_d = upload(own, np.full((len(PAIRS), MAX_PTS, 16), SENTINEL, np.uint8))
        own.match_batch_mutual(pts.ptr, cnt.ptr, N_FRAMES, MAX_PTS, PAIRS, rows_d.ptr, back_d.ptr, distance)
        own.synchronize()
        rows, back = rows_d.to_numpy(capi.MatchRow, (len(PAIRS), MAX_PTS)), back_d.to_numpy(capi.MatchRow, (len(PAIRS), MAX_PTS))
        own.set_cross_check(True)
        res, recs = pose_batch(own, frames, seed, distance)
        assert recs.tobytes() == frames.points.tobytes()
        own.set_cross_check(False)
        dropped = 0
        for p, (a, b) in enumerate(PAIRS):
            na, nb = int(frames.n[a]), int(frames.n[b])
            m = rows[p, :na]["match"]
            ok = (m >= 0) & (m < nb) if nb > 0 else np.zeros(na, bool)
            mutual = ok & (back[p, np.where(ok, m, 0)]["match"] == np.arange(na)) if nb > 0 else ok
            copy, _, _ = scatter(frames, rows[p], a, b, mutual=mutual, rule=rule)
            by_rule = candidates(scatter(frames, rows[p], a, b)[0][:na], rule, RULES[distance]["lo"], RULES[distance]["hi"], nb)
            dropped += int((~mutual[by_rule]).sum()) if na >= 8 else 0
            one, pose, after = staged(own, copy, na, nb, seed + p, distance)
            same_epipolar(res, p, one, after, na, "mutual rows")
            same_pose(res, p, pose, after, na, "mutual rows")
            assert not res.inliers[p][~mutual].any(), p
        print("distance %d: the cross-check dropped %d records that the thresholds let through" % (distance, dropped))
        assert dropped >= 1  # the setting bites
        own.set_cross_check(True)
        kw = dict(distance=distance, loops=LOOPS, thresh=THRESH, refine_loops=REFINE_LOOPS, refine_thresh=REFINE_THRESH)
        kw.update(RULES[distance])
        for p, (a, b) in enumerate(PAIRS):  # the self pair against a copy: the pair call refuses overlapping ranges
            na, nb = int(frames.n[a]), int(frames.n[b])
            d1, d2 = upload(own, frames.points[a, :max(na, 1)].copy()), upload(own, frames.points[b, :max(nb, 1)].copy())
            one = own.register_pose(d1.ptr, na, d2.ptr, nb, camera(CAM), None, seed=(seed + p) & MASK64, **kw)
            after = d1.to_numpy(SIFT_POINT_DTYPE, (max(na, 1),))[:na]
            same_epipolar(res, p, one, after, na, "register_pose, cross-check on")
            same_pose(res, p, one, after, na, "register_pose, cross-check on")


@pytest.mark.gpu
def test_degenerate_pairs_answer_as_documented_and_disturb_no_other_pair(ctx, frames):
    seed = 9
    res, recs = pose_batch(ctx, frames, seed)
    assert recs.tobytes() == frames.points.tobytes()
    ident = np.hstack([np.eye(3), np.zeros((3, 1))])
    for p in DEGENERATE_AT:
        assert not res.fundamental[p].any() and not res.ransac[p].any(), p  # nine zeros
        assert np.array_equal(res.rt[p], ident) and res.num_front[p] == 0 and not res.votes[p].any(), p
        assert res.num_matches[p] == 0 and res.num_fit[p] == 0 and res.best_loop[p] == 0 and not res.inliers[p].any(), p
        assert not res.points3d[p].any() and np.isnan(res.match_error[p]).all(), p
    print("candidates of the list:", res.num_candidates.tolist(), "counts:", res.counts.tolist())
    assert res.counts.tolist() == [int(frames.n[a]) for a, _ in PAIRS]  # frame 7's counter of 3000 means 1024
    assert [int(res.num_candidates[p]) for p in DEGENERATE_AT] == [0] * 6  # 5, 6 and 7 records are fewer than eight
    # every other pair is what a list with ordinary pairs in the degenerate places gives it
    clean = PAIRS.copy()
    clean[list(DEGENERATE_AT)] = (0, 1)
    ref, _ = pose_batch(ctx, frames, seed, pairs=clean)
    others = [p for p in range(len(PAIRS)) if p not in DEGENERATE_AT]
    assert same_results(res, ref, others) and all(ref.num_matches[p] >= 8 for p in DEGENERATE_AT)
    # a counter past max_pts means max_pts; no counters: every frame is full
    clamped = frames.counters.copy()
    clamped[7] = MAX_PTS
    assert same_results(res, pose_batch(ctx, frames, seed, counters=clamped)[0])
    full = np.full(N_FRAMES, MAX_PTS, np.uint32)
    some = PAIRS[[0, 4, 7, 5]]
    no_counters, recs = pose_batch(ctx, frames, seed, pairs=some, counters=None)
    assert same_results(no_counters, pose_batch(ctx, frames, seed, pairs=some, counters=full)[0])
    assert (no_counters.counts == MAX_PTS).all() and recs.tobytes() == frames.points.tobytes()
    rows = match_rows(ctx, frames, some, 1, counters=None)
    for p, (a, b) in enumerate(some):
        copy, na, nb = scatter(frames, rows[p], a, b, counts=full)
        one, pose, after = staged(ctx, copy, na, nb, seed + p, 1)
        same_epipolar(no_counters, p, one, after, MAX_PTS, "no counters")
        same_pose(no_counters, p, pose, after, MAX_PTS, "no counters")
    # no pairs: nothing to do
    none, recs = pose_batch(ctx, frames, seed, pairs=np.zeros((0, 2), np.int32))
    assert none.fundamental.shape == (0, 9) and none.rt.shape == (0, 3, 4) and recs.tobytes() == frames.points.tobytes()


@pytest.mark.gpu
def test_same_seed_same_bytes_other_seed_other_samples_and_no_refit(ctx, frames):
    a, _ = pose_batch(ctx, frames, 5)
    b, _ = pose_batch(ctx, frames, 5)
    assert same_results(a, b)
    c, _ = pose_batch(ctx, frames, 6)
    assert not np.array_equal(a.best_loop, c.best_loop) or a.ransac.tobytes() != c.ransac.tobytes()
    # pair 0 of seed 8 draws what pair 3 of seed 5 draws: (0, 1) sits at 0 and at 3
    d, _ = pose_batch(ctx, frames, 8)
    assert d.ransac[0].tobytes() == a.ransac[3].tobytes() and d.fundamental[0].tobytes() == a.fundamental[3].tobytes()
    assert d.rt[0].tobytes() == a.rt[3].tobytes()
    # refine_loops = 0: the refined estimate is the winner, and the staged route agrees
    e, _ = pose_batch(ctx, frames, 5, refine_loops=0)
    assert e.fundamental.tobytes() == e.ransac.tobytes() == a.ransac.tobytes()
    assert np.array_equal(e.num_matches, a.num_matches) and np.array_equal(e.num_fit, e.num_matches)
    rows = match_rows(ctx, frames, PAIRS, 1)
    for p, (u, v) in enumerate(PAIRS):
        copy, na, nb = scatter(frames, rows[p], u, v)
        one, pose, after = staged(ctx, copy, na, nb, 5 + p, 1, refine_loops=0)
        same_epipolar(e, p, one, after, na, "no refit")
        same_pose(e, p, pose, after, na, "no refit")


@pytest.mark.gpu
@pytest.mark.parametrize("which", ("epipolar", "pose"))
def test_refusals_leave_everything_untouched(ctx, frames, which):
    from cusift_amd import capi

    pts, cnt = frames.upload(ctx)
    n_pairs = len(PAIRS)
    fund, ran = np.full((n_pairs, 9), 9.0), np.full((n_pairs, 9), 9.0)
    ints = [np.full(n_pairs, -7, np.int32) for _ in range(4)]
    fl = np.full((n_pairs, MAX_PTS), 5, np.int8)
    err = np.full((n_pairs, MAX_PTS), -2.0, np.float32)
    rt, sig = np.full((n_pairs, 12), 9.0), np.full((n_pairs, 3), 9.0)
    front, votes = np.full(n_pairs, -7, np.int32), np.full((n_pairs, 4), -7, np.int32)
    xyz = np.full((n_pairs, MAX_PTS, 3), -2.0, np.float32)
    good = camera(CAM)

    def ptr(a):
        return a.ctypes.data if a is not None else None

    def cam_ptr(c):
        return C.byref(c) if c is not None else None

    def call(recs=pts.ptr, n_images=N_FRAMES, max_pts=MAX_PTS, pairs=PAIRS, n_pairs=n_pairs, dist=1, rule=1, lo=999.0,
             hi=0.8, loops=64, th=1.0, rl=5, rth=1.0, f=fund, r=ran, pc=ints[0], pm=ints[1], pf=ints[2], cam1=good,
             cam2=None, prt=rt, pfr=front):
        pairs = None if pairs is None else np.ascontiguousarray(pairs, np.int32)
        head = (ctx.handle, recs, cnt.ptr, n_images, max_pts, ptr(pairs), n_pairs, dist, rule, lo, hi, loops, th, rl, rth, 1)
        tail = (ptr(f), ptr(r), ptr(pc), ptr(pm), ptr(pf), ptr(ints[3]), ptr(fl), ptr(err))
        if which == "epipolar":
            return capi.lib().cusift_register_epipolar_batch(*(head + tail))
        return capi.lib().cusift_register_pose_batch(*(head + (cam_ptr(cam1), cam_ptr(cam2)) + tail +
                                                       (ptr(prt), ptr(pfr), ptr(votes), ptr(sig), ptr(xyz))))

    def untouched():
        return ((fund == 9.0).all() and (ran == 9.0).all() and all((v == -7).all() for v in ints) and (fl == 5).all() and
                (err == -2.0).all() and (rt == 9.0).all() and (sig == 9.0).all() and (front == -7).all() and
                (votes == -7).all() and (xyz == -2.0).all())

    nan = float("nan")
    low, high = PAIRS.copy(), PAIRS.copy()
    low[2, 1], high[5, 0] = -1, N_FRAMES
    cases = [  # every case of the pair call
        dict(f=None), dict(r=None), dict(pc=None), dict(pm=None), dict(pf=None), dict(loops=0), dict(loops=-3),
        dict(loops=(1 << 24) + 1), dict(th=0.0), dict(th=-1.0), dict(th=nan), dict(rth=0.0), dict(rth=nan), dict(lo=nan),
        dict(hi=nan), dict(rule=2), dict(rule=-1), dict(rl=-1), dict(recs=None), dict(dist=2), dict(dist=-1),
        # the pair list's own
        dict(pairs=low), dict(pairs=high), dict(n_pairs=-1), dict(n_pairs=65536, pairs=np.zeros((65536, 2))),
        dict(n_images=-1), dict(n_images=65536), dict(max_pts=-1), dict(max_pts=(1 << 20) + 1), dict(pairs=None),
        dict(n_images=3)]
    if which == "pose":
        cases += [dict(cam1=None), dict(prt=None), dict(pfr=None), dict(cam1=capi.Camera(0.0, 500.0, 320.0, 240.0, 0.0, 0.0, 7)),
                  dict(cam2=capi.Camera(500.0, nan, 320.0, 240.0, 0.0, 0.0, 7)),
                  dict(cam1=capi.Camera(500.0, 500.0, float("inf"), 240.0, 0.0, 0.0, 7))]
    for kw in cases:
        assert call(**kw) == -1, kw  # CUSIFT_ERR_INVALID
        assert untouched(), kw
    ctx.synchronize()
    assert pts.to_numpy(SIFT_POINT_DTYPE, (N_FRAMES, MAX_PTS)).tobytes() == frames.points.tobytes()
    # n_pairs == 0 is not an error and writes nothing
    assert call(n_pairs=0) == 0 and call(n_pairs=0, pairs=None) == 0 and untouched()
    # max_pts == 0 is answered from the arguments alone: every pair is degenerate
    assert call(max_pts=0, recs=None) == 0
    assert not fund.any() and not ran.any() and all(not v.any() for v in ints) and (fl == 5).all() and (err == -2.0).all()
    if which == "pose":
        assert np.array_equal(rt, np.tile(np.hstack([np.eye(3), np.zeros((3, 1))]).ravel(), (n_pairs, 1)))
        assert not front.any() and not votes.any() and not sig.any() and (xyz == -2.0).all()
    # and the same arguments without a fault run; a block's tail is not written
    assert call(loops=LOOPS) == 0
    for p, (a, b) in enumerate(PAIRS):
        na = int(frames.n[a])
        assert np.isin(fl[p, :na], (0, 1)).all() and (fl[p, na:] == 5).all(), p
        assert fl[p, :na].sum() == ints[1][p], p
        if p in DEGENERATE_AT:
            assert (err[p] == -2.0).all() and ints[1][p] == 0, p
        else:
            assert ints[0][p] >= 8 and ints[1][p] >= 8 and (err[p, :na] != -2.0).all() and (err[p, na:] == -2.0).all(), p
        if which == "pose":
            assert (xyz[p, :na] != -2.0).all() and (xyz[p, na:] == -2.0).all(), p
    assert pts.to_numpy(SIFT_POINT_DTYPE, (N_FRAMES, MAX_PTS)).tobytes() == frames.points.tobytes()


@pytest.mark.gpu
def test_restatement_recounts_every_integer_and_reproduces_the_pose(ctx, frames):
    """For the planted pairs: num_matches and the flags from the returned winner, num_fit and match_error from the returned
    F with the pinned Sampson test of tests/test_epipolar.py; the refit of the winner within its 1e-9; pose_model of
    tests/test_pose.py from the device's own F within test_pose.py's 1e-9, votes, num_front and the zero pattern of the
    points exactly; rotation and translation direction inside test_pose.py's truth bounds."""
    distance, skipped = 0, 0
    rows = match_rows(ctx, frames, PAIRS, distance)
    for seed in SEEDS[:2]:
        res, _ = pose_batch(ctx, frames, seed, distance)
        for p, (a, b) in PLANTED_PAIRS.items():
            copy, na, nb = scatter(frames, rows[p], a, b)
            rule = RULES[distance]
            cand = candidates(copy, rule["rule"], rule["lo"], rule["hi"], nb)
            xy = coords(copy, cand)
            assert res.num_candidates[p] == len(cand)
            win = inliers(res.ransac[p], xy, THRESH)
            flags = np.zeros(na, bool)
            flags[cand] = win
            assert res.num_matches[p] == int(win.sum()) and np.array_equal(res.inliers[p], flags), p
            assert res.num_fit[p] == int(inliers(res.fundamental[p], xy, REFINE_THRESH).sum()), p
            err = sampson_error(res.fundamental[p], coords(copy)).astype(np.float32)
            assert np.array_equal(res.match_error[p], err, equal_nan=True), p
            F, near = epi_refit(res.ransac[p], xy, REFINE_LOOPS, REFINE_THRESH)
            want = pose_model(res.fundamental[p], copy, CAM, CAM, thresh=REFINE_THRESH, n2=nb, **rule)
            d_f = float(np.abs(F - res.fundamental[p]).max())
            d_rt = float(np.abs(res.rt[p] - want.rt).max())
            R, t = frames.pose_of(a, b)
            r, d = rot_err(res.rt[p][:, :3], R), dir_err(res.rt[p][:, 3], t)
            print("seed %#x pair (%d, %d): %d candidates, %d inliers, %d fit, %d in front; F from the refit of the device's "
                  "winner by %.3g, [R | t] from the model by %.3g%s; rotation %.4f, direction %.4f degrees" %
                  (seed, a, b, len(cand), res.num_matches[p], res.num_fit[p], res.num_front[p], d_f, d_rt,
                   " (near: skipped)" if near or want.near else "", r, d))
            assert r <= ROT_BOUND and d <= DIR_BOUND, (r, d)
            assert abs(np.sqrt(res.rt[p][:, 3] @ res.rt[p][:, 3]) - 1.0) <= 1e-12
            if near or want.near:
                skipped += 1
                continue
            assert d_f <= 1e-9 and d_rt <= 1e-9, (d_f, d_rt)
            assert sorted(res.votes[p].tolist()) == sorted(want.votes.tolist()) and res.num_front[p] == want.num_front
            assert np.array_equal(res.points3d[p].any(axis=1), want.coords3D.any(axis=1))
    assert skipped <= 1


@pytest.mark.gpu
def test_sizes_where_the_loops_turn_a_second_time(ctx):
    """max_pts 4096, 3 pairs, 4096 loops: on 256 CUs score_splits gives 11 candidate splits of 6 tiles each (192
    workgroups before splitting), and the marking has 16 blocks per pair.  Frames of 4096 and 3000 records, 60 %
    planted."""
    big = Frames(n_points=4096, max_pts=4096, counts=(4096, 3000, 4096), seed=5, outliers=5)
    pairs = np.array([(0, 1), (1, 0), (2, 1)], np.int32)
    seed = 3
    res, recs = pose_batch(ctx, big, seed, 1, pairs=pairs, loops=4096)
    assert recs.tobytes() == big.points.tobytes()
    rows = match_rows(ctx, big, pairs, 1)
    for p, (a, b) in enumerate(pairs):
        copy, na, nb = scatter(big, rows[p], a, b)
        one, pose, after = staged(ctx, copy, na, nb, seed + p, 1, loops=4096)
        print("pair (%d, %d): %d candidates, %d inliers, %d fit" % (a, b, one.num_candidates, one.num_matches, one.num_fit))
        assert one.num_candidates > 6 * 64 * 6  # more than six splits of six tiles hold candidates
        same_epipolar(res, p, one, after, na, "large")
        same_pose(res, p, pose, after, na, "large")


@pytest.mark.gpu
def test_extractor_sequences_equal_the_context_calls(ctx):
    """BatchExtractor.register_epipolar_sequence / register_pose_sequence over the extractor's own buffers against the
    Context calls on the same pointers, as tests/test_pose.py's last test does for the pair call."""
    from cusift_amd.batch import BatchExtractor

    fb = the_frames()
    ex = BatchExtractor(3, W, H, num_octaves=3, max_pts=MAX_PTS)
    try:
        fill_extractor(ex, fb)
        before = [r.copy() for r in ex.to_host()]
        assert [len(r) for r in before] == fb.n[:3].tolist()
        cam = camera(CAM)
        kw = dict(distance=1, rule=1, lo=999.0, hi=0.8, loops=512, seed=21)
        points, counts = ex.slots[0]
        for pairs in (None, [(2, 0), (0, 2), (1, 1)]):
            want_pairs = [(0, 1), (1, 2)] if pairs is None else pairs
            seq = ex.register_epipolar_sequence(pairs=pairs, want_errors=True, **kw)
            ref = ex.ctx.register_epipolar_batch(points.data_ptr(), counts.data_ptr(), 3, ex.max_pts, want_pairs,
                                                 want_errors=True, **kw)
            assert same_results(seq, ref) and seq.counts.tolist() == [len(before[a]) for a, _ in want_pairs]
            seq = ex.register_pose_sequence(cam, pairs=pairs, want_errors=True, want_points=True, **kw)
            ref = ex.ctx.register_pose_batch(points.data_ptr(), counts.data_ptr(), 3, ex.max_pts, want_pairs, cam, None,
                                             want_errors=True, want_points=True, **kw)
            assert same_results(seq, ref) and seq.num_matches.min() >= 8
            # the shared context on an upload of the same frames gives the same bytes
            pts, cnt = upload(ctx, fb.points[:3].copy()), upload(ctx, fb.counters[:3].copy())
            own = ctx.register_pose_batch(pts.ptr, cnt.ptr, 3, MAX_PTS, want_pairs, cam, None, want_errors=True,
                                          want_points=True, **kw)
            assert same_results(seq, own)
            pts.free()
            cnt.free()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, ex.to_host()))  # the records: untouched
    finally:
        ex.close()
