"""The pair-list form of the absolute pose: cusift_register_pnp_batch (cusift_amd/csrc/sift_register.hip:
ransac_batch_run; sift_sequence.hip: sequence_pnp_mark_kernel; sift_pnp.hip with one grid layer per pair),
capi.Context.register_pnp_batch and BatchExtractor.register_pnp_sequence.  The frames are those of
tests/test_epipolar_batch.py, which describes them.

The defining equality is bit for bit: every output of pair p = (a, b) is what cusift_estimate_pnp gives on a copy of frame
a's records into which pair p's row of cusift_match_batch was scattered, with seed + p; where the rows equal
cusift_match's fields (asserted for every pair), also what cusift_register_pnp gives on copies of the two frames.
The list holds every degenerate kind: frame a or b empty, 5 records (fewer than six), every match rejected, every depth
zero (frame 2), a winner without support (frame 7: every candidate the same point) -- and the frames of 6 and of 7
records, which the pair call fits and which a literal 8 in the compaction would zero.
The restatement is tests/test_pnp.py's: every integer and match_error recounted exactly from the returned doubles with
its pinned test, [R | t] from its refit of the device's winner within its 1e-9, the truth errors of the pairs (0, 1)
(`sideways`) and (0, 2) (`rot20`) inside its ROT_BOUND / TRANS_BOUND.  No tolerance is new.
"""
import ctypes as C

import numpy as np
import pytest

from oracle_binding import SIFT_POINT_DTYPE
from test_epipolar_batch import (MAX_PTS, N_FRAMES, LOOPS, SEEDS, Frames, fill_extractor, same_results, scatter,
                                 the_frames)
from test_planar import upload
from test_planar_batch import RULES, match_rows, optional_outputs_three_ways
from test_pnp import (CAM, H, IDENT, REFINE_LOOPS, REFINE_THRESH, ROT_BOUND, THRESH, TRANS_BOUND, W, cam_of, camera,
                      coords5, match_error, pnp_candidates, pnp_inliers, refit, rot_err)
from test_rgbd_batch import MASK64, SENTINEL, tie_rows

# repeats, both directions, a self pair; then frame a empty, frame b empty, 5 records, every match rejected; the frames
# of 6 and of 7 records (fitted); every depth zero; a winner without support
PAIRS = np.array([(0, 1), (1, 0), (0, 2), (0, 1), (1, 1), (1, 2), (3, 1), (1, 3), (4, 0), (0, 4), (5, 0), (6, 0), (2, 0),
                  (7, 0)], np.int32)
DEGENERATE_AT = (6, 7, 8, 9, 12, 13)
SMALL_AT = {10: 6, 11: 7}
PLANTED_PAIRS = {0: (0, 1), 2: (0, 2)}


@pytest.fixture(scope="module")
def frames():
    return the_frames()


def batch_args(distance, loops=LOOPS, refine_loops=REFINE_LOOPS, **kw):
    args = dict(distance=distance, loops=loops, thresh=THRESH, refine_loops=refine_loops, refine_thresh=REFINE_THRESH,
                want_inliers=True, want_errors=True)
    args.update(RULES[distance])
    args.update(kw)
    return args


def pnp_batch(ctx, fb, seed, distance=1, pairs=PAIRS, counters="own", **kw):
    """register_pnp_batch on a fresh upload; returns (PnPBatchResult, the records afterwards)."""
    pts, cnt = fb.upload(ctx, counters)
    n_frames, max_pts = fb.points.shape
    res = ctx.register_pnp_batch(pts.ptr, cnt.ptr if cnt is not None else None, n_frames, max_pts, pairs, camera(CAM),
                                 seed=seed, **batch_args(distance, **kw))
    after = pts.to_numpy(SIFT_POINT_DTYPE, (n_frames, max_pts))
    pts.free()
    if cnt is not None:
        cnt.free()
    return res, after


def staged(ctx, copy, na, nb, seed, distance, loops=LOOPS, refine_loops=REFINE_LOOPS):
    """cusift_estimate_pnp over an upload of `copy`; returns (PnPResult, the records afterwards)."""
    buf = upload(ctx, copy)
    one = ctx.estimate_pnp(buf.ptr, na, camera(CAM), nb, loops=loops, thresh=THRESH, refine_loops=refine_loops,
                           refine_thresh=REFINE_THRESH, seed=seed & MASK64, **RULES[distance])
    after = buf.to_numpy(SIFT_POINT_DTYPE, (max(na, 1),))[:na]
    buf.free()
    return one, after


def same_pnp(res, p, one, after, na, what):
    """Pair p of a PnPBatchResult against a PnPResult of the pair routes and the records they left."""
    assert res.rt[p].tobytes() == one.rt.tobytes(), (what, p)
    assert res.ransac[p].tobytes() == one.ransac.tobytes(), (what, p)
    got = (res.num_candidates[p], res.num_matches[p], res.num_fit[p], res.best_loop[p])
    assert got == (one.num_candidates, one.num_matches, one.num_fit, one.best_loop), (what, p, got)
    assert res.counts[p] == na and len(res.inliers[p]) == na and len(res.match_error[p]) == na, (what, p)
    assert np.array_equal(res.inliers[p], one.inliers[:na]), (what, p)
    if one.num_matches >= 1:
        assert res.match_error[p].tobytes() == after["match_error"][:na].tobytes(), (what, p)
    else:  # no fit: the pair routes leave match_error alone and the batch writes none
        assert np.isnan(res.match_error[p]).all() and (after["match_error"][:na] == 7.0).all(), (what, p)


# ------------------------------------------------------------------------------------------------------------------
# on the GPU
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
@pytest.mark.parametrize("seed", SEEDS)
def test_batch_equals_the_staged_route_bit_for_bit(ctx, frames, seed, distance):
    res, recs = pnp_batch(ctx, frames, seed, distance)
    assert recs.tobytes() == frames.points.tobytes()  # the records: untouched, coords3D included
    rows = match_rows(ctx, frames, PAIRS, distance)
    for p, (a, b) in enumerate(PAIRS):
        copy, na, nb = scatter(frames, rows[p], a, b)
        one, after = staged(ctx, copy, na, nb, seed + p, distance)
        print("distance %d seed %#x pair %d (%d, %d): %d candidates, %d inliers, %d fit, loop %d" %
              (distance, seed, p, a, b, one.num_candidates, one.num_matches, one.num_fit, one.best_loop))
        same_pnp(res, p, one, after, na, "staged")
        if p not in DEGENERATE_AT:  # six records are one sample in every order: its own points count, how many is the data's
            assert one.num_candidates >= 6 and one.num_matches >= (1 if p in SMALL_AT else 6), p
    for p in PLANTED_PAIRS:
        assert res.num_fit[p] >= 0.6 * 0.9 * 0.9 * min(frames.n[PAIRS[p][0]], frames.n[PAIRS[p][1]]), p
    assert res.best_loop[0] != res.best_loop[3] or res.ransac[0].tobytes() != res.ransac[3].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
def test_batch_equals_register_pnp_bit_for_bit(ctx, frames, distance):
    seed = 77
    rows = match_rows(ctx, frames, PAIRS, distance)
    res, _ = pnp_batch(ctx, frames, seed, distance)
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
        one = ctx.register_pnp(d1.ptr, na, d2.ptr, nb, camera(CAM), seed=(seed + p) & MASK64, **kw)
        after = d1.to_numpy(SIFT_POINT_DTYPE, (max(na, 1),))[:na]
        same_pnp(res, p, one, after, na, "register_pnp")
        assert after["coords3D"].tobytes() == f1["coords3D"][:na].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
def test_cross_check_on_equals_the_staged_route_over_mutual_rows(frames, distance):
    from cusift_amd import capi

    if capi.device_count() < 1:
        pytest.fail("gpu test selected but no HIP device is visible")
    seed = 0xC0FFEE
    rule = RULES[distance]
    with capi.Context(0) as own:
        pts, cnt = frames.upload(own)
        rows_d = upload(own, np.full((len(PAIRS), MAX_PTS, 16), SENTINEL, np.uint8))
        back_d = upload(own, np.full((len(PAIRS), MAX_PTS, 16), SENTINEL, np.uint8))
        own.match_batch_mutual(pts.ptr, cnt.ptr, N_FRAMES, MAX_PTS, PAIRS, rows_d.ptr, back_d.ptr, distance)
        own.synchronize()
        rows, back = rows_d.to_numpy(capi.MatchRow, (len(PAIRS), MAX_PTS)), back_d.to_numpy(capi.MatchRow, (len(PAIRS), MAX_PTS))
        off, _ = pnp_batch(own, frames, seed, distance)
        own.set_cross_check(True)
        res, recs = pnp_batch(own, frames, seed, distance)
        assert recs.tobytes() == frames.points.tobytes()
        own.set_cross_check(False)
        dropped = 0
        for p, (a, b) in enumerate(PAIRS):
            na, nb = int(frames.n[a]), int(frames.n[b])
            m = rows[p, :na]["match"]
            ok = (m >= 0) & (m < nb) if nb > 0 else np.zeros(na, bool)
            mutual = ok & (back[p, np.where(ok, m, 0)]["match"] == np.arange(na)) if nb > 0 else ok
            plain = scatter(frames, rows[p], a, b)[0][:na]
            by_rule = pnp_candidates(plain, rule["rule"], rule["lo"], rule["hi"], nb) if na >= 6 else np.zeros(0, int)
            dropped += int((~mutual[by_rule]).sum())
            copy, _, _ = scatter(frames, rows[p], a, b, mutual=mutual, rule=rule["rule"])
            one, after = staged(own, copy, na, nb, seed + p, distance)
            same_pnp(res, p, one, after, na, "mutual rows")
            assert one.num_candidates == (int(mutual[by_rule].sum()) if na >= 6 else 0), p
            assert not res.inliers[p][~mutual].any(), p
        print("distance %d: the cross-check dropped %d records that the thresholds let through" % (distance, dropped))
        assert dropped >= 1 and not same_results(res, off)  # the setting bites: frame 0 holds 25 points twice
        own.set_cross_check(True)
        kw = dict(distance=distance, loops=LOOPS, thresh=THRESH, refine_loops=REFINE_LOOPS, refine_thresh=REFINE_THRESH)
        kw.update(rule)
        for p, (a, b) in enumerate(PAIRS):  # the self pair against a copy: the pair call refuses overlapping ranges
            na, nb = int(frames.n[a]), int(frames.n[b])
            d1, d2 = upload(own, frames.points[a, :max(na, 1)].copy()), upload(own, frames.points[b, :max(nb, 1)].copy())
            one = own.register_pnp(d1.ptr, na, d2.ptr, nb, camera(CAM), seed=(seed + p) & MASK64, **kw)
            same_pnp(res, p, one, d1.to_numpy(SIFT_POINT_DTYPE, (max(na, 1),))[:na], na, "register_pnp, cross-check on")


@pytest.mark.gpu
def test_degenerate_pairs_and_the_frames_of_six_and_seven_records(ctx, frames):
    seed = 9
    res, recs = pnp_batch(ctx, frames, seed)
    assert recs.tobytes() == frames.points.tobytes()
    for p in DEGENERATE_AT:
        assert np.array_equal(res.rt[p], IDENT) and np.array_equal(res.ransac[p], IDENT), p
        assert res.num_matches[p] == 0 and res.num_fit[p] == 0 and res.best_loop[p] == 0 and not res.inliers[p].any(), p
        assert np.isnan(res.match_error[p]).all(), p
    print("candidates of the list:", res.num_candidates.tolist(), "counts:", res.counts.tolist())
    assert res.counts.tolist() == [int(frames.n[a]) for a, _ in PAIRS]
    assert [int(res.num_candidates[p]) for p in (6, 7, 8, 9, 12)] == [0] * 5  # empty, empty, 5 records, NaN, no depth
    assert res.num_candidates[13] >= 600  # no support: the candidates are counted, every hypothesis counts nothing
    # the frames of 6 and 7 records are fitted: 6 and 7 candidates, the restatement's pose
    k = cam_of(CAM)
    rows = match_rows(ctx, frames, PAIRS, 1)
    for p, n in SMALL_AT.items():
        a, b = PAIRS[p]
        assert res.num_candidates[p] == n and res.counts[p] == n and res.num_matches[p] >= 1, (p, res.num_candidates[p])
        copy, na, nb = scatter(frames, rows[p], a, b)
        cand = pnp_candidates(copy, RULES[1]["rule"], RULES[1]["lo"], RULES[1]["hi"], nb)
        assert len(cand) == n
        c5 = coords5(copy, cand)
        want, near = refit(res.ransac[p].ravel(), k, c5, REFINE_LOOPS, REFINE_THRESH)
        d_rt = float(np.abs(want - res.rt[p].ravel()).max())
        R, t = frames.pose_of(a, b)
        print("pair (%d, %d): %d records, %d inliers, %d fit, [R | t] from the model's refit of the device's winner by %.3g; "
              "rotation %.3f degrees from the planted one" % (a, b, n, res.num_matches[p], res.num_fit[p], d_rt,
                                                              rot_err(res.rt[p][:, :3], R)))
        assert res.num_matches[p] == int(pnp_inliers(res.ransac[p].ravel(), k, c5, THRESH).sum())
        assert res.num_fit[p] == int(pnp_inliers(res.rt[p].ravel(), k, c5, REFINE_THRESH).sum())
        assert near or d_rt <= 1e-9, d_rt
    # the same frames under the epipolar call report no candidate: fewer than eight records
    pts, cnt = frames.upload(ctx)
    epi = ctx.register_epipolar_batch(pts.ptr, cnt.ptr, N_FRAMES, MAX_PTS, PAIRS[list(SMALL_AT)], loops=64, seed=seed)
    assert epi.num_candidates.tolist() == [0, 0] and not epi.fundamental.any() and epi.counts.tolist() == [6, 7]
    # every other pair is what a list with ordinary pairs in the degenerate places gives it
    clean = PAIRS.copy()
    clean[list(DEGENERATE_AT)] = (0, 1)
    ref, _ = pnp_batch(ctx, frames, seed, pairs=clean)
    others = [p for p in range(len(PAIRS)) if p not in DEGENERATE_AT]
    assert same_results(res, ref, others) and all(ref.num_matches[p] >= 6 for p in DEGENERATE_AT)
    # a counter past max_pts means max_pts; no counters: every frame is full
    clamped = frames.counters.copy()
    clamped[7] = MAX_PTS
    assert same_results(res, pnp_batch(ctx, frames, seed, counters=clamped)[0])
    full = np.full(N_FRAMES, MAX_PTS, np.uint32)
    some = PAIRS[[0, 1, 5]]
    no_counters, recs = pnp_batch(ctx, frames, seed, pairs=some, counters=None)
    assert (no_counters.counts == MAX_PTS).all() and recs.tobytes() == frames.points.tobytes()
    rows = match_rows(ctx, frames, some, 1, counters=None)
    for p, (a, b) in enumerate(some):
        copy, na, nb = scatter(frames, rows[p], a, b, counts=full)
        one, after = staged(ctx, copy, na, nb, seed + p, 1)
        same_pnp(no_counters, p, one, after, MAX_PTS, "no counters")
    none, recs = pnp_batch(ctx, frames, seed, pairs=np.zeros((0, 2), np.int32))
    assert none.rt.shape == (0, 3, 4) and recs.tobytes() == frames.points.tobytes()


@pytest.mark.gpu
def test_same_seed_same_bytes_other_seed_other_samples_and_no_refit(ctx, frames):
    a, _ = pnp_batch(ctx, frames, 5)
    b, _ = pnp_batch(ctx, frames, 5)
    assert same_results(a, b)
    c, _ = pnp_batch(ctx, frames, 6)
    assert not np.array_equal(a.best_loop, c.best_loop) or a.ransac.tobytes() != c.ransac.tobytes()
    d, _ = pnp_batch(ctx, frames, 8)  # pair 0 of seed 8 draws what pair 3 of seed 5 draws: (0, 1) sits at 0 and at 3
    assert d.ransac[0].tobytes() == a.ransac[3].tobytes() and d.rt[0].tobytes() == a.rt[3].tobytes()
    # refine_loops = 0 at the scoring threshold: the refined pose is the winner, and the staged route agrees
    e, _ = pnp_batch(ctx, frames, 5, refine_loops=0, refine_thresh=THRESH)
    assert e.rt.tobytes() == e.ransac.tobytes() == a.ransac.tobytes()
    assert np.array_equal(e.num_matches, a.num_matches) and np.array_equal(e.num_fit, e.num_matches)
    rows = match_rows(ctx, frames, PAIRS, 1)
    for p, (u, v) in enumerate(PAIRS):
        copy, na, nb = scatter(frames, rows[p], u, v)
        buf = upload(ctx, copy)
        one = ctx.estimate_pnp(buf.ptr, na, camera(CAM), nb, loops=LOOPS, thresh=THRESH, refine_loops=0,
                               refine_thresh=THRESH, seed=5 + p, **RULES[1])
        same_pnp(e, p, one, buf.to_numpy(SIFT_POINT_DTYPE, (max(na, 1),))[:na], na, "no refit")
        buf.free()


@pytest.mark.gpu
def test_refusals_leave_everything_untouched(ctx, frames):
    from cusift_amd import capi

    pts, cnt = frames.upload(ctx)
    n_pairs = len(PAIRS)
    rt, ran = np.full((n_pairs, 12), 9.0), np.full((n_pairs, 12), 9.0)
    ints = [np.full(n_pairs, -7, np.int32) for _ in range(4)]
    fl = np.full((n_pairs, MAX_PTS), 5, np.int8)
    err = np.full((n_pairs, MAX_PTS), -2.0, np.float32)
    good = camera(CAM)

    def ptr(a):
        return a.ctypes.data if a is not None else None

    def call(recs=pts.ptr, n_images=N_FRAMES, max_pts=MAX_PTS, pairs=PAIRS, n_pairs=n_pairs, dist=1, rule=1, lo=999.0,
             hi=0.8, cam=good, loops=64, th=3.0, rl=5, rth=2.0, m=rt, r=ran, pc=ints[0], pm=ints[1], pf=ints[2]):
        pairs = None if pairs is None else np.ascontiguousarray(pairs, np.int32)
        return capi.lib().cusift_register_pnp_batch(ctx.handle, recs, cnt.ptr, n_images, max_pts, ptr(pairs), n_pairs, dist,
                                                    rule, lo, hi, C.byref(cam) if cam is not None else None, loops, th, rl,
                                                    rth, 1, ptr(m), ptr(r), ptr(pc), ptr(pm), ptr(pf), ptr(ints[3]), ptr(fl),
                                                    ptr(err))

    def untouched():
        return ((rt == 9.0).all() and (ran == 9.0).all() and all((v == -7).all() for v in ints) and (fl == 5).all() and
                (err == -2.0).all())

    nan = float("nan")
    low, high = PAIRS.copy(), PAIRS.copy()
    low[2, 1], high[5, 0] = -1, N_FRAMES
    cases = (  # every case of cusift_register_pnp
        dict(m=None), dict(r=None), dict(pc=None), dict(pm=None), dict(pf=None), dict(loops=0), dict(loops=-3),
        dict(loops=(1 << 24) + 1), dict(th=0.0), dict(th=-1.0), dict(th=nan), dict(rth=0.0), dict(rth=nan), dict(lo=nan),
        dict(hi=nan), dict(rule=2), dict(rule=-1), dict(rl=-1), dict(recs=None), dict(dist=2), dict(dist=-1), dict(cam=None),
        dict(cam=capi.Camera(0.0, 500.0, 320.0, 240.0, 0.0, 0.0, 7)), dict(cam=capi.Camera(500.0, nan, 320.0, 240.0, 0.0, 0.0, 7)),
        dict(cam=capi.Camera(500.0, 500.0, 320.0, 240.0, float("inf"), 0.0, 7)),
        # the pair list's own
        dict(pairs=low), dict(pairs=high), dict(n_pairs=-1), dict(n_pairs=65536, pairs=np.zeros((65536, 2))),
        dict(n_images=-1), dict(n_images=65536), dict(max_pts=-1), dict(max_pts=(1 << 20) + 1), dict(pairs=None),
        dict(n_images=3))
    for kw in cases:
        assert call(**kw) == -1, kw  # CUSIFT_ERR_INVALID
        assert untouched(), kw
    ctx.synchronize()
    assert pts.to_numpy(SIFT_POINT_DTYPE, (N_FRAMES, MAX_PTS)).tobytes() == frames.points.tobytes()
    with pytest.raises(capi.CusiftError):
        ctx.register_pnp_batch(pts.ptr, cnt.ptr, N_FRAMES, MAX_PTS, high, good)
    assert call(n_pairs=0) == 0 and call(n_pairs=0, pairs=None) == 0 and untouched()
    # max_pts == 0 is answered from the arguments alone: every pair is degenerate
    assert call(max_pts=0, recs=None) == 0
    assert np.array_equal(rt, np.tile(IDENT.ravel(), (n_pairs, 1))) and np.array_equal(ran, rt)
    assert all(not v.any() for v in ints) and (fl == 5).all() and (err == -2.0).all()
    # and the same arguments without a fault run; a block's tail is not written
    assert call(loops=LOOPS) == 0
    for p, (a, b) in enumerate(PAIRS):
        na = int(frames.n[a])
        assert np.isin(fl[p, :na], (0, 1)).all() and (fl[p, na:] == 5).all(), p
        assert fl[p, :na].sum() == ints[1][p], p
        if p in DEGENERATE_AT:
            assert (err[p] == -2.0).all() and ints[1][p] == 0, p
        else:
            assert ints[0][p] >= 6 and ints[1][p] >= 1 and (err[p, :na] != -2.0).all() and (err[p, na:] == -2.0).all(), p
    assert pts.to_numpy(SIFT_POINT_DTYPE, (N_FRAMES, MAX_PTS)).tobytes() == frames.points.tobytes()
    # the optional outputs may be left out
    m2, r2 = np.zeros_like(rt), np.zeros_like(ran)
    c2 = [np.zeros(n_pairs, np.int32) for _ in range(3)]
    assert capi.lib().cusift_register_pnp_batch(ctx.handle, pts.ptr, cnt.ptr, N_FRAMES, MAX_PTS, PAIRS.ctypes.data, n_pairs,
                                                1, 1, 999.0, 0.8, C.byref(good), LOOPS, 3.0, 5, 2.0, 1, ptr(m2), ptr(r2),
                                                ptr(c2[0]), ptr(c2[1]), ptr(c2[2]), None, None, None) == 0
    assert m2.tobytes() == rt.tobytes() and r2.tobytes() == ran.tobytes() and all(
        np.array_equal(u, v) for u, v in zip(c2, ints))


@pytest.mark.gpu
def test_optional_outputs_left_out_change_nothing_else(ctx, frames):
    """tests/test_planar_batch.py's check of the read-back branches below the wrapper's, on the model whose winner may
    lack support: raw calls with neither flags nor errors, with errors only, with both, over the whole list.  Models and
    counts byte-equal; the third call's flags and errors are the wrapper's."""
    from cusift_amd import capi

    seed, n_pairs = 9, len(PAIRS)
    pts, cnt = frames.upload(ctx)
    rule = RULES[1]
    outs, fl, err = optional_outputs_three_ways(
        lambda *out: capi.lib().cusift_register_pnp_batch(ctx.handle, pts.ptr, cnt.ptr, N_FRAMES, MAX_PTS,
                                                          PAIRS.ctypes.data, n_pairs, 1, rule["rule"], rule["lo"],
                                                          rule["hi"], C.byref(camera(CAM)), LOOPS, THRESH, REFINE_LOOPS,
                                                          REFINE_THRESH, seed, *out),
        n_pairs, MAX_PTS, (3, 4), np.float64)
    res, _ = pnp_batch(ctx, frames, seed)
    for u, v in zip(outs, res[:6]):
        assert u.tobytes() == np.asarray(v).tobytes()
    for p in range(n_pairs):
        n = int((fl[p] >= 0).sum())
        assert n == res.counts[p] and (fl[p, :n] >= 0).all(), p
        assert np.array_equal(fl[p, :n] == 1, res.inliers[p]), p
        assert err[p, :n].tobytes() == res.match_error[p].tobytes() and np.isnan(err[p, n:]).all(), p
    assert np.isnan(err[list(DEGENERATE_AT)]).all() and not np.isnan(err[0, :frames.n[0]]).all()
    assert res.num_candidates[13] >= 6 and res.num_matches[13] == 0  # the winner without support is among them


@pytest.mark.gpu
def test_restatement_recounts_every_integer_and_reproduces_the_pose(ctx, frames):
    distance, skipped = 0, 0
    k = cam_of(CAM)
    rule = RULES[distance]
    rows = match_rows(ctx, frames, PAIRS, distance)
    for seed in SEEDS[:2]:
        res, _ = pnp_batch(ctx, frames, seed, distance)
        for p, (a, b) in PLANTED_PAIRS.items():
            copy, na, nb = scatter(frames, rows[p], a, b)
            cand = pnp_candidates(copy, rule["rule"], rule["lo"], rule["hi"], nb)
            c5 = coords5(copy, cand)
            assert res.num_candidates[p] == len(cand)
            win = pnp_inliers(res.ransac[p].ravel(), k, c5, THRESH)
            flags = np.zeros(na, bool)
            flags[cand] = win
            assert res.num_matches[p] == int(win.sum()) and np.array_equal(res.inliers[p], flags), p
            assert res.num_fit[p] == int(pnp_inliers(res.rt[p].ravel(), k, c5, REFINE_THRESH).sum()), p
            assert np.array_equal(res.match_error[p], match_error(res.rt[p].ravel(), k, coords5(copy)), equal_nan=True), p
            want, near = refit(res.ransac[p].ravel(), k, c5, REFINE_LOOPS, REFINE_THRESH)
            d_rt = float(np.abs(want - res.rt[p].ravel()).max())
            R, t = frames.pose_of(a, b)
            r = rot_err(res.rt[p][:, :3], R)
            d = float(np.sqrt(((res.rt[p][:, 3] - t) ** 2).sum()) / np.sqrt(t @ t))
            print("seed %#x pair (%d, %d): %d candidates, %d inliers, %d fit; [R | t] from the model's refit of the device's "
                  "winner by %.3g%s; rotation %.4f degrees, translation %.4f of |t|" %
                  (seed, a, b, len(cand), res.num_matches[p], res.num_fit[p], d_rt, " (near: skipped)" if near else "", r, d))
            assert r <= ROT_BOUND and d <= TRANS_BOUND, (r, d)
            Rm = res.rt[p][:, :3]
            assert np.abs(Rm @ Rm.T - np.eye(3)).max() <= 1e-12 and np.linalg.det(Rm) > 0.999
            if near:
                skipped += 1
                continue
            assert d_rt <= 1e-9, d_rt
    assert skipped <= 1


@pytest.mark.gpu
def test_sizes_where_the_loops_turn_a_second_time(ctx):
    """max_pts 4096, 3 pairs, 4096 loops: on 256 CUs score_splits gives 11 candidate splits of 6 tiles each, and the
    marking has 16 blocks per pair.  Frames of 4096 and 3000 records, 60 % planted."""
    big = Frames(n_points=4096, max_pts=4096, counts=(4096, 3000, 4096), seed=5, outliers=5)
    pairs = np.array([(0, 1), (1, 0), (2, 1)], np.int32)
    seed = 3
    res, recs = pnp_batch(ctx, big, seed, 1, pairs=pairs, loops=4096)
    assert recs.tobytes() == big.points.tobytes()
    rows = match_rows(ctx, big, pairs, 1)
    for p, (a, b) in enumerate(pairs):
        copy, na, nb = scatter(big, rows[p], a, b)
        one, after = staged(ctx, copy, na, nb, seed + p, 1, loops=4096)
        print("pair (%d, %d): %d candidates, %d inliers, %d fit" % (a, b, one.num_candidates, one.num_matches, one.num_fit))
        assert one.num_candidates > 6 * 64 * 6 and one.num_matches >= 1000
        same_pnp(res, p, one, after, na, "large")


@pytest.mark.gpu
def test_extractor_sequence_equals_the_context_calls_and_lifts_the_batch_first(ctx, frames):
    """BatchExtractor.register_pnp_sequence over the extractor's own buffers: the Context call on the same pointers, and --
    with d_depth -- lift_depth over the whole batch followed by register_pnp_batch, on a second extractor filled alike."""
    import torch
    from cusift_amd import capi
    from cusift_amd.batch import BatchExtractor

    cam = capi.Camera(CAM[0], CAM[1], CAM[2], CAM[3], CAM[4], 1000.0, 0)
    depth = np.random.default_rng(3).integers(2000, 6000, size=(3, H, W)).astype(np.uint16)
    kw = dict(distance=1, rule=1, lo=999.0, hi=0.8, loops=512, seed=21, want_errors=True)
    ex, ex2 = (BatchExtractor(3, W, H, num_octaves=3, max_pts=MAX_PTS) for _ in range(2))
    try:
        fill_extractor(ex, frames)
        fill_extractor(ex2, frames)
        before = [r.copy() for r in ex.to_host()]
        points, counts = ex.slots[0]
        for pairs in (None, [(1, 0), (0, 1), (1, 1)]):
            want_pairs = [(0, 1), (1, 2)] if pairs is None else pairs
            seq = ex.register_pnp_sequence(cam, pairs=pairs, **kw)
            ref = ex.ctx.register_pnp_batch(points.data_ptr(), counts.data_ptr(), 3, MAX_PTS, want_pairs, cam, **kw)
            assert same_results(seq, ref) and seq.num_matches.min() >= 6
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, ex.to_host()))  # the records: untouched
        # with depth: one lift over the batch first; only coords3D of the records changes
        d_depth = torch.from_numpy(depth.view(np.int16)).to(ex.device)
        seq = ex.register_pnp_sequence(cam, d_depth=d_depth, **kw)
        p2, c2 = ex2.slots[0]
        ex2.ctx.lift_depth(p2.data_ptr(), MAX_PTS, d_depth.data_ptr(), W, H, cam, pitch=W, n_images=3,
                           d_counters=c2.data_ptr(), image_stride=H * W)
        ref = ex2.ctx.register_pnp_batch(p2.data_ptr(), c2.data_ptr(), 3, MAX_PTS, [(0, 1), (1, 2)], cam, **kw)
        assert same_results(seq, ref) and seq.num_candidates.min() >= 6
        after, after2 = ex.to_host(), ex2.to_host()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(after, after2))
        for a, b in zip(before[:2], after[:2]):
            assert a["coords3D"].tobytes() != b["coords3D"].tobytes()
            rest = b.copy()
            rest["coords3D"] = a["coords3D"]
            assert rest.tobytes() == a.tobytes()
        chain = capi.chain_poses(seq.rt)
        assert chain.shape == (3, 4, 4) and np.isfinite(chain).all()
    finally:
        ex.close()
        ex2.close()
