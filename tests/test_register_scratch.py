"""One scratch block for every registration call (cusift_ctx::register_scratch, cusift_amd/csrc/sift_register.hip): rigid
RANSAC, the planar pair call, the match selection and the planar pair-list call lay their state out in the same device
block, one call after the other.  No call may read what an earlier one left there.

The check: on ONE context the calls run back to back, in an order that makes the block grow (rigid: a few KB; planar
pair: more; pair list: the most) and then be reused at a smaller size by the first three again.  Every output of every
call -- host results and what the call wrote on the device -- is byte for byte what the same call gives on a context of its
own, which has never held anything else.  No tolerance: the routes are deterministic.
"""
import numpy as np
import pytest

from oracle_binding import SIFT_POINT_DTYPE
from test_homography import planted
from test_planar import subset_scores, upload
from test_planar_batch import planted_frames
from test_rigid import scene


def as_bytes(outputs):
    return [np.ascontiguousarray(o).tobytes() for o in outputs]


def rigid(ctx):
    """cusift_estimate_rigid: 40 points, 64 hypotheses drawn on the device, everything asked for."""
    return as_bytes(ctx.estimate_rigid(scene(30, 10, seed=5), loops=64, thresh2=0.0025, seed=3, want_all=True))


def planar(ctx):
    """cusift_estimate_homography: 300 records -- two 256-record blocks, so the candidate scan crosses a block -- 128
    hypotheses, the samples / hypotheses / counts asked for; and the records afterwards (match_error is written)."""
    pts, _, _ = planted(200, 100, seed=7)
    buf = upload(ctx, pts)
    res = ctx.estimate_homography(buf.ptr, len(pts), -1, rule=0, lo=0.0, hi=0.8, loops=128, thresh=5.0, refine_loops=5,
                                  refine_thresh=3.0, seed=11, want_all=True)
    assert res.num_candidates == 300 and res.num_matches >= 100
    return as_bytes(res) + [buf.to_numpy(SIFT_POINT_DTYPE, (len(pts),)).tobytes()]


def select(ctx):
    """cusift_select_matches on 300 records, about half of them kept: the second block's rows start behind the first
    block's count, which lives in the scratch."""
    base, _, _ = planted(200, 100, seed=7)
    pts = subset_scores(base, 1, 21)  # scores, ambiguities and match indices in [0, 500), two of them out of range
    other = np.zeros(500, SIFT_POINT_DTYPE)
    other["coords3D"] = np.random.default_rng(2).uniform(0.5, 3.0, (500, 3)).astype(np.float32)
    b1, b2 = upload(ctx, pts), upload(ctx, other)
    pairs, coord = upload(ctx, np.full((300, 2), -1, np.int32)), upload(ctx, np.full((300, 6), -1, np.float32))
    count = upload(ctx, np.full(1, -1, np.int32))
    ctx.select_matches(b1.ptr, 300, b2.ptr, 500, pairs.ptr, coord.ptr, count.ptr, 0.7, 0.8, "2d")
    ctx.synchronize()
    k = int(count.to_numpy(np.int32, (1,))[0])
    got = pairs.to_numpy(np.int32, (300, 2))
    assert 100 < k < 200 and got[:k, 0].max() >= 256 and (np.diff(got[:k, 0]) > 0).all()
    return as_bytes([k, got, coord.to_numpy(np.float32, (300, 6))])


def planar_batch(ctx):
    """cusift_register_planar_batch: three frames (the planted pair of test_planar_batch and a cut of its first frame) in
    1024 slots, two pairs."""
    fa, fb, _, _ = planted_frames(np.zeros(1, SIFT_POINT_DTYPE))
    frames = [fa, fb, fa[:300]]
    points = np.zeros((3, 1024), SIFT_POINT_DTYPE)
    for k, f in enumerate(frames):
        points[k, :len(f)] = f
    pts, cnt = upload(ctx, points), upload(ctx, np.array([len(f) for f in frames], np.uint32))
    res = ctx.register_planar_batch(pts.ptr, cnt.ptr, 3, 1024, np.array([(0, 1), (2, 1)], np.int32), distance=1,
                                    loops=256, thresh=5.0, refine_loops=5, refine_thresh=3.0, seed=9, want_inliers=True,
                                    want_errors=True)
    assert res.counts.tolist() == [1024, 300] and (res.num_matches >= 100).all()
    flat = list(res[:7]) + list(res.inliers) + list(res.match_error)
    return as_bytes(flat) + [pts.to_numpy(SIFT_POINT_DTYPE, (3, 1024)).tobytes()]


@pytest.mark.gpu
def test_calls_sharing_one_scratch_block_equal_calls_on_fresh_contexts():
    from cusift_amd import capi

    order = [rigid, planar, select, planar_batch, rigid, planar, select]
    shared = capi.Context(0)
    try:
        for step, call in enumerate(order):
            got = call(shared)
            fresh = capi.Context(0)
            try:
                want = call(fresh)
            finally:
                fresh.close()
            assert len(got) == len(want) and all(len(g) > 0 for g in got), (step, call.__name__)
            for k, (g, w) in enumerate(zip(got, want)):
                assert g == w, "step %d (%s): output %d differs from the call on a fresh context" % (step, call.__name__, k)
    finally:
        shared.close()
