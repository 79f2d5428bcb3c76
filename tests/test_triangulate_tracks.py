"""cusift_triangulate_tracks (cusift_amd/csrc/sift_tracks.hip) against tests/tracks_model.py's restatement in numpy: the
six-camera scene with 300 tracks of 2 to 6 views, a track of two identical rays, a track behind one of its cameras, a
record that is not finite, rows past the track count, and the refusals.  The bar for fp64 against a numpy restatement is
the one of tests/test_pose.py and tests/test_pnp.py: 1e-9 * max(1, |value|).

The pixel origin (px = cx - origin): origin 1 with (cx + 1, cy + 1) must give the bytes of origin 0 with (cx, cy) -- 320
and 240 are exact in float32 --, and origin 0.5 on pixels generated for it must equal the model called with 0.5, which
the CPU test shows to be 0.004 to 0.1 per track away from the model with the origin dropped (0.008 to 0.2 with its sign
flipped).  Measured on an MI355X: largest deviation 0 for origin 0.5, as for origin 0.  Tried once in a scratch build
that was never committed, `cx + origin` in cusift_triangulate_tracks: test_origin_one_is_origin_zero_to_the_byte fails
on the bytes, test_origin_half_equals_the_model with a deviation of 3.16, and tests/test_bundle_batch.py on the bytes of
its origin-1 call; everything else of this file stays green (origin 0 throughout)."""
import ctypes as C

import numpy as np
import pytest

from oracle_binding import SIFT_POINT_DTYPE
from tracks_model import six_camera_scene, triangulate_model

N_TRACKS, MAX_PTS, N_CAMS = 300, 304, 6
FILL = -7.0


def scene():
    """(poses [7, 3, 4], records [7, MAX_PTS], offsets, obs, camera values): frame 6 is frame 0's pose again.  Track t <
    297 is record t of 2 to 6 of the six cameras; 297: frames 0 and 6 at the same pixel; 298: a point behind camera 5;
    299: a member whose x is NaN."""
    poses6, planted, pixels, cam = six_camera_scene(N_TRACKS, seed=21)
    fx, fy, cx, cy = cam
    rng = np.random.default_rng(4)
    poses = np.concatenate([poses6, poses6[:1]])
    recs = np.zeros((N_CAMS + 1, MAX_PTS), SIFT_POINT_DTYPE)
    recs["coords2D"][:N_CAMS, :N_TRACKS] = pixels
    recs["coords2D"][N_CAMS, :N_TRACKS] = pixels[0]
    # 298: half a unit behind camera 5 and a little off its axis; cameras 0 and 1 see it in front of them
    R5, c5 = poses[5, :, :3], poses[5, :, 3]
    behind = c5 - 0.5 * R5[:, 2] + 0.1 * R5[:, 0]
    for k in (0, 1, 5):
        c = (behind - poses[k, :, 3]) @ poses[k, :, :3]
        recs["coords2D"][k, 298] = (np.float32(fx * c[0] / c[2] + cx), np.float32(fy * c[1] / c[2] + cy))
    assert ((behind - c5) @ R5)[2] < 0 < ((behind - poses[0, :, 3]) @ poses[0, :, :3])[2]
    offsets, obs = [0], []
    for t in range(N_TRACKS):
        if t == 297:
            frames = [0, 6]
        elif t == 298:
            frames = [0, 1, 5]
        else:
            frames = sorted(rng.choice(N_CAMS, size=int(rng.integers(2, N_CAMS + 1)), replace=False).tolist())
        obs += [f * MAX_PTS + t for f in frames]
        offsets.append(len(obs))
    recs["coords2D"][obs[offsets[299]] // MAX_PTS, 299, 0] = np.nan
    return poses, recs, np.asarray(offsets, np.int32), np.asarray(obs, np.int32), cam


class Device:
    """The scene on the device, outputs filled with FILL."""

    def __init__(self, ctx, recs, offsets, obs, n_tracks, cap):
        self.ctx, self.cap = ctx, cap
        stats = np.zeros(8, np.uint32)
        stats[0], stats[1] = n_tracks, offsets[n_tracks]
        self.host = [recs, offsets, obs, stats, np.full((cap, 4), FILL), np.full(cap, int(FILL), np.int32)]
        self.ptrs = [ctx.malloc(max(a.nbytes, 16)) for a in self.host]
        for p, a in zip(self.ptrs, self.host):
            ctx.h2d(p, a)
        ctx.synchronize()

    def read(self):
        self.ctx.synchronize()
        out, front = np.empty((self.cap, 4)), np.empty(self.cap, np.int32)
        self.ctx.d2h(out, self.ptrs[4])
        self.ctx.d2h(front, self.ptrs[5])
        return out, front

    def close(self):
        for p in self.ptrs:
            self.ctx.free(p)


def test_the_scene_holds_every_kind_of_track():
    poses, recs, offsets, obs, (fx, fy, cx, cy) = scene()
    out, front = triangulate_model(recs["coords2D"], MAX_PTS, offsets, obs, poses, fx, fy, cx, cy)
    views = np.diff(offsets)
    assert set(views[:297].tolist()) == {2, 3, 4, 5, 6}
    assert (out[297] == 0).all() and front[297] == 0  # identical rays: q22 is rounding noise
    assert front[298] == 2 and views[298] == 3 and np.abs(out[298, :3]).max() > 1  # behind camera 5
    assert (out[299] == 0).all() and front[299] == 0  # a NaN coordinate
    assert (front[:297] == views[:297]).all() and (out[:297, 3] < 1e-3).all() and (out[:297, 3] > 0).all()
    # a parallax limit: 0.02 is 1 - cos(0.2 rad), the angle between neighbouring cameras
    strict, _ = triangulate_model(recs["coords2D"], MAX_PTS, offsets, obs, poses, fx, fy, cx, cy, min_pivot=0.02)
    assert 3 < (strict == 0).all(axis=1).sum() < N_TRACKS - 50


@pytest.mark.gpu
def test_points_equal_the_model(ctx):
    from cusift_amd import capi

    poses, recs, offsets, obs, (fx, fy, cx, cy) = scene()
    want, want_front = triangulate_model(recs["coords2D"], MAX_PTS, offsets, obs, poses, fx, fy, cx, cy)
    cam = capi.Camera(fx, fy, cx, cy)
    cap = N_TRACKS + 5
    dev = Device(ctx, recs, offsets, obs, N_TRACKS, cap)
    try:
        d_recs, d_offsets, d_obs, d_stats, d_out, d_front = dev.ptrs
        ctx.triangulate_tracks(d_recs, N_CAMS + 1, MAX_PTS, d_offsets, d_obs, d_stats, cap, poses, cam, d_out, d_front)
        out, front = dev.read()
        dev_err = np.abs(out[:N_TRACKS] - want) / np.maximum(1.0, np.abs(want))
        print("triangulate_tracks against the numpy model: largest deviation %.3g (bar 1e-9)" % dev_err.max())
        assert dev_err.max() <= 1e-9
        np.testing.assert_array_equal(front[:N_TRACKS], want_front)
        assert (out[297] == 0).all() and (out[299] == 0).all()
        # rows at and past the track count are not written
        assert (out[N_TRACKS:] == FILL).all() and (front[N_TRACKS:] == int(FILL)).all()
        # the records were only read
        back = np.empty_like(recs)
        ctx.d2h(back, d_recs)
        assert back.tobytes() == recs.tobytes()
        # max_tracks below the track count clamps it
        ctx.h2d(d_out, np.full((cap, 4), FILL))
        ctx.triangulate_tracks(d_recs, N_CAMS + 1, MAX_PTS, d_offsets, d_obs, d_stats, 100, poses, cam, d_out, d_front)
        out, _ = dev.read()
        assert (out[100:] == FILL).all() and np.array_equal(out[:100] == 0, want[:100] == 0) and (out[:100] != FILL).all()
        # 4 x 4 poses, as chain_poses returns them; a larger pivot threshold drops low-parallax tracks
        poses44 = np.tile(np.eye(4), (N_CAMS + 1, 1, 1))
        poses44[:, :3, :] = poses
        ctx.triangulate_tracks(d_recs, N_CAMS + 1, MAX_PTS, d_offsets, d_obs, d_stats, cap, poses44, cam, d_out, d_front,
                               min_pivot=0.02)
        out, front = dev.read()
        strict, strict_front = triangulate_model(recs["coords2D"], MAX_PTS, offsets, obs, poses, fx, fy, cx, cy,
                                                 min_pivot=0.02)
        dropped = (strict == 0).all(axis=1)
        assert np.array_equal((out[:N_TRACKS] == 0).all(axis=1), dropped)
        assert (np.abs(out[:N_TRACKS] - strict) <= 1e-9 * np.maximum(1.0, np.abs(strict))).all()
        np.testing.assert_array_equal(front[:N_TRACKS], strict_front)
    finally:
        dev.close()


def half_origin_scene():
    """scene() as a camera sees it whose cx / cy count from 0.5: every pixel moved by -0.5 (rounded to float32 again)."""
    poses, recs, offsets, obs, cam = scene()
    recs = recs.copy()
    recs["coords2D"] = (recs["coords2D"].astype(np.float64) - 0.5).astype(np.float32)
    return poses, recs, offsets, obs, cam


def test_the_origin_is_visible_to_the_model():
    """px = cx - origin: origin 1 with (cx + 1, cy + 1) is origin 0 with (cx, cy) to the bit; on pixels generated for
    origin 0.5 a dropped or flipped origin moves the points by far more than the bar of the device test."""
    poses, recs, offsets, obs, (fx, fy, cx, cy) = scene()
    assert np.float32(cx + 1.0) - np.float32(1.0) == np.float32(cx) and np.float32(cy + 1.0) - np.float32(1.0) == np.float32(cy)
    zero = triangulate_model(recs["coords2D"], MAX_PTS, offsets, obs, poses, fx, fy, cx, cy)
    one = triangulate_model(recs["coords2D"], MAX_PTS, offsets, obs, poses, fx, fy, cx + 1.0, cy + 1.0, origin=1.0)
    assert one[0].tobytes() == zero[0].tobytes() and one[1].tobytes() == zero[1].tobytes()
    poses, recs, offsets, obs, _ = half_origin_scene()
    half, front = triangulate_model(recs["coords2D"], MAX_PTS, offsets, obs, poses, fx, fy, cx, cy, origin=0.5)
    # the same geometry: the points of scene(), to the float32 rounding of the moved pixels
    assert np.abs(half[:297, :3] - zero[0][:297, :3]).max() < 1e-3 and (front == zero[1]).all()
    for what, origin in (("dropped", 0.0), ("flipped", -0.5)):
        other, _ = triangulate_model(recs["coords2D"], MAX_PTS, offsets, obs, poses, fx, fy, cx, cy, origin=origin)
        moved = (np.abs(other[:297] - half[:297]) / np.maximum(1.0, np.abs(half[:297]))).max(axis=1)
        print("origin %s: the points move by %.3g .. %.3g (bar 1e-9)" % (what, moved.min(), moved.max()))
        assert moved.min() > 1e-5  # ten thousand times the bar, on every track


@pytest.mark.gpu
def test_origin_one_is_origin_zero_to_the_byte(ctx):
    from cusift_amd import capi

    poses, recs, offsets, obs, (fx, fy, cx, cy) = scene()
    dev = Device(ctx, recs, offsets, obs, N_TRACKS, N_TRACKS)
    try:
        d_recs, d_offsets, d_obs, d_stats, d_out, d_front = dev.ptrs
        got = []
        for cam in (capi.Camera(fx, fy, cx, cy), capi.Camera(fx, fy, cx + 1.0, cy + 1.0, origin=1.0)):
            ctx.h2d(d_out, np.full((N_TRACKS, 4), FILL))
            ctx.h2d(d_front, np.full(N_TRACKS, int(FILL), np.int32))
            ctx.triangulate_tracks(d_recs, N_CAMS + 1, MAX_PTS, d_offsets, d_obs, d_stats, N_TRACKS, poses, cam, d_out,
                                   d_front)
            got.append(dev.read())
        assert (got[0][0][:297] != 0).any(axis=1).all() and (got[0][0] != FILL).all()
        assert got[1][0].tobytes() == got[0][0].tobytes() and got[1][1].tobytes() == got[0][1].tobytes()
    finally:
        dev.close()


@pytest.mark.gpu
def test_origin_half_equals_the_model(ctx):
    from cusift_amd import capi

    poses, recs, offsets, obs, (fx, fy, cx, cy) = half_origin_scene()
    want, want_front = triangulate_model(recs["coords2D"], MAX_PTS, offsets, obs, poses, fx, fy, cx, cy, origin=0.5)
    dev = Device(ctx, recs, offsets, obs, N_TRACKS, N_TRACKS)
    try:
        d_recs, d_offsets, d_obs, d_stats, d_out, d_front = dev.ptrs
        ctx.triangulate_tracks(d_recs, N_CAMS + 1, MAX_PTS, d_offsets, d_obs, d_stats, N_TRACKS, poses,
                               capi.Camera(fx, fy, cx, cy, origin=0.5), d_out, d_front)
        out, front = dev.read()
        dev_err = np.abs(out - want) / np.maximum(1.0, np.abs(want))
        print("triangulate_tracks, origin 0.5, against the numpy model: largest deviation %.3g (bar 1e-9)" % dev_err.max())
        assert dev_err.max() <= 1e-9
        np.testing.assert_array_equal(front, want_front)
    finally:
        dev.close()


@pytest.mark.gpu
def test_no_tracks_and_no_frames_write_nothing(ctx):
    """max_tracks = 0 and n_images = 0: CUSIFT_OK, nothing enqueued."""
    from cusift_amd import capi

    poses, recs, offsets, obs, (fx, fy, cx, cy) = scene()
    cam = capi.Camera(fx, fy, cx, cy)
    dev = Device(ctx, recs, offsets, obs, N_TRACKS, N_TRACKS)
    try:
        d_recs, d_offsets, d_obs, d_stats, d_out, d_front = dev.ptrs
        ctx.triangulate_tracks(d_recs, N_CAMS + 1, MAX_PTS, d_offsets, d_obs, d_stats, 0, poses, cam, d_out, d_front)
        ctx.triangulate_tracks(d_recs, 0, MAX_PTS, d_offsets, d_obs, d_stats, N_TRACKS, poses[:0], cam, d_out, d_front)
        ctx.triangulate_tracks(d_recs, 0, 0, d_offsets, d_obs, d_stats, N_TRACKS, poses[:0], cam, d_out, d_front)
        out, front = dev.read()
        assert (out == FILL).all() and (front == int(FILL)).all()
    finally:
        dev.close()


@pytest.mark.gpu
def test_refusals(ctx):
    from cusift_amd import capi

    poses, recs, offsets, obs, (fx, fy, cx, cy) = scene()
    n = N_CAMS + 1
    cap = N_TRACKS
    dev = Device(ctx, recs, offsets, obs, N_TRACKS, cap)
    try:
        d_recs, d_offsets, d_obs, d_stats, d_out, d_front = dev.ptrs
        flat = np.ascontiguousarray(poses.reshape(n, 12))
        bad = [flat.copy() for _ in range(2)]
        bad[0][3, 7], bad[1][6, 0] = np.nan, np.inf
        good = dict(recs=d_recs, n=n, max_pts=MAX_PTS, offsets=d_offsets, obs=d_obs, stats=d_stats, cap=cap,
                    poses=flat.ctypes.data, cam=capi.Camera(fx, fy, cx, cy), pivot=1e-12, out=d_out, front=d_front)
        cases = [dict(recs=None), dict(offsets=None), dict(obs=None), dict(stats=None), dict(poses=None), dict(cam=None),
                 dict(out=None), dict(front=None), dict(poses=bad[0].ctypes.data), dict(poses=bad[1].ctypes.data),
                 dict(cam=capi.Camera(0.0, fy, cx, cy)), dict(cam=capi.Camera(fx, np.inf, cx, cy)),
                 dict(cam=capi.Camera(fx, fy, np.nan, cy)), dict(cam=capi.Camera(fx, fy, cx, np.inf)),
                 dict(cam=capi.Camera(fx, fy, cx, cy, origin=np.nan)), dict(pivot=-1e-30), dict(pivot=np.nan),
                 dict(cap=-1), dict(n=4096, max_pts=1 << 20), dict(n=-1), dict(n=65536), dict(max_pts=-1), dict(max_pts=(1 << 20) + 1)]
        for case in cases:
            a = dict(good, **case)
            rc = capi.lib().cusift_triangulate_tracks(ctx.handle, a["recs"], a["n"], a["max_pts"], a["offsets"], a["obs"],
                                                      a["stats"], a["cap"], a["poses"],
                                                      C.byref(a["cam"]) if a["cam"] is not None else None, a["pivot"],
                                                      a["out"], a["front"])
            assert rc == -1, (case, rc)  # CUSIFT_ERR_INVALID
        out, front = dev.read()
        assert (out == FILL).all() and (front == int(FILL)).all()
    finally:
        dev.close()
