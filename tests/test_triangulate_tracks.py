"""cusift_triangulate_tracks (cusift_amd/csrc/sift_tracks.hip) against tests/tracks_model.py's restatement in numpy: the
six-camera scene with 300 tracks of 2 to 6 views, a track of two identical rays, a track behind one of its cameras, a
record that is not finite, rows past the track count, and the refusals.  The bar for fp64 against a numpy restatement is
the one of tests/test_pose.py and tests/test_pnp.py: 1e-9 * max(1, |value|)."""
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
