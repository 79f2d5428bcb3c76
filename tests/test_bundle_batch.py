"""The real route: BatchExtractor.build_tracks, triangulate_tracks and bundle_adjust behind one another on one stream,
on the planted records of a small sequence -- six cameras of tests/tracks_model.py's scene, every point seen by a frame
with probability 0.8 under a descriptor of its own, noise records besides, the poses a little off.  The cost must not
rise, and the result must be capi.Context.bundle_adjust on the same pointers, byte for byte."""
import numpy as np
import pytest

from oracle_binding import SIFT_POINT_DTYPE
from bundle_model import perturbed
from tracks_model import six_camera_scene

N, MAX_PTS, N_POINTS, N_NOISE = 6, 256, 170, 30
PAIRS = [(a, b) for a in range(N) for b in range(a + 1, min(a + 2, N - 1) + 1)]


def planted_frames():
    rng = np.random.default_rng(23)
    poses, planted, pixels, cam = six_camera_scene(N_POINTS, seed=8)
    base_desc = np.abs(rng.normal(size=(N_POINTS, 128)))
    recs = np.zeros((N, MAX_PTS), SIFT_POINT_DTYPE)
    counts = np.zeros(N, np.int32)
    for f in range(N):
        seen = np.flatnonzero(rng.random(N_POINTS) < 0.8)
        xy = np.r_[pixels[f, seen].astype(np.float64), rng.uniform([0, 0], [640, 480], size=(N_NOISE, 2))]
        desc = np.r_[base_desc[seen] + 0.05 * np.abs(rng.normal(size=(len(seen), 128))), np.abs(rng.normal(size=(N_NOISE, 128)))]
        desc /= np.linalg.norm(desc, axis=1, keepdims=True)
        order = rng.permutation(len(xy))
        counts[f] = len(xy)
        recs["coords2D"][f, : len(xy)] = xy[order]
        recs["data"][f, : len(xy)] = desc[order]
        recs["scale"][f, : len(xy)] = 2.0
    return recs, counts, poses, cam


@pytest.mark.gpu
def test_bundle_adjust_behind_tracks_and_triangulation():
    import torch
    from cusift_amd import capi
    from cusift_amd.batch import BatchExtractor

    recs, counts, true_poses, (fx, fy, cx, cy) = planted_frames()
    start = perturbed(true_poses, 0.01, 0.02, range(1, N))
    cam = capi.Camera(fx, fy, cx, cy)
    ex = BatchExtractor(N, 64, 64, max_pts=MAX_PTS)
    try:
        ex.points.copy_(torch.from_numpy(recs.view(np.uint8).reshape(N, MAX_PTS, -1)))
        ex.counts.copy_(torch.from_numpy(counts))
        tracks = ex.build_tracks(pairs=PAIRS, min_views=2)
        points3d, _ = ex.triangulate_tracks(tracks, start, cam)
        res = ex.bundle_adjust(tracks, start, cam, points3d, iterations=6, huber=2.0)
        poses, pts, history, summary = res.to_host()
        n_tracks = int(tracks.stats[0].item())
        print("%d tracks: cost %.6g -> %.6g, %d of %d steps accepted, %d used tracks, %d observations"
              % (n_tracks, summary[0], summary[1], summary[2], summary[3], summary[4], summary[5]))
        assert n_tracks > 100 and summary[4] > 100 and summary[6] == N - 1
        assert summary[1] <= summary[0] and summary[2] >= 1
        assert (np.diff(history[:, 0]) <= 0).all()
        assert poses.shape == (N, 4, 4) and (poses[:, 3] == [0, 0, 0, 1]).all()
        assert poses[0, :3].tobytes() == np.ascontiguousarray(start[0]).tobytes()
        # the input tensor was not written, and rows past the track count stay as triangulate_tracks left them: zero
        assert (pts[n_tracks:] == 0).all() and (points3d.cpu().numpy()[:n_tracks] != pts[:n_tracks]).any()
        # to_host's poses go straight back in: the cost of the result is the final cost, and nothing is left to accept
        again = ex.bundle_adjust(tracks, poses, cam, res.points3d, iterations=1, huber=2.0)
        assert abs(again.summary[0].item() / summary[1] - 1.0) < 1e-9
        # the camera is handed through: (cx + 1, cy + 1) counted from origin 1 is the same camera (320 and 240 are
        # exact in float32), so both calls give the bytes they gave
        cam1 = capi.Camera(fx, fy, cx + 1.0, cy + 1.0, origin=1.0)
        points3d_1, front_1 = ex.triangulate_tracks(tracks, start, cam1)
        res_1 = ex.bundle_adjust(tracks, start, cam1, points3d_1, iterations=6, huber=2.0)
        torch.cuda.synchronize()
        assert points3d_1.cpu().numpy().tobytes() == points3d.cpu().numpy().tobytes()
        for mine, theirs in ((res_1.points3d, res.points3d), (res_1.poses, res.poses), (res_1.history, res.history),
                             (res_1.summary, res.summary)):
            assert mine.cpu().numpy().tobytes() == theirs.cpu().numpy().tobytes()
        # the same call through Context.bundle_adjust on the same pointers: the same bytes
        cap = tracks.offsets.numel() - 1
        with torch.cuda.device(ex.device), torch.cuda.stream(ex.stream):
            x = points3d.clone()
            d_poses = torch.zeros((N, 12), dtype=torch.float64, device=ex.device)
            d_hist = torch.zeros((6, 4), dtype=torch.float64, device=ex.device)
            d_sum = torch.zeros((8,), dtype=torch.float64, device=ex.device)
            ex.ctx.bundle_adjust(ex.points.data_ptr(), N, MAX_PTS, tracks.offsets.data_ptr(), tracks.obs.data_ptr(),
                                 tracks.stats.data_ptr(), cap, start, cam, x.data_ptr(), d_poses.data_ptr(),
                                 d_hist.data_ptr(), d_sum.data_ptr(), iterations=6, huber=2.0)
        torch.cuda.synchronize()
        for mine, theirs in ((x, res.points3d), (d_poses, res.poses), (d_hist, res.history), (d_sum, res.summary)):
            assert mine.cpu().numpy().tobytes() == theirs.cpu().numpy().tobytes()
    finally:
        ex.close()
