"""The real route: BatchExtractor.build_tracks -- the pair-list matcher (float or 8-bit, mutual or not) and
cusift_build_tracks behind it on one stream -- on six frames of planted records.  What comes back must be the model
(tests/tracks_model.py) run on the very rows the matcher wrote; with the inliers of register_planar_sequence fed back,
every observation of every track is an inlier of one of its pairs."""
import numpy as np
import pytest

from oracle_binding import SIFT_POINT_DTYPE
from tracks_model import ROW, build_tracks_model

N, MAX_PTS, N_POINTS, N_NOISE = 6, 256, 170, 40
PAIRS = [(a, b) for a in range(N) for b in range(a + 1, min(a + 2, N - 1) + 1)]  # a window of 2: 9 pairs


def planted_frames():
    """170 scene points on a plane, each seen by a frame with probability 0.8 at its place under the frame's
    homography, with its descriptor plus a little noise; 40 records of noise per frame; every frame in an order of its
    own.  Returns (records [N, MAX_PTS], counts [N], point [N, MAX_PTS]: the scene point of a record, -1 for noise)."""
    rng = np.random.default_rng(17)
    base_xy = rng.uniform([20, 20], [620, 460], size=(N_POINTS, 2))
    base_desc = np.abs(rng.normal(size=(N_POINTS, 128)))
    recs = np.zeros((N, MAX_PTS), SIFT_POINT_DTYPE)
    counts, point = np.zeros(N, np.int32), np.full((N, MAX_PTS), -1, np.int32)
    for f in range(N):
        H = np.array([[1 + 0.01 * f, 0.02 * f, 5.0 * f], [-0.015 * f, 1 - 0.005 * f, -3.0 * f], [1e-5 * f, -2e-5 * f, 1.0]])
        seen = np.flatnonzero(rng.random(N_POINTS) < 0.8)
        xyw = np.c_[base_xy[seen], np.ones(len(seen))] @ H.T
        xy = np.r_[xyw[:, :2] / xyw[:, 2:], rng.uniform([0, 0], [640, 480], size=(N_NOISE, 2))]
        desc = np.r_[base_desc[seen] + 0.05 * np.abs(rng.normal(size=(len(seen), 128))), np.abs(rng.normal(size=(N_NOISE, 128)))]
        desc /= np.linalg.norm(desc, axis=1, keepdims=True)
        order = rng.permutation(len(xy))
        counts[f] = len(xy)
        recs["coords2D"][f, : len(xy)] = xy[order]
        recs["data"][f, : len(xy)] = desc[order]
        recs["scale"][f, : len(xy)] = 2.0
        point[f, : len(xy)] = np.r_[seen, np.full(N_NOISE, -1)][order]
    assert counts.max() <= MAX_PTS
    return recs, counts, point


def extractor(bits):
    import torch
    from cusift_amd.batch import BatchExtractor

    recs, counts, point = planted_frames()
    ex = BatchExtractor(N, 64, 64, max_pts=MAX_PTS, match_bits=bits)
    ex.points.copy_(torch.from_numpy(recs.view(np.uint8).reshape(N, MAX_PTS, -1)))
    ex.counts.copy_(torch.from_numpy(counts))
    return ex, counts, point


def host_rows(t):
    return None if t is None else t.cpu().numpy().view(ROW).reshape(len(PAIRS), MAX_PTS)


def assert_equals_model(tracks, counts, keep=None, **opts):
    import torch

    torch.cuda.synchronize()
    rows, back = host_rows(tracks.rows), host_rows(tracks.rows_back)
    track, offsets, obs, stats = build_tracks_model(counts, MAX_PTS, PAIRS, rows, back, keep, **opts)
    np.testing.assert_array_equal(tracks.stats.cpu().numpy().view(np.uint32), stats)
    np.testing.assert_array_equal(tracks.track.cpu().numpy(), track)
    np.testing.assert_array_equal(tracks.offsets.cpu().numpy()[: len(offsets)], offsets)
    np.testing.assert_array_equal(tracks.obs.cpu().numpy()[: len(obs)], obs)
    n_tracks, lists = tracks.to_host()
    assert n_tracks == stats[0] == len(lists)
    assert [v for nodes in lists for v in nodes] == [(int(v) // MAX_PTS, int(v) % MAX_PTS) for v in obs]
    return rows, back, offsets, obs, stats


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [32, 8])
def test_build_tracks_equals_the_model_on_the_matchers_rows(bits):
    ex, counts, point = extractor(bits)
    try:
        opts = dict(rule=1, lo=999.0, hi=0.8)
        tracks = ex.build_tracks(pairs=PAIRS, min_views=2)
        rows, back, offsets, obs, stats = assert_equals_model(tracks, counts, min_views=2, **opts)
        assert back is not None and stats[0] > 100 and np.diff(offsets).max() == N
        # the planted scene comes back: the members of a track are views of one scene point
        clean = sum(len(set(point.reshape(-1)[obs[offsets[t]:offsets[t + 1]]].tolist())) == 1 for t in range(stats[0]))
        print("match_bits %d: %d tracks, %d observations, %d tracks of one scene point; %d components shared a frame"
              % (bits, stats[0], stats[1], clean, stats[3]))
        assert clean >= 0.9 * stats[0]
        # one direction only, three views at least, rule 0 on its own thresholds
        one_way = ex.build_tracks(pairs=PAIRS, mutual=False, min_views=3)
        _, no_back, _, _, stats3 = assert_equals_model(one_way, counts, min_views=3, **opts)
        assert no_back is None and one_way.rows_back is None and stats3[0] > 50
        assert_equals_model(ex.build_tracks(pairs=PAIRS, rule=0, lo=0.0, hi=0.95), counts, rule=0, lo=0.0, hi=0.95)
    finally:
        ex.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [32, 8])
def test_inliers_of_the_planar_registration_go_back_in(bits):
    ex, counts, point = extractor(bits)
    try:
        res = ex.register_planar_sequence(pairs=PAIRS, loops=1000, seed=3)
        assert min(int(f.sum()) for f in res.inliers) >= 30
        # pair 0 as if its registration had failed: no inlier, so none of its rows may join anything
        inliers = [np.zeros_like(res.inliers[0])] + list(res.inliers[1:])
        tracks = ex.build_tracks(pairs=PAIRS, inliers=inliers)
        keep = np.zeros((len(PAIRS), MAX_PTS), np.uint8)
        for p, flags in enumerate(inliers):
            keep[p, : len(flags)] = flags
        rows, back, offsets, obs, stats = assert_equals_model(tracks, counts, keep=keep, rule=1, lo=999.0, hi=0.8)
        assert stats[0] > 50
        # every observation is an end of a row that the registration kept
        ends = set()
        for p, (a, b) in enumerate(PAIRS):
            for i in np.flatnonzero(keep[p]):
                ends.add(a * MAX_PTS + int(i))
                ends.add(b * MAX_PTS + int(rows[p, i]["match"]))
        assert set(obs.tolist()) <= ends
        unfiltered = ex.build_tracks(pairs=PAIRS)
        import torch
        torch.cuda.synchronize()
        assert int(unfiltered.stats[2].item()) > stats[2]  # pair 0's rows at the least
    finally:
        ex.close()
