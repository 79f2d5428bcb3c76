"""cusift_build_tracks where the two loops of tracks_order_kernel (cusift_amd/csrc/sift_tracks.hip) turn more than once,
and tracks of that length through cusift_triangulate_tracks.

tracks_order_kernel gives a wave to a track; lane e takes member e, e + 64, ...; the launch has at most 4,096
workgroups of four waves, beyond that a wave takes track t, t + n_waves, ...  The longest track of the other tests has
24 members and their largest track count is 5,209, so both loops ran once.

  * long_scene(): 130 frames x 8 records, record r of frame f on record (r + 1) mod 8 of frame f + 1, the pairs in
    descending order; the eight paths are cut so that the track lengths are 130, 129, 128, 67, 66, 65 (three times),
    64 (three times), 63 (twice), 3 and 2.  The order in which the members arrive behind a track's offset is the
    device's own affair; the bytes of d_obs must not depend on it, so two runs are compared.
  * many_scene(): 3 frames x 17,000 records, a random permutation as the first pair's matches and another, half of its
    rows empty, as the second pair's: 17,000 tracks of length 2 and 3 for 16,384 waves.  The offsets of the second turn
    are then no multiple of anything.  The plan (order_blocks) is restated here and the premise asserted from the model.
  * The tracks of long_scene() over 130 cameras on an arc, against tracks_model.triangulate_model at the project's
    bar for fp64 against a numpy restatement, 1e-9 * max(1, |value|).  Measured on an MI355X: largest deviation 0 on
    every one of the 15 tracks -- the header pins the order of the expressions, the library is built without
    contraction, and 130 accumulated views then give the model's bits; no third reference was needed.

Every device run of cusift_build_tracks must equal tests/tracks_model.py in all four outputs.

Tried once in a scratch build that was never committed (both edits stay in bounds and terminate):
  * the lane loop as a single pass, `if (lane < len)` with e = lane: test_every_output_equals_the_model[long] fails,
    203 of the 1,038 entries of d_obs never written -- the members past the 64th of the eight tracks longer than a wave;
  * the track loop as a single pass, `if (t < n_tracks)`: test_every_output_equals_the_model[many] fails, the 1,537
    observations of tracks 16,384 .. 16,999 never written.
Either way every other track test stays green (tests/test_tracks.py, test_tracks_sizes.py, test_tracks_batch.py,
test_tracks_probe.py): nothing else reaches the second turn of either loop.
"""
import numpy as np
import pytest

from oracle_binding import SIFT_POINT_DTYPE
from tracks_model import ROW, assert_tracks_equal, build_tracks_model, device_build_tracks, six_camera_scene, triangulate_model

OPTS = dict(rule=1, lo=0.8, hi=0.9, min_views=2)
LONG_N, LONG_PTS = 130, 8
# path -> the frames behind which it is cut: lengths c + 1 and 129 - c for one cut at c
CUTS = {1: (128,), 2: (127,), 3: (64,), 4: (63,), 5: (62,), 6: (0, 65), 7: (62, 126)}
LONG_LENGTHS = sorted([130, 129, 128, 2, 65, 65, 64, 66, 63, 67, 65, 64, 63, 64, 3])
MANY_PTS = 17000


def blank_rows(n_pairs, max_pts):
    rows = np.zeros((n_pairs, max_pts), ROW)
    rows["score"], rows["ambiguity"], rows["match"] = 0.5, 0.5, -1
    return rows


def long_scene():
    """Path r is record (r + f) mod 8 of frame f.  A cut behind frame c takes the row of pair (c, c + 1) away."""
    pairs = np.array([(f, f + 1) for f in range(LONG_N - 2, -1, -1)], np.int32)
    rows = blank_rows(len(pairs), LONG_PTS)
    rows["match"][:] = (np.arange(LONG_PTS, dtype=np.int32) + 1) % LONG_PTS
    for path, cuts in CUTS.items():
        for c in cuts:
            p = LONG_N - 2 - c
            assert tuple(pairs[p]) == (c, c + 1)
            rows["match"][p, (path + c) % LONG_PTS] = -1
    return pairs, rows


def many_scene():
    rng = np.random.default_rng(9)
    pairs = np.array([(0, 1), (1, 2)], np.int32)
    rows = blank_rows(2, MANY_PTS)
    rows["match"][0] = rng.permutation(MANY_PTS)
    rows["match"][1] = np.where(rng.random(MANY_PTS) < 0.5, rng.permutation(MANY_PTS), -1)
    return pairs, rows


def order_plan(n_images, max_pts):
    """(workgroups, waves) of the tracks_order_kernel launch."""
    n = n_images * max_pts
    order_blocks = max(1, min(4096, -(-(n // 2) // 4)))
    return order_blocks, 4 * order_blocks


@pytest.fixture(scope="module")
def models():
    out = {}
    for name, make, n, m in (("long", long_scene, LONG_N, LONG_PTS), ("many", many_scene, 3, MANY_PTS)):
        pairs, rows = make()
        out[name] = (n, m, pairs, rows, build_tracks_model([m] * n, m, pairs, rows, **OPTS))
    return out


def test_the_scene_has_tracks_longer_than_a_wave(models):
    n, m, pairs, rows, (track, offsets, obs, stats) = models["long"]
    lengths = np.diff(offsets).tolist()
    blocks, waves = order_plan(n, m)
    print("long: %d tracks of lengths %s; order_blocks %d, %d waves" % (stats[0], lengths, blocks, waves))
    assert sorted(lengths) == LONG_LENGTHS and {63, 64, 65, 128, 129, 130} <= set(lengths)
    assert stats[3] == 0 and stats[4] == 0 and stats[0] == len(LONG_LENGTHS) <= waves
    assert stats[1] == sum(LONG_LENGTHS) == n * m - 2  # two nodes are left alone: path 1's last, path 6's first
    # lane e + 64 exists for most tracks, lane e + 128 for two; 63 and 64 stay inside one pass
    assert sum(k > 64 for k in lengths) >= 8 and sum(k > 128 for k in lengths) == 2 and 128 in lengths
    # a track's members lie in consecutive frames, at the records of its path
    for t in range(stats[0]):
        nodes = obs[offsets[t]:offsets[t + 1]]
        assert (np.diff(nodes // m) == 1).all() and len({(v % m - v // m) % m for v in nodes.tolist()}) == 1


def test_the_scene_has_more_tracks_than_waves(models):
    n, m, pairs, rows, (track, offsets, obs, stats) = models["many"]
    blocks, waves = order_plan(n, m)
    lengths = np.diff(offsets)
    print("many: %d tracks (%d of length 2, %d of length 3), %d observations; order_blocks %d, %d waves"
          % (stats[0], (lengths == 2).sum(), (lengths == 3).sum(), stats[1], blocks, waves))
    assert blocks == 4096 and waves == 16384  # the cap
    assert stats[0] == MANY_PTS > 4 * blocks and stats[3] == 0
    assert set(lengths.tolist()) == {2, 3} and min((lengths == 2).sum(), (lengths == 3).sum()) > 8000
    # the second turn starts at an offset that is no multiple of a length, and both lengths occur in it
    assert offsets[waves] % 2 == 1 or offsets[waves] % 3 != 0
    assert set(lengths[waves:].tolist()) == {2, 3}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["long", "many"])
def test_every_output_equals_the_model(ctx, models, name):
    n, m, pairs, rows, model = models[name]
    first = device_build_tracks(ctx, None, n, m, pairs, rows, **OPTS)
    assert_tracks_equal(first, model)
    second = device_build_tracks(ctx, None, n, m, pairs, rows, **OPTS)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()


def long_views():
    """The tracks of long_scene() over 130 cameras: path r is scene point r.  -> (poses, records, camera values)."""
    poses, planted, pixels, cam = six_camera_scene(LONG_PTS, seed=33, n_cams=LONG_N)
    recs = np.zeros((LONG_N, LONG_PTS), SIFT_POINT_DTYPE)
    for f in range(LONG_N):
        recs["coords2D"][f, (np.arange(LONG_PTS) + f) % LONG_PTS] = pixels[f]
    return poses, recs, cam


def test_the_long_tracks_triangulate_to_the_planted_points(models):
    """The model on the 130-camera scene: every track is found where its point was planted, the short ones (two and
    three neighbouring cameras, 1 / 129 rad apart) included."""
    n, m, pairs, rows, (track, offsets, obs, stats) = models["long"]
    poses, recs, (fx, fy, cx, cy) = long_views()
    planted = six_camera_scene(LONG_PTS, seed=33, n_cams=LONG_N)[1]
    out, front = triangulate_model(recs["coords2D"], m, offsets, obs, poses, fx, fy, cx, cy)
    path = np.array([(int(obs[offsets[t]]) % m - int(obs[offsets[t]]) // m) % m for t in range(stats[0])])
    lengths = np.diff(offsets)
    assert (front == lengths).all() and (out[:, 3] < 1e-3).all() and (out[:, 3] > 0).all()
    long_ones = lengths >= 63
    assert np.abs(out[long_ones, :3] - planted[path[long_ones]]).max() < 1e-4
    assert np.abs(out[:, :3] - planted[path]).max() < 0.05


@pytest.mark.gpu
def test_long_tracks_through_triangulation(ctx, models):
    from cusift_amd import capi
    from test_triangulate_tracks import FILL, Device

    n, m, pairs, rows, (track, offsets, obs, stats) = models["long"]
    poses, recs, (fx, fy, cx, cy) = long_views()
    want, want_front = triangulate_model(recs["coords2D"], m, offsets, obs, poses, fx, fy, cx, cy)
    T = int(stats[0])
    cap = T + 3
    dev = Device(ctx, recs, offsets, obs, T, cap)
    try:
        d_recs, d_offsets, d_obs, d_stats, d_out, d_front = dev.ptrs
        ctx.triangulate_tracks(d_recs, n, m, d_offsets, d_obs, d_stats, cap, poses, capi.Camera(fx, fy, cx, cy), d_out,
                               d_front)
        out, front = dev.read()
        dev_err = np.abs(out[:T] - want) / np.maximum(1.0, np.abs(want))
        print("triangulate_tracks over tracks of up to 130 views against the numpy model: largest deviation %.3g "
              "(bar 1e-9), per track %s" % (dev_err.max(), ["%.1e" % e for e in dev_err.max(axis=1)]))
        assert dev_err.max() <= 1e-9
        np.testing.assert_array_equal(front[:T], want_front)
        assert (want_front == np.diff(offsets)).all()
        assert (out[T:] == FILL).all() and (front[T:] == int(FILL)).all()
    finally:
        dev.close()
