"""cusift_build_tracks at the shape where the linking kernel can go wrong, not the workload's: 24 frames x 4,096 records
and the pairs of a window of 3 give 66 x 16 = 1,056 workgroups that hook into shared components from every XCD at once.
Both scenes must equal tests/tracks_model.py exactly, and two calls must give the same bytes."""
import numpy as np
import pytest

from tracks_model import ROW, assert_tracks_equal, build_tracks_model, device_build_tracks

N, MAX_PTS, WINDOW = 24, 4096, 3
PAIRS = np.array([(i, j) for i in range(N) for j in range(i + 1, min(i + WINDOW, N - 1) + 1)], np.int32)
OPTS = dict(rule=1, lo=0.8, hi=0.9, min_views=2)


def blank_rows(n_pairs):
    rows = np.zeros((n_pairs, MAX_PTS), ROW)
    rows["score"], rows["ambiguity"], rows["match"] = 0.5, 0.5, -1
    return rows


def planted_scene():
    """Tracks as random one-record-per-frame subsets: track k is record perm[f][k] of every frame f of its subset, and
    every pair of the list that joins two of its frames has the row.  Then 5 % of all rows point somewhere else."""
    rng = np.random.default_rng(5)
    perm = np.stack([rng.permutation(MAX_PTS) for _ in range(N)])
    member = rng.random((N, MAX_PTS)) < 0.5  # [frame, track]
    rows = blank_rows(len(PAIRS))
    for p, (a, b) in enumerate(PAIRS):
        both = np.flatnonzero(member[a] & member[b])
        rows["match"][p, perm[a][both]] = perm[b][both]
    junk = rng.random(rows.shape) < 0.05
    rows["match"][junk] = rng.integers(0, MAX_PTS, size=int(junk.sum()))
    return PAIRS, rows


def path_scene():
    """Every record index is a path through all 24 frames, record r of frame f onto record (r + 1) mod max_pts of frame
    f + 1, with the pairs listed in descending order: the last pair's hooks meet the longest chains."""
    pairs = np.array([(f, f + 1) for f in range(N - 2, -1, -1)], np.int32)
    rows = blank_rows(len(pairs))
    rows["match"][:] = (np.arange(MAX_PTS, dtype=np.int32) + 1) % MAX_PTS
    return pairs, rows


@pytest.fixture(scope="module")
def models():
    out = {}
    for name, make in (("planted", planted_scene), ("path", path_scene)):
        pairs, rows = make()
        out[name] = (pairs, rows, build_tracks_model([MAX_PTS] * N, MAX_PTS, pairs, rows, **OPTS))
    return out


def test_the_scenes_are_what_they_claim(models):
    track, offsets, obs, stats = models["planted"][2]
    assert len(PAIRS) == 66
    assert stats[0] > 2000 and stats[3] > 100 and stats[2] > 60000, stats  # tracks, glued components, accepted rows
    assert np.diff(offsets).max() >= 12
    track, offsets, obs, stats = models["path"][2]
    assert stats[0] == MAX_PTS and (np.diff(offsets) == N).all() and stats[3] == 0 and stats[2] == (N - 1) * MAX_PTS


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["planted", "path"])
def test_many_workgroups_hook_into_shared_components(ctx, models, name):
    pairs, rows, model = models[name]
    first = device_build_tracks(ctx, None, N, MAX_PTS, pairs, rows, **OPTS)
    assert_tracks_equal(first, model)
    second = device_build_tracks(ctx, None, N, MAX_PTS, pairs, rows, **OPTS)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()
