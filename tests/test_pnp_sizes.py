"""cusift_estimate_pnp where tests/test_pnp.py's 400 records cannot reach: 6,500 candidates among 66,000 records at 4,096
loops.  The marking then has 258 workgroups, so planar_compact_kernel's walk over the block counts takes a second step,
and a scoring split holds several 64-candidate tiles with a ragged one that is not its first (on 256 CUs: 32 splits of
2,112; three full splits of 33 tiles, a fourth with 2 tiles + 36 candidates, 28 empty).  The premise is asserted with the
device's own CU count, planned with score_splits' arithmetic at the arguments of pnp_launch's call site, which
tests/test_register_source.py pins.  The check is DEVICE = MODEL of tests/test_pnp.py."""
import functools

import numpy as np
import pytest

from oracle_binding import SIFT_POINT_DTYPE
from test_pnp import CAM, H, RULE, W, about_y, check_device_equals_model, frustum, pnp_candidates, project, run
from test_ransac_sizes import device_cus, score_plan, several_tiles, split_tiles
from test_register_source import PNP as PLAN  # (per_cu, tile, round_to_tile) of pnp_launch's call of score_splits

N, N_IN, N_OUT, LOOPS, SEED = 66000, 3500, 3000, 4096, 1


@functools.lru_cache(maxsize=None)
def big_scene():
    """66,000 records: 3,500 planted and 3,000 outliers carry a depth, spread over the whole record range; the other 59,500
    carry coords3D = 0 (most) or fail the score rule."""
    rng = np.random.default_rng(N)
    R21 = about_y(0.05)
    t21 = -R21 @ np.array([0.4, 0.03, 0.1])
    X1, x2 = np.zeros((0, 3)), np.zeros((0, 2))
    while len(X1) < N_IN:
        X = frustum(rng, 2 * N_IN, (2.0, 6.0))
        X2 = X @ R21.T + t21
        b = project(X2, CAM)
        ok = (X2[:, 2] > 0.1) & ((b >= 0) & (b < [W, H])).all(axis=1)
        X1, x2 = np.r_[X1, X[ok]], np.r_[x2, b[ok]]
    X1, x2 = X1[:N_IN], x2[:N_IN] + rng.normal(0, 0.3, size=(N_IN, 2))
    pts = np.zeros(N, dtype=SIFT_POINT_DTYPE)
    pts["coords2D"] = rng.uniform([0, 0], [W, H], size=(N, 2)).astype(np.float32)
    pts["match_xpos"], pts["match_ypos"] = rng.uniform([0, 0], [W, H], size=(N, 2)).astype(np.float32).T
    pts["score"], pts["ambiguity"] = 0.9, 0.5
    pts["match"] = rng.integers(0, 500, N).astype(np.int32)
    pts["match_error"] = 7.0
    where = rng.permutation(N)
    a, b, c = where[:N_IN], where[N_IN:N_IN + N_OUT], where[N_IN + N_OUT:]
    pts["coords3D"][a] = X1.astype(np.float32)
    pts["match_xpos"][a], pts["match_ypos"][a] = x2[:, 0].astype(np.float32), x2[:, 1].astype(np.float32)
    pts["coords3D"][b] = frustum(rng, N_OUT, (2.0, 6.0)).astype(np.float32)
    pts["coords3D"][c[::7]] = frustum(rng, len(c[::7]), (2.0, 6.0)).astype(np.float32)  # a depth, but a score that fails
    pts["score"][c[::7]] = 0.5
    pts.setflags(write=False)
    return pts


def test_the_scene_has_6500_candidates_spread_over_258_blocks():
    pts = big_scene()
    cand = pnp_candidates(pts, **RULE)
    assert len(cand) == N_IN + N_OUT == 6500 and -(-N // 256) == 258
    assert cand[0] < 256 and cand[-1] >= 257 * 256  # the first and the last marking workgroup both keep some
    grid_y, per_split = score_plan(N, LOOPS // 64, *PLAN, 256)
    tiles = split_tiles(len(cand), grid_y, per_split, 64)
    assert (grid_y, per_split) == (32, 2112) and several_tiles(tiles, 64)
    assert [len(t) for t in tiles[:5]] == [33, 33, 33, 3, 0] and tiles[3][-1] == 36


@pytest.mark.gpu
def test_device_equals_model_with_several_tiles_per_split_and_258_marking_blocks(ctx):
    pts = big_scene()
    cand = pnp_candidates(pts, **RULE)
    grid_y, per_split = score_plan(N, LOOPS // 64, *PLAN, device_cus())
    tiles = split_tiles(len(cand), grid_y, per_split, 64)
    print("%d CUs: %d splits of %d; tiles per live split %s" % (device_cus(), grid_y, per_split, [len(t) for t in tiles if t]))
    assert several_tiles(tiles, 64)
    res, after = run(ctx, pts, CAM, loops=LOOPS, seed=SEED, **RULE)
    assert check_device_equals_model(res, after, pts, CAM, LOOPS, SEED, "66,000 records")
    assert res.num_fit >= 0.97 * N_IN
