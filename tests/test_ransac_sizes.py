"""The registration kernels at the sizes where their loops turn more than once.

Every other registration test is strict -- exact counts, byte-for-byte routes, float64 models -- but small: on a part
with 256 CUs the scoring launches they produce give every workgroup ONE tile of points (test_the_table_... below restates
that; the only exceptions are tests/test_planar.py's largest size and the nine-pair list of tests/test_planar_batch.py,
both in planar_score_kernel), their markings have at most 128 workgroups and their selections 4.  This file runs the same
models and the same assertions, imported from those tests, at the sizes the profiles describe:

  * score_splits (cusift_amd/csrc/sift_register.hip) cuts a scoring launch's points into grid.y splits; a workgroup then
    walks its split tile by tile.  The second trip round that loop is where epipolar_score_kernel, rigid_score_kernel and
    planar_score_kernel can be wrong: the barrier in front of the staging, the length of a ragged tile that is not the
    first, rigid tile starts that are no multiple of 256, a split that straddles the device-side count.
  * planar_compact_kernel and match_select_write_kernel add up the keeps of the workgroups before theirs in a loop of
    stride 256, which turns twice only from workgroup 257 on: 65,792 records.  pose_vote_kernel's atomic adds meet from
    as many workgroups.

The plans are restated here in Python (score_plan, split_tiles) and every GPU test first asserts, with the device's own
CU count, that its launch has a split of several tiles and a ragged tile that is not the first of its split -- a test fails
if its premise does not hold, it never passes vacuously on another part.  Each prints its plan: splits, points per split,
the tile lengths of the first, the straddling and the last split.

What the sizes are for, tried once in a scratch build that was never committed and otherwise reasoned on paper:
  * rigid_score_kernel's workgroup is four waves.  Without the __syncthreads() at the top of its tile loop a fast wave
    stages the next tile while a slow one still counts the previous: every other test of the suite stays green on 256 CUs
    (one tile per split: that barrier guards nothing), item 3 here fails -- both types, tried.  Items 4 and 6 compare two
    routes over scenes in which nearly every pair is an inlier and did not notice it; they are about the count.
  * epipolar_score_kernel and planar_score_kernel run ONE wave per workgroup, so that barrier orders nothing between
    waves there and no test can be expected to miss it; what items 1, 2 and 6 pin in them is the tile arithmetic.
  * kTile written for min(kTile, end - tile): elsewhere `end - tile` is only ever the first tile's length; here the ragged
    tile that is not the first counts stale or foreign points and moves the exact counts of items 1 to 3 (on paper).
  * the `before` loop as a single `if (tx < blockIdx.x)`: no other marking has more than 256 workgroups; here the base
    of the last workgroup, number 257 counting from 0, loses the keeps of workgroup 256, and items 2 and 5 fail (tried:
    4,985 candidates for 5,003).

Not to be confused with tests/test_epipolar_edges.py::test_loop_counts_beside_the_tile: the tile there is the HYPOTHESIS
tile (64 loops per workgroup, blockIdx.x); the tile here is the CANDIDATE tile a workgroup stages in LDS (blockIdx.y's
split, walked 64 or 256 points at a time).

CPU cost: the float64 recount of item 3 (16,384 hypotheses x 9,000 points, twice: 3-D and planar type) is the one slow
part of the file, about 25 s each; everything else takes a few seconds.
"""
import functools
import os
import time

import numpy as np
import pytest

import test_planar_batch as tpb
import test_rgbd_batch as tgb
from oracle_binding import SIFT_POINT_DTYPE, read_vlfeat_sift
from test_epipolar import (CX, CY, F_PIX, REFINE_LOOPS, THRESH, cameras, conditioned, coords, inliers, match_error, refit,
                           sample8, scene)
from test_epipolar import run as run_epipolar
from test_match_mutual import expected_selection
from test_planar import RULE_ARGS, candidates, upload
from test_pose import DIR_BOUND, ROT_BOUND, STALE, Case, camera, check_against_model, pose_model, stale, truth_errors
from test_register_source import EPI, PLANAR, RIGID  # score_splits' arguments, held to the call sites there
from test_rgbd import lift, other_bytes, select_numpy
from test_rigid import THRESH2, U, beta_of, check_flags, check_scoring, errors2, horn, hypotheses, planted, rot_dist, trans_dist
from test_rigid import scene as rigid_scene
from test_rigid import triples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

CU_COUNTS = (32, 64, 128, 256, 304)


# ------------------------------------------------------------------------------------------------------------------
# item 0: the plan, restated
# ------------------------------------------------------------------------------------------------------------------
def idiv_up(a, b):
    return -(-a // b)


def score_plan(num_pts, wgs, per_cu, tile, round_to_tile, num_cus):
    """score_splits of sift_register.hip: (grid.y, points per split) of a scoring launch over num_pts points (a capacity
    where the count stays on the device) that has `wgs` workgroups before splitting."""
    target = idiv_up(per_cu * num_cus, wgs)
    splits = max(1, min(target, idiv_up(num_pts, tile), 65535))
    per_split = idiv_up(idiv_up(num_pts, splits), tile) * tile if round_to_tile else idiv_up(num_pts, splits)
    return idiv_up(num_pts, per_split), per_split


def split_tiles(count, grid_y, per_split, tile):
    """The tile lengths every split's workgroup walks when `count` points are live: the kernels' `end = min(count, begin +
    per_split)` and `n = min(tile, end - tile_start)`.  An empty list is a split that adds nothing."""
    out = []
    for y in range(grid_y):
        begin = y * per_split
        n = max(0, min(count, begin + per_split) - begin)
        out.append([min(tile, n - s) for s in range(0, n, tile)])
    return out


def brief(tiles):
    if not tiles:
        return "empty"
    full = sum(1 for t in tiles if t == tiles[0])
    return "%d x %d" % (full, tiles[0]) + "".join(" + %d" % t for t in tiles[full:])


def describe(label, num_pts, count, wgs, params, num_cus):
    """Prints the plan of one launch and returns (grid.y, per_split, tiles per split)."""
    per_cu, tile, rounded = params
    grid_y, per_split = score_plan(num_pts, wgs, per_cu, tile, rounded, num_cus)
    tiles = split_tiles(count, grid_y, per_split, tile)
    live = [y for y, t in enumerate(tiles) if t]
    straddling = [y for y in live if sum(tiles[y]) < min(per_split, num_pts - y * per_split)]
    print("%s on %d CUs: capacity %d, %d live, %d workgroups before splitting -> %d splits of %d; first split %s; "
          "straddling split %s; last live split %s; %d empty" %
          (label, num_cus, num_pts, count, wgs, grid_y, per_split, brief(tiles[0]),
           ("%d: " % straddling[0] + brief(tiles[straddling[0]])) if straddling else "none",
           ("%d: " % live[-1] + brief(tiles[live[-1]])) if live else "none", grid_y - len(live)))
    return grid_y, per_split, tiles


def several_tiles(tiles, tile):
    """The premise of every size in this file: some split has at least two tiles, and some tile that is not the first of its
    split is ragged."""
    return max(len(t) for t in tiles) >= 2 and any(n < tile for t in tiles for n in t[1:])


def device_cus():
    """The CU count the library plans with: sift_context.hip reads the same attribute."""
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def premise(label, num_pts, count, wgs, params, at_least=2):
    """Asserts a GPU test's premise with the device's own CU count; returns (grid.y, per_split, tiles)."""
    cus = device_cus()
    grid_y, per_split, tiles = describe(label, num_pts, count, wgs, params, cus)
    assert several_tiles(tiles, params[1]), (label, cus, grid_y, per_split)
    assert max(len(t) for t in tiles) >= at_least, (label, cus, grid_y, per_split)
    return grid_y, per_split, tiles


# ------------------------------------------------------------------------------------------------------------------
# the sizes
# ------------------------------------------------------------------------------------------------------------------
LOOPS_EPI, LOOPS_RIGID = 4096, 16384
SEEDS1 = (1, 0xC0FFEE)            # item 1; both rechecked with the model alone (test_model_meets_the_caps_...)
N1_IN, N1_OUT = 4000, 2500        # item 1: 6,500 records, every one a candidate
N2_IN, N2_OUT, N2 = 3500, 62500, 66000  # item 2: 258 marking workgroups
# Item 2's generator seed and RANSAC seed, chosen like SCENE_SEEDS of tests/test_epipolar.py with the model alone: the
# first pair tried served (no near-threshold candidate, recall 0.999), and the CPU test rechecks it.
SCENE2_SEED, SEED2 = 66000, 1
N_CAND2 = 5003                    # 78 * 64 + 11: inside the third split of 2,112 on 256 CUs
LATE = 65792                      # 257 * 256: from here on the `before` loops of the compactions turn twice
N3_IN, N3_OUT = 6000, 3000        # item 3: 9,000 points
N4_A, N4_B = 9000, 7000           # item 4: the fused call's capacity and the records of frame 2
N6 = (4096, 3500, 4000)           # item 6: three frames in slots of 4,096
PAIRS6 = np.array([(0, 1), (1, 2), (0, 2), (2, 0)], np.int32)
N5 = 66000                        # item 5: records on either side of the selection


@functools.lru_cache(maxsize=None)
def few_candidates():
    """Item 2: (records, planted mask, block keeps [258]).  scene(3500, 62500) with the scores rewritten so that the
    candidates under RULE_ARGS[0] are: every planted record outside [512, 1024); every record of [0, 512) -- two marking
    workgroups with 256 keeps; none of [512, 1024) -- two with none; the last record; and as many further outliers, by a
    seeded draw, as make N_CAND2 in all (about 1,500 outliers with those of the first two blocks).  Two more outliers
    past record 65,792 pass by score and are no candidates: one has a NaN coordinate, one an infinite match position, as
    subset_scores of tests/test_planar.py places them."""
    base, mask = scene(N2_IN, N2_OUT, seed=SCENE2_SEED)
    n = len(base)
    keep = mask.copy()
    keep[:512], keep[512:1024], keep[n - 1] = True, False, True
    free = np.flatnonzero(~mask)
    free = free[(free >= 1024) & (free < n - 1)]
    late = free[free > LATE][:2]
    assert len(late) == 2
    rng = np.random.default_rng(2)
    keep[rng.choice(np.setdiff1d(free, late), N_CAND2 - int(keep.sum()), replace=False)] = True
    blocks = np.add.reduceat(keep.astype(np.int64), np.arange(0, n, 256))
    keep[late] = True
    pts = base.copy()
    pts["score"] = np.where(keep, 0.9, 0.3).astype(np.float32)
    pts["coords2D"][late[0], 1] = np.nan
    pts["match_xpos"][late[1]] = np.inf
    pts.setflags(write=False)
    return pts, mask, blocks


@functools.lru_cache(maxsize=None)
def rigid_case(kind):
    """Item 3: (coord [9000, 6], idx [16384, 3]); the planar type moves about y as test_two_point_planar_type does."""
    if kind == "3d":
        coord = rigid_scene(N3_IN, N3_OUT, seed=N3_IN + LOOPS_RIGID)
    else:
        R, t = planted(axis=(0, 1, 0), angle=0.35, t=(0.12, 0.0, 0.2))
        coord = rigid_scene(N3_IN, N3_OUT, seed=N3_IN + LOOPS_RIGID, R=R, t=t)
    return coord, triples(N3_IN + N3_OUT, LOOPS_RIGID, seed=3007)


def template():
    return read_vlfeat_sift(os.path.join(GOLDEN, "vlfeat_sift1.bin"))


def slots(frames, max_pts, **fields):
    """frames in max_pts slots as the FrameBatch classes lay them out: records past a count are live-looking copies with
    valid pixels, so that a stage that ignores a count shows; the match fields carry values no stage produces."""
    points = np.zeros((len(frames), max_pts), SIFT_POINT_DTYPE)
    points[:] = np.resize(frames[0], max_pts)
    points["coords2D"] = 17.0
    for k, f in enumerate(frames):
        points[k, :len(f)] = f
    points["score"], points["ambiguity"], points["match"] = 0.25, 0.5, -5
    for name, value in fields.items():
        points[name] = value
    return points


class PlanarFrames(tpb.FrameBatch):
    """Item 6: planted_frames' pair with 4,096 and 3,500 records and a third frame, 4,000 of frame 0's points under a
    second homography, with frame 0's descriptors plus 1 % noise like frame 1's -- three frames in slots of 4,096."""

    def __init__(self):
        fa, fb, self.seen, self.H = tpb.planted_frames(template(), n_a=N6[0], n_b=N6[1], n_planted=2800)
        r = np.random.default_rng(17)
        H2 = np.array([[1.02, 0.05, -22.0], [-0.06, 0.98, 14.0], [-1.5e-5, 2.1e-5, 1.0]])
        seen = r.permutation(N6[0])[:N6[2]]
        fc = fa[seen].copy()
        fc["coords2D"] = (tpb.apply(H2, fa["coords2D"][seen].astype(np.float64)) + r.normal(0, 0.3, (N6[2], 2))).astype(np.float32)
        d = fa["data"][seen] + r.normal(0, 0.01 / np.sqrt(128), (N6[2], 128)).astype(np.float32)
        fc["data"] = (d / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
        self.points = slots([fa, fb, fc], N6[0], match_xpos=-3.0, match_ypos=-4.0, match_error=7.0)
        self.n = np.array(N6)
        self.counters = self.n.astype(np.uint32)


class RgbdFrames(tgb.FrameBatch):
    """Item 6: synthetic_frames' pair with 4,096 and 3,500 records and its third frame, 4,000 of frame 0's points moved once
    more, each with its depth image -- three frames in slots of 4,096."""

    def __init__(self):
        fa, fb, da, db, self.seen, self.motion, fc, dc, _, _ = tgb.synthetic_frames(template(), n_a=N6[0], n_b=N6[1],
                                                                                    n_c=N6[2])
        self.points = slots([fa, fb, fc], N6[0], coords3D=7.0)
        self.n = np.array(N6)
        self.counters = self.n.astype(np.uint32)
        self.depth = np.stack([da, db, dc])


@functools.lru_cache(maxsize=None)
def selection_records():
    """Item 5: (r1, r2, forced rows) -- 66,000 records a side with score, ambiguity, match and coords3D by a seeded draw.
    About half pass the thresholds (1.0, 0.8); match is a permutation of frame 2 with -1, n2 and n2 + 5 on 300 records;
    z == 0 on about a quarter of either side; about half of the partners name their record back.  Records [0, 512) and
    the last are kept under every call and kind (two workgroups with 256 keeps), none of [512, 1024) passes."""
    rng = np.random.default_rng(5)
    n1 = n2 = N5
    r1, r2 = np.zeros(n1, SIFT_POINT_DTYPE), np.zeros(n2, SIFT_POINT_DTYPE)
    forced = np.r_[np.arange(512), n1 - 1]
    passes = rng.random(n1) < 0.5
    passes[forced], passes[512:1024] = True, False
    r1["score"] = np.where(passes, 0.2, 2.0).astype(np.float32)
    amb = np.where(rng.random(n1) < 0.9, 0.3, 0.9)
    amb[forced] = 0.3
    r1["ambiguity"] = amb.astype(np.float32)
    match = rng.permutation(n2).astype(np.int32)
    odd = rng.choice(np.arange(1024, n1 - 1), 300, replace=False)
    match[odd[:100]], match[odd[100:200]], match[odd[200:]] = -1, n2, n2 + 5
    r1["match"] = match
    for r in (r1, r2):
        r["coords3D"] = rng.uniform(0.5, 4.0, (len(r), 3)).astype(np.float32)
        r["coords3D"][rng.random(len(r)) < 0.25, 2] = 0.0
    r1["coords3D"][forced, 2] = 1.5
    r2["coords3D"][match[forced], 2] = 2.5
    r2["match"] = rng.integers(0, n1, n2).astype(np.int32)
    back = rng.random(n1) < 0.5
    back[forced] = True
    back &= (match >= 0) & (match < n2)
    r2["match"][match[back]] = np.flatnonzero(back).astype(np.int32)
    r2["score"], r2["ambiguity"] = rng.random(n2).astype(np.float32), rng.random(n2).astype(np.float32)
    r1.setflags(write=False)
    r2.setflags(write=False)
    return r1, r2, forced


SELECT = (1.0, 0.8)  # score and ambiguity thresholds of item 5 (the rule squares them)


def selection(r1, r2, three_d, mutual):
    """select_numpy of tests/test_rgbd.py extended by the cross-check: (pairs int32 [k, 2], coord float32 [k, 6])."""
    idx, m = select_numpy(r1, r2, SELECT[0], SELECT[1], three_d)
    if mutual:
        ok = r2["match"][m] == idx
        idx, m = idx[ok], m[ok]
    return np.c_[idx, m].astype(np.int32), np.hstack([r1["coords3D"][idx], r2["coords3D"][m]]).astype(np.float32)


def wgs_of(loops, tile, n_pairs=1):
    return idiv_up(loops, tile) * n_pairs


# every scoring launch of this file as (label, capacity, live points, workgroups before splitting, call site).  The counts
# of items 4 and 6 (RGB-D) that only the device knows stand here with the value the frames are built for: every record of
# frame 2 finds its partner; the GPU tests assert their premise again with what the device reported.
LAUNCHES = [
    ("item 1 epipolar", N1_IN + N1_OUT, N1_IN + N1_OUT, wgs_of(LOOPS_EPI, 64), EPI),
    ("item 2 epipolar", N2, N_CAND2, wgs_of(LOOPS_EPI, 64), EPI),
    ("item 3 rigid", N3_IN + N3_OUT, N3_IN + N3_OUT, wgs_of(LOOPS_RIGID, 256), RIGID),
    ("item 4 rigid, fused", N4_A, N4_B, wgs_of(LOOPS_RIGID, 256), RIGID),
    ("item 6 planar batch", N6[0], N6[1], wgs_of(LOOPS_EPI, 64, len(PAIRS6)), PLANAR),
    ("item 6 rgbd batch", N6[0], N6[1], wgs_of(LOOPS_RIGID, 256, len(PAIRS6)), RIGID),
]


# ------------------------------------------------------------------------------------------------------------------
# without a GPU
# ------------------------------------------------------------------------------------------------------------------
def test_the_table_of_the_other_tests_plans_on_256_cus():
    """Not a claim about the code: the reason this file exists.  The largest epipolar and rigid cases of the other tests
    give one tile per split on 256 CUs, and so do the RGB-D batch and the eight-pair planar list; planar_score_kernel
    alone gets further, in tests/test_planar.py's largest size and -- two whole tiles, a ragged second one where a
    frame's count falls -- under the nine-pair list of tests/test_planar_batch.py."""
    def tiles_per_split(num_pts, count, wgs, params):
        return max(len(t) for t in describe("table", num_pts, count, wgs, params, 256)[2])

    assert score_plan(650, wgs_of(512, 64), *EPI, 256) == (11, 64)  # test_epipolar.py; _edges has 450 records, 256 loops
    assert tiles_per_split(650, 650, wgs_of(512, 64), EPI) == 1 and tiles_per_split(450, 450, wgs_of(256, 64), EPI) == 1
    assert score_plan(4000, wgs_of(4096, 256), *RIGID, 256) == (16, 250)  # test_rigid.py
    assert tiles_per_split(4000, 4000, wgs_of(4096, 256), RIGID) == 1
    assert score_plan(32768, wgs_of(10000, 64), *PLANAR, 256) == (14, 2368)  # test_planar.py SIZES[3]
    assert tiles_per_split(32768, 32768, wgs_of(10000, 64), PLANAR) == 37
    assert tiles_per_split(1024, 1024, wgs_of(1024, 256, 8), RIGID) == 1  # test_rgbd_batch.py: 8 pairs, 1,024 loops
    assert tiles_per_split(1024, 1024, wgs_of(1008, 64, 8), PLANAR) == 1  # test_planar_batch.py DEGENERATE
    assert score_plan(1024, wgs_of(1008, 64, 9), *PLANAR, 256) == (8, 128)  # test_planar_batch.py PAIRS
    # the profiled sizes: this path is the whole scoring there
    assert score_plan(32768, wgs_of(10000, 64), *EPI, 256) == (14, 2368)


def test_the_chosen_sizes_give_several_tiles_per_split_from_32_to_304_cus():
    """Every size of this file, on every CU count: a split with at least two tiles and a ragged tile that is not the first
    of its split (with fewer CUs the splits only get longer).  And the plans the GPU tests are expected to print."""
    for cus in CU_COUNTS:
        for label, num_pts, count, wgs, params in LAUNCHES:
            assert several_tiles(describe(label, num_pts, count, wgs, params, cus)[2], params[1]), (label, cus)
    plans = {label: score_plan(num_pts, wgs, *params, 256) for label, num_pts, _, wgs, params in LAUNCHES}
    assert plans == {"item 1 epipolar": (26, 256), "item 2 epipolar": (32, 2112), "item 3 rigid": (16, 563),
                     "item 4 rigid, fused": (16, 563), "item 6 planar batch": (8, 512), "item 6 rgbd batch": (4, 1024)}, plans
    tiles = {label: split_tiles(count, *score_plan(num_pts, wgs, *params, 256), params[1])
             for label, num_pts, count, wgs, params in LAUNCHES}
    assert tiles["item 1 epipolar"][0] == [64] * 4 and tiles["item 1 epipolar"][25] == [64, 36]
    assert tiles["item 2 epipolar"][:2] == [[64] * 33] * 2 and tiles["item 2 epipolar"][2] == [64] * 12 + [11]
    assert tiles["item 2 epipolar"][3:] == [[]] * 29
    assert tiles["item 3 rigid"][0] == [256, 256, 51] and sum(tiles["item 3 rigid"][15]) == 555
    assert tiles["item 6 planar batch"][0] == [64] * 8 and tiles["item 6 rgbd batch"][0] == [256] * 4
    # the pair calls item 6 compares with get other plans: 32 splits of 128, 16 splits of one tile
    assert score_plan(N6[0], wgs_of(LOOPS_EPI, 64), *PLANAR, 256) == (32, 128)
    assert score_plan(N6[0], wgs_of(LOOPS_RIGID, 256), *RIGID, 256) == (16, 256)
    # 64 loops over item 2's records: one tile per split, nearly all of them empty -- that run is about the compaction
    assert score_plan(N2, 1, *EPI, 256) == (1032, 64)
    assert {label: score_plan(n, w, *p, 304) for label, n, _, w, p in LAUNCHES[:3]} == {
        "item 1 epipolar": (34, 192), "item 2 epipolar": (37, 1792), "item 3 rigid": (19, 474)}


def test_item_2_has_its_candidates_where_the_plan_needs_them():
    pts, mask, blocks = few_candidates()
    cand = candidates(pts, 0, RULE_ARGS[0]["lo"], RULE_ARGS[0]["hi"])
    assert len(pts) == N2 and idiv_up(N2, 256) == 258 and mask.sum() == N2_IN
    assert len(cand) == N_CAND2 and N_CAND2 % 64 == 11 and N_CAND2 % 64 not in (0, 63)
    assert blocks.sum() == N_CAND2 and len(blocks) == 258
    assert blocks[:2].tolist() == [256, 256] and blocks[2:4].tolist() == [0, 0] and cand[-1] == N2 - 1
    assert (blocks[257:] > 0).all() and blocks[256] > 0  # workgroups 256 and 257 keep something: a base that forgot them shows
    passing = np.flatnonzero(pts["score"] > np.float32(0.85))
    spoiled = np.setdiff1d(passing, cand)
    assert len(spoiled) == 2 and (spoiled > LATE).all()  # the NaN coordinate and the infinite match position
    assert mask[cand].sum() == mask.sum() - mask[512:1024].sum() and 1400 <= (~mask[cand]).sum() <= 1600
    grid_y, per_split = score_plan(N2, wgs_of(LOOPS_EPI, 64), *EPI, 256)
    assert 2 * per_split < N_CAND2 < 3 * per_split and grid_y == 32  # inside the third split


MODEL = {}


def epipolar_model(item, seed):
    """The float64 model alone on item 1's or item 2's records: (share of the loops left out, best count, refit keeps, a
    candidate near the threshold, recall over the planted records)."""
    if (item, seed) not in MODEL:
        pts, mask = scene(N1_IN, N1_OUT) if item == 1 else few_candidates()[:2]
        cand = candidates(pts, 0, RULE_ARGS[0]["lo"], RULE_ARGS[0]["hi"])  # model_run of test_epipolar_edges.py, with
        xy = coords(pts, cand)                                               # the conditioning kept from its one solve
        F, ok = conditioned(pts, cand[sample8(seed, len(cand), LOOPS_EPI)])
        counts = np.array([inliers(F[:, l], xy, THRESH).sum() for l in range(LOOPS_EPI)])
        best = int(np.argmax(counts))
        fit, near = refit(F[:, best], xy, REFINE_LOOPS, THRESH)
        with np.errstate(all="ignore"):
            recall = float((match_error(fit, coords(pts))[mask] < THRESH).mean())
        MODEL[item, seed] = (1.0 - ok.mean(), int(counts[best]), int(inliers(fit, xy, THRESH).sum()), bool(near), recall)
    return MODEL[item, seed]


@pytest.mark.parametrize("item,seeds", [(1, SEEDS1), (2, (SEED2,))])
def test_model_meets_the_caps_the_epipolar_gpu_tests_rely_on(item, seeds):
    """The caps of tests/test_epipolar.py for its larger scenes, with the model alone: at most 3 % of the loops left out
    (the GPU tests allow 15 %), recall 0.995 (they ask 0.99), at most one seed of item 1 with a candidate within 1e-9 of
    the threshold, and none for item 2, which has one seed."""
    skipped = 0
    for seed in seeds:
        dropped, best, kept, near, recall = epipolar_model(item, seed)
        print("item %d seed %#x: %.2f %% of the loops left out, best loop counts %d, refit keeps %d, near %s, recall %.4f" %
              (item, seed, 100 * dropped, best, kept, near, recall))
        assert dropped <= 0.03 and recall >= 0.995 and best >= 0.5 * (N1_IN if item == 1 else N2_IN)
        skipped += near
    assert skipped <= (1 if item == 1 else 0)


def test_model_meets_the_caps_the_rigid_gpu_test_relies_on():
    """Float64 hypotheses cast to fp32 stand in for the device.  The solve cap over all 16,384 loops; the scoring cap over
    the first 2,048 of them (eight workgroups' worth: the whole recount is the GPU test's 25 s)."""
    coord, idx = rigid_case("3d")
    rt64, w = hypotheses(coord, idx, "3d")
    g = (w[:, 1] - w[:, 0]) / w[:, 3]
    print("item 3, model alone: %.2f %% of the loops left out by g < 1e-3" % (100 * (g < 1e-3).mean()))
    assert (g < 1e-3).mean() <= 0.01
    rt32 = rt64[:2048].astype(np.float32)
    counts = np.concatenate([(errors2(rt32[a:a + 256], coord)[0] < float(THRESH2)).sum(1) for a in range(0, 2048, 256)])
    check_scoring(coord, rt32, counts, THRESH2)  # prints the borderline share and asserts it <= 0.1 %
    assert counts.max() >= 0.99 * N3_IN


def test_vectorised_selection_equals_the_restatement_of_test_match_mutual():
    """The test of item 5's reference: numpy's selection over 66,000 records against expected_selection's loop, for the
    call and kind that use every predicate; and the fixed block layout under all four."""
    r1, r2, forced = selection_records()
    want_p, want_c = expected_selection(r1, r2, SELECT[0], SELECT[1], True, True)
    got_p, got_c = selection(r1, r2, True, True)
    assert got_p.tobytes() == want_p.tobytes() and got_c.tobytes() == want_c.tobytes()
    sizes = {}
    for three_d in (False, True):
        for mutual in (False, True):
            p, _ = selection(r1, r2, three_d, mutual)
            keep = np.zeros(N5, bool)
            keep[p[:, 0]] = True
            blocks = np.add.reduceat(keep.astype(np.int64), np.arange(0, N5, 256))
            assert blocks[:2].tolist() == [256, 256] and blocks[2:4].tolist() == [0, 0] and keep[N5 - 1]
            assert keep[forced].all() and blocks[256] > 0 and blocks[257] > 0 and len(blocks) == 258
            sizes[three_d, mutual] = len(p)
    print("item 5: kept", sizes)
    assert sizes[False, False] > sizes[True, False] > sizes[True, True] and sizes[False, False] > sizes[False, True]
    assert 0.4 * sizes[False, False] < sizes[False, True] < 0.6 * sizes[False, False]  # about half are mutual
    assert set(r1["match"][(r1["match"] < 0) | (r1["match"] >= N5)].tolist()) == {-1, N5, N5 + 5}


# ------------------------------------------------------------------------------------------------------------------
# on the GPU: items 1 and 2, epipolar
# ------------------------------------------------------------------------------------------------------------------
def check_epipolar(pts, mask, res, after, seed, loops, label):
    """What test_counts_flags_and_winner_..., test_hypotheses_equal_the_svd_model and test_refit_equals_the_model_... of
    tests/test_epipolar.py assert, on one run.  Returns True when the refit comparison was skipped for a candidate within
    a relative 1e-9 of the threshold."""
    cand = candidates(pts, 0, RULE_ARGS[0]["lo"], RULE_ARGS[0]["hi"])
    # counts, flags, winner: exactly, with the device's own matrices
    assert res.num_candidates == len(cand)
    assert np.array_equal(res.drawn, cand[sample8(seed, len(cand), loops)])  # through the candidate list
    xy = coords(pts, cand)
    counts = np.array([inliers(res.all_fundamentals[:, l], xy, THRESH).sum() for l in range(loops)], dtype=np.int32)
    bad = np.flatnonzero(res.all_counts != counts)
    assert len(bad) == 0, (label, len(bad), bad[:5], res.all_counts[bad[:5]], counts[bad[:5]])
    assert res.best_loop == int(np.argmax(counts)) and res.num_matches == counts.max()
    assert res.ransac.tobytes() == res.all_fundamentals[:, res.best_loop].tobytes()
    flags = np.zeros(len(pts), dtype=bool)
    flags[cand] = inliers(res.ransac, xy, THRESH)
    assert np.array_equal(res.inliers, flags) and res.inliers.sum() == res.num_matches
    assert not res.inliers[np.setdiff1d(np.arange(len(pts)), cand)].any()  # a record that is no candidate is no inlier
    assert res.num_matches >= 8 and res.num_matches >= 0.5 * mask[cand].sum()
    # hypotheses against the SVD model
    want, ok = conditioned(pts, res.drawn)
    assert 1.0 - ok.mean() <= 0.15, (label, 1.0 - ok.mean())
    diff = np.abs(res.all_fundamentals - want).max(axis=0)
    nz = res.all_fundamentals[:, res.all_fundamentals.any(axis=0)]
    assert np.isfinite(res.all_fundamentals).all() and nz.shape[1] >= ok.sum()
    norms = np.sqrt((nz * nz).sum(axis=0))
    dets = np.abs([np.linalg.det(nz[:, l].reshape(3, 3)) for l in range(nz.shape[1])])
    print("%s: %.2f %% of the loops left out, largest difference of the others %.3g; best loop %d counts %d of %d candidates" %
          (label, 100 * (1.0 - ok.mean()), diff[ok].max(), res.best_loop, res.num_matches, len(cand)))
    assert np.abs(norms - 1).max() <= 1e-12 and dets.max() <= 1e-12
    assert diff[ok].max() <= 1e-6, diff[ok].max()
    # the refit against the model's, started from the device's winner
    want, near = refit(res.ransac, xy, REFINE_LOOPS, THRESH)
    if near:
        return True
    assert float(np.abs(res.fundamental - want).max()) <= 1e-6
    with np.errstate(all="ignore"):
        err = match_error(res.fundamental, coords(pts))
    got = after["match_error"]
    assert (got != pts["match_error"]).all()  # written for every record
    fin = np.isfinite(err)
    assert np.array_equal(np.isfinite(got), fin) and (~fin).sum() == len(pts) - np.isfinite(np.c_[coords(pts)]).all(axis=1).sum()
    rel = float((np.abs(got[fin].astype(np.float64) - err[fin]) / err[fin]).max())
    recall = float((got[mask] < THRESH).mean())
    print("%s: refit differs by %.3g, match_error by %.3g relative, num_fit %d, recall %.4f" %
          (label, float(np.abs(res.fundamental - want).max()), rel, res.num_fit, recall))
    assert res.num_fit == inliers(res.fundamental, xy, THRESH).sum() == inliers(want, xy, THRESH).sum()
    assert rel <= 1e-5 and recall >= 0.99
    rest = after.copy()
    rest["match_error"] = pts["match_error"]
    assert rest.tobytes() == pts.tobytes()  # nothing else of the records moved
    return False


@pytest.mark.gpu
def test_epipolar_with_every_record_a_candidate_four_tiles_per_split(ctx):
    """Item 1.  6,500 candidates: on 256 CUs 26 splits of 256, four tiles each, the last split a tile of 64 and one of 36;
    the solve kernel's gather takes a second step for part of its grid (6,500 candidates against 4,096 threads)."""
    pts, mask = scene(N1_IN, N1_OUT)
    n = len(pts)
    grid_y, per_split, tiles = premise("item 1 epipolar", n, n, wgs_of(LOOPS_EPI, 64), EPI)
    assert n > LOOPS_EPI  # the gather's second step
    if device_cus() == 256:
        assert (grid_y, per_split) == (26, 256) and tiles[0] == [64] * 4 and tiles[25] == [64, 36]
    skipped = 0
    for seed in SEEDS1:
        res, after = run_epipolar(ctx, pts, loops=LOOPS_EPI, seed=seed, **RULE_ARGS[0])
        skipped += check_epipolar(pts, mask, res, after, seed, LOOPS_EPI, "item 1 seed %#x" % seed)
    assert skipped <= 1


RESULT2 = {}


def run_item_2(ctx):
    if not RESULT2:
        pts = few_candidates()[0]
        RESULT2["epi"] = run_epipolar(ctx, pts, loops=LOOPS_EPI, seed=SEED2, **RULE_ARGS[0])
    return RESULT2["epi"]


@pytest.mark.gpu
def test_compaction_past_256_workgroups_and_a_split_that_straddles_the_candidates(ctx):
    """Item 2.  66,000 records mark in 258 workgroups, 5,003 of them candidates: on 256 CUs 32 splits of 2,112 sized from
    the capacity, two of 33 full tiles, the third of 12 and a ragged one, 29 that add nothing."""
    pts, mask, blocks = few_candidates()
    grid_y, per_split, tiles = premise("item 2 epipolar", N2, N_CAND2, wgs_of(LOOPS_EPI, 64), EPI)
    assert idiv_up(N2, 256) > 257 and blocks[256] > 0 and blocks[257] > 0  # the `before` loop's second turn
    straddle = N_CAND2 // per_split
    assert N_CAND2 % per_split and len(tiles[straddle]) >= 2 and tiles[straddle][-1] == N_CAND2 % 64
    assert straddle + 1 < grid_y and not any(tiles[straddle + 1:])  # splits past the candidates
    if device_cus() == 256:
        assert (grid_y, per_split, straddle) == (32, 2112, 2) and [len(t) for t in tiles[:3]] == [33, 33, 13]
    res, after = run_item_2(ctx)
    assert not check_epipolar(pts, mask, res, after, SEED2, LOOPS_EPI, "item 2"), "pick another SEED2: near the threshold"
    cand = candidates(pts, 0, RULE_ARGS[0]["lo"], RULE_ARGS[0]["hi"])
    assert set(np.unique(res.drawn)) <= set(cand.tolist()) and res.drawn.max() > LATE


@pytest.mark.gpu
def test_compaction_past_256_workgroups_with_one_tile_per_split(ctx):
    """Item 2 at 64 loops: one workgroup before splitting, so as many splits as the capacity has tiles (1,032 on 256 CUs),
    nearly all of them past the candidates -- and the same compaction.  The counts only."""
    pts, _, _ = few_candidates()
    cus = device_cus()
    grid_y, per_split, tiles = describe("item 2, 64 loops", N2, N_CAND2, 1, EPI, cus)
    assert grid_y - sum(1 for t in tiles if t) > 0 and idiv_up(N2, 256) > 257
    res, _ = run_epipolar(ctx, pts, loops=64, seed=SEED2, **RULE_ARGS[0])
    cand = candidates(pts, 0, RULE_ARGS[0]["lo"], RULE_ARGS[0]["hi"])
    assert res.num_candidates == len(cand) and np.array_equal(res.drawn, cand[sample8(SEED2, len(cand), 64)])
    xy = coords(pts, cand)
    counts = np.array([inliers(res.all_fundamentals[:, l], xy, THRESH).sum() for l in range(64)], dtype=np.int32)
    assert np.array_equal(res.all_counts, counts)
    assert res.best_loop == int(np.argmax(counts)) and res.num_matches == counts.max()


@pytest.mark.gpu
def test_pose_votes_from_258_workgroups(ctx):
    """Item 2's pose: estimate_pose with the F of the 4,096-loop run on a fresh upload whose coords3D are stale -- the four
    votes are atomic adds from 258 workgroups."""
    pts, mask, _ = few_candidates()
    epi, _ = run_item_2(ctx)
    cam = (F_PIX, F_PIX, CX, CY, 0.0)
    assert max(idiv_up(N2, 256), 1) == 258
    before = stale(pts)
    buf = upload(ctx, before)
    pose = ctx.estimate_pose(buf.ptr, N2, epi.fundamental, camera(cam), camera(cam), thresh=THRESH, **RULE_ARGS[0])
    after = buf.to_numpy(SIFT_POINT_DTYPE, (N2,))
    buf.free()
    want = pose_model(epi.fundamental, pts, cam, cam)
    assert not want.near, "pick another SEED2: a record of the fit set is within 1e-9 of the threshold or of a zero depth"
    check_against_model(pose, after, want, before, "item 2")  # votes as a sorted multiset, the zero pattern exactly
    assert pose.votes.sum() == want.votes.sum() and pose.num_front <= epi.num_fit
    assert (after["coords3D"] != STALE).all()  # every one of the 66,000 records is written
    R, t, _ = cameras()
    r, d = truth_errors(pose.rt, Case(pts, mask, cam, cam, LOOPS_EPI, (SEED2,), R, t, None))
    print("item 2: rotation %.4f, direction %.4f degrees from the planted pose" % (r, d))
    assert r <= ROT_BOUND and d <= DIR_BOUND, (r, d)


# ------------------------------------------------------------------------------------------------------------------
# item 3: rigid scoring
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_rigid_scoring_three_tiles_per_split(ctx):
    """Item 3, items 2, 3 and 4 of test_scenes_scoring_solve_selection_and_refit at 9,000 points and 16,384 loops: on 256
    CUs 16 splits of 563 points, tiles of 256, 256 and 51 that start at multiples of 563.  SLOW ON THE CPU: the float64
    recount of 147 M residuals takes about 25 s; the device's share is milliseconds.  The comparison with the planted
    motion is left to the smaller scenes: it does not depend on the size and would recount everything once more."""
    coord, idx = rigid_case("3d")
    n_pts = len(coord)
    grid_y, per_split, tiles = premise("item 3 rigid", n_pts, n_pts, wgs_of(LOOPS_RIGID, 256), RIGID, at_least=3)
    assert per_split % 256  # tile starts that are no multiple of the tile
    if device_cus() == 256:
        assert (grid_y, per_split) == (16, 563) and tiles[0] == [256, 256, 51] and sum(tiles[15]) == 555
    before = idx.copy()
    rt, n, best, flags, all_rt, all_c, drawn = ctx.estimate_rigid(coord, idx, thresh2=THRESH2, kind="3d", want_all=True)
    assert np.array_equal(idx, before) and np.array_equal(drawn, idx)
    assert np.isfinite(all_rt).all()
    t0 = time.time()
    check_scoring(coord, all_rt, all_c, THRESH2)
    print("item 3: the float64 recount took %.1f s" % (time.time() - t0))
    rt64, w = hypotheses(coord, idx, "3d")
    g = (w[:, 1] - w[:, 0]) / w[:, 3]
    keep = g >= 1e-3
    dist = np.linalg.norm((all_rt.astype(np.float64) - rt64)[:, :, :3], axis=(1, 2)) / np.sqrt(2)
    ratio = dist[keep] / (U / g[keep])
    print("solve: %d of %d left out (g < 1e-3, %.2f %%); |dR| / (2^-24 / g): median %.3g, max %.3g (bound 32)" %
          ((~keep).sum(), len(idx), 100 * (~keep).mean(), np.median(ratio), ratio.max()))
    assert (~keep).mean() <= 0.01
    assert ratio.max() <= 32
    assert best == len(all_c) - 1 - int(np.argmax(all_c[::-1]))
    assert n == all_c[best] == flags.sum() and n >= 3
    check_flags(coord, all_rt[best], flags, THRESH2)
    fit, wf, yc = horn(coord[flags, :3], coord[flags, 3:])
    beta = beta_of(wf)
    print("item 3: %d inliers, loop %d; refit |dR| %.3g (bound %.3g), |dt| %.3g" %
          (n, best, rot_dist(rt, fit), beta, trans_dist(rt, fit)))
    assert rot_dist(rt, fit) <= beta, (rot_dist(rt, fit), beta)
    assert trans_dist(rt, fit) <= beta * np.linalg.norm(yc) + 1e-6


@pytest.mark.gpu
def test_rigid_scoring_three_tiles_per_split_planar_type(ctx):
    """Item 3 with the two-point planar type over the same 9,000 points and 16,384 pairs: check_scoring alone.  SLOW ON
    THE CPU like the 3-D test: another 25 s of float64 recount."""
    coord, idx = rigid_case("2d")
    n_pts = len(coord)
    premise("item 3 rigid, planar type", n_pts, n_pts, wgs_of(LOOPS_RIGID, 256), RIGID, at_least=3)
    rt, n, best, flags, all_rt, all_c, drawn = ctx.estimate_rigid(coord, idx, thresh2=THRESH2, kind="2d", want_all=True)
    assert np.array_equal(drawn, idx) and all_c.max() >= 0.5 * N3_IN
    check_scoring(coord, all_rt, all_c, THRESH2)
    assert best == len(all_c) - 1 - int(np.argmax(all_c[::-1])) and n == all_c[best] == flags.sum()


# ------------------------------------------------------------------------------------------------------------------
# item 4: the fused RGB-D call, its count on the device
# ------------------------------------------------------------------------------------------------------------------
RGBD_ARGS = dict(distance=1, score_threshold=999.0, ambiguity_threshold=0.6, thresh2=THRESH2, kind="3d")


@pytest.mark.gpu
def test_fused_rgbd_call_with_a_device_side_count_below_the_capacity(ctx):
    """Item 4.  The fused call sizes its splits from the capacity, 9,000 records, and reads the count of selected pairs on
    the device; the staged route sizes them from the k the host read, about 7,000 -- another plan, the same bytes."""
    fa, fb, da, db, seen, motion = tgb.synthetic_frames(template(), n_a=N4_A, n_b=N4_B, seed=11)
    seed = 0xC0FFEE

    def fused():
        b1, b2, e1, e2 = upload(ctx, fa), upload(ctx, fb), upload(ctx, da), upload(ctx, db)
        out = ctx.register_rgbd(b1.ptr, N4_A, e1.ptr, b2.ptr, N4_B, e2.ptr, tgb.W, tgb.H, tgb.camera(), loops=LOOPS_RIGID,
                                seed=seed, **RGBD_ARGS)
        out += (b1.to_numpy(SIFT_POINT_DTYPE, (N4_A,)), b2.to_numpy(SIFT_POINT_DTYPE, (N4_B,)))
        for b in (b1, b2, e1, e2):
            b.free()
        return out

    rt, pairs, flags, n_in, f1, f2 = fused()
    # the staged route on copies
    c1, c2, e1, e2 = upload(ctx, fa), upload(ctx, fb), upload(ctx, da), upload(ctx, db)
    ctx.lift_depth(c1.ptr, N4_A, e1.ptr, tgb.W, tgb.H, tgb.camera())
    ctx.lift_depth(c2.ptr, N4_B, e2.ptr, tgb.W, tgb.H, tgb.camera())
    ctx.match(c1.ptr, N4_A, c2.ptr, N4_B, 1)
    d_pairs = upload(ctx, np.full((N4_A, 2), -1, np.int32))
    d_coord = upload(ctx, np.full((N4_A, 6), -1, np.float32))
    d_count = upload(ctx, np.full(1, -1, np.int32))
    ctx.select_matches(c1.ptr, N4_A, c2.ptr, N4_B, d_pairs.ptr, d_coord.ptr, d_count.ptr, 999.0, 0.6, "3d")
    ctx.synchronize()
    k = int(d_count.to_numpy(np.int32, (1,))[0])
    p3, coord = d_pairs.to_numpy(np.int32, (N4_A, 2))[:k].copy(), d_coord.to_numpy(np.float32, (N4_A, 6))[:k].copy()
    t1, t2 = c1.to_numpy(SIFT_POINT_DTYPE, (N4_A,)), c2.to_numpy(SIFT_POINT_DTYPE, (N4_B,))
    for b in (c1, c2, e1, e2, d_pairs, d_coord, d_count):
        b.free()
    # the premise: k strictly inside a split of the capacity plan, no multiple of the tile, and the staged plan another
    grid_y, per_split, tiles = premise("item 4 rigid, fused", N4_A, k, wgs_of(LOOPS_RIGID, 256), RIGID)
    staged_plan = describe("item 4 rigid, staged", k, k, wgs_of(LOOPS_RIGID, 256), RIGID, device_cus())
    assert 3 <= k < N4_A and k % 256 and k % per_split and staged_plan[:2] != (grid_y, per_split)
    assert len(pairs) == k and k >= 0.95 * N4_B
    srt, sn, _, sflags = ctx.estimate_rigid(coord, None, loops=LOOPS_RIGID, thresh2=THRESH2, kind="3d", seed=seed)
    assert rt.tobytes() == srt.tobytes() and n_in == sn
    assert np.array_equal(pairs, p3) and np.array_equal(flags, sflags) and flags.sum() == n_in
    assert f1.tobytes() == t1.tobytes() and f2.tobytes() == t2.tobytes()  # the records end up the same too
    again = fused()
    for u, v in zip((rt, pairs, flags, n_in, f1, f2), again):
        assert np.asarray(u).tobytes() == np.asarray(v).tobytes()
    # the refit against a float64 Horn over the restated coordinates of the reported inliers
    l1, l2 = lift(fa["coords2D"], da), lift(fb["coords2D"], db)
    fit, w, yc = horn(l1[pairs[flags, 0]], l2[pairs[flags, 1]])
    beta = beta_of(w)
    print("item 4: %d selected, %d inliers; against the anchor |dR| %.3g (bound %.3g), |dt| %.3g; from the planted motion %.3g" %
          (k, n_in, rot_dist(rt, fit), beta, trans_dist(rt, fit), np.abs(rt.astype(np.float64) - motion).max()))
    assert n_in >= 0.95 * k
    assert rot_dist(rt, fit) <= beta
    assert trans_dist(rt, fit) <= beta * np.linalg.norm(yc) + 1e-6


# ------------------------------------------------------------------------------------------------------------------
# item 5: selection past 256 workgroups
# ------------------------------------------------------------------------------------------------------------------
def first_wrong_base(pairs, want_pairs, n1):
    """Where a failure of the selection lies: for every 256-record workgroup with a keep, the output row of its first kept
    record must be the sum of the keeps of the workgroups before it.  Returns the first workgroup where it is not, or -1."""
    keep = np.zeros(n1, bool)
    keep[want_pairs[:, 0]] = True
    blocks = np.add.reduceat(keep.astype(np.int64), np.arange(0, n1, 256))
    base = np.r_[0, np.cumsum(blocks)[:-1]]
    row_of = np.full(n1, -1, np.int64)
    rows = np.flatnonzero((pairs[:, 0] >= 0) & (pairs[:, 0] < n1))
    row_of[pairs[rows, 0]] = rows
    first = np.array([b * 256 + int(np.argmax(keep[b * 256:(b + 1) * 256])) for b in range(len(blocks))])
    wrong = np.flatnonzero((blocks > 0) & (row_of[first] != base))
    return int(wrong[0]) if len(wrong) else -1


@pytest.mark.gpu
def test_selection_past_256_workgroups(ctx):
    """Item 5: select_matches and select_mutual, kinds 2d and 3d, over 66,000 records a side -- 258 workgroups, so the sum
    of the keeps in front of workgroups 256 and 257 takes the loop's second turn."""
    r1, r2, _ = selection_records()
    assert idiv_up(N5, 256) > 257
    d1, d2 = upload(ctx, r1), upload(ctx, r2)
    for call, mutual in ((ctx.select_matches, False), (ctx.select_mutual, True)):
        for kind in ("2d", "3d"):
            what = "%s %s" % ("mutual" if mutual else "plain", kind)
            want_p, want_c = selection(r1, r2, kind == "3d", mutual)
            d_pairs = upload(ctx, np.full((N5, 2), -9, np.int32))
            d_coord = upload(ctx, np.full((N5, 6), -9.0, np.float32))
            d_count = upload(ctx, np.full(1, -9, np.int32))
            call(d1.ptr, N5, d2.ptr, N5, d_pairs.ptr, d_coord.ptr, d_count.ptr, SELECT[0], SELECT[1], kind)
            ctx.synchronize()
            pairs, coord = d_pairs.to_numpy(np.int32, (N5, 2)), d_coord.to_numpy(np.float32, (N5, 6))
            count = int(d_count.to_numpy(np.int32, (1,))[0])
            for b in (d_pairs, d_coord, d_count):
                b.free()
            print("item 5 %s: %d kept of %d, %d of them past record %d" % (what, count, N5, (want_p[:, 0] >= LATE).sum(), LATE))
            assert (want_p[:, 0] >= LATE).sum() > 1 and want_p[-1, 0] == N5 - 1
            assert first_wrong_base(pairs, want_p, N5) == -1, (what, first_wrong_base(pairs, want_p, N5))
            assert count == len(want_p), (what, count, len(want_p))
            assert pairs[:count].tobytes() == want_p.tobytes(), what
            assert coord[:count].tobytes() == want_c.tobytes(), what
            assert (np.diff(pairs[:count, 0]) > 0).all(), what
            assert (pairs[count:] == -9).all() and (coord[count:] == -9.0).all(), what  # rows past the count: not written
    assert d1.to_numpy(SIFT_POINT_DTYPE, (N5,)).tobytes() == r1.tobytes()
    assert d2.to_numpy(SIFT_POINT_DTYPE, (N5,)).tobytes() == r2.tobytes()
    d1.free()
    d2.free()


# ------------------------------------------------------------------------------------------------------------------
# item 6: batches with several tiles per split
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planar_frames():
    return PlanarFrames()


@pytest.fixture(scope="module")
def rgbd_frames():
    return RgbdFrames()


PLANAR_BATCH = {}
SEED6 = 77


def planar_batch(ctx, fb):
    """The batch call and the match rows of its pairs, once."""
    if not PLANAR_BATCH:
        res, recs = tpb.register_batch(ctx, fb, SEED6, 1, pairs=PAIRS6, loops=LOOPS_EPI)
        assert recs.tobytes() == fb.points.tobytes()  # the records: untouched
        PLANAR_BATCH["out"] = (res, tpb.match_rows(ctx, fb, PAIRS6, 1))
    return PLANAR_BATCH["out"]


def planar_batch_premise(fb):
    """On 256 CUs the batch scores in 8 splits of 512 records, 8 tiles; pair (1, 2) has 3,500 records: inside a split."""
    wgs = wgs_of(LOOPS_EPI, 64, len(PAIRS6))
    for a in sorted(set(PAIRS6[:, 0].tolist())):
        grid_y, per_split, tiles = describe("item 6 planar batch, frame %d first" % a, N6[0], int(fb.n[a]), wgs, PLANAR,
                                            device_cus())
    grid_y, per_split, tiles = premise("item 6 planar batch", N6[0], N6[1], wgs, PLANAR)
    assert N6[1] % per_split and tiles[-1] == []  # a count inside a split, and a split past it
    pair = describe("item 6 planar, the pair call", N6[0], N6[0], wgs_of(LOOPS_EPI, 64), PLANAR, device_cus())
    assert pair[:2] != (grid_y, per_split)  # the routes compared run other plans
    if device_cus() == 256:
        assert (grid_y, per_split) == (8, 512) and tiles[0] == [64] * 8 and pair[:2] == (32, 128)


@pytest.mark.gpu
def test_planar_batch_with_eight_tiles_per_split_equals_the_staged_route(ctx, planar_frames):
    """Item 6, what test_batch_equals_the_staged_route_bit_for_bit asserts: every output and every record byte per pair."""
    fb = planar_frames
    planar_batch_premise(fb)
    res, rows = planar_batch(ctx, fb)
    for p, (a, b) in enumerate(PAIRS6):
        one, after = tpb.staged(ctx, fb, rows[p], a, b, SEED6 + p, 1, loops=LOOPS_EPI)
        print("pair %d (%d, %d): %d candidates, %d inliers, %d fit, loop %d" %
              (p, a, b, one.num_candidates, one.num_matches, one.num_fit, one.best_loop))
        assert one.num_candidates >= 8 and one.num_matches >= 4, p
        tpb.same_pair(res, p, one, after, int(fb.n[a]), "staged")
    assert res.counts.tolist() == [int(fb.n[a]) for a in PAIRS6[:, 0]]
    assert res.num_matches[0] >= 0.9 * 2800  # the planted pair: 2,800 planted correspondences
    assert tpb.corner_distance(res.homography[0][:8], fb.H.ravel()[:8]) < 1.0


@pytest.mark.gpu
def test_planar_batch_with_eight_tiles_per_split_equals_register_planar(ctx, planar_frames):
    """Item 6, what test_batch_equals_register_planar_bit_for_bit asserts: first that the batch rows are the pair matcher's
    fields for every pair, with no tied row among them, then the equality of every output."""
    fb = planar_frames
    planar_batch_premise(fb)
    res, rows = planar_batch(ctx, fb)
    for p, (a, b) in enumerate(PAIRS6):
        na, nb = int(fb.n[a]), int(fb.n[b])
        b1, b2 = upload(ctx, fb.points[a, :na].copy()), upload(ctx, fb.points[b, :nb].copy())
        ctx.match(b1.ptr, na, b2.ptr, nb, 1)
        ctx.synchronize()
        m = b1.to_numpy(SIFT_POINT_DTYPE, (na,))
        tie = tpb.tie_rows(m["score"], m["ambiguity"], 1) & (m["ambiguity"] != 0)
        assert not tie.any(), (p, np.nonzero(tie)[0][:10])
        for f in ("score", "ambiguity", "match"):
            assert rows[p, :na][f].tobytes() == m[f].tobytes(), (p, f)
        d1, d2 = upload(ctx, fb.points[a, :na].copy()), upload(ctx, fb.points[b, :nb].copy())
        one = ctx.register_planar(d1.ptr, na, d2.ptr, nb, distance=1, loops=LOOPS_EPI, thresh=5.0, refine_loops=5,
                                  refine_thresh=3.0, seed=(SEED6 + p) & tpb.MASK64, **tpb.RULES[1])
        tpb.same_pair(res, p, one, d1.to_numpy(SIFT_POINT_DTYPE, (na,)), na, "register_planar")
        for buf in (b1, b2, d1, d2):
            buf.free()


@pytest.mark.gpu
def test_rgbd_batch_with_four_tiles_per_split_equals_register_per_pair(ctx, rgbd_frames):
    """Item 6, what test_register_batch_equals_register_per_pair_bit_for_bit asserts.  On 256 CUs the batch scores in 4
    splits of 1,024 selected pairs, four tiles; the pair call in 16 splits of one tile.  The counts -- the selected pairs
    of each pair of frames -- stay on the device in both routes.  That file's exception for tied matcher rows stays as it
    states it: a tied row has an ambiguity of about 1 and is never selected at 0.6."""
    fb = rgbd_frames
    seed = 0xC0FFEE
    rt, n_match, n_in, sel, flags, recs = tgb.register_batch(ctx, fb, seed, "3d", pairs=PAIRS6, loops=LOOPS_RIGID)
    wgs = wgs_of(LOOPS_RIGID, 256, len(PAIRS6))
    ragged = 0
    for p, (a, b) in enumerate(PAIRS6):
        grid_y, per_split, tiles = describe("item 6 rgbd batch, pair %d (%d, %d)" % (p, a, b), N6[0], int(n_match[p]), wgs,
                                            RIGID, device_cus())
        assert max(len(t) for t in tiles) >= 2, p
        ragged += several_tiles(tiles, 256) and bool(n_match[p] % per_split)
    assert ragged >= 1  # some pair's count lies inside a split and leaves a ragged tile that is not the first
    pair = describe("item 6 rgbd, the pair call", N6[0], int(n_match[0]), wgs_of(LOOPS_RIGID, 256), RIGID, device_cus())
    assert pair[:2] != (grid_y, per_split)
    if device_cus() == 256:
        assert (grid_y, per_split) == (4, 1024) and pair[:2] == (16, 256)
    assert rt.shape == (len(PAIRS6), 3, 4) and len(sel) == len(PAIRS6) and len(flags) == len(PAIRS6)
    for p, (a, b) in enumerate(PAIRS6):
        prt, ppairs, pflags, pin = tgb.register_pair(ctx, fb, a, b, seed + p, "3d", loops=LOOPS_RIGID)
        print("pair %d (%d, %d): %d matches, %d inliers" % (p, a, b, n_match[p], n_in[p]))
        assert rt[p].tobytes() == prt.tobytes(), p
        assert n_match[p] == len(ppairs) and n_in[p] == pin, p
        assert sel[p].tobytes() == ppairs.tobytes() and np.array_equal(flags[p], pflags), p
    assert n_match[0] >= 0.95 * N6[1] and n_in[0] >= 0.95 * n_match[0]
    assert np.abs(rt[0].astype(np.float64) - fb.motion).max() < 5e-3
    # of the records only coords3D is written, and only below the counts
    assert np.array_equal(other_bytes(recs.reshape(-1)), other_bytes(fb.points.reshape(-1)))
    for k in range(len(N6)):
        assert (recs["coords3D"][k, fb.n[k]:] == 7.0).all()
        assert (recs["coords3D"][k, :fb.n[k]] != 7.0).all()
