"""8-bit guided matching (cusift_match8_guided, cusift_match8_projected and their pair-list forms; cusift_amd/csrc/
sift_match8_guided.hip: M8GuideH / M8GuideF / M8GuideP inside m8_block) held to zero tolerance: all five fields of every row.

The expectation is tests/match8_guided_model.py -- match8_model's exact integer keys over the columns that pass a mask --
and the mask is guide_mask of tests/test_match_guided.py or project_mask of tests/test_match_projected.py, the geometric
tests restated bit for bit.  Coordinates come from the records, descriptors from byte tables that are built directly, with
few distinct values, so that exactly tied keys are ordinary.  No tolerance appears in this file.

The matcher's workgroup is 256 rows and its LDS tile 64 columns: the shapes straddle both.  Every shape has a tight radius
at which rows with no passing column, with exactly one and with two or more are each at least a tenth of the rows -- the
conditions are asserted where a machine without a GPU sees them.
"""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from match8_guided_model import match8_guided_model, row_categories
from match8_model import FIELDS, INIT, ambiguity_model, assert_fields_equal, keys_model, match8_model, sums_model
from oracle_binding import SIFT_POINT_DTYPE
from test_match_guided import EPIPOLAR, HOMOGRAPHY, MILD, guide_mask, scattered_pair
from test_match_projected import CAM, RADIUS, RT, lift, pose, project_mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REC = SIFT_POINT_DTYPE.itemsize
SENTINEL = 0xAB
PROJECTED = 2  # beside HOMOGRAPHY = 0 and EPIPOLAR = 1
GUIDES = (HOMOGRAPHY, EPIPOLAR, PROJECTED)
SHAPES = [(1, 1), (255, 63), (257, 65), (300, 130), (300, 200)]
TAIL = 40  # records behind n1 that no call may touch
# the tight radius of every (shape, guide): each category of row -- no passing column, exactly one, two or more -- holds
# at least a tenth of the rows (test_tight_radii_give_every_category_of_row).  (1, 1) has one pair: no condition.
TIGHT = {
    (255, 63): {HOMOGRAPHY: 8.0, EPIPOLAR: 1.0, PROJECTED: 10.0},
    (257, 65): {HOMOGRAPHY: 8.0, EPIPOLAR: 1.0, PROJECTED: 10.0},
    (300, 130): {HOMOGRAPHY: 6.0, EPIPOLAR: 0.5, PROJECTED: 6.0},
    (300, 200): {HOMOGRAPHY: 5.0, EPIPOLAR: 0.4, PROJECTED: 6.0},
    (1, 1): {HOMOGRAPHY: 1.0, EPIPOLAR: 0.01, PROJECTED: 1.0},
}
MILD_RADIUS = {HOMOGRAPHY: MILD[HOMOGRAPHY][1], EPIPOLAR: MILD[EPIPOLAR][1], PROJECTED: RADIUS}
SYMBOLS = {"cusift_match8_guided": 13, "cusift_match8_projected": 13, "cusift_match8_batch_guided": 14,
           "cusift_match8_batch_projected": 14, "cusift_match8_guided_records": 9, "cusift_match8_projected_records": 9}


# ----------------------------------------------------------------------------------------------------------------------
# the inputs
# ----------------------------------------------------------------------------------------------------------------------
def few_valued_table(rng, n, base):
    """n byte descriptors with few distinct values: `base` with its first byte 0 or 200, so that a row's keys take two
    values and exactly tied keys are ordinary; every eighth descriptor is random bytes instead."""
    q = np.tile(base, (n, 1))
    q[:, 0] = rng.integers(0, 2, n) * 200
    rich = np.arange(n) % 8 == 7
    q[rich] = rng.integers(0, 256, (int(rich.sum()), 128))
    return q.astype(np.uint8)


def scene(n1, n2, seed=3):
    """(records 1 with TAIL more behind them, records 2, table 1, table 2): coords2D scattered as in test_match_guided.py,
    coords3D lifted as in test_match_projected.py -- rows without depth and behind the camera included, and with 17 rows
    or more a NaN and an infinite one -- descriptors that are garbage, match fields that carry a mark."""
    real1, s2 = scattered_pair(n1, n2, "sparse16", seed)
    lift(real1, np.random.default_rng(1000 + seed))
    if n1 >= 17:
        real1["coords3D"][8] = (np.nan, 1.0, 2.0)
        real1["coords3D"][9] = (0.5, np.inf, 2.0)
    if (n1, n2) == (1, 1):
        s2["coords2D"][0] = real1["coords2D"][0]
    for s in (real1, s2):
        s["data"] = np.float32(np.nan)
        s["score"], s["ambiguity"], s["match"], s["match_xpos"], s["match_ypos"] = -7.0, -7.0, -77, -7.0, -7.0
    s1 = np.full((n1 + TAIL, REC), SENTINEL, np.uint8).view(SIFT_POINT_DTYPE).reshape(-1)
    s1[:n1] = real1
    rng = np.random.default_rng(7000 + seed)
    base = rng.integers(0, 256, 128)
    return s1, s2, few_valued_table(rng, n1, base), few_valued_table(rng, n2, base)


def model_of(guide, p=0):
    """The mild model of a guide; pair p's differs (the pair-list test tells the pairs apart by it)."""
    if guide == PROJECTED:
        return pose(p)
    M = MILD[guide][0].copy()
    M[2 if guide == HOMOGRAPHY else 8] += 1.5 * p  # H: a shift in x; F: the lines move
    return M


def mask_of(guide, M, s1, s2, radius):
    if guide == PROJECTED:
        return project_mask(M, CAM, s1["coords3D"], s2["coords2D"], radius)
    return guide_mask(guide, M, s1["coords2D"], s2["coords2D"], radius)


def cols_per_split(n2, k):
    """The host's split plan (matcher_split_plan) for k splits asked, tiles of 64 columns."""
    k = min(k, -(-n2 // 64))
    return -(-(-(-n2 // k)) // 64) * 64


def nothing_fields(n, distance, s2):
    init = np.full(n, INIT[distance], np.float32)
    return {"score": init, "ambiguity": ambiguity_model(init, init, distance), "match": np.full(n, -1, np.int32),
            "match_xpos": np.full(n, s2["coords2D"][0, 0], np.float32),
            "match_ypos": np.full(n, s2["coords2D"][0, 1], np.float32)}


def fields_of(recs, n=None):
    return {f: np.ascontiguousarray(recs[f][:n]) for f in FIELDS}


# ----------------------------------------------------------------------------------------------------------------------
# without a GPU
# ----------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_bound():
    from cusift_amd import batch, capi

    extras = open(os.path.join(ROOT, "include", "cusift_amd_extras.h")).read()
    handle = C.CDLL(capi.LIB_PATH)
    for name, nargs in SYMBOLS.items():
        assert re.search(r"^int %s\(cusift_ctx \*ctx" % name, extras, flags=re.M), name
        assert hasattr(handle, name), name
        res, args = capi.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs, name
    for method in ("match8_guided", "match8_projected", "match8_batch_guided", "match8_batch_projected"):
        assert callable(getattr(capi.Context, method)), method
    assert callable(batch.BatchExtractor.match8_guided) and callable(batch.BatchExtractor.match8_projected)
    text = extras.split("int cusift_match8_guided(")[0].rsplit("/*", 1)[1].lower()
    for needle in ("lowest column of the passing set", "no column passes", "exactly one", "no atomics"):
        assert needle in text, needle
    for needle in ("cusift_match_guided", "cusift_match_projected", "-ffp-contract=off"):  # the test is referred to
        assert needle in text, needle


def test_new_kernels_compile_for_gfx950_on_the_int8_pipe_without_scratch_or_spills():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs

    asm = kernel_regs.assembly("sift_match8_guided.hip")
    assert "gfx950" in asm
    kernels = kernel_regs.kernels(asm)
    # three guides x both distances; the merges: both distances
    for needle, count, mfma in (("match8_guided_kernel", 6, True), ("match8_batch_guided_kernel", 6, True),
                                ("match8_guided_merge_kernel", 2, False), ("match8_batch_guided_merge_kernel", 2, False)):
        found = [k for k in kernels if needle in k["name"]]
        assert len(found) == count, (needle, [k["name"] for k in found])
        for k in found:
            assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
            start = asm.index("\n%s:" % k["name"])
            body = asm[start:asm.index("; codeLenInByte", start)]
            assert ("v_mfma_i32_16x16x64_i8" in body) == mfma, k["name"]
            assert "v_mfma_f32" not in body, k["name"]
            if mfma:
                assert "atomic" not in body, k["name"]


def tiny(keys_rows):
    """Byte tables whose L2 keys against row 0 are `keys_rows`: one row of zeros, column j with keys_rows[j] ones."""
    q2 = np.zeros((len(keys_rows), 128), np.uint8)
    for j, k in enumerate(keys_rows):
        q2[j, :k] = 1
    return np.zeros((1, 128), np.uint8), q2


def test_restatement_on_hand_made_cases():
    xy2 = np.arange(8, dtype=np.float32).reshape(4, 2)
    q1, q2 = tiny([1, 5, 3, 3])
    assert keys_model(q1, q2, 1).tolist() == [[1, 5, 3, 3]]
    scale = np.float32(2.0 ** -18)
    # a failing column with the smallest key and the lowest index is ignored
    got = match8_guided_model(q1, q2, 1, xy2, [[False, True, True, True]])
    assert got["match"][0] == 2 and got["score"][0] == 3 * scale
    # two passing columns with equal keys: the lower wins and second == best
    assert got["ambiguity"][0] == ambiguity_model(got["score"], got["score"], 1)[0]
    assert (got["match_xpos"][0], got["match_ypos"][0]) == (4.0, 5.0)
    # no passing column
    got = match8_guided_model(q1, q2, 1, xy2, [[False] * 4])
    assert_fields_equal(got, nothing_fields(1, 1, {"coords2D": xy2}), "none")
    assert got["match"][0] == -1 and got["score"][0] == 999.0 and (got["match_xpos"][0], got["match_ypos"][0]) == (0.0, 1.0)
    # one passing column: second is the initial value
    got = match8_guided_model(q1, q2, 1, xy2, [[False, True, False, False]])
    assert got["match"][0] == 1 and got["score"][0] == 5 * scale
    assert got["ambiguity"][0] == ambiguity_model(got["score"], np.float32([999.0]), 1)[0]
    # a single column, passing and failing, both distances
    for distance in (1, 0):
        got = match8_guided_model(q1, q2[:1], distance, xy2[:1], [[True]])
        assert_fields_equal(got, match8_model(q1, q2[:1], distance, xy2[:1]), "single, passing")
        got = match8_guided_model(q1, q2[:1], distance, xy2[:1], [[False]])
        assert_fields_equal(got, nothing_fields(1, distance, {"coords2D": xy2}), "single, failing")
    assert nothing_fields(1, 0, {"coords2D": xy2})["score"][0] == -1.0


@pytest.mark.parametrize("distance", (1, 0))
@pytest.mark.parametrize("n1,n2", SHAPES)
def test_restatement_with_every_pair_passing_is_match8_model(n1, n2, distance):
    s1, s2, q1, q2 = scene(n1, n2)
    got = match8_guided_model(q1, q2, distance, s2["coords2D"], np.ones((n1, n2), bool))
    assert_fields_equal(got, match8_model(q1, q2, distance, s2["coords2D"]), "all true")


@pytest.mark.parametrize("guide", GUIDES)
@pytest.mark.parametrize("n1,n2", SHAPES[1:])
def test_tight_radii_give_every_category_of_row(n1, n2, guide):
    """The conditions on the GPU tests' inputs, where a machine without a GPU sees them."""
    s1, s2, q1, q2 = scene(n1, n2)
    mask = mask_of(guide, model_of(guide), s1[:n1], s2, TIGHT[(n1, n2)][guide])
    shares = row_categories(mask)
    print("(%d, %d) guide %d radius %g: none / one / more = %.2f / %.2f / %.2f" % ((n1, n2, guide,
                                                                                   TIGHT[(n1, n2)][guide]) + shares))
    assert min(shares) >= 0.10, shares
    for distance in (1, 0):
        # an ignored guide cannot pass: the unguided winner fails the mask in a quarter of the rows at the least
        plain = match8_model(q1, q2, distance, s2["coords2D"])
        assert (~mask[np.arange(n1), plain["match"]]).mean() >= 0.25
        # a tenth of the rows have an exactly tied best among their passing columns
        K = np.where(mask, keys_model(q1, q2, distance), 1 << 40)
        best = K.min(1, keepdims=True)
        tied = ((K == best) & mask).sum(1) >= 2
        assert tied.mean() >= 0.10, tied.mean()
        # and a winner that is not the lowest passing column, so that "lowest index" is not "first passing"
        want = match8_guided_model(q1, q2, distance, s2["coords2D"], mask)
        assert (want["match"] > mask.argmax(1))[mask.any(1)].mean() >= 0.05
    if n2 == 200:  # a row whose only passing column lies in the last split, under 2 and 3 splits asked (both give 2)
        cps = cols_per_split(n2, 2)
        assert cps == cols_per_split(n2, 3) == 128
        assert ((mask.sum(1) == 1) & mask[:, cps:].any(1)).any()
    # the mild radius passes a tenth to a third of the pairs, and 1e6 all of them on usable rows
    share = mask_of(guide, model_of(guide), s1[:n1], s2, MILD_RADIUS[guide]).mean()
    assert 0.05 <= share <= 0.30, share
    wide = mask_of(guide, model_of(guide), s1[:n1], s2, 1e6)
    assert wide.all() if guide != PROJECTED else wide.any(1).mean() > 0.6


def test_batch_models_tell_the_pairs_apart():
    points, counters, q, pairs, _ = batch_scene()
    for guide in GUIDES:
        for p, (a, b) in enumerate(pairs):
            na, nb = counters[a], counters[b]
            if na == 0 or nb == 0:
                continue
            own = mask_of(guide, model_of(guide, p), points[a, :na], points[b, :nb], BATCH_RADIUS[guide])
            assert 0.02 <= own.mean() <= 0.30, (guide, p, own.mean())
            for o in range(len(pairs)):
                if o != p:
                    other = mask_of(guide, model_of(guide, o), points[a, :na], points[b, :nb], BATCH_RADIUS[guide])
                    assert (own != other).mean() > 0.005, (guide, p, o)


# ----------------------------------------------------------------------------------------------------------------------
# on the GPU
# ----------------------------------------------------------------------------------------------------------------------
class Pair8:
    """A scene on the device: both record sets, both tables and their sums (from the numpy model)."""

    def __init__(self, ctx, s1, s2, q1, q2):
        from cusift_amd.capi import DeviceBuffer

        self.ctx, self.s1, self.s2 = ctx, s1, s2
        self.bufs = [DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(a)) for a in (q1, sums_model(q1), q2, sums_model(q2),
                                                                                   s2)]
        self.d1 = DeviceBuffer(ctx, s1.nbytes)

    def run(self, guide, M, radius, distance, splits=0, n1=None, n2=None, plain=False):
        """All of set 1's records after the guided call (plain: cusift_match8) over the first n1 rows and n2 columns; set 2
        is checked to be unchanged."""
        from cusift_amd import capi

        n1 = len(self.s1) - TAIL if n1 is None else n1
        n2 = len(self.s2) if n2 is None else n2
        dq1, ds1, dq2, ds2, d2 = (b.ptr for b in self.bufs)
        self.ctx.h2d(self.d1.ptr, self.s1)
        try:
            self.ctx.set_policy(capi.POLICY_MATCH_SPLITS, splits)
            if plain:
                self.ctx.match8(self.d1.ptr, n1, dq1, ds1, d2, n2, dq2, ds2, distance)
            elif guide == PROJECTED:
                self.ctx.match8_projected(self.d1.ptr, n1, dq1, ds1, d2, n2, dq2, ds2, M, capi.Camera(*CAM), radius, distance)
            else:
                self.ctx.match8_guided(self.d1.ptr, n1, dq1, ds1, d2, n2, dq2, ds2, guide, M, radius, distance)
            self.ctx.synchronize()
        finally:
            self.ctx.set_policy(capi.POLICY_MATCH_SPLITS, 0)
        assert self.bufs[4].to_numpy(SIFT_POINT_DTYPE, (len(self.s2),)).tobytes() == self.s2.tobytes()
        return self.d1.to_numpy(SIFT_POINT_DTYPE, (len(self.s1),))

    def untouched(self, got, n1, what):
        """Rows past n1 and every byte of a row that is not one of the five fields, coords3D included."""
        outside = np.ones(REC, bool)
        for f in FIELDS:
            off = SIFT_POINT_DTYPE.fields[f][1]
            outside[off:off + 4] = False
        a, b = got.view(np.uint8).reshape(-1, REC), self.s1.view(np.uint8).reshape(-1, REC)
        assert np.array_equal(a[n1:], b[n1:]), what
        assert np.array_equal(a[:n1, outside], b[:n1, outside]), what

    def free(self):
        for b in self.bufs + [self.d1]:
            b.free()


@pytest.mark.gpu
@pytest.mark.parametrize("guide", GUIDES)
@pytest.mark.parametrize("n1,n2", SHAPES)
def test_gpu_every_field_every_row(ctx, n1, n2, guide):
    s1, s2, q1, q2 = scene(n1, n2)
    M = model_of(guide)
    pair = Pair8(ctx, s1, s2, q1, q2)
    try:
        for radius in (MILD_RADIUS[guide], TIGHT[(n1, n2)][guide]):
            mask = mask_of(guide, M, s1[:n1], s2, radius)
            for distance in (1, 0):
                want = match8_guided_model(q1, q2, distance, s2["coords2D"], mask)
                for k in (1, 2, 3, 0):
                    what = "(%d, %d) guide %d radius %g d%d, %d splits asked" % (n1, n2, guide, radius, distance, k)
                    got = pair.run(guide, M, radius, distance, k)
                    assert_fields_equal(fields_of(got, n1), want, what)
                    pair.untouched(got, n1, what)
    finally:
        pair.free()


@pytest.mark.gpu
@pytest.mark.parametrize("guide", GUIDES)
def test_gpu_models_that_pass_nothing_and_radii_that_pass_everything(ctx, guide):
    n1, n2 = 257, 65
    s1, s2, q1, q2 = scene(n1, n2)
    if guide == PROJECTED:  # every row usable: no holes, no NaN
        lift(s1, np.random.default_rng(5), holes=False)
    size = 12 if guide == PROJECTED else 9
    pair = Pair8(ctx, s1, s2, q1, q2)
    try:
        for distance in (1, 0):
            nothing = nothing_fields(n1, distance, s2)
            for M in (np.zeros(size), np.full(size, np.nan), np.full(size, np.inf)):
                for radius in (5.0, np.inf):
                    for k in (1, 2):
                        got = pair.run(guide, M, radius, distance, k)
                        assert_fields_equal(fields_of(got, n1), nothing, "guide %d, model of %r" % (guide, M[0]))
                        pair.untouched(got, n1, "nothing passes")
            for radius in (1e6, np.inf):
                assert mask_of(guide, model_of(guide), s1[:n1], s2, radius).all()
                for k in (1, 2, 0):
                    plain = pair.run(guide, None, None, distance, k, plain=True)
                    got = pair.run(guide, model_of(guide), radius, distance, k)
                    assert got.tobytes() == plain.tobytes(), (guide, radius, distance, k)
                    assert_fields_equal(fields_of(got, n1), match8_model(q1, q2, distance, s2["coords2D"]), "radius %g" % radius)
    finally:
        pair.free()


@pytest.mark.gpu
def test_gpu_refusals_and_empty_counts_write_nothing(ctx):
    from cusift_amd import capi
    from cusift_amd.capi import DeviceBuffer

    n1, n2 = 70, 95
    s1, s2, q1, q2 = scene(n1, n2)
    pair = Pair8(ctx, s1, s2, q1, q2)
    dq1, ds1, dq2, ds2, d2 = (b.ptr for b in pair.bufs)
    d1 = pair.d1.ptr
    ctx.h2d(d1, s1)
    pts = np.stack([s1[:n2], s2])
    d_pts = DeviceBuffer.from_numpy(ctx, pts)
    tq = np.concatenate([q2, q2])
    d_q, d_sums = DeviceBuffer.from_numpy(ctx, tq), DeviceBuffer.from_numpy(ctx, sums_model(tq))
    d_rows = DeviceBuffer.from_numpy(ctx, np.full((1, n2, 16), SENTINEL, np.uint8))
    good, H, nan = capi.Camera(*CAM), model_of(HOMOGRAPHY), float("nan")
    bad_cam = capi.Camera(0.0, 115.0, 50.5, 49.5, 1.0)

    def guided(s1_=d1, q1_=dq1, sums1_=ds1, s2_=d2, q2_=dq2, sums2_=ds2, model=HOMOGRAPHY, M=H, radius=5.0, distance=1):
        ctx.match8_guided(s1_, n1, q1_, sums1_, s2_, n2, q2_, sums2_, model, M, radius, distance)

    def projected(rt=RT, cam=good, radius=5.0, distance=1, q1_=dq1):
        ctx.match8_projected(d1, n1, q1_, ds1, d2, n2, dq2, ds2, rt, cam, radius, distance)

    def batch_guided(points=d_pts.ptr, q=d_q.ptr, rows=d_rows.ptr, model=HOMOGRAPHY, M=H, radius=5.0, distance=1,
                     pairs=((0, 1),)):
        ctx.match8_batch_guided(points, q, d_sums.ptr, None, 2, n2, pairs, model, M, radius, rows, distance)

    def batch_projected(points=d_pts.ptr, rt=RT, cam=good, radius=5.0, distance=1, rows=d_rows.ptr):
        ctx.match8_batch_projected(points, d_q.ptr, d_sums.ptr, None, 2, n2, [(0, 1)], rt, cam, radius, rows, distance)

    refused = [
        # what the fp32 guided and projected calls add
        lambda: guided(model=2), lambda: guided(M=None), lambda: guided(radius=0.0), lambda: guided(radius=-1.0),
        lambda: guided(radius=nan), lambda: projected(rt=None), lambda: projected(cam=None), lambda: projected(cam=bad_cam),
        lambda: projected(radius=0.0), lambda: projected(radius=nan),
        lambda: batch_guided(model=7), lambda: batch_guided(M=None), lambda: batch_guided(radius=0.0),
        lambda: batch_guided(radius=nan),
        lambda: batch_projected(rt=None), lambda: batch_projected(cam=None), lambda: batch_projected(cam=bad_cam),
        lambda: batch_projected(radius=-2.0),
        # what cusift_match8 and cusift_match8_batch refuse
        lambda: guided(distance=2), lambda: guided(s1_=None), lambda: guided(s2_=None), lambda: guided(q1_=None),
        lambda: guided(sums2_=None), lambda: guided(q1_=dq1 + 8), lambda: guided(sums1_=ds1 + 4),
        lambda: projected(distance=-1), lambda: projected(q1_=dq1 + 4),
        lambda: batch_guided(distance=2), lambda: batch_guided(points=None), lambda: batch_guided(q=None),
        lambda: batch_guided(q=d_q.ptr + 8), lambda: batch_guided(rows=None), lambda: batch_guided(pairs=((0, 2),)),
        lambda: batch_projected(points=None), lambda: batch_projected(rows=None), lambda: batch_projected(distance=3),
    ]
    for call in refused:
        with pytest.raises(capi.CusiftError):
            call()
    assert capi.lib().cusift_match8_guided(ctx.handle, d1, n1, dq1, ds1, d2, n2, dq2, ds2, 1, 5, None, 5.0) == -1  # INVALID
    # an empty list still refuses a bad model; with a good one it is fine and writes nothing
    with pytest.raises(capi.CusiftError):
        ctx.match8_batch_guided(d_pts.ptr, d_q.ptr, d_sums.ptr, None, 2, n2, np.zeros((0, 2), np.int32), 9,
                                np.zeros((0, 9)), 5.0, d_rows.ptr)
    ctx.match8_batch_guided(d_pts.ptr, d_q.ptr, d_sums.ptr, None, 2, n2, np.zeros((0, 2), np.int32), HOMOGRAPHY,
                            np.zeros((0, 9)), 5.0, d_rows.ptr)
    ctx.match8_batch_projected(None, None, None, None, 2, 0, [(0, 1)], RT, good, 5.0, None)  # a capacity of zero
    # counts <= 0: fine, and nothing happens -- whatever the rest says
    ctx.match8_guided(d1, 0, dq1, ds1, d2, n2, dq2, ds2, 5, None, -1.0, 1)
    ctx.match8_guided(d1, n1, None, None, d2, 0, None, None, HOMOGRAPHY, H, 5.0, 1)
    ctx.match8_projected(d1, 0, dq1, ds1, d2, n2, dq2, ds2, None, None, -1.0, 1)
    ctx.match8_projected(d1, n1, dq1, ds1, d2, -3, dq2, ds2, RT, good, 5.0, 1)
    ctx.synchronize()
    assert pair.d1.to_numpy(SIFT_POINT_DTYPE, (len(s1),)).tobytes() == s1.tobytes()
    assert pair.bufs[4].to_numpy(SIFT_POINT_DTYPE, (n2,)).tobytes() == s2.tobytes()
    assert d_pts.to_numpy(SIFT_POINT_DTYPE, pts.shape).tobytes() == pts.tobytes()
    assert (d_rows.to_numpy(np.uint8, (1, n2, 16)) == SENTINEL).all()
    for d in (d_pts, d_q, d_sums, d_rows):
        d.free()
    pair.free()


# ---- the pair-list forms ---------------------------------------------------------------------------------------------
BATCH_MAX = 320
BATCH_RADIUS = {HOMOGRAPHY: 12.0, EPIPOLAR: 2.0, PROJECTED: 12.0}


def batch_scene():
    """Four frames in 320-record slots holding 300, 200, 0 and 130 records; a list with a repeated frame, (a, a) and the
    empty frame on either side."""
    counters = np.array([300, 200, 0, 130], np.int64)
    pairs = np.array([(0, 1), (1, 0), (0, 0), (2, 1), (1, 2), (3, 0), (0, 3)], np.int32)
    points = np.zeros((4, BATCH_MAX), SIFT_POINT_DTYPE)
    q = np.zeros((4, BATCH_MAX, 128), np.uint8)
    for f in range(4):
        s1, _, q1, _ = scene(BATCH_MAX - TAIL, 1, seed=20 + f)
        s1["coords3D"][BATCH_MAX - TAIL:] = 1.0  # records past a count: live-looking
        s1["coords2D"][BATCH_MAX - TAIL:] = 50.0
        points[f] = s1
        q[f, :BATCH_MAX - TAIL] = q1
        q[f, BATCH_MAX - TAIL:] = q1[:TAIL]
    return points, counters, q, pairs, sums_model(q)


@pytest.mark.gpu
@pytest.mark.parametrize("guide", GUIDES)
def test_gpu_batch_rows_equal_the_pair_call(ctx, guide):
    from cusift_amd import capi
    from cusift_amd.capi import DeviceBuffer

    points, counters, q, pairs, sums = batch_scene()
    models = np.stack([model_of(guide, p) for p in range(len(pairs))])
    radius = BATCH_RADIUS[guide]
    bufs = [DeviceBuffer.from_numpy(ctx, a) for a in (points, q, sums, counters.astype(np.uint32))]
    d_pts, d_q, d_sums, d_cnt = bufs
    d_rows = DeviceBuffer(ctx, len(pairs) * BATCH_MAX * 16)
    bufs.append(d_rows)
    try:
        for distance in (1, 0):
            rows = {}
            for k in (1, 2, 0):
                ctx.h2d(d_rows.ptr, np.full((len(pairs), BATCH_MAX, 16), SENTINEL, np.uint8))
                try:
                    ctx.set_policy(capi.POLICY_MATCH_SPLITS, k)
                    if guide == PROJECTED:
                        ctx.match8_batch_projected(d_pts.ptr, d_q.ptr, d_sums.ptr, d_cnt.ptr, 4, BATCH_MAX, pairs, models,
                                                   capi.Camera(*CAM), radius, d_rows.ptr, distance)
                    else:
                        ctx.match8_batch_guided(d_pts.ptr, d_q.ptr, d_sums.ptr, d_cnt.ptr, 4, BATCH_MAX, pairs, guide,
                                                models, radius, d_rows.ptr, distance)
                    ctx.synchronize()
                finally:
                    ctx.set_policy(capi.POLICY_MATCH_SPLITS, 0)
                rows[k] = d_rows.to_numpy(capi.MatchRow, (len(pairs), BATCH_MAX))
                assert rows[k].tobytes() == rows[1].tobytes(), (guide, distance, k)  # the same bytes under every split
            assert d_pts.to_numpy(SIFT_POINT_DTYPE, points.shape).tobytes() == points.tobytes()
            for p, (a, b) in enumerate(pairs):
                na, nb = int(counters[a]), int(counters[b])
                what = "guide %d d%d pair %d (%d, %d)" % (guide, distance, p, a, b)
                got = rows[1][p]
                if na == 0 or nb == 0:  # no row for a pair with an empty frame
                    assert (got.view(np.uint8) == SENTINEL).all(), what
                    continue
                assert (got[na:].view(np.uint8) == SENTINEL).all(), what
                assert (got["reserved"][:na] == 0).all(), what
                s1 = np.concatenate([points[a, :na], points[a, :TAIL]])
                pair = Pair8(ctx, s1, points[b, :nb].copy(), q[a, :na], q[b, :nb])
                try:
                    call = pair.run(guide, models[p], radius, distance, 1)
                finally:
                    pair.free()
                for f in ("score", "ambiguity", "match"):
                    assert got[f][:na].tobytes() == np.ascontiguousarray(call[f][:na]).tobytes(), (what, f)
                mask = mask_of(guide, models[p], points[a, :na], points[b, :nb], radius)
                want = match8_guided_model(q[a, :na], q[b, :nb], distance, points[b, :nb]["coords2D"], mask)
                for f in ("score", "ambiguity", "match"):
                    assert got[f][:na].tobytes() == want[f].tobytes(), (what, f)
    finally:
        for b in bufs:
            b.free()
