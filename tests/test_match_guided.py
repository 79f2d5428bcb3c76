"""Guided matching (cusift_match_guided, cusift_match_batch_guided; cusift_amd/csrc/sift_match.hip: GuideH / GuideF) held
to zero tolerance: every field of every row.

The expectation is the matcher's model of tests/test_matching_exact.py applied to np.where(mask, S, INIT): a column that
fails the geometric test scores the initial value for that row.  `guide_mask` restates the definition of
include/cusift_amd_extras.h in numpy -- float64 per row, float32 per pair, the same parenthesisation -- so the mask is
the kernel's bit for bit; the descriptors are the exact families of that file, so the scores are too.  No tolerance
appears in this file.
"""
import numpy as np
import pytest

from oracle_binding import SIFT_POINT_DTYPE
from test_matching_exact import (ambiguity, assert_same_fields, auto_candidates, cols_per_split, exact_descriptors,
                                 match_model, records, score_matrix)

FIELDS = ("score", "ambiguity", "match", "match_xpos", "match_ypos")
REC = SIFT_POINT_DTYPE.itemsize
INIT = {1: np.float32(999.0), 0: np.float32(-1.0)}
SENTINEL = 0xAB
HOMOGRAPHY, EPIPOLAR = 0, 1
H_MILD = np.array([1.02, 0.03, -2.0, -0.02, 0.98, 3.0, 1e-4, -2e-4, 1.0])
F_MILD = np.array([0.0, 1e-3, -0.05, -1e-3, 0.0, -1.0, 0.05, 1.0, 0.5])
MILD = {HOMOGRAPHY: (H_MILD, 27.0), EPIPOLAR: (F_MILD, 10.0)}  # (model, radius): 10-30 % of the pairs below pass


# ----------------------------------------------------------------------------------------------------------------------
# the definition, restated
# ----------------------------------------------------------------------------------------------------------------------
def guide_mask(model, M, xy1, xy2, radius):
    """bool [n1, n2]: does column j pass the test against row i.  xy1 / xy2: float32 [n, 2] coords2D."""
    M = np.asarray(M, np.float64).reshape(9)
    xy1, xy2 = np.asarray(xy1, np.float32), np.asarray(xy2, np.float32)
    x1, y1 = xy1[:, 0].astype(np.float64), xy1[:, 1].astype(np.float64)
    x2, y2 = xy2[None, :, 0], xy2[None, :, 1]
    r2 = np.float32(radius) * np.float32(radius)
    with np.errstate(all="ignore"):
        t0 = (M[0] * x1 + M[1] * y1) + M[2]
        t1 = (M[3] * x1 + M[4] * y1) + M[5]
        t2 = (M[6] * x1 + M[7] * y1) + M[8]
        if model == HOMOGRAPHY:
            px, py = (t0 / t2).astype(np.float32)[:, None], (t1 / t2).astype(np.float32)[:, None]
            dx, dy = x2 - px, y2 - py
            out = dx * dx + dy * dy < r2
        else:
            assert model == EPIPOLAR
            n = np.sqrt(t0 * t0 + t1 * t1)
            line = (n > 0) & (n < np.inf) & (np.abs(t2) < np.inf)
            a, b, c = (np.where(line, t / n, np.nan).astype(np.float32)[:, None] for t in (t0, t1, t2))
            d = (a * x2 + b * y2) + c
            out = d * d < r2
    assert out.dtype == bool and out.shape == (len(xy1), len(xy2))
    return out


def guided_fields(s1, s2, l2, cps, mask):
    """The five match fields of cusift_match_guided(s1, s2) by the model at `cps` columns per split."""
    S = np.where(mask, score_matrix(s1["data"], s2["data"], l2), INIT[int(l2)]).astype(np.float32)
    best, second, idx = match_model(S, l2, cps)
    m = np.where((idx >= 0) & (idx < len(s2)), idx, 0)
    return {"score": best, "ambiguity": ambiguity(best, second, l2), "match": idx,
            "match_xpos": s2["coords2D"][m, 0].copy(), "match_ypos": s2["coords2D"][m, 1].copy()}


def fields_of(recs):
    return {f: np.ascontiguousarray(recs[f]) for f in FIELDS}


def same_fields(got, want):
    return all(np.ascontiguousarray(got[f]).tobytes() == np.ascontiguousarray(want[f]).tobytes() for f in FIELDS)


def nothing_fields(n, l2, s2):
    init = np.full(n, INIT[int(l2)], np.float32)
    return {"score": init, "ambiguity": ambiguity(init, init, l2), "match": np.full(n, -1, np.int32),
            "match_xpos": np.full(n, s2["coords2D"][0, 0], np.float32),
            "match_ypos": np.full(n, s2["coords2D"][0, 1], np.float32)}


# ----------------------------------------------------------------------------------------------------------------------
# the inputs
# ----------------------------------------------------------------------------------------------------------------------
def scattered(rng, data):
    """records() around `data` with coords2D on a quarter-pixel grid in [0, 100)^2."""
    p = records(data)
    p["coords2D"] = (rng.integers(0, 400, (len(data), 2)) / 4.0).astype(np.float32)
    return p


def scattered_pair(n1, n2, family, seed=3):
    rng = np.random.default_rng(seed)
    return scattered(rng, exact_descriptors(rng, n1, family)), scattered(rng, exact_descriptors(rng, n2, family))


# ----------------------------------------------------------------------------------------------------------------------
# without a GPU: the restatement on hand-made cases
# ----------------------------------------------------------------------------------------------------------------------
def test_mask_homography_radius_is_strict():
    x1, x2 = np.array([[10, 20]], np.float32), np.array([[13, 24]], np.float32)
    assert not guide_mask(HOMOGRAPHY, np.eye(3), x1, x2, 5.0)[0, 0]  # 25 < 25 is false
    assert guide_mask(HOMOGRAPHY, np.eye(3), x1, x2, np.nextafter(np.float32(5), np.float32(np.inf)))[0, 0]
    assert guide_mask(HOMOGRAPHY, np.eye(3), x1, x2, np.inf)[0, 0]


def test_mask_epipolar_horizontal_lines():
    F = [[0, 0, 0], [0, 0, -1], [0, 1, 0]]  # l = (0, -1, y1): d = y1 - y2
    x1 = np.array([[3, 7], [50, 9.5]], np.float32)
    x2 = np.array([[80, 7], [-4, 8.5], [0, 9.5], [1, 5]], np.float32)
    got = guide_mask(EPIPOLAR, F, x1, x2, 1.0)
    assert got.tolist() == [[True, False, False, False], [False, False, True, False]]  # |d| = 1 is no pass
    assert guide_mask(EPIPOLAR, F, x1, x2, 1.5).tolist() == [[True, False, False, False], [False, True, True, False]]
    assert guide_mask(EPIPOLAR, F, x1, x2, 2.25).tolist() == [[True, True, False, True], [False, True, True, False]]


@pytest.mark.parametrize("model", (HOMOGRAPHY, EPIPOLAR))
def test_mask_zero_and_nan_models_pass_nothing(model):
    s1, s2 = scattered_pair(17, 33, "sparse16")
    for M in (np.zeros(9), np.full(9, np.nan), np.r_[np.eye(3).ravel()[:8], np.nan], np.full(9, np.inf)):
        for radius in (1.0, 1e6, np.inf):
            assert not guide_mask(model, M, s1["coords2D"], s2["coords2D"], radius).any()


def test_mask_rows_with_w_zero_pass_nothing():
    H = [1, 0, 0, 0, 1, 0, 1, 0, -10]  # W = x1 - 10
    x1 = np.array([[10, 5], [10, 0], [0, 0], [11, 5]], np.float32)  # X / 0 = inf, the same, 0 / -10, 11 / 1
    x2 = np.array([[0, 0], [11, 5], [1e30, 1e30]], np.float32)
    for radius in (1.0, 1e6, np.inf):
        got = guide_mask(HOMOGRAPHY, H, x1, x2, radius)
        assert not got[:2].any()
        assert got[2, 0] and got[3, 1]
    # and an epipolar row whose line has no direction: l0 = l1 = 0 at x1 = (0, 0) only
    F = [1, 0, 0, 0, 1, 0, 0, 0, 1]
    got = guide_mask(EPIPOLAR, F, np.array([[0, 0], [3, 4]], np.float32), x2, 1e6)
    assert not got[0].any() and got[1, :2].all()


@pytest.mark.parametrize("model", (HOMOGRAPHY, EPIPOLAR))
@pytest.mark.parametrize("n1,n2", [(17, 33), (64, 31), (65, 257), (70, 95), (129, 160)])
def test_mild_models_pass_a_tenth_to_a_third(n1, n2, model):
    """The condition on the GPU test's inputs, where a machine without a GPU sees it too."""
    s1, s2 = scattered_pair(n1, n2, "sparse16")
    share = guide_mask(model, MILD[model][0], s1["coords2D"], s2["coords2D"], MILD[model][1]).mean()
    assert 0.10 <= share <= 0.30, share


# ----------------------------------------------------------------------------------------------------------------------
# on the GPU
# ----------------------------------------------------------------------------------------------------------------------
def gpu_guided(ctx, s1, s2, distance, model, M, radius, splits=0, lead2=0, n1=None, n2=None, both=False):
    """cusift_match_guided with POLICY_MATCH_SPLITS = splits over uploads of the whole arrays, as gpu_match of
    test_matching_exact.py.  Returns all of s1 read back (both=True: and all of s2)."""
    from cusift_amd import capi
    from cusift_amd.capi import DeviceBuffer

    n1 = len(s1) if n1 is None else n1
    n2 = len(s2) - lead2 if n2 is None else n2
    d1, d2 = DeviceBuffer.from_numpy(ctx, s1), DeviceBuffer.from_numpy(ctx, s2)
    try:
        ctx.set_policy(capi.POLICY_MATCH_SPLITS, splits)
        ctx.match_guided(d1.ptr, n1, d2.ptr + lead2 * REC, n2, model, M, radius, distance)
        ctx.synchronize()
        out1, out2 = d1.to_numpy(SIFT_POINT_DTYPE, (len(s1),)), d2.to_numpy(SIFT_POINT_DTYPE, (len(s2),))
    finally:
        ctx.set_policy(capi.POLICY_MATCH_SPLITS, 0)
        d1.free()
        d2.free()
    return (out1, out2) if both else out1


def check_every_split_setting(ctx, s1, s2, distance, model, M, radius, mask, what, forced=(1, 2, 3, 1000)):
    n2 = len(s2)
    models = {}

    def want(cps):
        if cps not in models:
            models[cps] = guided_fields(s1, s2, distance, cps, mask)
        return models[cps]

    for k in forced:
        got = gpu_guided(ctx, s1, s2, distance, model, M, radius, k)
        assert_same_fields(fields_of(got), want(cols_per_split(n2, k)), "%s, %d splits asked" % (what, k))
        assert got["data"].tobytes() == s1["data"].tobytes()
    got = fields_of(gpu_guided(ctx, s1, s2, distance, model, M, radius, 0))
    cands = auto_candidates(n2)
    if not any(same_fields(got, want(c)) for c in cands):
        assert_same_fields(got, want(cands[-1]), "%s, automatic splits (none of %s columns per split fits)" % (what, cands))


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
@pytest.mark.parametrize("family", ("sparse16", "ties"))
@pytest.mark.parametrize("n1,n2", [(1, 1), (17, 33), (64, 31), (65, 257), (70, 95), (129, 160)])
def test_gpu_every_field_every_row(ctx, n1, n2, family, distance):
    s1, s2 = scattered_pair(n1, n2, family)
    if (n1, n2) == (1, 1):  # one pair cannot pass by a fifth: it passes here, and fails under the far model below
        s2["coords2D"][0] = s1["coords2D"][0]
    for model in (HOMOGRAPHY, EPIPOLAR):
        M, radius = MILD[model]
        mask = guide_mask(model, M, s1["coords2D"], s2["coords2D"], radius)
        print("(%d, %d) model %d: %.1f %% of the pairs pass" % (n1, n2, model, 100 * mask.mean()))
        assert (0.10 <= mask.mean() <= 0.30) if n1 * n2 > 1 else mask.all()
        check_every_split_setting(ctx, s1, s2, distance, model, M, radius, mask,
                                  "(%d, %d) %s d%d model %d" % (n1, n2, family, distance, model))


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
@pytest.mark.parametrize("n1,n2", [(1, 1), (70, 95), (65, 257)])
def test_gpu_radius_1e6_equals_cusift_match(ctx, n1, n2, distance):
    from test_matching_exact import gpu_match

    for family in ("sparse16", "ties"):
        s1, s2 = scattered_pair(n1, n2, family)
        for k in (1, 2, 0):
            plain = gpu_match(ctx, s1, s2, distance, k)
            for model in (HOMOGRAPHY, EPIPOLAR):
                assert guide_mask(model, MILD[model][0], s1["coords2D"], s2["coords2D"], 1e6).all()
                got = gpu_guided(ctx, s1, s2, distance, model, MILD[model][0], 1e6, k)
                assert_same_fields(fields_of(got), fields_of(plain), "%s, %d splits, model %d" % (family, k, model))
                assert got.tobytes() == plain.tobytes()


def sentinel_buffers(n1, n2, lead2, rng):
    """Image 1: n1 real records in front of 70 of sentinel bytes; image 2: records [lead2, lead2 + n2) of a buffer whose
    other records would win every row (64 on every element) and lie at the origin."""
    real1, real2 = exact_descriptors(rng, n1, "sparse16"), exact_descriptors(rng, n2, "sparse16")
    buf2 = scattered(rng, np.full((lead2 + n2 + 40, 128), 64.0, np.float32))
    buf2["coords2D"] = 0.0
    buf2[lead2:lead2 + n2] = scattered(rng, real2)
    raw1 = np.full((n1 + 70, REC), SENTINEL, np.uint8)
    buf1 = raw1.view(SIFT_POINT_DTYPE).reshape(-1)
    buf1[:n1] = scattered(rng, real1)
    return buf1, buf2


def match_field_mask():
    mask = np.zeros(REC, bool)
    for f in FIELDS:
        off = SIFT_POINT_DTYPE.fields[f][1]
        mask[off:off + 4] = True
    assert mask.sum() == 20
    return mask


@pytest.mark.gpu
@pytest.mark.parametrize("model", (HOMOGRAPHY, EPIPOLAR))
@pytest.mark.parametrize("n1,n2", [(1, 1), (63, 33), (65, 95)])
def test_gpu_nothing_passes(ctx, n1, n2, model):
    """A model that puts every partner 1e5 pixels away: every row is (init, the init ambiguity, -1, record 0's
    coordinates), and no other byte of either record set changes."""
    buf1, buf2 = sentinel_buffers(n1, n2, 3, np.random.default_rng(100 * n1 + n2))
    s2 = buf2[3:3 + n2].copy()
    M = [1, 0, 1e5, 0, 1, 1e5, 0, 0, 1] if model == HOMOGRAPHY else [0, 0, 0, 0, 0, -1, 0, 1, 1e5]
    assert not guide_mask(model, M, buf1["coords2D"][:n1], s2["coords2D"], 5.0).any()
    before1, before2 = buf1.copy().view(np.uint8).reshape(-1, REC), buf2.copy()
    fields = match_field_mask()
    for distance in (1, 0):
        for k in (1, 2):
            what = "(%d, %d) model %d d%d, %d splits" % (n1, n2, model, distance, k)
            got, got2 = gpu_guided(ctx, buf1, buf2, distance, model, M, 5.0, k, lead2=3, n1=n1, n2=n2, both=True)
            assert_same_fields(fields_of(got[:n1]), nothing_fields(n1, distance, s2), what)
            after = got.view(np.uint8).reshape(-1, REC)
            assert np.array_equal(after[n1:], before1[n1:]), what
            assert np.array_equal(after[:n1][:, ~fields], before1[:n1][:, ~fields]), what
            assert got2.tobytes() == before2.tobytes(), what


@pytest.mark.gpu
@pytest.mark.parametrize("at_origin", (0, 2))
@pytest.mark.parametrize("n2", (33, 95))
def test_gpu_padded_columns_at_the_origin_never_pass(ctx, n2, at_origin):
    """Every row is sent to (0, 0), where the columns past col_end -- zeros from the range-checked loads -- seem to lie,
    with a descriptor of zeros that scores 2 (0 in dot): only `live` keeps them out.  With no real column at the origin
    every row must come back unmatched; with two, the rows' second best must still be a real column's or the initial
    value."""
    n1 = 70
    buf1, buf2 = sentinel_buffers(n1, n2, 5, np.random.default_rng(n2 + at_origin))
    real = buf2[5:5 + n2]
    real["coords2D"] = np.maximum(real["coords2D"], 1.0)  # nobody at the origin ...
    real["coords2D"][[7, n2 - 1][:at_origin]] = 0.0  # ... but these
    s1, s2 = buf1[:n1].copy(), real.copy()
    H = [0, 0, 0, 0, 0, 0, 0, 0, 1]
    mask = guide_mask(HOMOGRAPHY, H, s1["coords2D"], s2["coords2D"], 0.5)
    assert mask.sum() == n1 * at_origin
    for distance in (1, 0):
        for k in (1, 2, 1000):
            what = "n2 %d, %d at the origin, d%d, %d splits" % (n2, at_origin, distance, k)
            got = gpu_guided(ctx, buf1, buf2, distance, HOMOGRAPHY, H, 0.5, k, lead2=5, n1=n1, n2=n2)[:n1]
            assert (got["match"] < n2).all(), what
            assert_same_fields(fields_of(got), guided_fields(s1, s2, distance, cols_per_split(n2, k), mask), what)
            if not at_origin:
                assert (got["match"] == -1).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
@pytest.mark.parametrize("column", (31, 32, 96, 64))
def test_gpu_one_passing_column_at_a_tile_boundary(ctx, column, distance):
    """Exactly one passing column per row -- the last of a tile, the first of the next, the last of all, the first of the
    second of two splits (97 columns: 64 per split): the winner is that column, the second best the initial value."""
    n1, n2 = 70, 97
    assert cols_per_split(n2, 2) == 64
    s1, s2 = scattered_pair(n1, n2, "sparse16", seed=column)
    s1["coords2D"] = (50.0, 50.0)
    s2["coords2D"][:, 0] += 200.0
    s2["coords2D"][column] = (50.25, 49.75)
    mask = guide_mask(HOMOGRAPHY, np.eye(3), s1["coords2D"], s2["coords2D"], 1.0)
    assert mask.sum(axis=1).tolist() == [1] * n1 and mask[:, column].all()
    S = score_matrix(s1["data"], s2["data"], distance)
    init = np.full(n1, INIT[distance], np.float32)
    for k in (1, 2, 1000):
        got = fields_of(gpu_guided(ctx, s1, s2, distance, HOMOGRAPHY, np.eye(3), 1.0, k))
        what = "column %d, d%d, %d splits" % (column, distance, k)
        assert_same_fields(got, guided_fields(s1, s2, distance, cols_per_split(n2, k), mask), what)
        if distance == 0:  # a dot product of 0 does beat -1; in L2 a score is never 999 here
            assert (S[:, column] > -1).all()
        assert np.array_equal(got["match"], np.full(n1, column)), what
        assert got["score"].tobytes() == S[:, column].tobytes(), what
        assert got["ambiguity"].tobytes() == ambiguity(S[:, column], init, distance).tobytes(), what


@pytest.mark.gpu
@pytest.mark.parametrize("model", (HOMOGRAPHY, EPIPOLAR))
@pytest.mark.parametrize("lead2", (3, 37))
def test_gpu_record_offset_of_image_2(ctx, lead2, model):
    """d_sift2 starts `lead2` records into its buffer: the coordinate staging must use the descriptors' base."""
    n1, n2 = 70, 95
    buf1, buf2 = sentinel_buffers(n1, n2, lead2, np.random.default_rng(lead2))
    s1, s2 = buf1[:n1].copy(), buf2[lead2:lead2 + n2].copy()
    M, radius = MILD[model]
    mask = guide_mask(model, M, s1["coords2D"], s2["coords2D"], radius)
    assert 0.10 <= mask.mean() <= 0.30
    for distance in (1, 0):
        for k in (1, 2):
            got = gpu_guided(ctx, buf1, buf2, distance, model, M, radius, k, lead2=lead2, n1=n1, n2=n2)[:n1]
            assert_same_fields(fields_of(got), guided_fields(s1, s2, distance, cols_per_split(n2, k), mask),
                               "lead %d, model %d, d%d, %d splits" % (lead2, model, distance, k))


@pytest.mark.gpu
def test_gpu_refusals_write_nothing(ctx):
    from cusift_amd import capi
    from cusift_amd.capi import DeviceBuffer

    s1, s2 = scattered_pair(70, 95, "sparse16")
    d1, d2 = DeviceBuffer.from_numpy(ctx, s1), DeviceBuffer.from_numpy(ctx, s2)
    pts = np.stack([s2, s2])
    d_pts = DeviceBuffer.from_numpy(ctx, pts)
    d_rows = DeviceBuffer.from_numpy(ctx, np.full((1, 95, 16), SENTINEL, np.uint8))
    bad = [(2, H_MILD, 5.0), (-1, H_MILD, 5.0), (HOMOGRAPHY, None, 5.0), (EPIPOLAR, None, 5.0), (HOMOGRAPHY, H_MILD, 0.0),
           (EPIPOLAR, F_MILD, -1.0), (HOMOGRAPHY, H_MILD, float("nan"))]
    for model, M, radius in bad:
        with pytest.raises(capi.CusiftError):
            ctx.match_guided(d1.ptr, 70, d2.ptr, 95, model, M, radius, 1)
        with pytest.raises(capi.CusiftError):
            ctx.match_batch_guided(d_pts.ptr, None, 2, 95, [(0, 1)], model, M, radius, d_rows.ptr, 1)
    with pytest.raises(capi.CusiftError):  # what cusift_match refuses
        ctx.match_guided(d1.ptr, 70, d2.ptr, 95, HOMOGRAPHY, H_MILD, 5.0, 2)
    ctx.synchronize()
    assert d1.to_numpy(SIFT_POINT_DTYPE, (70,)).tobytes() == s1.tobytes()
    assert d2.to_numpy(SIFT_POINT_DTYPE, (95,)).tobytes() == s2.tobytes()
    assert d_pts.to_numpy(SIFT_POINT_DTYPE, pts.shape).tobytes() == pts.tobytes()
    assert (d_rows.to_numpy(np.uint8, (1, 95, 16)) == SENTINEL).all()
    # counts <= 0: fine, and nothing happens -- whatever the geometry says
    ctx.match_guided(d1.ptr, 0, d2.ptr, 95, 7, None, -1.0, 1)
    ctx.match_guided(d1.ptr, 70, d2.ptr, 0, 7, None, -1.0, 1)
    ctx.match_guided(d1.ptr, 70, d2.ptr, 95, EPIPOLAR, F_MILD, np.inf, 1)  # an infinite radius is legal
    ctx.synchronize()
    assert d2.to_numpy(SIFT_POINT_DTYPE, (95,)).tobytes() == s2.tobytes()
    for d in (d1, d2, d_pts, d_rows):
        d.free()


BATCH_MAX = 160
BATCH_COUNTERS = np.array([95, 160, 33], np.uint32)
BATCH_PAIRS = np.array([(0, 1), (1, 0), (2, 2), (0, 2)], np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
@pytest.mark.parametrize("model", (HOMOGRAPHY, EPIPOLAR))
def test_gpu_batch_rows_equal_the_pair_call(ctx, model, distance):
    """Three frames of 95, 160 and 33 records in 160-record slots, four pairs, a model of its own per pair: pair p's rows
    are the fields the pair call writes under model p (and the numpy model's), rows past frame 1's count keep their
    bytes, the records are not written."""
    from cusift_amd import capi
    from cusift_amd.capi import DeviceBuffer

    rng = np.random.default_rng(11)
    points = np.stack([scattered(rng, exact_descriptors(rng, BATCH_MAX, "ties")) for _ in range(3)])
    base, radius = MILD[model]
    models = np.tile(base, (len(BATCH_PAIRS), 1))
    models[:, 2 if model == HOMOGRAPHY else 8] += 7.0 * np.arange(len(BATCH_PAIRS))  # pair p: 7 p pixels further along

    def mask_of(p, m):
        a, b = BATCH_PAIRS[p]
        return guide_mask(model, m, points[a, :BATCH_COUNTERS[a]]["coords2D"], points[b, :BATCH_COUNTERS[b]]["coords2D"],
                          radius)

    masks = [mask_of(p, models[p]) for p in range(len(BATCH_PAIRS))]
    assert all(0.05 <= m.mean() <= 0.35 for m in masks), [m.mean() for m in masks]
    for p in range(1, len(BATCH_PAIRS)):  # another pair's model would show
        assert all((masks[p] != mask_of(p, models[o])).mean() > 0.02 for o in range(len(BATCH_PAIRS)) if o != p)
    for k in (1, 2):
        d_pts, d_cnt = DeviceBuffer.from_numpy(ctx, points), DeviceBuffer.from_numpy(ctx, BATCH_COUNTERS)
        d_rows = DeviceBuffer.from_numpy(ctx, np.full((len(BATCH_PAIRS), BATCH_MAX, 16), SENTINEL, np.uint8))
        try:
            ctx.set_policy(capi.POLICY_MATCH_SPLITS, k)
            ctx.match_batch_guided(d_pts.ptr, d_cnt.ptr, 3, BATCH_MAX, BATCH_PAIRS, model, models, radius, d_rows.ptr,
                                   distance)
            ctx.synchronize()
        finally:
            ctx.set_policy(capi.POLICY_MATCH_SPLITS, 0)
        assert d_pts.to_numpy(SIFT_POINT_DTYPE, points.shape).tobytes() == points.tobytes()
        rows = d_rows.to_numpy(capi.MatchRow, (len(BATCH_PAIRS), BATCH_MAX))
        for d in (d_pts, d_cnt, d_rows):
            d.free()
        cps = cols_per_split(BATCH_MAX, k)  # the batch sizes its splits from max_pts
        for p, (a, b) in enumerate(BATCH_PAIRS):
            na, nb = int(BATCH_COUNTERS[a]), int(BATCH_COUNTERS[b])
            s1, s2 = points[a, :na].copy(), points[b, :nb].copy()
            what = "pair %d (%d, %d), %d splits" % (p, a, b, k)
            want = guided_fields(s1, s2, distance, cps, masks[p])
            for f in ("score", "ambiguity", "match"):
                assert rows[f][p, :na].tobytes() == want[f].tobytes(), (what, f)
            assert (rows["reserved"][p, :na] == 0).all(), what
            assert (rows[p, na:].view(np.uint8) == SENTINEL).all(), what
            if cols_per_split(nb, k) == cps or k == 1:  # the pair call sizes its splits from n2: the same scan
                pair = gpu_guided(ctx, s1, s2, distance, model, models[p], radius, k)
                for f in ("score", "ambiguity", "match"):
                    assert rows[f][p, :na].tobytes() == np.ascontiguousarray(pair[f]).tobytes(), (what, f)
