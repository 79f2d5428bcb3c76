"""The matcher (cusift_amd/csrc/sift_match.hip, match_tile.inc) held to zero tolerance: every field of every row.

The model.  `match_model` is the scan the kernel's header states, written out in numpy for a float32 score matrix:
sixteen lanes scan their columns (c mod 16) with strict compares, a tree over the lanes (len = 8, 4, 2, 1: lane tx takes
lane tx + len, ties keep the lower lane), and the column splits folded in ascending order with the tree's two steps.
With one split it is the reference's FindMaxCorr / FindMinCorr, and the oracle agrees with it byte for byte (a CPU test
below).

The inputs.  Descriptors whose entries are small integers, or small integers over 16 or 64, and sparse: every partial
sum of every dot product is then exact in float32 in any order, so the MFMA chain, the oracle's wrapped fmaf chain and
a float64 matrix product all give the same bits, and 2 - 2 dot is exact too.  What remains is routing (which element
meets which), masking (which columns count), the tie rule and the arithmetic of the ambiguity -- all of it compared with
`tobytes()`.  No tolerance appears in this file.

Forced splits go through POLICY_MATCH_SPLITS = k; `cols_per_split` mirrors the host's arithmetic (cusift_match sizes
the splits from n2, cusift_match_batch from max_pts).  The binding does not expose the CU count, so an automatic run
must equal the model at one of the split counts the host can choose, 1 .. ceil(n / 128).
"""
import numpy as np
import pytest

from oracle_binding import SIFT_POINT_DTYPE

FIELDS = ("score", "ambiguity", "match", "match_xpos", "match_ypos")
REC = SIFT_POINT_DTYPE.itemsize  # 588
HUGE = 1 << 30
INIT = {1: np.float32(999.0), 0: np.float32(-1.0)}  # extras/matching.cu:3 and the padded columns of ComputeDistance
SENTINEL = 0xAB


# ----------------------------------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------------------------------
def _beats(val, cur, l2):
    return val < cur if l2 else val > cur


def _scan(best, second, idx, val, i, l2):
    """FindMinCorr / FindMaxCorr's update over row vectors: a strict compare moves the old best to second, otherwise
    a strict compare against second replaces it.  A NaN changes nothing: both compares are false."""
    win = _beats(val, best, l2)
    place = ~win & _beats(val, second, l2)
    return np.where(win, val, best), np.where(win, best, np.where(place, val, second)), np.where(win, i, idx)


def _take(best, second, idx, ob, os_, oi, l2):
    """What the tree and the split fold do: the update with the other's best and index, then its second against ours."""
    best, second, idx = _scan(best, second, idx, ob, oi, l2)
    return best, np.where(_beats(os_, second, l2), os_, second), idx


def match_model(S, l2, cols_per_split):
    """(best float32 [n1], second float32 [n1], idx int32 [n1]) of the float32 score matrix S[n1, n2]."""
    S = np.asarray(S)
    assert S.dtype == np.float32 and S.ndim == 2
    l2 = bool(l2)
    n1, n2 = S.shape
    init = INIT[int(l2)]
    acc = None
    for c0 in range(0, max(n2, 1), cols_per_split):
        best = np.full((n1, 16), init, np.float32)
        second = np.full((n1, 16), init, np.float32)
        idx = np.full((n1, 16), -1, np.int32)
        for c in range(c0, min(c0 + cols_per_split, n2)):
            t = c % 16
            best[:, t], second[:, t], idx[:, t] = _scan(best[:, t], second[:, t], idx[:, t], S[:, c], np.int32(c), l2)
        for ln in (8, 4, 2, 1):
            best[:, :ln], second[:, :ln], idx[:, :ln] = _take(best[:, :ln], second[:, :ln], idx[:, :ln],
                                                              best[:, ln:2 * ln], second[:, ln:2 * ln],
                                                              idx[:, ln:2 * ln], l2)
        part = (best[:, 0].copy(), second[:, 0].copy(), idx[:, 0].copy())
        acc = part if acc is None else _take(*acc, *part, l2)
    return acc[0].astype(np.float32), acc[1].astype(np.float32), acc[2].astype(np.int32)


def ambiguity(best, second, l2):
    """extras/matching.cu:143,222: the 1e-6 is a double constant, `1 - x` is float arithmetic; stored as float."""
    with np.errstate(all="ignore"):
        if l2:
            return (best.astype(np.float64) / (second.astype(np.float64) + 1e-6)).astype(np.float32)
        one = np.float32(1)
        return ((one - best).astype(np.float64) / ((one - second).astype(np.float64) + 1e-6)).astype(np.float32)


def cols_per_split(n, k):
    """The host's split arithmetic for POLICY_MATCH_SPLITS = k over n columns (n2, or max_pts in the batch)."""
    splits = min(k, -(-n // 32))
    return -(-(-(-n // splits)) // 32) * 32


def auto_candidates(n):
    """cols_per_split of every split count the automatic choice can make: 1 .. ceil(n / 128)."""
    return sorted({cols_per_split(n, k) for k in range(1, -(-n // 128) + 1)})


def score_matrix(d1, d2, l2, exact=True):
    """float32 S[n1, n2] of two descriptor arrays from a float64 product.  With exact=True the product must survive the
    float32 round trip (NaNs aside): then every summation order gives these bits."""
    with np.errstate(all="ignore"):
        dot64 = d1.astype(np.float64) @ d2.astype(np.float64).T
        dot = dot64.astype(np.float32)
        if exact:
            ok = np.isnan(dot64) | (dot.astype(np.float64) == dot64)
            assert ok.all(), "the inputs are not exact in float32"
        if not l2:
            return dot
        # ComputeL2Distance :71-72; 2 * dot is exact, one rounding in the subtraction
        return np.where(dot > np.float32(-1), np.float32(2) - np.float32(2) * dot, np.float32(999.0)).astype(np.float32)


def expected_fields(s1, s2, l2, cps, exact=True):
    """The five match fields of cusift_match(s1, s2) by the model at `cps` columns per split."""
    best, second, idx = match_model(score_matrix(s1["data"], s2["data"], l2, exact), l2, cps)
    m = np.where((idx >= 0) & (idx < len(s2)), idx, 0)  # the reference reads sift2[-1]; kernel and oracle read [0]
    return {"score": best, "ambiguity": ambiguity(best, second, l2), "match": idx,
            "match_xpos": s2["coords2D"][m, 0].copy(), "match_ypos": s2["coords2D"][m, 1].copy()}


def fields_of(recs):
    return {f: np.ascontiguousarray(recs[f]) for f in FIELDS}


def assert_same_fields(got, want, what):
    for f in FIELDS:
        g, w = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        assert g.dtype == w.dtype and g.shape == w.shape, (what, f, g.dtype, w.dtype)
        if g.tobytes() != w.tobytes():
            bad = np.nonzero(g.view(np.uint32) != w.view(np.uint32))[0]
            raise AssertionError("%s: %s differs on %d of %d rows, first %s: got %s, want %s"
                                 % (what, f, len(bad), len(g), bad[:8], g[bad[:8]], w[bad[:8]]))


def same_fields(got, want):
    return all(np.ascontiguousarray(got[f]).tobytes() == np.ascontiguousarray(want[f]).tobytes() for f in FIELDS)


# ----------------------------------------------------------------------------------------------------------------------
# the inputs
# ----------------------------------------------------------------------------------------------------------------------
def records(data):
    """Records around a descriptor array, every other field distinct so that match_xpos / match_ypos name a record."""
    n = len(data)
    p = np.zeros(n, SIFT_POINT_DTYPE)
    p["data"] = data
    p["coords2D"][:, 0] = 10.0 + np.arange(n)
    p["coords2D"][:, 1] = 5000.0 - 3.0 * np.arange(n)
    p["score"], p["ambiguity"], p["match"] = 0.25, 0.5, -5
    p["match_xpos"], p["match_ypos"] = -77.0, -78.0
    return p


def exact_descriptors(rng, n, family):
    """'sparse16': entries k / 16, k in 0..15, 15 % non-zero.  'ties': entries 0..3, 10 % non-zero -- rich in tied
    scores.  Either way a dot product is a short sum of small multiples of 1 / 256: exact in float32 in any order."""
    if family == "sparse16":
        return (rng.integers(0, 16, (n, 128)) * (rng.random((n, 128)) < 0.15) / 16.0).astype(np.float32)
    assert family == "ties"
    return (rng.integers(0, 4, (n, 128)) * (rng.random((n, 128)) < 0.10)).astype(np.float32)


def exact_pair(n1, n2, family):
    rng = np.random.default_rng(2)
    return records(exact_descriptors(rng, n1, family)), records(exact_descriptors(rng, n2, family))


def one_hot(ks, scale=1.0):
    d = np.zeros((len(ks), 128), np.float32)
    d[np.arange(len(ks)), ks] = scale
    return d


# ----------------------------------------------------------------------------------------------------------------------
# without a GPU
# ----------------------------------------------------------------------------------------------------------------------
def oracle_fields(oracle, s1, s2, distance):
    want = s1.copy()
    oracle.match(want, s2, distance)
    return fields_of(want)


@pytest.mark.parametrize("family", ("sparse16", "ties"))
@pytest.mark.parametrize("n1,n2", [(1, 1), (17, 33), (70, 95), (65, 257)])
def test_model_equals_oracle_on_exact_inputs(oracle, n1, n2, family):
    s1, s2 = exact_pair(n1, n2, family)
    dot64 = s1["data"].astype(np.float64) @ s2["data"].astype(np.float64).T
    assert np.array_equal(dot64.astype(np.float32).astype(np.float64), dot64)  # exact: any order, the same bits
    for distance in (1, 0):
        assert_same_fields(expected_fields(s1, s2, distance, HUGE), oracle_fields(oracle, s1, s2, distance),
                           "model against oracle, distance %d" % distance)


@pytest.mark.parametrize("n1,n2", [(70, 95), (65, 257)])
def test_tie_inputs_exercise_the_rule(n1, n2):
    """Conditions on the tie-rich inputs, not on the kernel: they must be able to tell the documented tie rule from
    'lowest index wins' and from 'the split layout does not matter'."""
    s1, s2 = exact_pair(n1, n2, "ties")
    for l2 in (1, 0):
        S = score_matrix(s1["data"], s2["data"], l2)
        top = S.min(axis=1) if l2 else S.max(axis=1)
        tied = (S == top[:, None]).sum(axis=1) > 1
        one = match_model(S, l2, HUGE)[2]
        tiles = match_model(S, l2, 32)[2]
        lowest = (S == top[:, None]).argmax(axis=1)
        print("(%d, %d) l2=%d: %d tied rows, %d rows differ between one split and 32-column splits, %d winners are not "
              "the lowest index" % (n1, n2, l2, tied.sum(), (one != tiles).sum(), (one != lowest).sum()))
        assert tied.sum() >= 5
        assert (one != tiles).any()
        assert (one != lowest).any()
        assert not (one != tiles)[~tied].any() and not (one != lowest)[~tied].any()  # only a tie can move an index


def test_cols_per_split_mirrors_the_host_arithmetic():
    """The figures the issue and the planted-position test rely on."""
    assert [cols_per_split(97, k) for k in (1, 2, 4, 1000)] == [97 // 32 * 32 + 32, 64, 32, 32]
    assert [cols_per_split(160, k) for k in (1, 2)] == [160, 96]
    assert cols_per_split(1, 1000) == 32 and cols_per_split(257, 3) == 96
    assert auto_candidates(95) == [96] and auto_candidates(257) == [96, 160, 288]


# ----------------------------------------------------------------------------------------------------------------------
# on the GPU
# ----------------------------------------------------------------------------------------------------------------------
def gpu_match(ctx, s1, s2, distance, splits=0, lead2=0, n1=None, n2=None):
    """cusift_match with POLICY_MATCH_SPLITS = splits (0: automatic) over uploads of the whole arrays s1 and s2; the
    call names n1 records of s1 and n2 records of s2 starting at record `lead2`.  Returns all of s1 read back."""
    from cusift_amd import capi
    from cusift_amd.capi import DeviceBuffer

    n1 = len(s1) if n1 is None else n1
    n2 = len(s2) - lead2 if n2 is None else n2
    d1, d2 = DeviceBuffer.from_numpy(ctx, s1), DeviceBuffer.from_numpy(ctx, s2)
    try:
        ctx.set_policy(capi.POLICY_MATCH_SPLITS, splits)
        ctx.match(d1.ptr, n1, d2.ptr + lead2 * REC, n2, distance)
        ctx.synchronize()
    finally:
        ctx.set_policy(capi.POLICY_MATCH_SPLITS, 0)
    out = d1.to_numpy(SIFT_POINT_DTYPE, (len(s1),))
    d1.free()
    d2.free()
    return out


def check_all_split_settings(ctx, oracle, s1, s2, distance, forced, what):
    """Forced splits against the model at the mirrored cols_per_split, one split against the oracle too, the automatic
    choice against the model at one of the host's possible split counts."""
    n2 = len(s2)
    models = {}

    def model(cps):
        if cps not in models:
            models[cps] = expected_fields(s1, s2, distance, cps)
        return models[cps]

    for k in forced:
        got = gpu_match(ctx, s1, s2, distance, k)
        assert_same_fields(fields_of(got), model(cols_per_split(n2, k)), "%s, %d splits asked, model" % (what, k))
        if k == 1:
            assert_same_fields(fields_of(got), oracle_fields(oracle, s1, s2, distance), "%s, one split, oracle" % what)
        assert got["data"].tobytes() == s1["data"].tobytes()
    got = fields_of(gpu_match(ctx, s1, s2, distance, 0))
    cands = auto_candidates(n2)
    if not any(same_fields(got, model(c)) for c in cands):
        assert_same_fields(got, model(cands[-1]), "%s, automatic splits (none of %s columns per split fits)" % (what, cands))


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
@pytest.mark.parametrize("family", ("sparse16", "ties"))
@pytest.mark.parametrize("n1,n2", [(1, 1), (16, 32), (17, 33), (64, 31), (65, 257), (70, 95), (129, 160)])
def test_gpu_exact_inputs_every_field_every_row(ctx, oracle, n1, n2, family, distance):
    s1, s2 = exact_pair(n1, n2, family)
    check_all_split_settings(ctx, oracle, s1, s2, distance, (1, 2, 3, 1000), "(%d, %d) %s d%d" % (n1, n2, family, distance))


def routing_inputs(variant):
    """(a) 'b': 128 rows e_k against 64 columns whose element k is perm_k[c] / 64, a permutation of 0..63 per k: the dot
    product of row k and column c is element k of column c, so row k is decided by that one k lane of the B staging
    (chunk, LDS row and float offset), with a unique winner (63) and runner-up (62).
    (b) 'a' / 'a-swapped': the transpose, 128 columns e_k against 64 rows, so that one k lane of the A fragments decides.
    Sixty-four rows cannot each have 128 distinct values out of 0..63, so a row takes 63 at one k, 62 at another and
    values below 62 elsewhere: row i is won by column i with runner-up 64 + i, and the other way round when swapped.
    Over the two variants every k is some row's winner and some row's runner-up."""
    rng = np.random.default_rng(7)
    if variant == "b":
        cols = np.stack([rng.permutation(64) for _ in range(128)], axis=1)  # [c, k]
        return records(one_hot(np.arange(128))), records((cols / 64.0).astype(np.float32))
    m = rng.integers(0, 62, (64, 128))
    hi, lo = (63, 62) if variant == "a" else (62, 63)
    m[np.arange(64), np.arange(64)] = hi
    m[np.arange(64), 64 + np.arange(64)] = lo
    return records((m / 64.0).astype(np.float32)), records(one_hot(np.arange(128)))


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
@pytest.mark.parametrize("variant", ("b", "a", "a-swapped"))
def test_gpu_operand_routing_every_k_lane_decides_a_row(ctx, oracle, variant, distance):
    s1, s2 = routing_inputs(variant)
    S = score_matrix(s1["data"], s2["data"], 0)
    srt = np.sort(S, axis=1)
    assert (srt[:, -1] > srt[:, -2]).all() and (srt[:, -2] > srt[:, -3]).all()  # unique winner and runner-up
    win, run = S.argmax(axis=1), np.argsort(S, axis=1)[:, -2]
    if variant == "b":  # the deciding element of row k is k
        assert np.array_equal(np.nonzero(s1["data"])[1], np.arange(128))
    else:  # winners and runners-up together are every k
        assert sorted(np.r_[win, run]) == list(range(128))
    want = oracle_fields(oracle, s1, s2, distance)
    assert np.array_equal(want["match"], win)
    for k in (1, 2):
        got = fields_of(gpu_match(ctx, s1, s2, distance, k))
        assert_same_fields(got, expected_fields(s1, s2, distance, cols_per_split(len(s2), k)), "%s, %d splits" % (variant, k))
        assert_same_fields(got, want, "%s, %d splits, oracle" % (variant, k))


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
@pytest.mark.parametrize("shift", (1, 16, 32, 33, 96))
def test_gpu_planted_positions(ctx, shift, distance):
    """Rows e_i, columns 8 e_c + 4 e_((c - shift) mod 97): row i scores 8 at column i, 4 at column (i + shift) mod 97
    and 0 elsewhere, so every column is one row's best and another row's second.  The shifts put the two in the same
    lane (16, 32), neighbouring lanes (1, 33), neighbouring tiles (32, 33), different splits, and wrapped round the end
    (96); 1, 2 and 4 splits are 97, 64 and 32 columns per split."""
    n = 97
    cols = one_hot(np.arange(n), 8.0) + one_hot((np.arange(n) - shift) % n, 4.0)
    s1, s2 = records(one_hot(np.arange(n))), records(cols)
    dot = score_matrix(s1["data"], s2["data"], 0)
    assert np.array_equal(dot, 8 * np.eye(n, dtype=np.float32) + 4 * np.roll(np.eye(n, dtype=np.float32), shift, axis=1))
    best = np.full(n, -14.0 if distance else 8.0, np.float32)
    second = np.full(n, -6.0 if distance else 4.0, np.float32)
    for k, cps in ((1, 128), (2, 64), (4, 32)):
        assert cols_per_split(n, k) == cps
        got = fields_of(gpu_match(ctx, s1, s2, distance, k))
        what = "shift %d, %d splits" % (shift, k)
        assert np.array_equal(got["match"], np.arange(n)), what
        assert got["score"].tobytes() == best.tobytes(), what
        assert got["ambiguity"].tobytes() == ambiguity(best, second, distance).tobytes(), what
        assert_same_fields(got, expected_fields(s1, s2, distance, cps), what)


def match_field_mask():
    mask = np.zeros(REC, bool)
    for f in FIELDS:
        off = SIFT_POINT_DTYPE.fields[f][1]
        mask[off:off + 4] = True
    assert mask.sum() == 20
    return mask


@pytest.mark.gpu
@pytest.mark.parametrize("n2", (1, 31, 33, 95))
@pytest.mark.parametrize("n1", (1, 63, 65))
def test_gpu_bounds_and_untouched_bytes(ctx, n1, n2):
    """Image 2 is records [3, 3 + n2) of a buffer whose other 43 records would win every row (64 on every element); image
    1 is the first n1 records of a buffer of n1 + 70, a sentinel in every other byte.  Only the n2 real columns may be
    candidates, and only the five match fields of the n1 real rows may change."""
    rng = np.random.default_rng(1000 * n1 + n2)
    real1, real2 = exact_descriptors(rng, n1, "sparse16"), exact_descriptors(rng, n2, "sparse16")
    assert (real1.sum(axis=1) > 0).all()  # every row would take a super winner
    buf2 = records(np.full((3 + n2 + 40, 128), 64.0, np.float32))
    buf2["data"][3:3 + n2] = real2
    s2 = buf2[3:3 + n2].copy()
    raw1 = np.full((n1 + 70, REC), SENTINEL, np.uint8)
    buf1 = raw1.view(SIFT_POINT_DTYPE).reshape(-1)
    buf1["data"][:n1] = real1
    s1 = buf1[:n1].copy()
    before = buf1.copy().view(np.uint8).reshape(-1, REC)
    mask = match_field_mask()
    for distance in (1, 0):
        for k in (1, 2):
            what = "(%d, %d) d%d, %d splits" % (n1, n2, distance, k)
            got = gpu_match(ctx, buf1, buf2, distance, k, lead2=3, n1=n1, n2=n2)
            after = got.view(np.uint8).reshape(-1, REC)
            assert np.array_equal(after[n1:], before[n1:]), what  # the 70 trailing records
            assert np.array_equal(after[:n1][:, ~mask], before[:n1][:, ~mask]), what
            assert ((got["match"][:n1] >= 0) & (got["match"][:n1] < n2)).all(), what
            assert_same_fields(fields_of(got[:n1]), expected_fields(s1, s2, distance, cols_per_split(n2, k)), what)


def check_against_model_and_oracle(ctx, oracle, s1, s2, what, splits=(1, 2)):
    out = {}
    for distance in (1, 0):
        want = oracle_fields(oracle, s1, s2, distance)
        for k in splits:
            got = fields_of(gpu_match(ctx, s1, s2, distance, k))
            assert_same_fields(got, expected_fields(s1, s2, distance, cols_per_split(len(s2), k)),
                               "%s, d%d, %d splits" % (what, distance, k))
            if k == 1:
                assert_same_fields(got, want, "%s, d%d, oracle" % (what, distance))
            out[distance, k] = got
    return out


@pytest.mark.gpu
def test_gpu_nan_column_is_never_chosen_and_disturbs_no_row(ctx, oracle):
    """Element 127 is 1 in every row and 0 in every column but one, which is -e_127: it scores a dot product of exactly
    -1 against every row, the clamp in L2 and no strict win in dot -- out of contention, like the padded columns.  The
    same column with a NaN in it must give the same bytes on every row."""
    n1, n2, c = 37, 47, 37
    rng = np.random.default_rng(5)
    d1, d2 = exact_descriptors(rng, n1, "sparse16"), exact_descriptors(rng, n2, "sparse16")
    d1[:, 127], d2[:, 127] = 1.0, 0.0
    d2[c] = 0.0
    d2[c, 127] = -1.0
    quiet = check_against_model_and_oracle(ctx, oracle, records(d1), records(d2), "column out of contention")
    d2[c, 19] = np.nan
    nan = check_against_model_and_oracle(ctx, oracle, records(d1), records(d2), "NaN column")
    for key in quiet:
        assert_same_fields(nan[key], quiet[key], "NaN column against the quiet column, %s" % (key,))
        assert (nan[key]["match"] != c).all() and (nan[key]["match"] >= 0).all()


@pytest.mark.gpu
def test_gpu_nan_row_matches_nothing(ctx, oracle):
    n1, n2, r = 37, 47, 21
    rng = np.random.default_rng(6)
    d1, d2 = exact_descriptors(rng, n1, "sparse16"), exact_descriptors(rng, n2, "sparse16")
    clean = check_against_model_and_oracle(ctx, oracle, records(d1), records(d2), "clean rows")
    d1[r, 77] = np.nan
    s2 = records(d2)
    out = check_against_model_and_oracle(ctx, oracle, records(d1), s2, "NaN row")
    others = np.arange(n1) != r
    for (distance, k), got in out.items():
        init = INIT[distance]
        assert got["match"][r] == -1 and got["score"][r].tobytes() == init.tobytes()
        assert got["ambiguity"][r].tobytes() == ambiguity(init.reshape(1), init.reshape(1), distance)[0].tobytes()
        assert got["match_xpos"][r] == s2["coords2D"][0, 0] and got["match_ypos"][r] == s2["coords2D"][0, 1]
        assert_same_fields({f: got[f][others] for f in FIELDS}, {f: clean[distance, k][f][others] for f in FIELDS},
                           "rows beside the NaN row")


@pytest.mark.gpu
def test_gpu_clamp_at_exactly_minus_one(ctx, oracle):
    """ComputeL2Distance keeps 2 - 2 dot only where dot > -1 (extras/matching.cu:71-72): e_k against -e_k scores 999, and
    -0.5 e_k scores exactly 3."""
    ks = np.array([0, 5, 64, 127])
    rows = records(one_hot(ks))
    for j, k in enumerate(ks):
        for scale, score, match in ((-1.0, 999.0, -1), (-0.5, 3.0, 0)):
            col = records(one_hot([k], scale))
            got = check_against_model_and_oracle(ctx, oracle, rows, col, "k %d, column %g e_k" % (k, scale), splits=(1,))
            l2 = got[1, 1]
            assert l2["score"][j] == np.float32(score) and l2["match"][j] == match
            others = np.arange(len(ks)) != j
            assert (l2["score"][others] == np.float32(2.0)).all() and (l2["match"][others] == 0).all()
            dot = got[0, 1]  # -1 is no strict win over the initial -1; -0.5 and 0 are
            assert dot["score"][j] == np.float32(scale) and dot["match"][j] == match
    # every row against every column's negative: the own column is clamped, the other 127 tie at 2 (0 in dot)
    every = records(one_hot(np.arange(128)))
    out = check_against_model_and_oracle(ctx, oracle, every, records(one_hot(np.arange(128), -1.0)), "128 negatives")
    for (distance, k), got in out.items():
        assert (got["match"] != np.arange(128)).all() and (got["match"] >= 0).all()
        assert (got["score"] == np.float32(2.0 if distance else 0.0)).all()


@pytest.mark.gpu
def test_gpu_all_zero_descriptors(ctx, oracle):
    n1, n2 = 37, 47
    rng = np.random.default_rng(8)
    d1, d2 = exact_descriptors(rng, n1, "sparse16"), exact_descriptors(rng, n2, "sparse16")
    d1[[0, 20]] = 0.0  # such a row ties every column at 2 (0 in dot)
    d2[[7, 46]] = 0.0
    out = check_against_model_and_oracle(ctx, oracle, records(d1), records(d2), "zero descriptors")
    for (distance, k), got in out.items():
        assert (got["score"][[0, 20]] == np.float32(2.0 if distance else 0.0)).all()
        assert (got["ambiguity"][[0, 20]] == ambiguity(got["score"][[0, 20]], got["score"][[0, 20]], distance)).all()
    check_against_model_and_oracle(ctx, oracle, records(np.zeros((5, 128), np.float32)),
                                   records(np.zeros((40, 128), np.float32)), "nothing but zeros")


BATCH_MAX = 160
BATCH_COUNTERS = np.array([95, 160, 0, 33, 4000], np.uint32)
BATCH_PAIRS = np.array([(0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (2, 2), (4, 1), (1, 4), (3, 4), (4, 3), (3, 3)], np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
@pytest.mark.parametrize("family", ("sparse16", "ties"))
def test_gpu_batch_rows_equal_the_model(ctx, family, distance):
    """cusift_match_batch over five frames in 160-record slots with counters 95, 160, 0, 33 and 4000 (clamped to 160):
    a self pair, the empty frame on either side, the clamped frame on either side.  Every slot holds a live-looking
    record, so a stage that ignores a count shows.  The splits are sized from max_pts."""
    from cusift_amd import capi
    from cusift_amd.capi import DeviceBuffer

    rng = np.random.default_rng(2)
    points = np.stack([records(exact_descriptors(rng, BATCH_MAX, family)) for _ in range(5)])
    for f in range(5):
        points["coords2D"][f] += 1000.0 * f
    counts = np.minimum(BATCH_COUNTERS, BATCH_MAX).astype(int)
    n_pairs = len(BATCH_PAIRS)

    def expected(cps):
        raw = np.full((n_pairs, BATCH_MAX, 16), SENTINEL, np.uint8)
        rows = raw.view(capi.MatchRow).reshape(n_pairs, BATCH_MAX)
        for p, (a, b) in enumerate(BATCH_PAIRS):
            na, nb = counts[a], counts[b]
            if na == 0 or nb == 0:
                continue  # nothing to match: no row of the pair is written
            want = expected_fields(points[a, :na], points[b, :nb], distance, cps)
            rows["score"][p, :na], rows["ambiguity"][p, :na] = want["score"], want["ambiguity"]
            rows["match"][p, :na], rows["reserved"][p, :na] = want["match"], 0
        return rows

    def run(k):
        d_pts, d_cnt = DeviceBuffer.from_numpy(ctx, points), DeviceBuffer.from_numpy(ctx, BATCH_COUNTERS)
        d_rows = DeviceBuffer.from_numpy(ctx, np.full((n_pairs, BATCH_MAX, 16), SENTINEL, np.uint8))
        try:
            ctx.set_policy(capi.POLICY_MATCH_SPLITS, k)
            ctx.match_batch(d_pts.ptr, d_cnt.ptr, 5, BATCH_MAX, BATCH_PAIRS, d_rows.ptr, distance)
            ctx.synchronize()
        finally:
            ctx.set_policy(capi.POLICY_MATCH_SPLITS, 0)
        assert d_pts.to_numpy(SIFT_POINT_DTYPE, points.shape).tobytes() == points.tobytes()  # the records: untouched
        return d_rows.to_numpy(capi.MatchRow, (n_pairs, BATCH_MAX))

    def compare(got, want, what):
        for p, (a, b) in enumerate(BATCH_PAIRS):
            for f in capi.MatchRow.names:
                bad = np.nonzero(got[f][p].view(np.uint32) != want[f][p].view(np.uint32))[0]
                assert not len(bad), "%s, pair %d (%d, %d): %s differs on rows %s: got %s, want %s" % (
                    what, p, a, b, f, bad[:8], got[f][p][bad[:8]], want[f][p][bad[:8]])
        assert got.tobytes() == want.tobytes(), what

    for k in (1, 2):
        compare(run(k), expected(cols_per_split(BATCH_MAX, k)), "%d splits" % k)
    got = run(0)
    cands = [expected(c) for c in auto_candidates(BATCH_MAX)]
    if not any(got.tobytes() == c.tobytes() for c in cands):
        compare(got, cands[-1], "automatic splits")
