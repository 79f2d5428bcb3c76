"""Mutual nearest neighbours from one pass: cusift_match_mutual, cusift_select_mutual, cusift_match_batch_mutual
(cusift_amd/csrc/sift_match.hip, match_block with a ColumnSide), held to zero tolerance like the matcher.

The row side must be byte for byte what cusift_match writes under the same split setting.  The column side is defined by
`column_model`: FindMinCorr / FindMaxCorr's update run over the rows 0, 1, ..., n1 - 1 in ascending order from
(init, init, -1) with strict compares -- the lowest row wins an exactly tied best, a tie for best gives second == best, a
NaN changes nothing -- and the ambiguity arithmetic of the row side.  It depends on no split count and no grid.

The inputs, helpers and the score matrix come from test_matching_exact.py (exact float32 families: every summation order
gives the same bits).  No tolerance appears in this file: every comparison is on `tobytes()`.
"""
import os

import numpy as np
import pytest

from oracle_binding import SIFT_POINT_DTYPE, read_vlfeat_sift
from test_matching_exact import (FIELDS, HUGE, INIT, REC, SENTINEL, ambiguity, assert_same_fields, cols_per_split,
                                 exact_descriptors, exact_pair, fields_of, gpu_match, match_field_mask, match_model,
                                 records, routing_inputs, score_matrix)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SHAPES = [(1, 1), (16, 32), (17, 33), (64, 31), (65, 257), (70, 95), (129, 160)]


# ----------------------------------------------------------------------------------------------------------------------
# the model of the column side
# ----------------------------------------------------------------------------------------------------------------------
def column_model(S, l2):
    """(best float32 [n2], second float32 [n2], idx int32 [n2]) of the float32 score matrix S[n1, n2]: top2_scan over the
    rows in ascending order."""
    S = np.asarray(S)
    assert S.dtype == np.float32 and S.ndim == 2
    n1, n2 = S.shape
    init = INIT[int(bool(l2))]
    best, second, idx = np.full(n2, init, np.float32), np.full(n2, init, np.float32), np.full(n2, -1, np.int32)
    for i in range(n1):
        v = S[i]
        win = v < best if l2 else v > best
        place = ~win & (v < second if l2 else v > second)
        second = np.where(win, best, np.where(place, v, second))
        idx = np.where(win, np.int32(i), idx)
        best = np.where(win, v, best)
    return best.astype(np.float32), second.astype(np.float32), idx.astype(np.int32)


def column_fields(s1, s2, l2, exact=True):
    """The five match fields of s2 after cusift_match_mutual(s1, s2)."""
    best, second, idx = column_model(score_matrix(s1["data"], s2["data"], l2, exact), l2)
    m = np.where((idx >= 0) & (idx < len(s1)), idx, 0)
    return {"score": best, "ambiguity": ambiguity(best, second, l2), "match": idx,
            "match_xpos": s1["coords2D"][m, 0].copy(), "match_ypos": s1["coords2D"][m, 1].copy()}


# ----------------------------------------------------------------------------------------------------------------------
# without a GPU
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ("sparse16", "ties"))
@pytest.mark.parametrize("n1,n2", [(1, 1), (17, 33), (70, 95), (65, 257)])
def test_column_model_has_the_stated_properties(n1, n2, family):
    """Brute force, column by column: best is the extreme, idx the lowest row attaining it, second the extreme after one
    instance of the best is removed (init when nothing is left or nothing beats it)."""
    s1, s2 = exact_pair(n1, n2, family)
    for l2 in (1, 0):
        S = score_matrix(s1["data"], s2["data"], l2)
        best, second, idx = column_model(S, l2)
        init = INIT[l2]
        for j in range(n2):
            col = [float(v) for v in S[:, j]]
            cand = [v for v in col if (v < init if l2 else v > init)]  # what can enter at all
            if not cand:
                assert best[j] == init and second[j] == init and idx[j] == -1
                continue
            top = min(cand) if l2 else max(cand)
            assert best[j] == np.float32(top)
            assert idx[j] == col.index(top)
            cand.remove(top)
            rest = (min(cand) if l2 else max(cand)) if cand else float(init)
            assert second[j] == np.float32(rest), (j, second[j], rest)


@pytest.mark.parametrize("n1,n2", [(70, 95), (129, 160)])
def test_tie_inputs_exercise_the_column_rule(n1, n2):
    """A condition on the inputs, not on the kernel: enough columns have a tied best, and for some of them 'lowest row'
    differs from what the row side's scan (sixteen lanes and a tree) of the transposed matrix would name."""
    s1, s2 = exact_pair(n1, n2, "ties")
    for l2 in (1, 0):
        S = score_matrix(s1["data"], s2["data"], l2)
        best, _, idx = column_model(S, l2)
        tied = (S == best[None, :]).sum(axis=0) > 1
        other = match_model(np.ascontiguousarray(S.T), l2, HUGE)[2]
        print("(%d, %d) l2=%d: %d tied columns, %d winners differ from the transposed row scan"
              % (n1, n2, l2, tied.sum(), (idx != other).sum()))
        assert tied.sum() >= 5
        assert (idx != other)[tied].any()
        assert not (idx != other)[~tied].any()  # only a tie can move an index


# ----------------------------------------------------------------------------------------------------------------------
# on the GPU
# ----------------------------------------------------------------------------------------------------------------------
def gpu_mutual(ctx, s1, s2, distance, splits=0, lead2=0, n1=None, n2=None):
    """cusift_match_mutual with POLICY_MATCH_SPLITS = splits over uploads of the whole arrays; the call names n1 records
    of s1 and n2 records of s2 from record `lead2`.  Returns all of s1 and all of s2 read back."""
    from cusift_amd import capi
    from cusift_amd.capi import DeviceBuffer

    n1 = len(s1) if n1 is None else n1
    n2 = len(s2) - lead2 if n2 is None else n2
    d1, d2 = DeviceBuffer.from_numpy(ctx, s1), DeviceBuffer.from_numpy(ctx, s2)
    try:
        ctx.set_policy(capi.POLICY_MATCH_SPLITS, splits)
        ctx.match_mutual(d1.ptr, n1, d2.ptr + lead2 * REC, n2, distance)
        ctx.synchronize()
    finally:
        ctx.set_policy(capi.POLICY_MATCH_SPLITS, 0)
    out = d1.to_numpy(SIFT_POINT_DTYPE, (len(s1),)), d2.to_numpy(SIFT_POINT_DTYPE, (len(s2),))
    d1.free()
    d2.free()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
@pytest.mark.parametrize("family", ("sparse16", "ties"))
@pytest.mark.parametrize("n1,n2", SHAPES)
def test_gpu_every_field_of_both_sets(ctx, n1, n2, family, distance):
    s1, s2 = exact_pair(n1, n2, family)
    want2 = column_fields(s1, s2, distance)
    for k in (1, 2, 3, 1000, 0):
        what = "(%d, %d) %s d%d, splits %d" % (n1, n2, family, distance, k)
        got1, got2 = gpu_mutual(ctx, s1, s2, distance, k)
        assert got1.tobytes() == gpu_match(ctx, s1, s2, distance, k).tobytes(), what + ": the row side"
        assert_same_fields(fields_of(got2), want2, what + ": the column side")
        assert got2["data"].tobytes() == s2["data"].tobytes() and got2["coords2D"].tobytes() == s2["coords2D"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n1,n2", [(1, 1), (63, 31), (65, 33), (70, 95)])
def test_gpu_untouched_bytes_on_both_sides(ctx, n1, n2):
    """Both buffers hold more records than the call names: 3 before and 40 behind image 2's that would win every row, 70
    behind image 1's that would win every column, a sentinel in every byte that is not a descriptor."""
    rng = np.random.default_rng(1000 * n1 + n2)
    real1, real2 = exact_descriptors(rng, n1, "sparse16"), exact_descriptors(rng, n2, "sparse16")
    raw1 = np.full((n1 + 70, REC), SENTINEL, np.uint8)
    buf1 = raw1.view(SIFT_POINT_DTYPE).reshape(-1)
    buf1["data"] = 64.0
    buf1["data"][:n1] = real1
    raw2 = np.full((3 + n2 + 40, REC), SENTINEL, np.uint8)
    buf2 = raw2.view(SIFT_POINT_DTYPE).reshape(-1)
    buf2["data"] = 64.0
    buf2["data"][3:3 + n2] = real2
    s1, s2 = buf1[:n1].copy(), buf2[3:3 + n2].copy()
    before1 = buf1.copy().view(np.uint8).reshape(-1, REC)
    before2 = buf2.copy().view(np.uint8).reshape(-1, REC)
    mask = match_field_mask()
    for distance in (1, 0):
        for k in (1, 2):
            what = "(%d, %d) d%d, %d splits" % (n1, n2, distance, k)
            got1, got2 = gpu_mutual(ctx, buf1, buf2, distance, k, lead2=3, n1=n1, n2=n2)
            a1, a2 = got1.view(np.uint8).reshape(-1, REC), got2.view(np.uint8).reshape(-1, REC)
            assert np.array_equal(a1[n1:], before1[n1:]), what
            assert np.array_equal(a1[:n1][:, ~mask], before1[:n1][:, ~mask]), what
            assert np.array_equal(a2[:3], before2[:3]) and np.array_equal(a2[3 + n2:], before2[3 + n2:]), what
            assert np.array_equal(a2[3:3 + n2][:, ~mask], before2[3:3 + n2][:, ~mask]), what
            assert got1.tobytes() == gpu_match(ctx, buf1, buf2, distance, k, lead2=3, n1=n1, n2=n2).tobytes(), what
            assert_same_fields(fields_of(got2[3:3 + n2]), column_fields(s1, s2, distance), what)
            assert ((got2["match"][3:3 + n2] >= 0) & (got2["match"][3:3 + n2] < n1)).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
@pytest.mark.parametrize("variant", ("b", "a", "a-swapped"))
def test_gpu_operand_routing_for_the_column_side(ctx, variant, distance):
    """routing_inputs with the two sets swapped where needed, so that the COLUMNS are the decided side: every k lane of
    the A fragments ('b' transposed) or of the B staging ('a' transposed) decides some column's winner or runner-up."""
    r1, r2 = routing_inputs(variant)
    for s1, s2 in ((r1, r2), (r2, r1)):
        S = score_matrix(s1["data"], s2["data"], 0)
        want = column_fields(s1, s2, distance)
        if s1 is r2:  # the columns are routing_inputs' rows: a unique winner and runner-up each
            srt = np.sort(S, axis=0)
            assert (srt[-1] > srt[-2]).all() and (srt[-2] > srt[-3]).all()
            assert np.array_equal(want["match"], S.argmax(axis=0))
        for k in (1, 2):
            got1, got2 = gpu_mutual(ctx, s1, s2, distance, k)
            what = "%s%s d%d, %d splits" % (variant, " swapped sets" if s1 is r2 else "", distance, k)
            assert_same_fields(fields_of(got2), want, what)
            assert got1.tobytes() == gpu_match(ctx, s1, s2, distance, k).tobytes(), what


def fixture_pair():
    s1 = read_vlfeat_sift(os.path.join(GOLDEN, "vlfeat_sift1.bin"))
    s2 = read_vlfeat_sift(os.path.join(GOLDEN, "vlfeat_sift2.bin"))
    assert (len(s1), len(s2)) == (884, 856)
    return s1, s2


def check_reverse_agreement(ctx, s1, s2, distance, what):
    """The column side against cusift_match(s2, s1): score and ambiguity byte for byte, match wherever the column's best
    is unique (the reverse call's tie rule is the sixteen-lane scan, the column side's is the lowest row)."""
    _, got2 = gpu_mutual(ctx, s1, s2, distance)
    rev = gpu_match(ctx, s2, s1, distance)
    for f in ("score", "ambiguity"):
        bad = np.nonzero(got2[f].view(np.uint32) != rev[f].view(np.uint32))[0]
        if len(bad):
            with np.errstate(all="ignore"):
                rel = np.abs(got2[f][bad].astype(np.float64) - rev[f][bad]) / np.abs(rev[f][bad].astype(np.float64))
            print("%s: %s differs on %d of %d columns, largest relative difference %.3g" % (what, f, len(bad), len(rev),
                                                                                           np.nanmax(rel)))
        assert got2[f].tobytes() == rev[f].tobytes(), (what, f, len(bad))
    # a unique best: the runner-up differs from it (a tie for best gives second == best, i.e. ambiguity of equal scores)
    with np.errstate(all="ignore"):
        S = score_matrix(s1["data"], s2["data"], distance, exact=False)
    unique = (S == (S.min(axis=0) if distance else S.max(axis=0))[None, :]).sum(axis=0) == 1
    assert unique.sum() > 0
    assert np.array_equal(got2["match"][unique], rev["match"][unique]), what
    for f in ("match_xpos", "match_ypos"):
        assert got2[f][unique].tobytes() == rev[f][unique].tobytes(), (what, f)
    return got2, rev


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
@pytest.mark.parametrize("family", ("sparse16", "ties"))
def test_gpu_column_side_agrees_with_the_reverse_call_on_exact_inputs(ctx, family, distance):
    for n1, n2 in ((70, 95), (129, 160)):
        s1, s2 = exact_pair(n1, n2, family)
        check_reverse_agreement(ctx, s1, s2, distance, "(%d, %d) %s d%d" % (n1, n2, family, distance))


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
def test_gpu_column_side_agrees_with_the_reverse_call_on_real_descriptors(ctx, distance):
    """884 x 856 VLFeat descriptors: S[i][j] is the same products in the same k order whichever operand is A."""
    s1, s2 = fixture_pair()
    check_reverse_agreement(ctx, s1, s2, distance, "VLFeat pair d%d" % distance)


def expected_selection(r1, r2, score_thresh, amb_thresh, kind3d, mutual):
    """cusift_select_matches / cusift_select_mutual from the fields, in float32 like the kernel."""
    s2, a2 = np.float32(score_thresh) * np.float32(score_thresh), np.float32(amb_thresh) * np.float32(amb_thresh)
    pairs, coord = [], []
    for i in range(len(r1)):
        p = r1[i]
        if not (p["score"] < s2 and p["ambiguity"] < a2):
            continue
        m = int(p["match"])
        if m < 0 or m >= len(r2):
            continue
        if kind3d and not (p["coords3D"][2] != 0 and r2["coords3D"][m, 2] != 0):
            continue
        if mutual and int(r2["match"][m]) != i:
            continue
        pairs.append((i, m))
        coord.append(np.r_[p["coords3D"], r2["coords3D"][m]])
    return np.array(pairs, np.int32).reshape(-1, 2), np.array(coord, np.float32).reshape(-1, 6)


def run_selection(ctx, call, r1, r2, score_thresh, amb_thresh, kind):
    from cusift_amd.capi import DeviceBuffer

    n1 = len(r1)
    d1, d2 = DeviceBuffer.from_numpy(ctx, r1), DeviceBuffer.from_numpy(ctx, r2)
    d_pairs = DeviceBuffer.from_numpy(ctx, np.full((n1, 2), -9, np.int32))
    d_coord = DeviceBuffer.from_numpy(ctx, np.full((n1, 6), -9.0, np.float32))
    d_count = DeviceBuffer.from_numpy(ctx, np.full(1, -9, np.int32))
    call(d1.ptr, n1, d2.ptr, len(r2), d_pairs.ptr, d_coord.ptr, d_count.ptr, score_thresh, amb_thresh, kind)
    ctx.synchronize()
    out = (d_pairs.to_numpy(np.int32, (n1, 2)), d_coord.to_numpy(np.float32, (n1, 6)),
           int(d_count.to_numpy(np.int32, (1,))[0]))
    for b in (d1, d2, d_pairs, d_coord, d_count):
        b.free()
    return out


def with_depths(recs, seed):
    """coords3D with non-zero z on about three records in four, z == 0 (the 'no depth' mark) on the rest."""
    rng = np.random.default_rng(seed)
    recs = recs.copy()
    recs["coords3D"] = rng.uniform(0.5, 4.0, (len(recs), 3)).astype(np.float32)
    recs["coords3D"][rng.random(len(recs)) < 0.25, 2] = 0.0
    assert (recs["coords3D"][:, 2] == 0).any() and (recs["coords3D"][:, 2] != 0).any()
    return recs


@pytest.mark.gpu
@pytest.mark.parametrize("case", ("fixture", "ties"))
def test_gpu_select_mutual(ctx, case):
    if case == "fixture":
        s1, s2 = fixture_pair()
        thresholds = (999.0, 0.95)
    else:
        s1, s2 = exact_pair(129, 160, "ties")
        thresholds = (999.0, 1.01)  # tied bests (ambiguity 1 - ulps) stay in: the cross-check decides among them
    r1, r2 = gpu_mutual(ctx, with_depths(s1, 1), with_depths(s2, 2), 1)
    for kind in ("2d", "3d"):
        want_p, want_c = expected_selection(r1, r2, *thresholds, kind == "3d", True)
        pairs, coord, count = run_selection(ctx, ctx.select_mutual, r1, r2, *thresholds, kind)
        what = "%s %s" % (case, kind)
        assert count == len(want_p), (what, count, len(want_p))
        assert pairs[:count].tobytes() == want_p.tobytes(), what
        assert coord[:count].tobytes() == want_c.tobytes(), what
        assert (pairs[count:] == -9).all() and (coord[count:] == -9.0).all(), what  # rows past the count: not written
        _, _, plain = run_selection(ctx, ctx.select_matches, r1, r2, *thresholds, kind)
        assert plain == len(expected_selection(r1, r2, *thresholds, kind == "3d", False)[0]), what
        print("%s: %d mutual of %d selected" % (what, count, plain))
        if case == "fixture":
            assert 0 < count < plain, (what, count, plain)  # the predicate bites


MUTUAL_MAX = 160
MUTUAL_COUNTERS = np.array([95, 160, 0], np.uint32)
MUTUAL_PAIRS = np.array([(0, 1), (1, 0), (1, 1), (0, 2), (2, 0)], np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
@pytest.mark.parametrize("family", ("sparse16", "ties"))
def test_gpu_batch_mutual(ctx, family, distance):
    """Three frames in 160-record slots with 95, 160 and 0 records; every slot holds a live-looking record, so a stage
    that ignores a count shows."""
    from cusift_amd import capi
    from cusift_amd.capi import DeviceBuffer

    rng = np.random.default_rng(3)
    points = np.stack([records(exact_descriptors(rng, MUTUAL_MAX, family)) for _ in range(3)])
    counts = MUTUAL_COUNTERS.astype(int)
    n_pairs = len(MUTUAL_PAIRS)
    want = np.full((n_pairs, MUTUAL_MAX, 16), SENTINEL, np.uint8).view(capi.MatchRow).reshape(n_pairs, MUTUAL_MAX)
    for p, (a, b) in enumerate(MUTUAL_PAIRS):
        na, nb = counts[a], counts[b]
        if na == 0 or nb == 0:
            continue  # frame 1 empty: no back row; frame 2 empty: no record to write a back row for
        best, second, idx = column_model(score_matrix(points[a, :na]["data"], points[b, :nb]["data"], distance), distance)
        want["score"][p, :nb], want["ambiguity"][p, :nb] = best, ambiguity(best, second, distance)
        want["match"][p, :nb], want["reserved"][p, :nb] = idx, 0
    fill = np.full((n_pairs, MUTUAL_MAX, 16), SENTINEL, np.uint8)
    for k in (1, 3):
        d_pts, d_cnt = DeviceBuffer.from_numpy(ctx, points), DeviceBuffer.from_numpy(ctx, MUTUAL_COUNTERS)
        d_rows, d_back, d_fwd = (DeviceBuffer.from_numpy(ctx, fill) for _ in range(3))
        try:
            ctx.set_policy(capi.POLICY_MATCH_SPLITS, k)
            ctx.match_batch_mutual(d_pts.ptr, d_cnt.ptr, 3, MUTUAL_MAX, MUTUAL_PAIRS, d_rows.ptr, d_back.ptr, distance)
            ctx.match_batch(d_pts.ptr, d_cnt.ptr, 3, MUTUAL_MAX, MUTUAL_PAIRS, d_fwd.ptr, distance)
            ctx.synchronize()
        finally:
            ctx.set_policy(capi.POLICY_MATCH_SPLITS, 0)
        what = "%s d%d, %d splits" % (family, distance, k)
        assert d_pts.to_numpy(SIFT_POINT_DTYPE, points.shape).tobytes() == points.tobytes(), what  # records: untouched
        rows, fwd = d_rows.to_numpy(capi.MatchRow, want.shape), d_fwd.to_numpy(capi.MatchRow, want.shape)
        assert (fwd["match"][0, :95] >= 0).all()  # the forward call did write
        assert rows.tobytes() == fwd.tobytes(), what + ": d_rows against cusift_match_batch"
        back = d_back.to_numpy(capi.MatchRow, want.shape)
        for p, (a, b) in enumerate(MUTUAL_PAIRS):
            for f in capi.MatchRow.names:
                bad = np.nonzero(back[f][p].view(np.uint32) != want[f][p].view(np.uint32))[0]
                assert not len(bad), "%s, pair %d (%d, %d): %s differs on back rows %s: got %s, want %s" % (
                    what, p, a, b, f, bad[:8], back[f][p][bad[:8]], want[f][p][bad[:8]])
        for b in (d_pts, d_cnt, d_rows, d_back, d_fwd):
            b.free()


@pytest.mark.gpu
def test_gpu_refusals_write_nothing(ctx):
    from cusift_amd import capi
    from cusift_amd.capi import DeviceBuffer

    lib, INVALID = capi.lib(), -1
    s1, s2 = exact_pair(40, 50, "sparse16")
    both = np.concatenate([s1, s2])
    d = DeviceBuffer.from_numpy(ctx, both)
    h = ctx.handle
    # overlapping ranges: the same set, a shifted window, the second set starting inside the first
    assert lib.cusift_match_mutual(h, d.ptr, 40, d.ptr, 40, 1) == INVALID
    assert lib.cusift_match_mutual(h, d.ptr, 40, d.ptr + 39 * REC, 50, 1) == INVALID
    assert lib.cusift_match_mutual(h, d.ptr + 10 * REC, 40, d.ptr, 11, 0) == INVALID
    # an unknown distance, a missing buffer
    assert lib.cusift_match_mutual(h, d.ptr, 40, d.ptr + 40 * REC, 50, 2) == INVALID
    assert lib.cusift_match_mutual(h, d.ptr, 40, None, 50, 1) == INVALID
    # a count of 0 on either side: nothing to match, nothing written
    assert lib.cusift_match_mutual(h, d.ptr, 0, d.ptr + 40 * REC, 50, 1) == 0
    assert lib.cusift_match_mutual(h, d.ptr, 40, d.ptr + 40 * REC, 0, 1) == 0
    # the pair-list form: a NULL d_rows_back, a bad pair index, an unknown distance
    pairs = np.array([(0, 1)], np.int32)
    rows = DeviceBuffer.from_numpy(ctx, np.full((2, 45, 16), SENTINEL, np.uint8))
    back = rows.ptr + 45 * 16
    args = (h, d.ptr, None, 2, 45)
    assert lib.cusift_match_batch_mutual(*args, pairs.ctypes.data, 1, 1, rows.ptr, None) == INVALID
    assert lib.cusift_match_batch_mutual(*args, np.array([(0, 2)], np.int32).ctypes.data, 1, 1, rows.ptr, back) == INVALID
    assert lib.cusift_match_batch_mutual(*args, pairs.ctypes.data, 1, 7, rows.ptr, back) == INVALID
    assert lib.cusift_match_batch_mutual(*args, None, 1, 1, rows.ptr, back) == INVALID
    # the selection keeps cusift_select_matches' refusals
    assert lib.cusift_select_mutual(h, d.ptr, 40, d.ptr + 40 * REC, 50, 999.0, 1.0, 2, rows.ptr, rows.ptr, rows.ptr) == INVALID
    assert lib.cusift_select_mutual(h, d.ptr, 40, d.ptr + 40 * REC, 50, 999.0, 1.0, 0, rows.ptr, rows.ptr, None) == INVALID
    ctx.synchronize()
    assert d.to_numpy(SIFT_POINT_DTYPE, both.shape).tobytes() == both.tobytes()
    assert (rows.to_numpy(np.uint8, (2, 45, 16)) == SENTINEL).all()
    # and the accepted call on the same buffers does write
    ctx.match_mutual(d.ptr, 40, d.ptr + 40 * REC, 50, 1)
    ctx.synchronize()
    after = d.to_numpy(SIFT_POINT_DTYPE, both.shape)
    assert (after["match"] >= 0).all()
    d.free()
    rows.free()
