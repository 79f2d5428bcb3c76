"""The fp32 matchers on DENSE descriptors, byte for byte against recorded results.

The exact suites (test_matching_exact.py, test_match_mutual.py, test_match_guided.py) use descriptors whose products and
sums are exactly representable, so they cannot see the ORDER of a dot product's fp32 sum.  Here the descriptors are
seeded dense unit vectors: every score depends on the k order of the MFMA chain, and every index and ambiguity on the
scores.  129 x 150 records: three row blocks, the last with one row; five tiles, the last partial; 96 + 54 columns at
two forced splits.  tests/golden/match_dense.json holds the SHA-256 of every field array each call wrote, recorded on an
MI355X from the build BEFORE the matchers were put on one block body (sift_match_common.h), and of the input.  No
tolerance, no case left out.  `digests(ctx)` is the whole procedure; a new golden is `json.dump` of it, run against the
build that is to be the reference, never against the code under test.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle_binding import SIFT_POINT_DTYPE
from test_match_guided import EPIPOLAR, HOMOGRAPHY, MILD, guide_mask

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "match_dense.json")
N1, N2, SLOTS = 129, 150, 160
PAIRS = ((0, 1), (1, 0), (2, 0), (0, 2))  # frame 2 is empty: on either side of a pair
POINT_FIELDS = ("score", "ambiguity", "match", "match_xpos", "match_ypos")
ROW_FIELDS = ("score", "ambiguity", "match", "reserved")
SENTINEL = 0xAB


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def dense_records(rng, n):
    """n records: a dense unit-length descriptor each (normal deviates, the norm a strictly sequential float64 sum),
    coords2D on a quarter-pixel grid in [0, 100)^2, match fields that no matcher writes."""
    d = rng.standard_normal((n, 128))
    d /= np.sqrt(np.cumsum(d * d, axis=1)[:, -1:])
    p = np.zeros(n, SIFT_POINT_DTYPE)
    p["data"] = d.astype(np.float32)
    p["coords2D"] = (rng.integers(0, 400, (n, 2)) / 4.0).astype(np.float32)
    p["score"], p["ambiguity"], p["match"] = 0.25, 0.5, -5
    p["match_xpos"], p["match_ypos"] = -77.0, -78.0
    return p


def inputs():
    """(s1, s2, batch): the pair, and batch [3][SLOTS] = s1, s2, nothing -- the slots past a count hold NaN descriptors."""
    rng = np.random.default_rng(20240607)
    s1, s2 = dense_records(rng, N1), dense_records(rng, N2)
    batch = np.zeros((3, SLOTS), SIFT_POINT_DTYPE)
    batch["data"] = np.float32(np.nan)
    batch["coords2D"] = np.float32(50.0)
    batch[0, :N1], batch[1, :N2] = s1, s2
    return s1, s2, batch


def input_digests():
    s1, s2, batch = inputs()
    return {"set1": sha(s1), "set2": sha(s2), "batch": sha(batch)}


def digests(ctx):
    """{call/distance/splits/array.field: sha256} of everything the fp32 matcher calls write for inputs()."""
    from cusift_amd import capi
    from cusift_amd.capi import MATCH_ROW_DTYPE, DeviceBuffer

    s1, s2, batch = inputs()
    counts = np.array([N1, N2, 0], np.uint32)
    models = {m: np.tile(np.asarray(MILD[m][0], np.float64), (len(PAIRS), 1)) for m in (HOMOGRAPHY, EPIPOLAR)}
    out = {}

    def put(key, arr, fields):
        for f in fields:
            out["%s.%s" % (key, f)] = sha(arr[f])

    def pair_call(key, run):
        d1, d2 = DeviceBuffer.from_numpy(ctx, s1), DeviceBuffer.from_numpy(ctx, s2)
        try:
            run(d1.ptr, d2.ptr)
            ctx.synchronize()
            put(key + "/set1", d1.to_numpy(SIFT_POINT_DTYPE, (N1,)), POINT_FIELDS)
            put(key + "/set2", d2.to_numpy(SIFT_POINT_DTYPE, (N2,)), POINT_FIELDS)  # unwritten unless mutual
        finally:
            d1.free()
            d2.free()

    def batch_call(key, run):
        d_pts, d_cnt = DeviceBuffer.from_numpy(ctx, batch), DeviceBuffer.from_numpy(ctx, counts)
        nbytes = len(PAIRS) * SLOTS * MATCH_ROW_DTYPE.itemsize
        d_rows, d_back = DeviceBuffer(ctx, nbytes), DeviceBuffer(ctx, nbytes)
        try:
            ctx.memset(d_rows.ptr, SENTINEL, nbytes)  # rows that are not written keep these bytes
            ctx.memset(d_back.ptr, SENTINEL, nbytes)
            run(d_pts.ptr, d_cnt.ptr, d_rows.ptr, d_back.ptr)
            ctx.synchronize()
            put(key + "/rows", d_rows.to_numpy(MATCH_ROW_DTYPE, (len(PAIRS), SLOTS)), ROW_FIELDS)
            put(key + "/rows_back", d_back.to_numpy(MATCH_ROW_DTYPE, (len(PAIRS), SLOTS)), ROW_FIELDS)
        finally:
            for b in (d_pts, d_cnt, d_rows, d_back):
                b.free()

    try:
        for dist in (1, 0):
            for splits in (1, 2):
                ctx.set_policy(capi.POLICY_MATCH_SPLITS, splits)
                tag = "/%s/splits%d" % ("l2" if dist else "dot", splits)
                pair_call("match" + tag, lambda a, b: ctx.match(a, N1, b, N2, dist))
                pair_call("match_mutual" + tag, lambda a, b: ctx.match_mutual(a, N1, b, N2, dist))
                batch_call("match_batch" + tag,
                           lambda p, c, r, rb: ctx.match_batch(p, c, 3, SLOTS, PAIRS, r, dist))
                batch_call("match_batch_mutual" + tag,
                           lambda p, c, r, rb: ctx.match_batch_mutual(p, c, 3, SLOTS, PAIRS, r, rb, dist))
                for model, name in ((HOMOGRAPHY, "h"), (EPIPOLAR, "f")):
                    M, radius = MILD[model]
                    pair_call("match_guided_%s%s" % (name, tag),
                              lambda a, b: ctx.match_guided(a, N1, b, N2, model, M, radius, dist))
                    batch_call("match_batch_guided_%s%s" % (name, tag),
                               lambda p, c, r, rb: ctx.match_batch_guided(p, c, 3, SLOTS, PAIRS, model, models[model],
                                                                          radius, r, dist))
    finally:
        ctx.set_policy(capi.POLICY_MATCH_SPLITS, 0)
    return out


def test_the_input_is_the_recorded_one_and_the_mild_models_pass_a_share_of_it():
    """FIRST: the random stream and the float arithmetic of `inputs` give the recorded bytes.  If this fails the generated
    input changed (numpy's generator or its arithmetic), not the matcher: the golden below then says nothing."""
    want = json.load(open(GOLDEN))["input"]
    assert input_digests() == want, "the generated INPUT differs from the recorded one: not a matcher change"
    s1, s2, _ = inputs()
    for model in (HOMOGRAPHY, EPIPOLAR):
        share = guide_mask(model, MILD[model][0], s1["coords2D"], s2["coords2D"], MILD[model][1]).mean()
        assert 0.05 <= share <= 0.35, (model, share)


@pytest.mark.gpu
def test_gpu_every_written_field_of_every_fp32_matcher_call_has_the_recorded_bytes(ctx):
    golden = json.load(open(GOLDEN))
    # the input first, and plainly: a difference here is a change of the generated input, not of the matcher
    assert input_digests() == golden["input"], "the generated INPUT differs from the recorded one: not a matcher change"
    got, want = digests(ctx), golden["output"]
    assert sorted(got) == sorted(want)
    wrong = sorted(k for k in want if got[k] != want[k])
    assert not wrong, "%d of %d field arrays differ from the recorded bytes: %s" % (len(wrong), len(want), wrong[:12])
