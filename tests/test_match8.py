"""8-bit descriptors (cusift_quantize_descriptors, cusift_desc8_sums, cusift_match8; cusift_amd/csrc/sift_match8.hip) held to
zero tolerance against tests/match8_model.py, the numpy int64 restatement of include/cusift_amd_extras.h: every byte of the
tables, both sums, and all five fields of every row.  No tolerance appears in this file.

The matcher's workgroup is 256 rows and its LDS tile 64 columns, so the size sweep adds 255 / 256 / 257 rows and
63 / 64 / 65 columns to the sizes around the fp32 matcher's 64 / 32.
"""
import numpy as np
import pytest

from match8_model import (FIELDS, INIT, SCALE, assert_fields_equal, keys_model, match8_model, quantize_model, sums_model)
from oracle_binding import SIFT_POINT_DTYPE

REC = SIFT_POINT_DTYPE.itemsize
SENTINEL = 0xAB
N1_SIZES = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257)
N2_SIZES = (1, 31, 32, 33, 63, 64, 65, 127, 129, 1000)
SPLITS = (0, 1, 2, 3, 7)


def records(n, seed=0):
    """n records whose descriptors are garbage (the 8-bit matcher must not read them) and whose match fields carry a
    sentinel; coords2D on a quarter-pixel grid."""
    rng = np.random.default_rng(seed)
    p = np.zeros(n, SIFT_POINT_DTYPE)
    p["coords2D"] = (rng.integers(0, 4000, (n, 2)) / 4.0).astype(np.float32)
    p["data"] = np.float32(np.nan)
    p["score"], p["ambiguity"], p["match"] = -7.0, -7.0, -77
    p["match_xpos"], p["match_ypos"] = -7.0, -7.0
    return p


class Tables:
    """Two byte tables and their sums on the device, the sums from the numpy model (desc8_sums has a test of its own)."""

    def __init__(self, ctx, q1, q2):
        from cusift_amd.capi import DeviceBuffer

        self.ctx, self.q1, self.q2 = ctx, np.ascontiguousarray(q1, np.uint8), np.ascontiguousarray(q2, np.uint8)
        self.s1, self.s2 = records(len(q1), 1), records(len(q2), 2)
        self.bufs = [DeviceBuffer.from_numpy(ctx, a) for a in (self.q1, sums_model(self.q1), self.q2, sums_model(self.q2),
                                                               self.s2)]
        self.d1 = DeviceBuffer(ctx, self.s1.nbytes)

    def match(self, distance, splits=0, n1=None, n2=None):
        """All of set 1's records after cusift_match8 over the first n1 rows and n2 columns."""
        from cusift_amd import capi

        n1 = len(self.q1) if n1 is None else n1
        n2 = len(self.q2) if n2 is None else n2
        dq1, ds1, dq2, ds2, d2 = (b.ptr for b in self.bufs)
        self.ctx.h2d(self.d1.ptr, self.s1)
        try:
            self.ctx.set_policy(capi.POLICY_MATCH_SPLITS, splits)
            self.ctx.match8(self.d1.ptr, n1, dq1, ds1, d2, n2, dq2, ds2, distance)
            self.ctx.synchronize()
        finally:
            self.ctx.set_policy(capi.POLICY_MATCH_SPLITS, 0)
        return self.d1.to_numpy(SIFT_POINT_DTYPE, (len(self.s1),))

    def check(self, distance, splits=0, n1=None, n2=None, what=""):
        n1 = len(self.q1) if n1 is None else n1
        n2 = len(self.q2) if n2 is None else n2
        got = self.match(distance, splits, n1, n2)
        want = match8_model(self.q1[:n1], self.q2[:n2], distance, self.s2["coords2D"][:n2])
        assert_fields_equal({f: got[f][:n1] for f in FIELDS}, want,
                            "%s %d x %d, distance %d, %d splits asked" % (what, n1, n2, distance, splits))
        # rows past n1 and everything that is not a match field: untouched
        assert got[n1:].tobytes() == self.s1[n1:].tobytes()
        for f in ("coords2D", "scale", "orientation"):
            assert got[f].tobytes() == self.s1[f].tobytes()
        assert got["data"].view(np.uint32).tobytes() == self.s1["data"].view(np.uint32).tobytes()
        return got

    def free(self):
        for b in self.bufs + [self.d1]:
            b.free()


# ----------------------------------------------------------------------------------------------------------------------
# without a GPU: the restatement on hand-made cases
# ----------------------------------------------------------------------------------------------------------------------
def test_model_quantiser_edges():
    f = np.float32
    up, down = (lambda x: np.nextafter(f(x), f(np.inf))), (lambda x: np.nextafter(f(x), f(-np.inf)))
    v = np.array([0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, 255 / 512, down(255 / 512), up(255 / 512), 1.0,
                  0.5 / 512, down(0.5 / 512), 1.5 / 512, down(1.5 / 512), 254.5 / 512, down(254.5 / 512)], np.float32)
    # the float below 0.5 / 512 still gives 1: t + 0.5 = 1 - 2^-25 is a tie between two floats and rounds to even, 1.0 --
    # the "one rounding" of the definition
    assert quantize_model(v).tolist() == [0, 0, 0, 0, 255, 0, 255, 255, 255, 255, 1, 1, 2, 1, 255, 254]
    assert quantize_model(np.array([0.25 / 512, 0.4999 / 512], np.float32)).tolist() == [0, 0]


def test_model_all_zero_and_all_255():
    z, o = np.zeros((3, 128), np.uint8), np.full((2, 128), 255, np.uint8)
    assert keys_model(o, o, 1).tolist() == [[0, 0]] * 2 and keys_model(o, o, 0).tolist() == [[-8323200] * 2] * 2
    assert keys_model(z, o, 1).tolist() == [[8323200] * 2] * 3 and keys_model(z, z, 0).tolist() == [[0] * 3] * 3
    m = match8_model(z, o, 1, np.zeros((2, 2), np.float32))
    assert m["match"].tolist() == [0, 0, 0] and m["score"][0] == np.float32(8323200) * SCALE
    assert m["ambiguity"][0] == np.float32(np.float64(m["score"][0]) / (np.float64(m["score"][0]) + 1e-6))  # second == best
    one = match8_model(z, o[:1], 0, np.zeros((1, 2), np.float32))
    assert one["score"].tolist() == [0.0] * 3 and one["ambiguity"][0] == np.float32(1.0 / (2.0 + 1e-6))  # second = -1


# ----------------------------------------------------------------------------------------------------------------------
# the quantiser on the GPU
# ----------------------------------------------------------------------------------------------------------------------
def quantize_on_gpu(ctx, pts, n_images, max_pts, counters):
    """(q uint8 [n_images, max_pts, 128], sums int32 [n_images, max_pts, 2]) over a 0xAB prefill."""
    from cusift_amd.capi import DeviceBuffer

    d_pts = DeviceBuffer.from_numpy(ctx, pts)
    d_cnt = None if counters is None else DeviceBuffer.from_numpy(ctx, np.asarray(counters, np.uint32))
    d_q, d_s = DeviceBuffer(ctx, n_images * max_pts * 128), DeviceBuffer(ctx, n_images * max_pts * 8)
    try:
        ctx.memset(d_q.ptr, SENTINEL, d_q.nbytes)
        ctx.memset(d_s.ptr, SENTINEL, d_s.nbytes)
        ctx.quantize_descriptors(d_pts.ptr, max_pts, d_q.ptr, d_s.ptr, n_images, None if d_cnt is None else d_cnt.ptr)
        ctx.synchronize()
        back = d_pts.to_numpy(SIFT_POINT_DTYPE, pts.shape)
        assert back.view(np.uint8).tobytes() == np.ascontiguousarray(pts).view(np.uint8).tobytes()  # records: read only
        return d_q.to_numpy(np.uint8, (n_images, max_pts, 128)), d_s.to_numpy(np.int32, (n_images, max_pts, 2))
    finally:
        for b in (d_pts, d_cnt, d_q, d_s):
            if b is not None:
                b.free()


def crafted_values():
    f = np.float32
    k = np.arange(0, 257, dtype=np.float32)
    centres = np.concatenate([k / f(512), (k + f(0.5)) / f(512)]).astype(np.float32)  # k/512 and the rounding points
    around = np.concatenate([centres, np.nextafter(centres, f(np.inf)), np.nextafter(centres, f(-np.inf))])
    special = np.array([0.0, -0.0, -1.0, -1e-30, 1e-45, -1e-45, np.nan, -np.nan, np.inf, -np.inf, 1.0, 3e38, -3e38,
                        255 / 512, np.nextafter(f(255 / 512), f(1)), np.nextafter(f(255 / 512), f(0))], np.float32)
    v = np.concatenate([special, around]).astype(np.float32)
    return np.concatenate([v, np.zeros(-len(v) % 128, np.float32)]).reshape(-1, 128)


@pytest.mark.gpu
def test_quantiser_on_extracted_descriptors(ctx, oracle, gray1):
    pts = oracle.extract(gray1, num_octaves=4, peak_thresh=1.0, max_pts=4096).view(SIFT_POINT_DTYPE).copy()
    assert len(pts) > 500
    q, s = quantize_on_gpu(ctx, pts, 1, len(pts), None)
    want = quantize_model(pts["data"])
    assert 0 < want.max() <= 255 and (want > 0).mean() > 0.3
    assert q[0].tobytes() == want.tobytes()
    assert s[0].tobytes() == sums_model(want).tobytes()


@pytest.mark.gpu
def test_quantiser_on_crafted_values(ctx):
    data = crafted_values()
    pts = records(len(data))
    pts["data"] = data
    q, s = quantize_on_gpu(ctx, pts, 1, len(pts), None)
    want = quantize_model(data)
    assert set(np.unique(want)) == set(range(256))  # the crafted set reaches every byte
    assert q[0].tobytes() == want.tobytes()
    assert s[0].tobytes() == sums_model(want).tobytes()


@pytest.mark.gpu
def test_quantiser_batch_counts_and_untouched_rows(ctx):
    max_pts = 37
    counters = [0, 1, max_pts - 1, max_pts, 4000]  # the last is clamped to max_pts on the device
    rng = np.random.default_rng(5)
    pts = records(len(counters) * max_pts).reshape(len(counters), max_pts)
    pts["data"] = (rng.random((len(counters), max_pts, 128)) * 0.6 - 0.05).astype(np.float32)
    q, s = quantize_on_gpu(ctx, pts, len(counters), max_pts, counters)
    want_q, want_s = quantize_model(pts["data"]), None
    want_s = sums_model(want_q)
    for i, c in enumerate(counters):
        n = min(c, max_pts)
        assert q[i, :n].tobytes() == want_q[i, :n].tobytes(), i
        assert s[i, :n].tobytes() == want_s[i, :n].tobytes(), i
        assert (q[i, n:] == SENTINEL).all() and (s[i, n:].view(np.uint8) == SENTINEL).all(), i
    # no counters: every frame is full
    q, s = quantize_on_gpu(ctx, pts, len(counters), max_pts, None)
    assert q.tobytes() == want_q.tobytes() and s.tobytes() == want_s.tobytes()


@pytest.mark.gpu
def test_desc8_sums_on_random_bytes(ctx):
    from cusift_amd.capi import DeviceBuffer

    rng = np.random.default_rng(6)
    for n in (1, 31, 32, 33, 1000):
        q = rng.integers(0, 256, (n, 128), dtype=np.uint8)
        d_q, d_s = DeviceBuffer.from_numpy(ctx, q), DeviceBuffer(ctx, (n + 1) * 8)
        try:
            ctx.memset(d_s.ptr, SENTINEL, d_s.nbytes)
            ctx.desc8_sums(d_q.ptr, n, d_s.ptr)
            ctx.synchronize()
            s = d_s.to_numpy(np.int32, (n + 1, 2))
            assert s[:n].tobytes() == sums_model(q).tobytes(), n
            assert (s[n:].view(np.uint8) == SENTINEL).all()
        finally:
            d_q.free()
            d_s.free()


# ----------------------------------------------------------------------------------------------------------------------
# the matcher on the GPU
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_tables(ctx):
    rng = np.random.default_rng(11)
    t = Tables(ctx, rng.integers(0, 256, (max(N1_SIZES), 128), dtype=np.uint8),
               rng.integers(0, 256, (max(N2_SIZES), 128), dtype=np.uint8))
    yield t
    t.free()


@pytest.mark.gpu
@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("distance", (1, 0))
def test_every_size_every_field(random_tables, distance, splits):
    """Random bytes over the full range, every n1 x n2 of the sweep as a prefix of one pair of tables."""
    for n1 in N1_SIZES:
        for n2 in N2_SIZES:
            random_tables.check(distance, splits, n1, n2, "random")


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
def test_five_thousand_square(ctx, distance):
    """Every loop turns many times: 20 row blocks, 79 tiles; automatic splits and three forced settings."""
    rng = np.random.default_rng(12)
    # SIFT-like bytes: mostly small, some large, so that D and S spread
    q1 = np.minimum(rng.gamma(0.6, 40.0, (5003, 128)), 255).astype(np.uint8)
    q2 = np.minimum(rng.gamma(0.6, 40.0, (4999, 128)), 255).astype(np.uint8)
    t = Tables(ctx, q1, q2)
    try:
        first = t.check(distance, 0, what="5k")
        for k in (1, 2, 7):
            got = t.match(distance, k)
            assert got.tobytes() == first.tobytes(), k
    finally:
        t.free()


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
def test_constant_tables(ctx, distance):
    """All-0 and all-255 in every combination: 128 * 255^2 = 8,323,200 is the largest key there is; every column ties."""
    for a, b in ((0, 0), (255, 255), (0, 255), (255, 0)):
        t = Tables(ctx, np.full((70, 128), a, np.uint8), np.full((130, 128), b, np.uint8))
        try:
            for k in (0, 1, 2):
                got = t.check(distance, k, what="constant %d / %d" % (a, b))
                assert (got["match"] == 0).all()  # the lowest of 130 equal columns
            S = a * b * 128
            want = (a * a * 128 + b * b * 128 - 2 * S) if distance == 1 else S
            assert (got["score"] == np.float32(want) * SCALE).all()
        finally:
            t.free()


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
def test_asymmetric_tables(ctx, distance):
    """Data for which swapping rows and columns changes the answer: a C/D map with rows and columns exchanged, or an A
    fragment read as B, cannot pass both directions."""
    i, j, k = np.arange(83)[:, None], np.arange(149)[:, None], np.arange(128)[None, :]
    q1 = ((i * 7 + k * 3 + (i * k) % 5) % 256).astype(np.uint8)
    q2 = ((j * j + 5 * k + (j * k) % 11) % 251).astype(np.uint8)
    fwd = match8_model(q1, q2[:83], distance, np.zeros((83, 2), np.float32))["match"]
    bwd = match8_model(q2[:83], q1, distance, np.zeros((83, 2), np.float32))["match"]
    assert (fwd != bwd).mean() > 0.5  # the square part is far from symmetric
    for a, b in ((q1, q2), (q2, q1)):
        t = Tables(ctx, a, b)
        try:
            for ks in (0, 1, 3):
                t.check(distance, ks, what="asymmetric")
        finally:
            t.free()


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
def test_ties_lowest_column_wins_under_every_split(ctx, distance):
    """700 columns drawn from 40 distinct descriptors, 300 rows from the same 40 plus 20 others: equal bests in the same
    tile, in different tiles and -- under 2, 3, 7 and 11 splits -- in different splits.  The lowest column wins, second
    equals best, and the bytes are the same under every split count."""
    rng = np.random.default_rng(13)
    base = rng.integers(0, 256, (60, 128), dtype=np.uint8)
    pick2 = rng.integers(0, 40, 700)
    pick2[[0, 1, 64, 350, 699]] = 7  # one descriptor in a tile twice, in the next tile, in another split, in the last column
    q2 = base[pick2]
    q1 = base[rng.integers(0, 60, 300)]
    t = Tables(ctx, q1, q2)
    try:
        first = t.check(distance, 1, what="ties")
        K = keys_model(q1, q2, distance)
        tied = (K == K.min(1)[:, None]).sum(1) > 1
        assert tied.mean() > 0.6
        best = first["score"][tied].astype(np.float64)
        amb = best / (best + 1e-6) if distance == 1 else (1 - best) / (1 - best + 1e-6)
        assert first["ambiguity"][tied].tobytes() == amb.astype(np.float32).tobytes()  # second == best
        assert (first["match"] == np.array([np.flatnonzero(r == r.min())[0] for r in K])).all()
        for k in (0, 2, 3, 7, 11):
            assert t.check(distance, k, what="ties").tobytes() == first.tobytes(), k
    finally:
        t.free()


@pytest.mark.gpu
def test_refusals_and_empty_sets(ctx, random_tables):
    from cusift_amd import capi

    t = random_tables
    dq1, ds1, dq2, ds2, d2 = (b.ptr for b in t.bufs)
    ctx.h2d(t.d1.ptr, t.s1)
    for n1, n2 in ((0, 5), (5, 0), (-1, 5), (5, -3), (0, 0)):  # nothing enqueued, even with nothing to read
        ctx.match8(t.d1.ptr, n1, dq1, ds1, d2, n2, dq2, ds2, 1)
        ctx.match8(None, n1, None, None, None, n2, None, None, 7)
    ctx.desc8_sums(None, 0, None)
    ctx.quantize_descriptors(None, 0, None, None, 3, None)
    ctx.synchronize()
    assert t.d1.to_numpy(SIFT_POINT_DTYPE, (len(t.s1),)).tobytes() == t.s1.tobytes()
    bad = [
        lambda: ctx.match8(t.d1.ptr, 5, dq1 + 1, ds1, d2, 5, dq2, ds2, 1),  # misaligned tables
        lambda: ctx.match8(t.d1.ptr, 5, dq1, ds1, d2, 5, dq2 + 8, ds2, 1),
        lambda: ctx.match8(None, 5, dq1, ds1, d2, 5, dq2, ds2, 1),  # NULL, one pointer at a time
        lambda: ctx.match8(t.d1.ptr, 5, None, ds1, d2, 5, dq2, ds2, 1),
        lambda: ctx.match8(t.d1.ptr, 5, dq1, None, d2, 5, dq2, ds2, 1),
        lambda: ctx.match8(t.d1.ptr, 5, dq1, ds1, None, 5, dq2, ds2, 1),
        lambda: ctx.match8(t.d1.ptr, 5, dq1, ds1, d2, 5, None, ds2, 1),
        lambda: ctx.match8(t.d1.ptr, 5, dq1, ds1, d2, 5, dq2, None, 1),
        lambda: ctx.match8(t.d1.ptr, 5, dq1, ds1, d2, 5, dq2, ds2, 2),  # a bad distance
        lambda: ctx.match8(t.d1.ptr, 5, dq1, ds1, d2, 5, dq2, ds2, -1),
        lambda: ctx.desc8_sums(dq1 + 4, 5, ds1),
        lambda: ctx.desc8_sums(None, 5, ds1),
        lambda: ctx.desc8_sums(dq1, 5, None),
        lambda: ctx.quantize_descriptors(d2, 5, dq1 + 2, ds1),
        lambda: ctx.quantize_descriptors(None, 5, dq1, ds1),
        lambda: ctx.quantize_descriptors(d2, 5, None, ds1),
        lambda: ctx.quantize_descriptors(d2, 5, dq1, None),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(capi.CusiftError):
            call()
            pytest.fail("refusal %d did not raise" % i)
    ctx.synchronize()
    assert t.d1.to_numpy(SIFT_POINT_DTYPE, (len(t.s1),)).tobytes() == t.s1.tobytes()  # a refusal writes nothing
    assert INIT[1] == 999.0
