"""cusift_match8_mutual and cusift_match8_batch_mutual (cusift_amd/csrc/sift_match8.hip): both directions of the 8-bit
matcher from one pass over the integer scores.  Every pin is bit equality against tests/match8_model.py -- set 1 is
match8_model(q1, q2), set 2 is match8_model(q2, q1) with set 1's coordinates, because the keys are symmetric integers --
or against cusift_match8 / cusift_match8_batch called in both directions.  No tolerance appears in this file.

The workgroup is 256 rows (4 waves of 64, a wave's rows 16 i + 4 g + j in lane group g) and the LDS tile 64 columns:
n1 = 257 and 513 engage the column partials [row block][column] and their merge kernel.
"""
import numpy as np
import pytest

from match8_model import FIELDS, assert_fields_equal, keys_model, match8_model, sums_model
from oracle_binding import SIFT_POINT_DTYPE
from test_match8 import records

N1_SIZES = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513)
N2_SIZES = (1, 63, 64, 65, 129, 1000)
SPLITS = (0, 1, 2, 3, 7)
SENTINEL = 0xAB
ROW = np.dtype([("score", "<f4"), ("ambiguity", "<f4"), ("match", "<i4"), ("reserved", "<i4")])
OTHER = ("coords2D", "scale", "orientation")


class Tables:
    """Two byte tables, their sums (from the numpy model) and two record sets with sentinel match fields on the device."""

    def __init__(self, ctx, q1, q2):
        from cusift_amd.capi import DeviceBuffer

        self.ctx, self.q1, self.q2 = ctx, np.ascontiguousarray(q1, np.uint8), np.ascontiguousarray(q2, np.uint8)
        self.s1, self.s2 = records(len(q1), 1), records(len(q2), 2)
        self.tables = [DeviceBuffer.from_numpy(ctx, a) for a in (self.q1, sums_model(self.q1), self.q2, sums_model(self.q2))]
        self.d1, self.d2 = DeviceBuffer(ctx, self.s1.nbytes), DeviceBuffer(ctx, self.s2.nbytes)
        self.models = {}

    def run(self, call, distance, splits, n1, n2):
        from cusift_amd import capi

        dq1, ds1, dq2, ds2 = (b.ptr for b in self.tables)
        self.ctx.h2d(self.d1.ptr, self.s1)
        self.ctx.h2d(self.d2.ptr, self.s2)
        try:
            self.ctx.set_policy(capi.POLICY_MATCH_SPLITS, splits)
            call(self.d1.ptr, n1, dq1, ds1, self.d2.ptr, n2, dq2, ds2, distance)
            self.ctx.synchronize()
        finally:
            self.ctx.set_policy(capi.POLICY_MATCH_SPLITS, 0)
        return (self.d1.to_numpy(SIFT_POINT_DTYPE, (len(self.s1),)), self.d2.to_numpy(SIFT_POINT_DTYPE, (len(self.s2),)))

    def mutual(self, distance, splits=0, n1=None, n2=None):
        n1 = len(self.q1) if n1 is None else n1
        n2 = len(self.q2) if n2 is None else n2
        return self.run(self.ctx.match8_mutual, distance, splits, n1, n2)

    def model(self, distance, n1, n2):
        key = (distance, n1, n2)
        if key not in self.models:
            self.models[key] = (match8_model(self.q1[:n1], self.q2[:n2], distance, self.s2["coords2D"][:n2]),
                                match8_model(self.q2[:n2], self.q1[:n1], distance, self.s1["coords2D"][:n1]))
        return self.models[key]

    def check(self, distance, splits=0, n1=None, n2=None, what=""):
        n1 = len(self.q1) if n1 is None else n1
        n2 = len(self.q2) if n2 is None else n2
        got1, got2 = self.mutual(distance, splits, n1, n2)
        want1, want2 = self.model(distance, n1, n2)
        what = "%s %d x %d, distance %d, %d splits asked" % (what, n1, n2, distance, splits)
        assert_fields_equal({f: got1[f][:n1] for f in FIELDS}, want1, what + ", set 1")
        assert_fields_equal({f: got2[f][:n2] for f in FIELDS}, want2, what + ", set 2")
        for got, held, n in ((got1, self.s1, n1), (got2, self.s2, n2)):
            assert got[n:].tobytes() == held[n:].tobytes(), what  # records past the count: untouched
            for f in OTHER:
                assert got[f].tobytes() == held[f].tobytes(), (what, f)
            assert got["data"].view(np.uint32).tobytes() == held["data"].view(np.uint32).tobytes(), what
        return got1, got2

    def free(self):
        for b in self.tables + [self.d1, self.d2]:
            b.free()


def tie_tables():
    """Rows and columns from 40 distinct descriptors, one of them planted at rows 0, 1, 4, 16, 64, 256 and the last: copies
    in the same lane, another 16-lane group, another A fragment, another wave and another row block."""
    rng = np.random.default_rng(31)
    base = rng.integers(0, 256, (40, 128), dtype=np.uint8)
    pick1 = rng.integers(0, 40, 300)
    pick1[pick1 == 7] = 8
    pick1[[0, 1, 4, 16, 64, 256, 299]] = 7
    pick2 = rng.integers(0, 40, 200)
    pick2[[0, 3, 70, 199]] = 7
    return base[pick1], base[pick2], pick1, pick2


# ----------------------------------------------------------------------------------------------------------------------
# without a GPU
# ----------------------------------------------------------------------------------------------------------------------
def test_model_column_side_of_the_tie_tables():
    """From the model alone: more than half the columns have a tied best, the planted descriptor's columns name row 0 with
    second == best, and a single row gives the initial second."""
    q1, q2, pick1, pick2 = tie_tables()
    for distance in (1, 0):
        K = keys_model(q2, q1, distance)  # [column, row]
        tied = (K == K.min(1)[:, None]).sum(1) > 1
        assert tied.mean() > 0.5
        m = match8_model(q2, q1, distance, np.zeros((len(q1), 2), np.float32))
        assert (m["match"] == np.array([np.flatnonzero(r == r.min())[0] for r in K])).all()
    m = match8_model(q2, q1, 1, np.zeros((len(q1), 2), np.float32))  # L2: an identical descriptor is the best there is
    planted = np.flatnonzero(pick2 == 7)
    assert len(planted) >= 4 and (m["match"][planted] == 0).all() and (m["score"][planted] == 0).all()
    assert (m["ambiguity"][planted] == 0).all()  # 0 / (0 + 1e-6): second == best
    one = match8_model(q2, q1[:1], 1, np.zeros((1, 2), np.float32))
    best = one["score"].astype(np.float64)
    assert one["ambiguity"].tobytes() == (best / (999.0 + 1e-6)).astype(np.float32).tobytes()
    assert sorted(set(pick1[[0, 1, 4, 16, 64, 256, 299]])) == [7]


# ----------------------------------------------------------------------------------------------------------------------
# the pair call
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_tables(ctx):
    rng = np.random.default_rng(32)
    t = Tables(ctx, rng.integers(0, 256, (max(N1_SIZES), 128), dtype=np.uint8),
               rng.integers(0, 256, (max(N2_SIZES), 128), dtype=np.uint8))
    yield t
    t.free()


@pytest.mark.gpu
@pytest.mark.parametrize("splits", SPLITS)
@pytest.mark.parametrize("distance", (1, 0))
def test_every_size_both_sides(random_tables, distance, splits):
    for n1 in N1_SIZES:
        for n2 in N2_SIZES:
            random_tables.check(distance, splits, n1, n2, "random")


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
def test_symmetry_on_asymmetric_tables(ctx, distance):
    """Set 2 after match8_mutual(A, B) is set 1 after match8(B, A); set 1 is match8(A, B)'s.  Both orders."""
    i, j, k = np.arange(83)[:, None], np.arange(149)[:, None], np.arange(128)[None, :]
    q1 = ((i * 7 + k * 3 + (i * k) % 5) % 256).astype(np.uint8)
    q2 = ((j * j + 5 * k + (j * k) % 11) % 251).astype(np.uint8)
    for a, b in ((q1, q2), (q2, q1)):
        t = Tables(ctx, a, b)
        try:
            for ks in (0, 1, 3):
                got1, got2 = t.check(distance, ks, what="asymmetric")
                fwd, untouched = t.run(ctx.match8, distance, ks, len(a), len(b))
                assert untouched.tobytes() == t.s2.tobytes()
                assert got1.tobytes() == fwd.tobytes(), ks
                # the swapped call: B's records are set 1 (they live in d2), A's are set 2
                dq1, ds1, dq2, ds2 = (x.ptr for x in t.tables)
                ctx.h2d(t.d1.ptr, t.s1)
                ctx.h2d(t.d2.ptr, t.s2)
                ctx.match8(t.d2.ptr, len(b), dq2, ds2, t.d1.ptr, len(a), dq1, ds1, distance)
                ctx.synchronize()
                assert got2.tobytes() == t.d2.to_numpy(SIFT_POINT_DTYPE, (len(b),)).tobytes(), ks
        finally:
            t.free()


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
def test_ties_lowest_row_wins_under_every_split(ctx, distance):
    q1, q2, _, _ = tie_tables()
    t = Tables(ctx, q1, q2)
    try:
        first1, first2 = t.check(distance, 1, what="ties")
        K = keys_model(q2, q1, distance)
        assert (first2["match"] == np.array([np.flatnonzero(r == r.min())[0] for r in K])).all()  # the lowest row
        tied = (K == K.min(1)[:, None]).sum(1) > 1
        best = first2["score"][tied].astype(np.float64)
        amb = best / (best + 1e-6) if distance == 1 else (1 - best) / (1 - best + 1e-6)
        assert first2["ambiguity"][tied].tobytes() == amb.astype(np.float32).tobytes()  # second == best
        for k in (0, 2, 3, 7, 11):
            got1, got2 = t.check(distance, k, what="ties")
            assert got1.tobytes() == first1.tobytes() and got2.tobytes() == first2.tobytes(), k
    finally:
        t.free()


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
def test_constant_tables(ctx, distance):
    for a, b in ((0, 0), (255, 255), (0, 255), (255, 0)):
        t = Tables(ctx, np.full((70, 128), a, np.uint8), np.full((130, 128), b, np.uint8))
        try:
            for k in (0, 1, 2):
                got1, got2 = t.check(distance, k, what="constant %d / %d" % (a, b))
                assert (got1["match"] == 0).all() and (got2["match"] == 0).all()  # every row ties, every column ties
        finally:
            t.free()


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
def test_five_thousand_square(ctx, distance):
    rng = np.random.default_rng(12)
    q1 = np.minimum(rng.gamma(0.6, 40.0, (5003, 128)), 255).astype(np.uint8)
    q2 = np.minimum(rng.gamma(0.6, 40.0, (4999, 128)), 255).astype(np.uint8)
    t = Tables(ctx, q1, q2)
    try:
        first1, first2 = t.check(distance, 0, what="5k")
        for k in (1, 2, 7):
            got1, got2 = t.mutual(distance, k)
            assert got1.tobytes() == first1.tobytes() and got2.tobytes() == first2.tobytes(), k
    finally:
        t.free()


@pytest.mark.gpu
def test_refusals_and_empty_sets(ctx, random_tables):
    from cusift_amd import capi

    t = random_tables
    dq1, ds1, dq2, ds2 = (b.ptr for b in t.tables)
    d1, d2 = t.d1.ptr, t.d2.ptr
    ctx.h2d(d1, t.s1)
    ctx.h2d(d2, t.s2)

    def untouched():
        ctx.synchronize()
        assert t.d1.to_numpy(SIFT_POINT_DTYPE, (len(t.s1),)).tobytes() == t.s1.tobytes()
        assert t.d2.to_numpy(SIFT_POINT_DTYPE, (len(t.s2),)).tobytes() == t.s2.tobytes()

    for n1, n2 in ((0, 5), (5, 0), (-1, 5), (5, -3), (0, 0)):  # nothing enqueued, even with nothing to read
        ctx.match8_mutual(d1, n1, dq1, ds1, d2, n2, dq2, ds2, 1)
        ctx.match8_mutual(None, n1, None, None, None, n2, None, None, 7)
    untouched()
    rec = SIFT_POINT_DTYPE.itemsize
    bad = [
        lambda: ctx.match8_mutual(d1, 5, dq1 + 1, ds1, d2, 5, dq2, ds2, 1),  # misaligned tables
        lambda: ctx.match8_mutual(d1, 5, dq1, ds1, d2, 5, dq2 + 8, ds2, 1),
        lambda: ctx.match8_mutual(d1, 5, dq1, ds1 + 4, d2, 5, dq2, ds2, 1),
        lambda: ctx.match8_mutual(d1, 5, dq1, ds1, d2, 5, dq2, ds2 + 4, 1),
        lambda: ctx.match8_mutual(None, 5, dq1, ds1, d2, 5, dq2, ds2, 1),  # NULL, one pointer at a time
        lambda: ctx.match8_mutual(d1, 5, None, ds1, d2, 5, dq2, ds2, 1),
        lambda: ctx.match8_mutual(d1, 5, dq1, None, d2, 5, dq2, ds2, 1),
        lambda: ctx.match8_mutual(d1, 5, dq1, ds1, None, 5, dq2, ds2, 1),
        lambda: ctx.match8_mutual(d1, 5, dq1, ds1, d2, 5, None, ds2, 1),
        lambda: ctx.match8_mutual(d1, 5, dq1, ds1, d2, 5, dq2, None, 1),
        lambda: ctx.match8_mutual(d1, 5, dq1, ds1, d2, 5, dq2, ds2, 2),  # a bad distance
        lambda: ctx.match8_mutual(d1, 5, dq1, ds1, d2, 5, dq2, ds2, -1),
        lambda: ctx.match8_mutual(d1, 5, dq1, ds1, d1, 5, dq1, ds1, 1),  # overlapping record ranges
        lambda: ctx.match8_mutual(d1, 5, dq1, ds1, d1 + 4 * rec, 5, dq2, ds2, 1),
        lambda: ctx.match8_mutual(d1 + 4 * rec, 5, dq1, ds1, d1, 5, dq2, ds2, 1),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(capi.CusiftError):
            call()
            pytest.fail("refusal %d did not raise" % i)
    untouched()
    ctx.match8_mutual(d1, 5, dq1, ds1, d1 + 5 * rec, 5, dq2, ds2, 1)  # adjacent ranges are disjoint
    ctx.synchronize()


# ----------------------------------------------------------------------------------------------------------------------
# the pair list
# ----------------------------------------------------------------------------------------------------------------------
BATCH_PAIRS = ((0, 1), (1, 0), (2, 2), (3, 4), (4, 3), (0, 4))


@pytest.mark.gpu
@pytest.mark.parametrize("max_pts", (300, 37))
@pytest.mark.parametrize("distance", (1, 0))
def test_batch_rows_and_back_rows(ctx, distance, max_pts):
    from cusift_amd import capi
    from cusift_amd.capi import DeviceBuffer

    counters = (0, 1, max_pts - 1, max_pts, 4000)  # the last is clamped to max_pts on the device
    counts = [min(c, max_pts) for c in counters]
    rng = np.random.default_rng(33)
    q = rng.integers(0, 256, (len(counters), max_pts, 128), dtype=np.uint8)
    q[4, max_pts // 2:max_pts // 2 + 10] = q[4, 0:10]  # tied rows / columns wherever frame 4 takes part
    P = len(BATCH_PAIRS)
    bufs = [DeviceBuffer.from_numpy(ctx, q), DeviceBuffer.from_numpy(ctx, sums_model(q)),
            DeviceBuffer.from_numpy(ctx, np.asarray(counters, np.uint32))] + \
           [DeviceBuffer(ctx, P * max_pts * ROW.itemsize) for _ in range(3)]
    d_q, d_s, d_cnt, d_rows, d_back, d_plain = bufs
    zeros = np.zeros((max_pts, 2), np.float32)
    want = {}
    try:
        for splits in (0, 1, 2, 3):
            for b in (d_rows, d_back, d_plain):
                ctx.memset(b.ptr, SENTINEL, b.nbytes)
            ctx.set_policy(capi.POLICY_MATCH_SPLITS, splits)
            ctx.match8_batch_mutual(d_q.ptr, d_s.ptr, d_cnt.ptr, len(counters), max_pts, BATCH_PAIRS, d_rows.ptr,
                                    d_back.ptr, distance)
            ctx.match8_batch(d_q.ptr, d_s.ptr, d_cnt.ptr, len(counters), max_pts, BATCH_PAIRS, d_plain.ptr, distance)
            ctx.synchronize()
            assert d_rows.to_numpy(np.uint8, (d_rows.nbytes,)).tobytes() == \
                d_plain.to_numpy(np.uint8, (d_plain.nbytes,)).tobytes(), splits
            rows, back = d_rows.to_numpy(ROW, (P, max_pts)), d_back.to_numpy(ROW, (P, max_pts))
            for p, (a, b) in enumerate(BATCH_PAIRS):
                n1, n2 = counts[a], counts[b]
                what = "pair %d = (%d, %d), %d splits asked, max_pts %d" % (p, a, b, splits, max_pts)
                if n1 == 0 or n2 == 0:
                    assert (rows[p].view(np.uint8) == SENTINEL).all() and (back[p].view(np.uint8) == SENTINEL).all(), what
                    continue
                if p not in want:
                    want[p] = (match8_model(q[a, :n1], q[b, :n2], distance, zeros[:n2]),
                               match8_model(q[b, :n2], q[a, :n1], distance, zeros[:n1]))
                for got, w, n in ((rows[p], want[p][0], n1), (back[p], want[p][1], n2)):
                    assert (got[n:].view(np.uint8) == SENTINEL).all(), what  # rows past the count: untouched
                    for f in ("score", "ambiguity", "match"):
                        assert got[:n][f].tobytes() == w[f].tobytes(), (what, f)
                    assert (got[:n]["reserved"] == 0).all(), what
    finally:
        ctx.set_policy(capi.POLICY_MATCH_SPLITS, 0)
        for b in bufs:
            b.free()


@pytest.mark.gpu
def test_batch_refusals(ctx):
    from cusift_amd import capi
    from cusift_amd.capi import DeviceBuffer

    rows_b = 2 * 64 * 16
    d = DeviceBuffer(ctx, 4 * 64 * 128 + 4 * 64 * 8 + 2 * rows_b)
    d_q, d_s = d.ptr, d.ptr + 4 * 64 * 128
    d_rows, d_back = d_s + 4 * 64 * 8, d_s + 4 * 64 * 8 + rows_b
    try:
        ctx.memset(d.ptr, SENTINEL, d.nbytes)
        ctx.match8_batch_mutual(d_q, d_s, None, 4, 64, np.zeros((0, 2), np.int32), d_rows, d_back)  # nothing enqueued
        ctx.match8_batch_mutual(d_q, d_s, None, 4, 0, [(0, 1)], d_rows, d_back)
        for call in (lambda: ctx.match8_batch_mutual(d_q, d_s, None, 4, 64, [(0, 4)], d_rows, d_back),
                     lambda: ctx.match8_batch_mutual(d_q, d_s, None, 4, 64, [(-1, 0)], d_rows, d_back),
                     lambda: ctx.match8_batch_mutual(d_q, d_s, None, 4, 64, [(0, 1)], d_rows, d_back, distance=2),
                     lambda: ctx.match8_batch_mutual(None, d_s, None, 4, 64, [(0, 1)], d_rows, d_back),
                     lambda: ctx.match8_batch_mutual(d_q, None, None, 4, 64, [(0, 1)], d_rows, d_back),
                     lambda: ctx.match8_batch_mutual(d_q, d_s, None, 4, 64, [(0, 1)], None, d_back),
                     lambda: ctx.match8_batch_mutual(d_q, d_s, None, 4, 64, [(0, 1)], d_rows, None),
                     lambda: ctx.match8_batch_mutual(d_q, d_s, None, 4, 64, [(0, 1)], d_rows, d_rows),
                     lambda: ctx.match8_batch_mutual(d_q + 4, d_s, None, 4, 64, [(0, 1)], d_rows, d_back),
                     lambda: ctx.match8_batch_mutual(d_q, d_s + 4, None, 4, 64, [(0, 1)], d_rows, d_back)):
            with pytest.raises(capi.CusiftError):
                call()
        ctx.synchronize()
        assert (d.to_numpy(np.uint8, (d.nbytes,)) == SENTINEL).all()  # a refusal writes nothing
    finally:
        d.free()


@pytest.mark.gpu
def test_batch_extractor_match8_mutual(gray1):
    """BatchExtractor.match8_mutual(i, j) on the tensors of quantize(): frame j's fields are what match8(j, i) writes."""
    import torch

    from cusift_amd import capi
    from cusift_amd.batch import BatchExtractor

    h, w = gray1.shape
    ex = BatchExtractor(2, w, h, num_octaves=4, peak_thresh=2.0, max_pts=4096)
    try:
        with pytest.raises(capi.CusiftError):
            ex.match8_mutual(0, 1)  # nothing quantised yet
        ex.extract(ex.images_from_numpy(np.stack([gray1, np.ascontiguousarray(gray1[::-1, ::-1])])))
        ex.quantize()
        ex.match8_mutual(0, 1)
        torch.cuda.synchronize()
        both = ex.to_host()
        ex.match8(1, 0)
        ex.match8(0, 1)
        torch.cuda.synchronize()
        staged = ex.to_host()
        assert len(both[0]) > 100 and len(both[1]) > 100
        for i in range(2):
            assert both[i].tobytes() == staged[i].tobytes(), i
    finally:
        ex.close()
