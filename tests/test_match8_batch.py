"""cusift_match8_batch (cusift_amd/csrc/sift_match8.hip): the pair-list form of the 8-bit matcher, byte for byte against
the pair call cusift_match8 on the same tables and against the numpy model of tests/match8_model.py.  No tolerance."""
import numpy as np
import pytest

from match8_model import match8_model, sums_model
from oracle_binding import SIFT_POINT_DTYPE

MAX_PTS = 256
COUNTS = (0, 6, 64, 200)
# a frame on both sides and more than once, the empty frame on either side, and (i, i)
PAIRS = ((1, 2), (2, 1), (2, 3), (3, 2), (3, 1), (0, 1), (1, 0), (0, 0), (2, 2), (3, 3), (1, 2))
SENTINEL = 0xAB
ROW = np.dtype([("score", "<f4"), ("ambiguity", "<f4"), ("match", "<i4"), ("reserved", "<i4")])


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
def test_rows_equal_the_pair_call(ctx, distance):
    from cusift_amd import capi
    from cusift_amd.capi import DeviceBuffer

    rng = np.random.default_rng(21)
    q = rng.integers(0, 256, (len(COUNTS), MAX_PTS, 128), dtype=np.uint8)
    q[3, 100:150] = q[3, 0:50]  # tied columns for every row that meets frame 3
    sums = sums_model(q)
    recs = np.zeros(MAX_PTS, SIFT_POINT_DTYPE)
    d_q, d_s = DeviceBuffer.from_numpy(ctx, q), DeviceBuffer.from_numpy(ctx, sums)
    d_cnt = DeviceBuffer.from_numpy(ctx, np.asarray(COUNTS, np.uint32))
    d_rows = DeviceBuffer(ctx, len(PAIRS) * MAX_PTS * ROW.itemsize)
    d_r1, d_r2 = DeviceBuffer.from_numpy(ctx, recs), DeviceBuffer.from_numpy(ctx, recs)
    try:
        for splits in (0, 1, 2, 3):
            ctx.memset(d_rows.ptr, SENTINEL, d_rows.nbytes)
            ctx.set_policy(capi.POLICY_MATCH_SPLITS, splits)
            ctx.match8_batch(d_q.ptr, d_s.ptr, d_cnt.ptr, len(COUNTS), MAX_PTS, PAIRS, d_rows.ptr, distance)
            ctx.synchronize()
            rows = d_rows.to_numpy(ROW, (len(PAIRS), MAX_PTS))
            for p, (a, b) in enumerate(PAIRS):
                n1, n2 = COUNTS[a], COUNTS[b]
                what = "pair %d = (%d, %d), %d splits asked" % (p, a, b, splits)
                if n1 == 0 or n2 == 0:
                    assert (rows[p].view(np.uint8) == SENTINEL).all(), what  # no row at all
                    continue
                assert (rows[p, n1:].view(np.uint8) == SENTINEL).all(), what  # rows past the count: untouched
                ctx.match8(d_r1.ptr, n1, d_q.ptr + a * MAX_PTS * 128, d_s.ptr + a * MAX_PTS * 8, d_r2.ptr, n2,
                           d_q.ptr + b * MAX_PTS * 128, d_s.ptr + b * MAX_PTS * 8, distance)
                ctx.synchronize()
                pair = d_r1.to_numpy(SIFT_POINT_DTYPE, (MAX_PTS,))[:n1]
                want = match8_model(q[a, :n1], q[b, :n2], distance, np.zeros((n2, 2), np.float32))
                for f in ("score", "ambiguity", "match"):
                    assert rows[p, :n1][f].tobytes() == np.ascontiguousarray(pair[f]).tobytes(), (what, f, "pair call")
                    assert rows[p, :n1][f].tobytes() == want[f].tobytes(), (what, f, "model")
                assert (rows[p, :n1]["reserved"] == 0).all(), what
        # no counters: every frame is full
        ctx.set_policy(capi.POLICY_MATCH_SPLITS, 0)
        ctx.match8_batch(d_q.ptr, d_s.ptr, None, len(COUNTS), MAX_PTS, [(0, 3), (3, 3)], d_rows.ptr, distance)
        ctx.synchronize()
        rows = d_rows.to_numpy(ROW, (len(PAIRS), MAX_PTS))
        for p, (a, b) in enumerate(((0, 3), (3, 3))):
            want = match8_model(q[a], q[b], distance, np.zeros((MAX_PTS, 2), np.float32))
            for f in ("score", "ambiguity", "match"):
                assert rows[p][f].tobytes() == want[f].tobytes(), (p, f)
    finally:
        ctx.set_policy(capi.POLICY_MATCH_SPLITS, 0)
        for b in (d_q, d_s, d_cnt, d_rows, d_r1, d_r2):
            b.free()


@pytest.mark.gpu
def test_refusals(ctx):
    from cusift_amd import capi
    from cusift_amd.capi import DeviceBuffer

    d = DeviceBuffer(ctx, 4 * 64 * 128 + 4 * 64 * 8 + 64 * 16 + 64)
    d_q, d_s, d_rows = d.ptr, d.ptr + 4 * 64 * 128, d.ptr + 4 * 64 * 128 + 4 * 64 * 8
    try:
        ctx.match8_batch(d_q, d_s, None, 4, 64, np.zeros((0, 2), np.int32), d_rows)  # no pairs: nothing enqueued
        ctx.match8_batch(d_q, d_s, None, 4, 0, [(0, 1)], d_rows)  # no records
        for call in (lambda: ctx.match8_batch(d_q, d_s, None, 4, 64, [(0, 4)], d_rows),
                     lambda: ctx.match8_batch(d_q, d_s, None, 4, 64, [(-1, 0)], d_rows),
                     lambda: ctx.match8_batch(d_q, d_s, None, 4, 64, [(0, 1)], d_rows, distance=2),
                     lambda: ctx.match8_batch(None, d_s, None, 4, 64, [(0, 1)], d_rows),
                     lambda: ctx.match8_batch(d_q, None, None, 4, 64, [(0, 1)], d_rows),
                     lambda: ctx.match8_batch(d_q, d_s, None, 4, 64, [(0, 1)], None),
                     lambda: ctx.match8_batch(d_q + 4, d_s, None, 4, 64, [(0, 1)], d_rows)):
            with pytest.raises(capi.CusiftError):
                call()
    finally:
        d.free()


@pytest.mark.gpu
def test_batch_extractor_quantize_and_match8(gray1):
    """BatchExtractor.quantize(slot) / match8(i, j): the tensors a caller hands to OpenCV or COLMAP are the model's bytes of
    the extractor's own records, allocated once per slot, and match8 runs on them."""
    import torch

    from cusift_amd import capi
    from cusift_amd.batch import BatchExtractor
    from match8_model import FIELDS, quantize_model

    h, w = gray1.shape
    ex = BatchExtractor(2, w, h, num_octaves=4, peak_thresh=2.0, max_pts=4096)
    try:
        with pytest.raises(capi.CusiftError):
            ex.match8(0, 1)  # nothing quantised yet
        ex.extract(ex.images_from_numpy(np.stack([gray1, np.ascontiguousarray(gray1[::-1, ::-1])])))
        q, sums = ex.quantize()
        assert q.dtype == torch.uint8 and tuple(q.shape) == (2, 4096, 128)
        assert sums.dtype == torch.int32 and tuple(sums.shape) == (2, 4096, 2)
        again = ex.quantize()
        assert again[0].data_ptr() == q.data_ptr() and again[1].data_ptr() == sums.data_ptr()  # once per slot
        ex.match8(0, 1)
        torch.cuda.synchronize()
        recs = ex.to_host()
        qh, sh = q.cpu().numpy(), sums.cpu().numpy()
        assert 100 < len(recs[1]) < 4096 and 100 < len(recs[0]) < 4096
        for i in range(2):
            n = len(recs[i])
            want = quantize_model(recs[i]["data"])
            assert qh[i, :n].tobytes() == want.tobytes() and sh[i, :n].tobytes() == sums_model(want).tobytes(), i
            assert not qh[i, n:].any() and not sh[i, n:].any(), i  # rows past the count keep the allocation's zeros
        want = match8_model(qh[0, :len(recs[0])], qh[1, :len(recs[1])], 1, recs[1]["coords2D"])
        for f in FIELDS:
            assert np.ascontiguousarray(recs[0][f]).tobytes() == want[f].tobytes(), f
    finally:
        ex.close()
