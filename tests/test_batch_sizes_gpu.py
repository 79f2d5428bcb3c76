"""Per-image bookkeeping beyond one wave: batches of 63 .. 257 images through cusift_extract_batch, and the three pack
kernels at 1 .. 256 images.

`running_sums_in_place` (sift_keypoints.hip) scans 64 images per pass and carries a sum into the next; its callers are
describe_all_kernel (with the segment ends of join_counts_kernel, or joining the segments itself) and the pack
kernels.  With it go describe_all_kernel's walk over empty images, the kept / room clamp of the join under
saturation, and the switch to the launch-per-octave path beyond 256 images.  Tiny images reach all of it: every image
of a batch must come out exactly as it does alone.
"""
import numpy as np
import pytest

from cusift_amd import capi, synth
from cusift_amd.capi import SIFT_POINT_DTYPE, DeviceBuffer
from oracle_binding import pitched
from parity_utils import canonical_order
from test_compact import UNWRITTEN, WRITTEN, compact_reference
from test_octave_overlap_gpu import FIELDS, MODES, context_with

W, H = 128, 96
KW = dict(num_octaves=3, init_blur=0.5, peak_thresh=2.0)  # test_forked_equals_one_stream's (5, 128, 96, 3, 0.5) case
MAX_PTS = 256
FILL = 0x5A
CANARIES = 2
SIZES = (63, 64, 65, 128, 129, 255, 256, 257)
TILE_SEEDS = (4003, 4004, 4005, 4006, 4009)  # five tiles (pre-blurred by 0.5): keypoints in all three octaves but one
RAW_SEED = 4010                              # a raw tile (preblur 0): the most keypoints
_distinct = []


def distinct_images():
    """Seven images: five tiles, a constant one (no keypoints), the raw tile (the most keypoints)."""
    if not _distinct:
        imgs = [synth.tile(s, W, H, 0.5) for s in TILE_SEEDS]
        imgs.append(np.full((H, W), 9.0, dtype=np.float32))
        imgs.append(synth.tile(RAW_SEED, W, H, 0.0))
        _distinct.append(imgs)
    return _distinct[0]


def pattern(n):
    """Which distinct image is image i of a batch: steps of 3 through the seven, shifted by one every seven images.  (A
    quadratic such as (i * i + 3 * i) % 7 takes only four of the seven values and repeats one at i = 5, 6: it cannot have
    the properties test_batch_pattern_properties asks for.)"""
    return [(3 * i + i // 7) % 7 for i in range(n)]


def test_batch_pattern_properties(oracle):
    pat = pattern(max(SIZES))
    assert all(a != b for a, b in zip(pat, pat[1:]))  # no two neighbours equal
    for b in range(0, 256, 64):  # every distinct image in every 64-image block
        assert set(pat[b:b + 64]) == set(range(7)), b
    assert pat[256] != pat[255]
    want = [len(oracle.extract(img, max_pts=MAX_PTS, **KW)) for img in distinct_images()]
    assert want[5] == 0 and all(c > 0 for i, c in enumerate(want) if i != 5)
    nonzero = [c for i, c in enumerate(want) if i != 5]
    assert len(set(nonzero)) == 6 and max(nonzero) == want[6] < MAX_PTS  # pairwise different, the raw tile the most
    # under the saturating max_pts (the third-largest count) three images fill the list, with room for octave 0 to lose
    cap = sorted(want)[-3]
    assert sum(c >= cap for c in want) == 3 and sum(c > cap for c in want) == 2
    for i, img in enumerate(distinct_images()):
        if want[i] >= cap:
            pts = oracle.extract(img, max_pts=MAX_PTS, **KW)
            assert 0 < (pts["subsampling"] > 1.0).sum() < cap


# ------------------------------------------------------------------------------------------------
# Extraction
# ------------------------------------------------------------------------------------------------
def run_batch(ctx, n, max_pts, graph=False):
    """cusift_extract_batch of the pattern's first n images into sentinel-filled records (+ canaries behind them)."""
    imgs = distinct_images()
    stack = np.stack([pitched(imgs[k]) for k in pattern(n)])
    p = stack.shape[2]
    prm = capi.default_params(max_pts=max_pts, **KW)
    d_imgs = DeviceBuffer.from_numpy(ctx, stack)
    d_pts = DeviceBuffer(ctx, (n * max_pts + CANARIES) * 588)
    ctx.memset(d_pts.ptr, FILL, d_pts.nbytes)
    d_cnt = DeviceBuffer(ctx, 4 * n)
    ctx.memset(d_cnt.ptr, FILL, 4 * n)
    if graph:
        g = ctx.record_graph(d_imgs.ptr, n, W, H, p, H * p, prm, d_pts.ptr, d_cnt.ptr)
        g.launch()
        ctx.synchronize()
        g.close()
    else:
        ctx.extract_batch(d_imgs.ptr, n, W, H, p, H * p, prm, d_pts.ptr, d_cnt.ptr)
        ctx.synchronize()
    cnt = d_cnt.to_numpy(np.uint32, (n,)).copy()
    rec = d_pts.to_numpy(SIFT_POINT_DTYPE, (n * max_pts + CANARIES,)).copy()
    for b in (d_imgs, d_pts, d_cnt):
        b.free()
    return cnt, rec[:n * max_pts].reshape(n, max_pts), rec[n * max_pts:]


def field_bytes(recs, fields=FIELDS):
    return [np.ascontiguousarray(recs[f]).tobytes() for f in fields]


def row_keys(recs):
    """One bytes key per record over the fields extraction writes."""
    cols = [np.ascontiguousarray(recs[f]).view(np.uint8).reshape(len(recs), -1) for f in FIELDS]
    joined = np.concatenate(cols, axis=1)
    return [r.tobytes() for r in joined]


def untouched(recs):
    return all((np.ascontiguousarray(recs[f]).view(np.uint8) == FILL).all() for f in UNWRITTEN)


@pytest.fixture(scope="module")
def expected():
    """Every distinct image extracted alone (n = 1) on the one-stream context: (count, records in canonical order)."""
    imgs = distinct_images()
    prm = capi.default_params(max_pts=MAX_PTS, **KW)
    out = []
    with context_with(0, 0) as c:
        for img in imgs:
            src = pitched(img)
            d_img = DeviceBuffer.from_numpy(c, src)
            d_pts = DeviceBuffer(c, MAX_PTS * 588)
            c.memset(d_pts.ptr, FILL, d_pts.nbytes)
            d_cnt = DeviceBuffer(c, 4)
            c.extract_batch(d_img.ptr, 1, W, H, src.shape[1], H * src.shape[1], prm, d_pts.ptr, d_cnt.ptr)
            c.synchronize()
            k = int(d_cnt.to_numpy(np.uint32, (1,))[0])
            rec = d_pts.to_numpy(SIFT_POINT_DTYPE, (MAX_PTS,)).copy()
            assert k < MAX_PTS and (rec[k:].view(np.uint8) == FILL).all()
            out.append((k, canonical_order(rec[:k])))
            for b in (d_img, d_pts, d_cnt):
                b.free()
    return out


@pytest.mark.gpu
def test_expected_records_match_the_oracle(expected, oracle):
    from test_gpu_parity import compare_sets

    counts = [k for k, _ in expected]
    print("expected counts of the seven images:", counts)
    assert counts[5] == 0
    for i in range(5):
        want = oracle.extract(distinct_images()[i], max_pts=MAX_PTS, **KW)
        compare_sets(want, expected[i][1])
    assert counts[6] == len(oracle.extract(distinct_images()[6], max_pts=MAX_PTS, **KW))


def check_batch(cnt, pts, canaries, n, expected, max_pts=MAX_PTS):
    pat = pattern(n)
    assert len(cnt) == n
    np.testing.assert_array_equal(cnt, [expected[k][0] for k in pat])  # the counters
    assert (canaries.view(np.uint8) == FILL).all()
    want_bytes = {k: field_bytes(expected[k][1]) for k in set(pat)}
    for i, k in enumerate(pat):
        count, whole = expected[k]
        valid = min(count, max_pts)
        got = pts[i, :valid]
        assert (pts[i, valid:].view(np.uint8) == FILL).all(), i  # slots beyond the count
        assert untouched(got), i                                  # the fields extraction does not write
        assert np.all(np.diff(got["subsampling"]) <= 0), i        # coarsest octave first
        if count <= max_pts:
            assert field_bytes(canonical_order(got)) == want_bytes[k], (i, k)
            continue
        # saturated: the counter counted on (asserted above), exactly max_pts records are valid, octaves >= 1 are complete
        # and equal, the octave-0 rows are distinct members of the unsaturated octave-0 set
        assert np.isin(got["subsampling"], (1.0, 2.0, 4.0)).all(), i
        coarse = canonical_order(got[got["subsampling"] > 1.0])
        assert field_bytes(coarse) == field_bytes(whole[whole["subsampling"] > 1.0]), (i, k)
        fine = got[got["subsampling"] == 1.0]
        assert len(fine) == max_pts - len(coarse) > 0
        have = set(row_keys(whole[whole["subsampling"] == 1.0]))
        seen = set(row_keys(fine))
        assert len(seen) == len(fine) and seen <= have, (i, k)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_every_image_of_a_batch_equals_the_image_alone(ctx, expected, n):
    """All eight sizes on the default context; 257 leaves the flattened path (a launch per octave and stage)."""
    cnt, pts, canaries = run_batch(ctx, n, MAX_PTS)
    check_batch(cnt, pts, canaries, n, expected)


@pytest.mark.gpu
@pytest.mark.parametrize("n", (65, 129, 256))
@pytest.mark.parametrize("mode", sorted(MODES))
def test_every_staged_driver_beyond_one_wave_of_images(expected, mode, n):
    with context_with(*MODES[mode]) as c:
        cnt, pts, canaries = run_batch(c, n, MAX_PTS)
    check_batch(cnt, pts, canaries, n, expected)


@pytest.mark.gpu
@pytest.mark.parametrize("n", (65, 256))
@pytest.mark.parametrize("mode", ["default"] + sorted(MODES))
def test_saturation_beyond_one_wave_of_images(ctx, expected, mode, n):
    """max_pts = the third-largest count: three of the seven images fill their list (one of them exactly), and for them
    test_saturation_keeps_the_coarser_octaves' assertions hold; the others are as before."""
    cap = sorted(k for k, _ in expected)[-3]
    assert sum(k > cap for k, _ in expected) == 2
    if mode == "default":
        cnt, pts, canaries = run_batch(ctx, n, cap)
    else:
        with context_with(*MODES[mode]) as c:
            cnt, pts, canaries = run_batch(c, n, cap)
    check_batch(cnt, pts, canaries, n, expected, max_pts=cap)


@pytest.mark.gpu
def test_graph_replay_at_65_images(ctx, expected):
    n = 65
    cnt_e, pts_e, can_e = run_batch(ctx, n, MAX_PTS)
    cnt_g, pts_g, can_g = run_batch(ctx, n, MAX_PTS, graph=True)
    check_batch(cnt_g, pts_g, can_g, n, expected)
    np.testing.assert_array_equal(cnt_g, cnt_e)
    assert can_g.tobytes() == can_e.tobytes()
    for i in range(n):  # the same bytes, whole records, in the order that is specified (inside an octave it is not)
        k = int(cnt_e[i])
        assert canonical_order(pts_g[i, :k]).tobytes() == canonical_order(pts_e[i, :k]).tobytes(), i
        assert pts_g[i, k:].tobytes() == pts_e[i, k:].tobytes(), i


# ------------------------------------------------------------------------------------------------
# The pack kernels
# ------------------------------------------------------------------------------------------------
PACK_MAX_PTS = 5
PACK_SIZES = (1, 64, 65, 130, 256)


def pack_inputs(n):
    """Counters from 0 to 7 (some 0, some beyond max_pts, an empty image in every 64-image block) and records whose every
    byte is random but finite as a float."""
    rng = np.random.default_rng(100 + n)
    cnt = rng.integers(0, 8, n).astype(np.uint32)
    if n == 1:
        cnt[0] = 7
    else:
        for b in range(0, n, 64):
            m = min(64, n - b)
            cnt[b + 17 % m] = 0
            cnt[b + 18 % m] = 7
            cnt[b + m - 1] = 6 if m > 2 else cnt[b + m - 1]
        assert all((cnt[b:b + 64] == 0).any() for b in range(0, n, 64) if n - b >= 2) and (cnt > PACK_MAX_PTS).any()
    words = rng.integers(0, 1 << 32, n * PACK_MAX_PTS * 147, dtype=np.uint64).astype(np.uint32)
    words = np.where((words & 0x7F800000) == 0x7F800000, words & ~np.uint32(0x00800000), words).astype(np.uint32)
    rec = words.view(SIFT_POINT_DTYPE).reshape(n, PACK_MAX_PTS)
    assert np.isfinite(words.view(np.float32)).all()
    valid = np.minimum(cnt, PACK_MAX_PTS)
    flat = np.concatenate([rec[i, : valid[i]] for i in range(n)])
    offsets = np.concatenate([[0], np.cumsum(valid)]).astype(np.uint32)
    return cnt, rec, flat, offsets


def packed_call(ctx, call, cnt, rec, rec_bytes, capacity, slots):
    n = len(cnt)
    d_pts = DeviceBuffer.from_numpy(ctx, rec)
    d_cnt = DeviceBuffer.from_numpy(ctx, cnt)
    d_out = DeviceBuffer(ctx, slots * rec_bytes)
    ctx.memset(d_out.ptr, 0xEE, d_out.nbytes)
    d_off = DeviceBuffer(ctx, 4 * (n + 2))
    ctx.memset(d_off.ptr, 0xEE, 4 * (n + 2))
    call(d_pts.ptr, d_cnt.ptr, n, PACK_MAX_PTS, d_out.ptr, capacity, d_off.ptr)
    ctx.synchronize()
    out = d_out.to_numpy(np.uint8, (slots, rec_bytes)).copy()
    off = d_off.to_numpy(np.uint32, (n + 2,)).copy()
    for b in (d_pts, d_cnt, d_off):
        b.free()
    return out, off, d_out


@pytest.mark.gpu
@pytest.mark.parametrize("n", PACK_SIZES)
def test_pack_points_at_batch_sizes(ctx, n):
    cnt, rec, flat, offsets = pack_inputs(n)
    total = len(flat)
    for capacity in (total, total + 3, max(total - 3, 0), 1):
        out, off, d_out = packed_call(ctx, ctx.pack_points, cnt, rec, 588, capacity, total + 4)
        d_out.free()
        np.testing.assert_array_equal(off[: n + 1], offsets)  # the clamped running sums, whatever the capacity
        assert off[n + 1] == 0xEEEEEEEE
        m = min(total, capacity)
        assert out[:m].tobytes() == flat[:m].tobytes(), capacity
        assert (out[m:] == 0xEE).all(), capacity  # nothing behind the capacity (or the total)


@pytest.mark.gpu
@pytest.mark.parametrize("n", PACK_SIZES)
def test_pack_points_trimmed_at_batch_sizes(ctx, n):
    cnt, rec, flat, offsets = pack_inputs(n)
    total = len(flat)
    out, off, d_out = packed_call(ctx, ctx.pack_points_trimmed, cnt, rec, 540, total, total + 4)
    np.testing.assert_array_equal(off[: n + 1], offsets)
    assert (out[total:] == 0xEE).all()
    d_back = DeviceBuffer(ctx, (total + 1) * 588)
    ctx.memset(d_back.ptr, 0x77, d_back.nbytes)
    ctx.expand_trimmed(d_out.ptr, total, d_back.ptr)
    ctx.synchronize()
    back_raw = d_back.to_numpy(np.uint8, (total + 1, 588)).copy()
    assert (back_raw[total] == 0x77).all()
    back = back_raw[:total].copy().view(SIFT_POINT_DTYPE).reshape(-1)
    for f in WRITTEN:  # the 135 floats the header names
        assert np.ascontiguousarray(back[f]).tobytes() == np.ascontiguousarray(flat[f]).tobytes(), f
    for f in UNWRITTEN:
        assert not np.ascontiguousarray(back[f]).view(np.uint8).any(), f
    for b in (d_out, d_back):
        b.free()


@pytest.mark.gpu
@pytest.mark.parametrize("n", PACK_SIZES)
def test_pack_points_compact_at_batch_sizes(ctx, n):
    cnt, rec, flat, offsets = pack_inputs(n)
    total = len(flat)
    out, off, d_out = packed_call(ctx, ctx.pack_points_compact, cnt, rec, 160, total, total + 4)
    d_out.free()
    np.testing.assert_array_equal(off[: n + 1], offsets)
    assert (out[total:] == 0xEE).all()
    assert out[:total].tobytes() == compact_reference(flat).tobytes()


@pytest.mark.gpu
def test_pack_refuses_257_images(ctx):
    cnt = np.zeros(257, dtype=np.uint32)
    d_cnt = DeviceBuffer.from_numpy(ctx, cnt)
    d_pts = DeviceBuffer(ctx, 257 * PACK_MAX_PTS * 588)
    d_out = DeviceBuffer(ctx, 588)
    for call in (ctx.pack_points, ctx.pack_points_trimmed, ctx.pack_points_compact):
        with pytest.raises(capi.CusiftError, match=r"n_images must be in \[1, 256\]"):
            call(d_pts.ptr, d_cnt.ptr, 257, PACK_MAX_PTS, d_out.ptr, 1, None)
    for b in (d_cnt, d_pts, d_out):
        b.free()
