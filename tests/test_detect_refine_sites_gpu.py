"""The candidate block of the fused detection (detect_chunk.inc) has ONE check-and-refine per row step, behind a switch
whose 20 (scale, column) cases only push.  What must still hold, against the CPU oracle and for EVERY keypoint:

  (a) candidate-dense rows: one wave collects more than 64 candidates inside a single row, so the check-and-refine fires
      between columns and between scales of that row, several times per chunk;
  (b) overflow beyond max_pts is dropped while the counter keeps counting;
  (c) a sparse image, where only the call at the end of the chunk refines anything;
  (d) every route that pastes the chunk body: identity taps or not (init_blur 1.0 / 0.0, and 0.9: general taps on a
      dense image), records or staged heads, the next octave emitted or not, the multi-octave launch -- reached through
      the pyramid policies 0, 1, 2 and concurrent_batches 1 and 4, on batches of two (per-image lists).

Sizes: widths 256 and 481 cross a strip border (240 columns per wave), 481 and 241 are ragged (w % 4 != 0); chunks are two
rows tall at these sizes (sift_stages.hip: detect_rows), and the 3-row image is one chunk of one row.
"""
import numpy as np
import pytest

from cusift_amd import capi
from cusift_amd.capi import SIFT_POINT_DTYPE, DeviceBuffer
from oracle_binding import pitched
from parity_utils import canonical_order

HEAD = ("subsampling", "coords2D", "scale", "sharpness", "edgeness", "orientation")
STRIP = 240  # columns of extremum centres per wave (kDetStrip)
THRESH = 0.1


def noise(seed, w, h):
    return (np.random.RandomState(seed).rand(h, w) * 255.0).astype(np.float32)


def blob(w, h):
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    return (50.0 + 100.0 * np.exp(-((x - w // 2) ** 2 + (y - h // 2) ** 2) / (2 * 2.0 ** 2))).astype(np.float32)


def candidates(oracle, img, blur, thr):
    """[5, h, w] bool: the strict 26-neighbour extrema beyond the threshold in the oracle's DoG planes 1..5 -- what the
    detection pushes BEFORE refinement (border pixels are never extrema)."""
    h, w = img.shape
    dog = oracle.laplace_multi(pitched(img), w, h, blur)[:, :, :w]
    out = np.zeros((5, h, w), dtype=bool)
    for s in range(1, 6):
        c = dog[s, 1:-1, 1:-1]
        mx = np.full_like(c, -np.inf)
        mn = np.full_like(c, np.inf)
        for p in (s - 1, s, s + 1):
            for dy in range(3):
                for dx in range(3):
                    if (p, dy, dx) != (s, 1, 1):
                        n = dog[p, dy:h - 2 + dy, dx:w - 2 + dx]
                        mx, mn = np.maximum(mx, n), np.minimum(mn, n)
        out[s - 1, 1:-1, 1:-1] = ((c > thr) & (c > mx)) | ((c < -thr) & (c < mn))
    return out


DENSE = [(256, 40), (481, 33)]
SEEDS = (11, 12)  # the two images of a batch


@pytest.mark.parametrize("w,h", DENSE + [(241, 3)])
@pytest.mark.parametrize("blur", [1.0, 0.9])
def test_dense_images_push_more_than_a_batch_per_row(oracle, w, h, blur):
    """The premise of (a), on the oracle: some row of some 240-column strip holds more than 64 candidates."""
    for seed in SEEDS:
        c = candidates(oracle, noise(seed, w, h), blur, THRESH)
        per_row = max(int(c[:, :, x0:x0 + STRIP].sum(axis=(0, 2)).max()) for x0 in range(0, w, STRIP))
        assert per_row > 64, (w, h, blur, seed, per_row)


# ---- detection alone (records, no next octave): cusift_detect_multi against the oracle's FindPointsMulti ----------------
def detect(ctx, img, blur, max_pts):
    h, w = img.shape
    src = pitched(img)
    d_img = DeviceBuffer.from_numpy(ctx, src)
    d_pts = DeviceBuffer(ctx, max_pts * 588)
    d_pts.zero()
    d_cnt = DeviceBuffer(ctx, 4)
    d_cnt.zero()
    ctx.detect_multi(d_img.ptr, w, h, src.shape[1], blur, THRESH, 10.0, 4.0, d_pts.ptr, max_pts, d_cnt.ptr)
    n = int(d_cnt.to_numpy(np.uint32, (1,))[0])
    got = d_pts.to_numpy(SIFT_POINT_DTYPE, (max_pts,)).copy()
    for b in (d_img, d_pts, d_cnt):
        b.free()
    return n, got


def oracle_detect(oracle, img, blur, max_pts=32768):
    h, w = img.shape
    src = pitched(img)
    want, n = oracle.find_points_multi(oracle.laplace_multi(src, w, h, blur), w, h, THRESH, 10.0, 4.0, max_pts)
    return want[:n]


DETECTED = ("coords2D", "scale", "sharpness", "edgeness")


def head_keys(pts, fields):
    return [b"".join(np.ascontiguousarray(r[f]).tobytes() for f in fields) for r in pts]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", DENSE + [(241, 3)])
@pytest.mark.parametrize("blur", [1.0, 0.9, 1.1, 0.0])  # dense at scale 0 (identity taps / general taps), at scale 1, sparse
def test_detection_of_dense_rows_equals_the_oracle(ctx, oracle, w, h, blur):
    img = noise(SEEDS[0], w, h)
    want = canonical_order(oracle_detect(oracle, img, blur))
    n, got = detect(ctx, img, blur, 32768)
    assert n == len(want) and (blur == 0.0 or h == 3 or n > 500), (n, len(want))
    got = canonical_order(got[:n])
    for f in DETECTED:
        np.testing.assert_array_equal(want[f], got[f], err_msg=f)
    # (b) the same image with room for 100: the counter keeps counting, the list holds 100 of the image's keypoints, none twice
    n_small, small = detect(ctx, img, blur, 100)
    assert n_small == len(want)
    kept = small[:min(100, n_small)]
    keys = head_keys(kept, DETECTED)
    assert len(set(keys)) == len(keys) and set(keys) <= set(head_keys(want, DETECTED))


@pytest.mark.gpu
def test_sparse_image_refines_at_the_end_of_the_chunk_only(ctx, oracle):
    """(c) one blob on a flat 64 x 16 image."""
    img = blob(64, 16)
    for blur in (1.0, 0.0):
        want = canonical_order(oracle_detect(oracle, img, blur))
        n, got = detect(ctx, img, blur, 1024)
        assert n == len(want)
        for f in DETECTED:
            np.testing.assert_array_equal(want[f], canonical_order(got[:n])[f], err_msg=f)
    assert sum(len(oracle_detect(oracle, img, b)) for b in (1.0, 0.0)) >= 1


# ---- (d) every route of cusift_extract_batch, against the oracle's whole extraction --------------------------------------
# (side stream, a list per octave, a launch per octave, pyramid policy): see tests/test_octave_overlap_gpu.py
ROUTES = {"records, ScaleDown chain first": (0, 0, False, 0),
          "heads, one launch for the coarser octaves": (0, 1, False, 0),
          "heads, a launch per octave": (0, 1, True, 0),
          "heads, octave 0 emits octave 1, then one launch": (0, 1, False, 1),
          "heads, octave 0 emits octave 1, then a launch per octave": (0, 1, True, 1),
          "heads, every detection emits the next octave": (0, 1, False, 2)}


@pytest.fixture(scope="module")
def routes():
    ctxs = {}
    for name, (side, lists, per_octave, pyramid) in ROUTES.items():
        c = capi.Context(0)
        c.set_policy(capi.POLICY_SIDE_STREAM, side)
        c.set_policy(capi.POLICY_OCTAVE_LISTS, lists)
        if per_octave:
            c.set_policy(capi.POLICY_LAUNCH_PER_OCTAVE, 1)
        c.set_policy(capi.POLICY_PYRAMID_IN_DETECT, pyramid)
        ctxs[name] = c
    yield ctxs
    for c in ctxs.values():
        c.close()


def run_batch(ctx, imgs, prm):
    n = len(imgs)
    h, w = imgs[0].shape
    stack = np.stack([pitched(i) for i in imgs])
    p = stack.shape[2]
    d_imgs = DeviceBuffer.from_numpy(ctx, stack)
    d_pts = DeviceBuffer(ctx, n * prm.max_pts * 588)
    d_pts.zero()
    d_cnt = DeviceBuffer(ctx, 4 * n)
    ctx.extract_batch(d_imgs.ptr, n, w, h, p, h * p, prm, d_pts.ptr, d_cnt.ptr)
    ctx.synchronize()
    cnt = d_cnt.to_numpy(np.uint32, (n,)).copy()
    pts = d_pts.to_numpy(SIFT_POINT_DTYPE, (n, prm.max_pts)).copy()
    for b in (d_imgs, d_pts, d_cnt):
        b.free()
    return cnt, pts


def same_set(want, got, label):
    """EVERY keypoint: the head fields bit for bit (NaN orientations in the same places), every finite descriptor within the
    1e-4 L2 of the existing same-set tests (only the summation order differs)."""
    assert len(want) == len(got), (label, len(want), len(got))
    a, b = canonical_order(want), canonical_order(got)
    for f in HEAD:
        np.testing.assert_array_equal(a[f], b[f], err_msg="%s: %s" % (label, f))
    fin = np.isfinite(a["data"]).all(axis=1)
    np.testing.assert_array_equal(np.isfinite(b["data"]).all(axis=1), fin, err_msg=label)
    if fin.any():
        l2 = np.linalg.norm(a["data"][fin].astype(np.float64) - b["data"][fin].astype(np.float64), axis=1)
        assert l2.max() < 1e-4, (label, float(l2.max()))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", DENSE)
@pytest.mark.parametrize("blur", [1.0, 0.0, 0.9])
def test_every_route_equals_the_oracle(routes, oracle, w, h, blur):
    imgs = [noise(s, w, h) for s in SEEDS]
    kw = dict(num_octaves=3, init_blur=blur, peak_thresh=THRESH, edge_thresh=10.0, max_pts=8192)
    want = [oracle.extract(i, **kw) for i in imgs]  # once, shared by the routes
    assert all(0 < len(x) < kw["max_pts"] for x in want)
    assert blur == 0.0 or min(len(x) for x in want) > 300
    for name, c in routes.items():
        for concurrent in (1, 4):
            label = "%s, concurrent_batches %d" % (name, concurrent)
            cnt, pts = run_batch(c, imgs, capi.default_params(concurrent_batches=concurrent, **kw))
            for i in range(2):
                assert cnt[i] == len(want[i]), (label, i, int(cnt[i]), len(want[i]))
                got = pts[i, : cnt[i]]
                assert np.all(np.diff(got["subsampling"]) <= 0), label  # coarsest octave first
                same_set(want[i], got, label)


@pytest.mark.gpu
@pytest.mark.parametrize("blur", [1.0, 0.9])
def test_every_route_drops_the_overflow_and_counts_on(routes, oracle, blur):
    """(b) through the drivers: max_pts 100 on the dense image."""
    w, h = DENSE[0]
    imgs = [noise(s, w, h) for s in SEEDS]
    kw = dict(num_octaves=3, init_blur=blur, peak_thresh=THRESH, edge_thresh=10.0)
    want = [canonical_order(oracle.extract(i, max_pts=8192, **kw)) for i in imgs]
    for name, c in routes.items():
        cnt, pts = run_batch(c, imgs, capi.default_params(max_pts=100, **kw))
        for i in range(2):
            assert cnt[i] == len(want[i]) > 100, (name, int(cnt[i]), len(want[i]))
            got = pts[i]
            assert np.all(np.diff(got["subsampling"]) <= 0), name
            # the coarser octaves are searched first in the reference: they survive whole (or fill the list alone)
            coarse = want[i][want[i]["subsampling"] > 1.0]
            got_coarse = got[got["subsampling"] > 1.0]
            assert len(got_coarse) == min(100, len(coarse)), (name, len(got_coarse), len(coarse))
            keys = head_keys(got, HEAD)
            assert len(set(keys)) == 100 and set(keys) <= set(head_keys(want[i], HEAD)), name
