"""cusift_describe_batch on the device: an extraction's records come back byte for byte (recorded octave, and octave from
the scale); keypoints the detector never saw equal the CPU oracle's stages at the project's parity bar; kept orientations;
batches, counts and sentinels; skipped records; refusals."""
import itertools

import numpy as np
import pytest

import describe_model as dm
from oracle_binding import pitched

pytestmark = pytest.mark.gpu

KW = dict(num_octaves=5, peak_thresh=1.0)
NAN_PATTERN = np.uint32(0x7fc0beef)


def _capi():
    from cusift_amd import capi

    return capi


def gpu_extract(ctx, img, **kw):
    """cusift_extract_batch on one image: the records straight from the device."""
    capi = _capi()
    prm = capi.default_params(**kw)
    h, w = img.shape
    src = pitched(img)
    d_img = capi.DeviceBuffer.from_numpy(ctx, src)
    d_pts = capi.DeviceBuffer(ctx, prm.max_pts * 588)
    d_pts.zero()
    d_cnt = capi.DeviceBuffer(ctx, 4)
    ctx.extract_batch(d_img.ptr, 1, w, h, src.shape[1], h * src.shape[1], prm, d_pts.ptr, d_cnt.ptr)
    ctx.synchronize()
    n = int(d_cnt.to_numpy(np.uint32, (1,))[0])
    assert 0 < n < prm.max_pts, (n, prm.max_pts)  # nothing saturates
    out = d_pts.to_numpy(capi.SIFT_POINT_DTYPE, (prm.max_pts,))[:n].copy()
    for b in (d_img, d_pts, d_cnt):
        b.free()
    return out


def gpu_describe(ctx, imgs, recs, counts=None, flags=0, **kw):
    """cusift_describe_batch: imgs [n, h, w], recs [n, max_pts] records uploaded as they are, counts uint32 [n] or None.
    Returns the records as the call left them."""
    capi = _capi()
    imgs = np.asarray(imgs, dtype=np.float32)
    recs = np.ascontiguousarray(recs)
    n, h, w = imgs.shape
    assert recs.shape[0] == n and recs.dtype == capi.SIFT_POINT_DTYPE
    prm = capi.default_params(**dict(kw, max_pts=recs.shape[1]))
    src = np.stack([pitched(i) for i in imgs])
    d_img = capi.DeviceBuffer.from_numpy(ctx, src)
    d_pts = capi.DeviceBuffer.from_numpy(ctx, recs)
    d_cnt = capi.DeviceBuffer.from_numpy(ctx, np.asarray(counts, dtype=np.uint32)) if counts is not None else None
    try:
        ctx.describe_batch(d_img.ptr, n, w, h, src.shape[2], h * src.shape[2], prm, d_pts.ptr,
                           d_cnt.ptr if d_cnt else None, flags)
        ctx.synchronize()
        return d_pts.to_numpy(capi.SIFT_POINT_DTYPE, recs.shape)
    finally:
        for b in (d_img, d_pts, d_cnt):
            if b:
                b.free()


def wiped(recs):
    """A copy with orientation and data overwritten by a NaN pattern."""
    out = recs.copy()
    out["orientation"].view(np.uint32)[...] = NAN_PATTERN
    out["data"].view(np.uint32)[...] = NAN_PATTERN
    return out


def assert_same_bytes(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.tobytes() == want.tobytes():
        return
    bad = np.flatnonzero((got.view(np.uint8).reshape(len(got), -1) != want.view(np.uint8).reshape(len(want), -1)).any(axis=1))
    fields = [f for f in got.dtype.names if not np.array_equal(got[f][bad[0]], want[f][bad[0]], equal_nan=False)]
    raise AssertionError("%d of %d records differ, first %d in %s" % (len(bad), len(got), bad[0], fields))


SETTINGS = [dict(root_sift=r, tex_frac_bits=t, upsample=u, subsampling=s)
            for r, t, u, s in itertools.product((0, 1), (8, 0), (0, 1), (1.0, 2.0))]


@pytest.mark.parametrize("setting", SETTINGS, ids=lambda s: "root%d-frac%d-up%d-sub%g" % tuple(s.values()))
def test_round_trip_returns_the_extractions_bytes(ctx, gray1, setting):
    """The same device functions on the same pyramid bits: every one of the 588 bytes of every record -- with the
    recorded octave, with the record's subsampling zeroed, and with CUSIFT_DESCRIBE_OCTAVE_FROM_SCALE."""
    kw = dict(KW, max_pts=16384, **setting)
    want = gpu_extract(ctx, gray1, **kw)
    kw.pop("max_pts")
    print("%d records, subsamplings %s" % (len(want), sorted(set(want["subsampling"].tolist()))))
    assert_same_bytes(gpu_describe(ctx, gray1[None], wiped(want)[None], **kw)[0], want)
    zeroed = wiped(want)
    zeroed["subsampling"] = 0
    assert_same_bytes(gpu_describe(ctx, gray1[None], zeroed[None], **kw)[0], want)
    assert_same_bytes(gpu_describe(ctx, gray1[None], wiped(want)[None], flags=dm.OCTAVE_FROM_SCALE, **kw)[0], want)


def assert_parity(got, want, recs):
    """README "Parity": orientation bit-identical (NaN in the same places), every descriptor within 1e-4 L2, non-finite
    descriptor entries in the same positions, no tolerated fraction; and nothing else of a record moved."""
    np.testing.assert_array_equal(got["subsampling"], want["subsampling"])
    bad = np.flatnonzero(~((got["orientation"] == want["orientation"]) |
                           (np.isnan(got["orientation"]) & np.isnan(want["orientation"]))))
    assert not len(bad), "orientation differs at records %s: %s" % (bad[:8], recs[bad[:8]][["coords2D", "scale"]])
    np.testing.assert_array_equal(np.isfinite(got["data"]), np.isfinite(want["data"]))
    fin = np.isfinite(want["data"]).all(axis=1)
    l2 = np.linalg.norm(got["data"][fin].astype(np.float64) - want["data"][fin].astype(np.float64), axis=1)
    print("%d records, %d finite descriptors, max L2 %.3e" % (len(got), int(fin.sum()), float(l2.max())))
    worst = np.flatnonzero(fin)[np.argsort(l2)[::-1][:4]]
    assert l2.max() < 1e-4, "descriptor L2 %s at records %s: %s" % (np.sort(l2)[::-1][:4], worst, recs[worst][["coords2D", "scale"]])
    rest_got, rest_want = got.copy(), recs.copy()
    for r in (rest_got, rest_want):
        r["orientation"] = 0
        r["data"] = 0
        r["subsampling"] = 0
    assert_same_bytes(rest_got, rest_want)


@pytest.fixture(scope="module")
def unseen(oracle, gray1):
    """Keypoints the detector never saw, as records (everything but coords2D and scale a marker)."""
    capi = _capi()
    pts = oracle.extract(gray1, **KW)
    h, w = gray1.shape
    rows = []
    for dx, dy in ((0.3, -0.45), (3.0, 2.0), (-7.25, 11.5)):  # the extraction's keypoints, displaced
        rows.append(np.stack([pts["coords2D"][:, 0] + np.float32(dx), pts["coords2D"][:, 1] + np.float32(dy), pts["scale"]], 1))
    gx, gy = np.meshgrid(np.arange(4, w, 8, dtype=np.float32), np.arange(4, h, 8, dtype=np.float32))
    for s in (1.5, 4.0, 11.0):  # an 8-pixel grid at three scales (octaves 0, 2, 3)
        rows.append(np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, s, np.float32)], 1))
    border = []
    for t in np.arange(-20.0, 21.0, 6.5, dtype=np.float32):  # up to 20 px outside each border, and the corners
        for s in (1.2, 3.0, 20.0):
            border += [(t, 100.5, s), (w - 1 + t, 200.25, s), (300.75, t, s), (123.0, h - 1 + t, s), (t, t, s),
                       (w - 1 + t, h - 1 + t, s)]
    rows.append(np.array(border, dtype=np.float32))
    # below the detector's range at subsampling 1 (octave -1 with upsample)
    rows.append(np.stack([gx.ravel()[::9] + np.float32(0.37), gy.ravel()[::9], np.full(gx.ravel()[::9].size, 0.7, np.float32)], 1))
    # kscale around 40 in the coarsest octave (no patch holds it: the global sampler), and |x| > 1e5
    rows.append(np.array([(320.0, 240.0, 640.0), (100.0, 400.0, 600.0), (-30.0, 500.0, 700.0), (639.0, 0.0, 2000.0),
                          (250000.0, 100.0, 2.0), (-150000.0, -3.0, 20.0), (10.0, 2.0e5, 1.5)], dtype=np.float32))
    kp = np.concatenate(rows).astype(np.float32)
    recs = np.zeros(len(kp), dtype=capi.SIFT_POINT_DTYPE)
    recs.view(np.uint8)[...] = 0x5A  # whatever the call does not write must come back
    recs["coords2D"], recs["scale"] = kp[:, :2], kp[:, 2]
    recs["subsampling"] = 0
    return recs


@pytest.mark.parametrize("setting", [dict(), dict(root_sift=1, upsample=1), dict(tex_frac_bits=0, subsampling=2.0)],
                         ids=["default", "root-up", "frac0-sub2"])
def test_unseen_keypoints_equal_the_oracle(ctx, oracle, gray1, unseen, setting):
    want, octv, ok = dm.oracle_describe(oracle, gray1, unseen, num_octaves=5, **setting)
    assert ok.all() and len(set(octv.tolist())) == 5, np.bincount(octv)
    got = gpu_describe(ctx, gray1[None], unseen[None], num_octaves=5, **setting)[0]
    assert_parity(got, want, unseen)


def test_kept_orientation(ctx, oracle, gray1, unseen):
    """CUSIFT_DESCRIBE_KEEP_ORIENTATION: the descriptor stage alone, at orientation 0 (upright) and at fixed angles; the
    orientation's bytes stay."""
    recs = unseen[::3].copy()
    angles = np.array([0.0, 37.5, 90.0, 181.25, 359.0, -45.0, 725.0], dtype=np.float32)
    for ori in (np.zeros(len(recs), np.float32), angles[np.arange(len(recs)) % len(angles)]):
        recs["orientation"] = ori
        want, _, _ = dm.oracle_describe(oracle, gray1, recs, flags=dm.KEEP_ORIENTATION, num_octaves=5)
        got = gpu_describe(ctx, gray1[None], recs[None], flags=dm.KEEP_ORIENTATION, num_octaves=5)[0]
        np.testing.assert_array_equal(got["orientation"].view(np.uint32), ori.view(np.uint32))
        assert_parity(got, want, recs)


def crops(gray1, n=3):
    return np.stack([gray1[40 + 90 * (i % 3):88 + 90 * (i % 3), 100 + 150 * (i % 3):164 + 150 * (i % 3)] for i in range(n)])


def crop_records(n_images, max_pts, seed=5):
    capi = _capi()
    rng = np.random.default_rng(seed)
    recs = np.zeros((n_images, max_pts), dtype=capi.SIFT_POINT_DTYPE)
    recs.view(np.uint8)[...] = 0xA5  # the sentinel
    recs["coords2D"][..., 0] = rng.uniform(-4, 68, (n_images, max_pts)).astype(np.float32)
    recs["coords2D"][..., 1] = rng.uniform(-4, 52, (n_images, max_pts)).astype(np.float32)
    recs["scale"] = np.exp(rng.uniform(np.log(1.0), np.log(12.0), (n_images, max_pts))).astype(np.float32)
    recs["subsampling"] = 0
    return recs


@pytest.mark.parametrize("n_images,max_pts", [(3, 32), (257, 5)], ids=["flat", "image-rows"])
def test_batch_counts_and_sentinels(ctx, gray1, n_images, max_pts):
    """Three different 64 x 48 crops (cycled beyond three: 257 images take the walk with an image per grid row): a count
    of 0, a count above max_pts, d_counters = NULL; records beyond a count come back untouched; every image equals its
    single-image result."""
    imgs = crops(gray1, n_images)
    assert not np.array_equal(imgs[0], imgs[1]) and not np.array_equal(imgs[1], imgs[2])
    recs = crop_records(n_images, max_pts)
    single = [gpu_describe(ctx, imgs[i:i + 1], recs[i:i + 1], num_octaves=3)[0] for i in range(3)]
    for i in range(3):
        assert (single[i]["subsampling"] > 0).all() and not np.array_equal(single[i]["data"], recs[i]["data"])
    base = np.array([0, max_pts + 8, max_pts // 2 + 1], dtype=np.uint32)
    for counts in (None, np.resize(base, n_images), np.resize(base[::-1], n_images)):
        got = gpu_describe(ctx, imgs, recs, counts, num_octaves=3)
        for i in range(n_images):
            c = max_pts if counts is None else min(int(counts[i]), max_pts)
            if i < 3:
                assert_same_bytes(got[i, :c], single[i][:c])
            assert_same_bytes(got[i, c:], recs[i, c:])
    if n_images > 3:  # every image against a single-image call of its own, for a sample of the rows
        got = gpu_describe(ctx, imgs, recs, None, num_octaves=3)
        for i in (3, 128, 255, 256):
            assert_same_bytes(got[i], gpu_describe(ctx, imgs[i:i + 1], recs[i:i + 1], num_octaves=3)[0])


def test_skipped_records(ctx, gray1):
    """Every invalid form between valid neighbours: 128 zeros, subsampling 0, the orientation and every other byte as
    they were; the neighbours as if the invalid records were not there."""
    img = crops(gray1, 1)
    recs = crop_records(1, 24, seed=9)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    forms = {1: (0, nan), 3: (1, inf), 5: (2, nan), 7: (2, inf), 9: (2, 0.0), 11: (2, -1.5), 13: (0, -inf), 15: (1, nan),
             17: (2, -inf), 18: (2, -0.0)}
    for i, (field, value) in forms.items():
        if field < 2:
            recs["coords2D"][0, i, field] = value
        else:
            recs["scale"][0, i] = value
    assert not dm.valid(recs["coords2D"][0, :, 0], recs["coords2D"][0, :, 1], recs["scale"][0])[sorted(forms)].any()
    keep = np.array([i for i in range(24) if i not in forms])
    for flags in (0, dm.KEEP_ORIENTATION, dm.OCTAVE_FROM_SCALE):
        got = gpu_describe(ctx, img, recs, flags=flags, num_octaves=3)[0]
        want = recs[0].copy()
        want[keep] = gpu_describe(ctx, img, recs[:, keep], flags=flags, num_octaves=3)[0]
        for i in forms:
            want["data"][i] = 0
            want["subsampling"][i] = 0
        assert_same_bytes(got, want)
        assert (got["subsampling"][keep] > 0).all()


def test_refusals_leave_the_records_alone(ctx, gray1):
    capi = _capi()
    img = pitched(crops(gray1, 1)[0])
    h, w, pitch = 48, 64, img.shape[1]
    recs = crop_records(2, 8)
    d_img = capi.DeviceBuffer.from_numpy(ctx, np.stack([img, img]))
    d_pts = capi.DeviceBuffer.from_numpy(ctx, recs)
    prm = capi.default_params(num_octaves=3, max_pts=8)

    def call(n=2, w=w, h=h, pitch=pitch, stride=h * pitch, prm=prm, imgs=d_img.ptr, pts=d_pts.ptr, flags=0):
        return capi.lib().cusift_describe_batch(ctx.handle, imgs, n, w, h, pitch, stride, capi.C.byref(prm), pts, None, flags)

    bad = [dict(w=0), dict(h=0), dict(pitch=w - 1), dict(n=-1), dict(n=65536), dict(stride=h * pitch - 1),
           dict(flags=4), dict(flags=0x80000001), dict(imgs=None), dict(pts=None),
           dict(prm=capi.default_params(num_octaves=3, max_pts=-1)),
           dict(prm=capi.default_params(num_octaves=3, max_pts=8, upsample=1), w=(1 << 27) + 1, pitch=(1 << 27) + 1),
           dict(prm=capi.default_params(num_octaves=3, max_pts=8, upsample=1), h=4 * 65535 + 1)]
    for kw in bad:
        assert call(**kw) == -1, kw  # CUSIFT_ERR_INVALID
        assert capi.lib().cusift_last_error()
    assert capi.lib().cusift_describe_batch(ctx.handle, d_img.ptr, 2, w, h, pitch, h * pitch, None, d_pts.ptr, None, 0) == -1
    # nothing to do is no error
    assert call(n=0) == 0 and call(prm=capi.default_params(num_octaves=3, max_pts=0)) == 0
    assert call(n=0, imgs=None, pts=None) == 0
    ctx.synchronize()
    assert_same_bytes(d_pts.to_numpy(capi.SIFT_POINT_DTYPE, recs.shape).ravel(), recs.ravel())
    # and the same arguments, unbroken, are accepted
    assert call() == 0
    ctx.synchronize()
    assert (d_pts.to_numpy(capi.SIFT_POINT_DTYPE, recs.shape)["subsampling"] > 0).all()
    d_img.free()
    d_pts.free()


def test_settings_of_the_context_do_not_reach_the_call(ctx, gray1):
    """keep_strongest, cross-check and match-bits belong to other calls; the stage timers see the pyramid and the launch."""
    img, recs = crops(gray1, 1), crop_records(1, 16)
    want = gpu_describe(ctx, img, recs, num_octaves=3)
    ctx.set_keep_strongest(4)
    ctx.set_cross_check(True)
    ctx.set_match_bits(8)
    ctx.timing_enable(True)
    ctx.timing_reset()
    try:
        got = gpu_describe(ctx, img, recs, num_octaves=3)
        t = ctx.timing_read()
    finally:
        ctx.timing_enable(False)
        ctx.set_keep_strongest(0)
        ctx.set_cross_check(False)
        ctx.set_match_bits(32)
    assert_same_bytes(got.ravel(), want.ravel())
    assert t["scale_down"][1] == 2 and t["describe_all"][1] == 1, t
    assert t["detect_multi"][1] == 0 and t["total"][1] == 0, t


def test_host_convenience_and_batch_extractor(ctx, oracle, gray1):
    """Context.describe (host arrays, three or four columns) and BatchExtractor.describe (the slot's own tensors)."""
    import torch

    from cusift_amd.batch import BatchExtractor

    capi = _capi()
    pts = oracle.extract(gray1, **KW)[::7]
    kp3 = np.stack([pts["coords2D"][:, 0], pts["coords2D"][:, 1], pts["scale"]], 1)
    got = ctx.describe(gray1, kp3, num_octaves=5)
    for f in ("coords2D", "scale", "orientation", "subsampling"):
        np.testing.assert_array_equal(got[f], pts[f], err_msg=f)
    assert np.abs(got["data"] - pts["data"]).max() < 1e-4
    kp4 = np.concatenate([kp3, np.zeros((len(kp3), 1), np.float32)], 1)
    upright = ctx.describe(gray1, kp4, num_octaves=5)
    assert (upright["orientation"] == 0).all() and not np.array_equal(upright["data"], got["data"])
    np.testing.assert_array_equal(ctx.describe(gray1, kp4, keep_orientation=False, num_octaves=5)["data"], got["data"])
    assert len(ctx.describe(gray1, np.zeros((0, 3), np.float32))) == 0
    with pytest.raises(ValueError):
        ctx.describe(gray1, kp3, keep_orientation=True)

    imgs = np.stack([gray1, gray1[::-1].copy()])
    ex = BatchExtractor(2, 640, 480, num_octaves=5, peak_thresh=1.0, max_pts=4096)
    try:
        d_imgs = ex.images_from_numpy(imgs)
        points, counts = ex.extract(d_imgs)
        want = points.clone()
        view = points.view(torch.float32).view(2, 4096, 147)
        view[:, :, 5] = float("nan")   # orientation
        view[:, :, 16:144] = float("nan")  # data
        back, _ = ex.describe(d_imgs)
        torch.cuda.synchronize()
        n = torch.clamp(counts, max=4096).tolist()
        assert min(n) > 500
        for i in range(2):
            assert torch.equal(back[i, :n[i]], want[i, :n[i]])
            assert torch.isnan(back.view(torch.float32).view(2, 4096, 147)[i, n[i]:, 5]).all()  # beyond the count: untouched
    finally:
        ex.close()
