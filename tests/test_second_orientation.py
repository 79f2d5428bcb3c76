"""Second-peak orientations on the device (cusift_ctx_set_second_orientation, cusift_second_orientations_batch) against
second_orientation_model.py: every record of every run, no tolerated record -- test_second_orientation_model.py asserts
that no input here has a keypoint whose peak ratio lies within 1e-5 of a tested ratio.

The detection appends an octave's keypoints in the order of an atomic counter, so two extractions may hold the same
records in another order inside an octave.  Records of different runs are therefore paired by the bits of (subsampling,
coords2D, scale) -- unique on every input, asserted -- and the STAGE's own order (duplicates in ascending parent index
behind the records, cut at max_pts) is checked inside every run."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import describe_model as dm
import second_orientation_model as som
from cusift_amd import capi
from cusift_amd.capi import SIFT_POINT_DTYPE, DeviceBuffer
from oracle_binding import pitched
from parity_utils import HEAD_FIELDS

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0x5A


# ------------------------------------------------------------------------------------------------------------------
# surface, without a GPU
# ------------------------------------------------------------------------------------------------------------------
def test_headers_library_and_binding_agree():
    extras = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "cusift_amd_extras.h")).read())
    assert "int cusift_ctx_set_second_orientation(cusift_ctx *ctx, float ratio);" in extras
    assert ("int cusift_second_orientations_batch(cusift_ctx *ctx, const float *d_imgs, int n_images, int w, int h, int pitch, "
            "size_t image_stride, const cusift_params *p, cusift_point *d_points, "
            "unsigned int *d_counters /* in-out, not NULL */, float ratio, unsigned int flags);") in extras
    handle = C.CDLL(capi.LIB_PATH)
    assert hasattr(handle, "cusift_ctx_set_second_orientation") and hasattr(handle, "cusift_second_orientations_batch")
    assert capi.SIGNATURES["cusift_ctx_set_second_orientation"] == (C.c_int, [C.c_void_p, C.c_float])
    assert capi.SIGNATURES["cusift_second_orientations_batch"] == (
        C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(capi.Params),
                  C.c_void_p, C.c_void_p, C.c_float, C.c_uint])
    assert callable(capi.Context.set_second_orientation) and callable(capi.Context.second_orientations)
    from cusift_amd import batch
    assert inspect.signature(batch.BatchExtractor.__init__).parameters["second_orientation"].default == 0.0
    assert callable(batch.BatchExtractor.second_orientations)
    # the contract names its expressions
    for phrase in ("maxval2 > ratio * maxval1", "0.5f * (v1 - v2) / (2.0f * maxval2 - v1 - v2)", "ascending parent index",
                   "d_counters[i] = min(n + m, max_pts)"):
        assert phrase in extras, phrase
    shim = open(os.path.join(ROOT, "include", "cuSIFT.h")).read()
    assert "float secondOrientation;" in shim and "secondOrientation(0.0f)" in shim
    assert shim.count("cusift_ctx_set_second_orientation(cusift_dropin::ctx(), secondOrientation)") == 2
    assert "inline void SecondOrientationsSift(SiftData &siftData, cuImage &img, int numOctaves, float ratio = 0.8f" in shim


def test_binding_rejects_bad_ratios_before_any_device_call():
    ctx = object.__new__(capi.Context)  # no device behind it
    assert capi.check_second_orientation(0) == 0.0 and capi.check_second_orientation(1) == 1.0
    assert capi.check_second_orientation(0.8) == float(np.float32(0.8))
    assert capi.check_second_orientation(np.float32(0.5), allow_off=False) == 0.5
    for bad in (-0.1, 1.0001, float("nan"), float("inf"), "0.8", None, True):
        with pytest.raises(ValueError):
            capi.check_second_orientation(bad)
        with pytest.raises(ValueError):
            capi.Context.set_second_orientation(ctx, bad)
        with pytest.raises(ValueError):
            capi.Context.second_orientations(ctx, 0x1000, 1, 64, 48, 128, 48 * 128, capi.default_params(), 0x2000, 0x3000, bad)
    with pytest.raises(ValueError):  # 0 turns the SETTING off; the stage has nothing to do with it
        capi.check_second_orientation(0.0, allow_off=False)
    with pytest.raises(ValueError):  # the counters are in-out
        capi.Context.second_orientations(ctx, 0x1000, 1, 64, 48, 128, 48 * 128, capi.default_params(), 0x2000, None, 0.8)


# ------------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def sctx():
    """A context of this module's own (the setting is sticky: the session's shared context is never given one)."""
    c = capi.Context(0)
    yield c
    c.close()


_ORACLE_INPUTS = {}


def oracle_input(oracle, gray1, image, **kw):
    """som.oracle_input, computed once per (image, settings) and shared by the tests; never modified."""
    key = (image, tuple(sorted(kw.items())))
    if key not in _ORACLE_INPUTS:
        img = som.other_crop(gray1) if image == "other" else som.case_image(gray1, image)
        _ORACLE_INPUTS[key] = (img,) + som.oracle_input(oracle, img, **kw)
    return _ORACLE_INPUTS[key]


def run_batch(ctx, imgs, prm):
    n = len(imgs)
    h, w = imgs[0].shape
    stack = np.stack([pitched(i) for i in imgs])
    p = stack.shape[2]
    d_imgs = DeviceBuffer.from_numpy(ctx, stack)
    d_pts = DeviceBuffer(ctx, n * prm.max_pts * 588)
    ctx.memset(d_pts.ptr, FILL, n * prm.max_pts * 588)
    d_cnt = DeviceBuffer(ctx, 4 * n)
    try:
        ctx.extract_batch(d_imgs.ptr, n, w, h, p, h * p, prm, d_pts.ptr, d_cnt.ptr)
        ctx.synchronize()
        return d_cnt.to_numpy(np.uint32, (n,)).copy(), d_pts.to_numpy(SIFT_POINT_DTYPE, (n, prm.max_pts)).copy()
    finally:
        for b in (d_imgs, d_pts, d_cnt):
            b.free()


def run_stage(ctx, imgs, pts, cnt, prm, ratio, flags=0):
    """cusift_second_orientations_batch on uploaded records [n, max_pts] and counts [n]."""
    n = len(imgs)
    h, w = imgs[0].shape
    stack = np.stack([pitched(i) for i in imgs])
    p = stack.shape[2]
    d_imgs = DeviceBuffer.from_numpy(ctx, stack)
    d_pts = DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(pts))
    d_cnt = DeviceBuffer.from_numpy(ctx, np.asarray(cnt, dtype=np.uint32))
    try:
        ctx.second_orientations(d_imgs.ptr, n, w, h, p, h * p, prm, d_pts.ptr, d_cnt.ptr, ratio, flags)
        ctx.synchronize()
        return d_cnt.to_numpy(np.uint32, (n,)).copy(), d_pts.to_numpy(SIFT_POINT_DTYPE, pts.shape).copy()
    finally:
        for b in (d_imgs, d_pts, d_cnt):
            b.free()


def keys(recs):
    """One bytes key per record: the bits of (subsampling, coords2D, scale)."""
    k = np.concatenate([recs["subsampling"].reshape(-1, 1), recs["coords2D"].reshape(-1, 2), recs["scale"].reshape(-1, 1)],
                       axis=1).astype(np.float32).view(np.uint32)
    return [row.tobytes() for row in k]


def index_by_key(recs):
    ks = keys(recs)
    table = {k: i for i, k in enumerate(ks)}
    assert len(table) == len(ks), "records with equal (subsampling, coords2D, scale): they cannot be paired"
    return table


def rows_of(recs, table_of_other):
    """For every record the index of the record with the same key in the other set."""
    return np.array([table_of_other[k] for k in keys(recs)], dtype=np.int64)


def heads_only(recs):
    out = recs.copy()
    out["data"] = 0
    return out


def check_image(oracle, cnt, pts, off, orc, ratio, max_pts, tex_frac_bits=8, root_sift=0, label=""):
    """One image of a run with the setting on (cnt, pts [max_pts]) against the run with it off (`off`: its records) and
    the model on the oracle's input `orc` = (records, tap, octave images, subsamplings).  `off` may be a subset of the
    oracle's records (keep_strongest).  Returns the number of duplicates."""
    orc_recs, tap, levels, sub = orc
    n = len(off)
    assert n <= len(orc_recs) and n <= max_pts
    on = pts[:n]
    # the parents: the oracle's records (head fields and orientation bit for bit), every byte of the run with the setting off
    to_orc = rows_of(on, index_by_key(orc_recs))
    for f in HEAD_FIELDS:
        assert np.array_equal(on[f].view(np.uint32), orc_recs[f][to_orc].view(np.uint32)), (label, f)
    assert on.tobytes() == off[rows_of(on, index_by_key(off))].tobytes(), (label, "parents' bytes")
    # the duplicates: the model in THIS run's order
    want, par = som.expected_records(oracle, on, tap[to_orc], ratio, max_pts, levels, sub, tex_frac_bits=tex_frac_bits,
                                     root_sift=root_sift)
    m = len(par)
    total = int(som.parents_of(tap[to_orc], ratio).sum())
    assert m == min(total, max_pts - n)
    print("%s: %d records, %d parents above %g, %d duplicates placed" % (label, n, total, ratio, m))
    assert cnt == n + m == len(want), (label, cnt, n, m)
    got = pts[n:n + m]
    assert heads_only(got).tobytes() == heads_only(want[n:]).tobytes(), (label, "duplicates' heads / orientation / order")
    assert np.array_equal(got["orientation"].view(np.uint32), tap[to_orc][par, 1].view(np.uint32))
    if m:
        l2 = np.linalg.norm(got["data"].astype(np.float64) - want[n:]["data"].astype(np.float64), axis=1)
        print("%s: largest descriptor L2 %.3e" % (label, l2.max()))
        assert np.isfinite(got["data"]).all() and l2.max() < 1e-4, (label, l2.max())
        assert (np.abs(np.linalg.norm(got["data"], axis=1) - 1.0) < 1e-3).all() or root_sift
    assert (pts[cnt:].view(np.uint8) == FILL).all(), (label, "beyond the count")
    return m


def on_and_off(sctx, imgs, prm, ratio):
    sctx.set_second_orientation(0.0)
    cnt0, pts0 = run_batch(sctx, imgs, prm)
    sctx.set_second_orientation(ratio)
    cnt1, pts1 = run_batch(sctx, imgs, prm)
    sctx.set_second_orientation(0.0)
    return cnt0, pts0, cnt1, pts1


def canonical(cnt, pts, n):
    """A run's records in an order that does not depend on the append order: the first n by key, the rest by key."""
    def by_key(recs):
        ks = keys(recs)
        return recs[sorted(range(len(ks)), key=ks.__getitem__)]

    return np.concatenate([by_key(pts[:n]), by_key(pts[n:cnt])]).tobytes()


# ------------------------------------------------------------------------------------------------------------------
# extraction with the setting against the model
# ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("variant", sorted(som.VARIANTS))
def test_crop_against_the_model(sctx, oracle, gray1, variant):
    kw = dict(som.CASES[som.CROP][2], max_pts=1024, **som.VARIANTS[variant])
    img, *orc = oracle_input(oracle, gray1, som.CROP, **dict(kw, max_pts=32768))
    prm = capi.default_params(**kw)
    cnt0, pts0, cnt1, pts1 = on_and_off(sctx, [img], prm, som.RATIO)
    assert cnt0[0] == len(orc[0])
    m = check_image(oracle, int(cnt1[0]), pts1[0], pts0[0, :cnt0[0]], orc, som.RATIO, 1024,
                    tex_frac_bits=kw.get("tex_frac_bits", 8), root_sift=kw.get("root_sift", 0), label=variant)
    assert m > 0
    if variant == "upsample":
        assert (pts1[0, cnt0[0]:cnt1[0]]["subsampling"] == 0.5).any()


@gpu
def test_batch_of_three_with_an_empty_image(sctx, oracle, gray1):
    kw = dict(som.CASES[som.CROP][2], max_pts=512)
    a, *orc_a = oracle_input(oracle, gray1, som.CROP, **dict(kw, max_pts=32768))
    b, *orc_b = oracle_input(oracle, gray1, "other", **dict(kw, max_pts=32768))
    flat = np.full(a.shape, 93.0, dtype=np.float32)
    cnt0, pts0, cnt1, pts1 = on_and_off(sctx, [a, flat, b], capi.default_params(**kw), som.RATIO)
    assert cnt0[1] == 0 and cnt1[1] == 0 and (pts1[1].view(np.uint8) == FILL).all()
    for i, orc in ((0, orc_a), (2, orc_b)):
        assert check_image(oracle, int(cnt1[i]), pts1[i], pts0[i, :cnt0[i]], orc, som.RATIO, 512, label="image %d" % i) > 0


@gpu
@pytest.mark.parametrize("max_pts", [32768, 10000])
def test_full_fixture_at_low_threshold(sctx, oracle, gray1, max_pts):
    """9,501 records and 2,687 parents: the scan's loop turns 38 times; with max_pts 10,000 the image ends at exactly
    10,000 records, the first 499 duplicates in parent order."""
    kw = dict(som.CASES["full-0.1"][2])
    img, *orc = oracle_input(oracle, gray1, "full-0.1", **kw)
    prm = capi.default_params(**dict(kw, max_pts=max_pts))
    cnt0, pts0, cnt1, pts1 = on_and_off(sctx, [img], prm, som.RATIO)
    assert cnt0[0] == 9501
    m = check_image(oracle, int(cnt1[0]), pts1[0], pts0[0, :9501], orc, som.RATIO, max_pts, label="max_pts %d" % max_pts)
    assert (m, int(cnt1[0])) == ((2687, 9501 + 2687) if max_pts == 32768 else (499, 10000))


@gpu
def test_second_ratio_and_ratio_one(sctx, oracle, gray1):
    kw = dict(som.CASES[som.CROP][2], max_pts=1024)
    img, *orc = oracle_input(oracle, gray1, som.CROP, **dict(kw, max_pts=32768))
    prm = capi.default_params(**kw)
    cnt0, pts0, cnt1, pts1 = on_and_off(sctx, [img], prm, som.RATIO_LOW)
    assert check_image(oracle, int(cnt1[0]), pts1[0], pts0[0, :cnt0[0]], orc, som.RATIO_LOW, 1024, label="ratio 0.5") == 100
    _, _, cnt2, pts2 = on_and_off(sctx, [img], prm, 1.0)
    assert cnt2[0] == cnt0[0] == 234
    assert canonical(cnt2[0], pts2[0], 234) == canonical(cnt0[0], pts0[0], 234)
    assert (pts2[0, 234:].view(np.uint8) == FILL).all()


# ------------------------------------------------------------------------------------------------------------------
# the stage call
# ------------------------------------------------------------------------------------------------------------------
def parent_rows(cnt, pts, n):
    """The parent index of every duplicate of a run (by key); asserts the stage's order."""
    par = rows_of(pts[n:cnt], index_by_key(pts[:n]))
    assert (np.diff(par) > 0).all(), "duplicates are not in ascending parent index"
    return par


@gpu
def test_stage_call_and_setting_agree(sctx, oracle, gray1):
    """cusift_second_orientations_batch on the records of a plain extraction: the bytes of the setting, all records, on a
    batch; and the same input twice gives the same bytes, in the same places."""
    kw = dict(som.CASES[som.CROP][2], max_pts=300)  # 234 + 32 fit, the other crop's 64 + 26 too
    imgs = [som.case_image(gray1, som.CROP), np.full((150, 200), 7.0, np.float32), som.other_crop(gray1)]
    prm = capi.default_params(**kw)
    cnt0, pts0, cnt1, pts1 = on_and_off(sctx, imgs, prm, som.RATIO)
    cnt_s, pts_s = run_stage(sctx, imgs, pts0, cnt0, prm, som.RATIO)
    assert list(cnt_s) == list(cnt1) and cnt_s[1] == 0 and cnt_s[0] == 234 + 32
    for i in range(3):
        assert pts_s[i, :cnt0[i]].tobytes() == pts0[i, :cnt0[i]].tobytes()  # records [0, n) keep every byte
        assert canonical(cnt_s[i], pts_s[i], cnt0[i]) == canonical(cnt1[i], pts1[i], cnt0[i]), i
        parent_rows(cnt_s[i], pts_s[i], cnt0[i])
        parent_rows(cnt1[i], pts1[i], cnt0[i])
        assert (pts_s[i, cnt_s[i]:].view(np.uint8) == FILL).all()
    cnt_t, pts_t = run_stage(sctx, imgs, pts0, cnt0, prm, som.RATIO)
    assert cnt_t.tobytes() == cnt_s.tobytes() and pts_t.tobytes() == pts_s.tobytes()
    # a raw counter above max_pts: every slot is a record, nothing is appended, the counter comes back as max_pts
    full = np.ascontiguousarray(pts_s[:1, :266])
    cnt_f, pts_f = run_stage(sctx, imgs[:1], full, [4000], capi.default_params(**dict(kw, max_pts=266)), som.RATIO)
    assert cnt_f[0] == 266 and pts_f.tobytes() == full.tobytes()


@gpu
def test_caller_supplied_keypoints(sctx, oracle, gray1):
    """An 8-pixel grid at two scales with an invalid record and one outside the image: cusift_describe_batch, then the
    stage, against the oracle's orientation stage with the tap registered and its descriptor stage."""
    img = som.case_image(gray1, som.CROP)
    grid = som.grid_records(SIFT_POINT_DTYPE)
    n, max_pts = len(grid), 1100  # 952 records and 217 parents: the last 69 do not fit
    recs = np.zeros((1, max_pts), dtype=SIFT_POINT_DTYPE)
    recs.view(np.uint8)[...] = FILL
    recs[0, :n] = grid
    prm = capi.default_params(num_octaves=4, max_pts=max_pts)
    stack = pitched(img)[None]
    p = stack.shape[2]
    d_img = DeviceBuffer.from_numpy(sctx, stack)
    d_pts = DeviceBuffer.from_numpy(sctx, recs)
    d_cnt = DeviceBuffer.from_numpy(sctx, np.array([n], dtype=np.uint32))
    try:
        sctx.describe_batch(d_img.ptr, 1, 200, 150, p, 150 * p, prm, d_pts.ptr, d_cnt.ptr, 0)
        sctx.synchronize()
        described = d_pts.to_numpy(SIFT_POINT_DTYPE, recs.shape).copy()[0]
        sctx.second_orientations(d_img.ptr, 1, 200, 150, p, 150 * p, prm, d_pts.ptr, d_cnt.ptr, som.RATIO)
        sctx.synchronize()
        cnt = int(d_cnt.to_numpy(np.uint32, (1,))[0])
        got = d_pts.to_numpy(SIFT_POINT_DTYPE, recs.shape).copy()[0]
    finally:
        for b in (d_img, d_pts, d_cnt):
            b.free()
    levels = dm.oracle_pyramid(oracle, img, 4)
    sub = dm.octave_subsamplings(4, 1.0, 0, 200, 150)
    tap = som.oracle_tap(oracle, levels, sub, grid)
    # the orientation stage of the describe call and the tap's first peak are one histogram: bit-identical
    want_desc, _, ok = dm.oracle_describe(oracle, img, grid, num_octaves=4)
    assert (~ok).sum() == 1
    assert np.array_equal(described[:n]["orientation"][ok].view(np.uint32), want_desc["orientation"][ok].view(np.uint32))
    want, par = som.expected_records(oracle, described[:n], tap, som.RATIO, max_pts, levels, sub)
    assert int(som.parents_of(tap, som.RATIO).sum()) == 217 and len(par) == max_pts - n == 148 and cnt == max_pts
    assert got[:n].tobytes() == described[:n].tobytes()
    assert heads_only(got[n:]).tobytes() == heads_only(want[n:]).tobytes()
    l2 = np.linalg.norm(got[n:]["data"].astype(np.float64) - want[n:]["data"].astype(np.float64), axis=1)
    print("grid: %d duplicates placed of 217, largest descriptor L2 %.3e" % (len(par), l2.max()))
    assert l2.max() < 1e-4
    assert not np.isin(np.flatnonzero(~ok), par).any()


@gpu
def test_keep_strongest_with_the_setting(sctx, oracle, gray1):
    """The selection runs first: the first 100 records are its bytes, the duplicates those of the kept parents only."""
    kw = dict(som.CASES[som.CROP][2], max_pts=1024)
    img, *orc = oracle_input(oracle, gray1, som.CROP, **dict(kw, max_pts=32768))
    prm = capi.default_params(**kw)
    sctx.set_keep_strongest(100)
    cnt0, pts0, cnt1, pts1 = on_and_off(sctx, [img], prm, som.RATIO)
    assert cnt0[0] == 100
    m = check_image(oracle, int(cnt1[0]), pts1[0], pts0[0, :100], orc, som.RATIO, 1024, label="keep 100")
    assert m == 16 and cnt1[0] == 116  # 16 of the oracle's 100 strongest have a second peak above 0.8


# ------------------------------------------------------------------------------------------------------------------
# repeated runs, recordings, refusals
# ------------------------------------------------------------------------------------------------------------------
@gpu
def test_repeated_runs_graph_replay_and_reset(sctx, gray1):
    img = som.case_image(gray1, som.CROP)
    prm = capi.default_params(**dict(som.CASES[som.CROP][2], max_pts=1024))
    sctx.set_second_orientation(som.RATIO)
    cnt_a, pts_a = run_batch(sctx, [img], prm)
    cnt_b, pts_b = run_batch(sctx, [img], prm)
    assert cnt_a[0] == cnt_b[0] == 234 + 32
    assert canonical(cnt_a[0], pts_a[0], 234) == canonical(cnt_b[0], pts_b[0], 234)
    # a recording made with the setting on replays it, whatever the setting is at replay
    src = pitched(img)
    h, w = img.shape
    p = src.shape[1]
    d_img = DeviceBuffer.from_numpy(sctx, src)
    d_pts = DeviceBuffer(sctx, prm.max_pts * 588)
    d_cnt = DeviceBuffer(sctx, 4)
    g = sctx.record_graph(d_img.ptr, 1, w, h, p, h * p, prm, d_pts.ptr, d_cnt.ptr)
    sctx.set_second_orientation(0.0)
    for _ in range(2):
        sctx.memset(d_pts.ptr, FILL, prm.max_pts * 588)
        g.launch()
        sctx.synchronize()
        n = int(d_cnt.to_numpy(np.uint32, (1,))[0])
        rec = d_pts.to_numpy(SIFT_POINT_DTYPE, (prm.max_pts,)).copy()
        assert n == cnt_a[0] and canonical(n, rec, 234) == canonical(cnt_a[0], pts_a[0], 234)
        parent_rows(n, rec, 234)
        assert (rec[n:].view(np.uint8) == FILL).all()
    g.close()
    for b in (d_img, d_pts, d_cnt):
        b.free()
    # on, then off: the bytes of a context that never had it
    cnt0, pts0 = run_batch(sctx, [img], prm)
    with capi.Context(0) as fresh:
        cnt1, pts1 = run_batch(fresh, [img], prm)
    assert cnt0[0] == cnt1[0] == 234
    assert canonical(234, pts0[0], 234) == canonical(234, pts1[0], 234)
    assert (pts0[0, 234:].view(np.uint8) == FILL).all()


@gpu
def test_refusals_enqueue_nothing(sctx, gray1):
    img = som.case_image(gray1, som.CROP)
    kw = dict(som.CASES[som.CROP][2], max_pts=512)
    prm = capi.default_params(**kw)
    lib = capi.lib()
    nan = float("nan")
    for bad in (-0.5, 1.5, nan, float("inf")):  # straight at the library
        assert lib.cusift_ctx_set_second_orientation(sctx.handle, bad) == -1 and lib.cusift_last_error()
    cnt0, pts0 = run_batch(sctx, [img], prm)  # ... and none of them stuck
    assert cnt0[0] == 234

    stack = pitched(img)[None]
    p = stack.shape[2]
    d_img = DeviceBuffer.from_numpy(sctx, stack)
    d_pts = DeviceBuffer.from_numpy(sctx, pts0)
    d_cnt = DeviceBuffer.from_numpy(sctx, cnt0)

    def stage(ratio=0.8, counters=d_cnt.ptr, flags=0, w=200, prm=prm, imgs=d_img.ptr):
        return lib.cusift_second_orientations_batch(sctx.handle, imgs, 1, w, 150, p, 150 * p, C.byref(prm) if prm else None,
                                                    d_pts.ptr, counters, ratio, flags)

    for kwargs in (dict(ratio=-0.1), dict(ratio=0.0), dict(ratio=1.25), dict(ratio=nan), dict(counters=None),
                   dict(flags=1), dict(flags=4), dict(w=0), dict(prm=None), dict(imgs=None)):
        assert stage(**kwargs) == -1, kwargs
        assert lib.cusift_last_error()
    sctx.synchronize()
    assert d_pts.to_numpy(SIFT_POINT_DTYPE, pts0.shape).tobytes() == pts0.tobytes()
    assert d_cnt.to_numpy(np.uint32, (1,))[0] == 234
    assert stage() == 0  # the same arguments, unbroken, are accepted
    sctx.synchronize()
    assert d_cnt.to_numpy(np.uint32, (1,))[0] == 234 + 32
    for b in (d_img, d_pts, d_cnt):
        b.free()

    def refused(prm, word):
        with pytest.raises(capi.CusiftError) as e:
            run_batch(sctx, [img], prm)
        assert "cusift error -1:" in str(e.value) and word in str(e.value), str(e.value)

    sctx.set_second_orientation(0.8)
    refused(capi.default_params(fused_detect=0, **kw), "fused_detect")
    sctx.set_policy(capi.POLICY_GENERIC_KERNELS, 1)
    refused(prm, "GENERIC_KERNELS")
    sctx.set_policy(capi.POLICY_GENERIC_KERNELS, 0)
    with pytest.raises(capi.CusiftError) as e:  # the tiled path
        capi.Tiled(sctx, None, 0, 1, 256, 768, prm)
    assert "cusift error -1:" in str(e.value) and "second_orientation" in str(e.value)
    cnt, _ = run_batch(sctx, [img], prm)  # ... and the setting still works afterwards
    assert cnt[0] == 234 + 32
    sctx.set_second_orientation(0.0)
    cnt, _ = run_batch(sctx, [img], capi.default_params(fused_detect=0, **kw))  # off: the per-octave sequence is accepted
    assert cnt[0] == 234


@gpu
def test_batch_extractor_option_and_stage(oracle, gray1):
    import torch

    from cusift_amd.batch import BatchExtractor

    imgs = np.stack([som.case_image(gray1, som.CROP), som.other_crop(gray1)])
    kw = dict(som.CASES[som.CROP][2], max_pts=512)
    on = BatchExtractor(2, 200, 150, second_orientation=0.8, **kw)
    off = BatchExtractor(2, 200, 150, **kw)
    try:
        _, counts_on = on.extract(on.images_from_numpy(imgs))
        d_imgs = off.images_from_numpy(imgs)
        _, counts_off = off.extract(d_imgs)
        torch.cuda.synchronize()
        assert counts_off.tolist() == [234, 64] and counts_on.tolist() == [234 + 32, 64 + 26]
        _, counts_st = off.second_orientations(d_imgs)
        torch.cuda.synchronize()
        assert counts_st.tolist() == counts_on.tolist()
    finally:
        on.close()
        off.close()
