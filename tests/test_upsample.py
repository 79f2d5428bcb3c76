"""Octave -1: the 2x enlargement (cusift_scale_up) and cusift_params.upsample through every extraction driver.

The enlargement is defined bit for bit (include/cusift_amd.h); `up2` below restates it in numpy float32.  The yardstick
of the extraction is the CPU oracle run on the numpy-enlarged image with subsampling 0.5 and twice the init_blur: the
driver option must give exactly that, at the project's every-keypoint bar (same point set, header fields and orientation
identical, every descriptor within 1e-4 L2)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle_binding import pitched
from parity_utils import canonical_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_upsample")
BIN = os.path.join(CPP, "upsample_dropin")
PGM = os.path.join(ROOT, "tests", "golden", "gray1.pgm")
FIELDS = ("coords2D", "scale", "sharpness", "edgeness", "orientation", "subsampling", "data")


def up2(img):
    """The four formulas of cusift_scale_up in numpy float32, associated as the header writes them."""
    s = np.ascontiguousarray(img, dtype=np.float32)
    h, w = s.shape
    x1 = np.minimum(np.arange(w) + 1, w - 1)
    y1 = np.minimum(np.arange(h) + 1, h - 1)
    sx, sy, sxy = s[:, x1], s[y1, :], s[y1][:, x1]
    half, quarter = np.float32(0.5), np.float32(0.25)
    d = np.empty((2 * h, 2 * w), dtype=np.float32)
    d[0::2, 0::2] = s
    d[0::2, 1::2] = half * (s + sx)
    d[1::2, 0::2] = half * (s + sy)
    d[1::2, 1::2] = quarter * ((s + sx) + (sy + sxy))
    assert d.dtype == np.float32
    return d


def up2_scalar(img):
    """The same, pixel by pixel with numpy float32 scalars: an independent statement for the handcrafted cases."""
    s = np.asarray(img, dtype=np.float32)
    h, w = s.shape
    d = np.zeros((2 * h, 2 * w), dtype=np.float32)
    f = np.float32
    for y in range(h):
        for x in range(w):
            xn, yn = min(x + 1, w - 1), min(y + 1, h - 1)
            d[2 * y, 2 * x] = s[y, x]
            d[2 * y, 2 * x + 1] = f(0.5) * f(s[y, x] + s[y, xn])
            d[2 * y + 1, 2 * x] = f(0.5) * f(s[y, x] + s[yn, x])
            d[2 * y + 1, 2 * x + 1] = f(0.25) * f(f(s[y, x] + s[y, xn]) + f(s[yn, x] + s[yn, xn]))
    return d


# ------------------------------------------------------------------------------------------------------------------
# without a GPU
# ------------------------------------------------------------------------------------------------------------------
def test_restatement_on_handcrafted_cases():
    one = up2(np.array([[7.25]], np.float32))
    np.testing.assert_array_equal(one, np.full((2, 2), 7.25, np.float32))
    row = np.array([[1.0, 2.0, 4.0, 8.0, 9.5]], np.float32)  # 1 x N: both output rows are the same
    want = np.array([1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0, 8.75, 9.5, 9.5], np.float32)
    np.testing.assert_array_equal(up2(row), np.stack([want, want]))
    np.testing.assert_array_equal(up2(row.T.copy()), np.stack([want, want]).T)  # N x 1
    two = np.array([[0.0, 4.0], [8.0, 20.0]], np.float32)
    np.testing.assert_array_equal(up2(two), np.array([[0, 2, 4, 4], [4, 8, 12, 12], [8, 14, 20, 20], [8, 14, 20, 20]],
                                                     np.float32))
    rng = np.random.default_rng(3)
    for h, w in ((5, 7), (3, 1), (1, 1), (4, 6)):  # odd sizes included
        img = (rng.random((h, w)) * 255).astype(np.float32)
        d = up2(img)
        assert d.shape == (2 * h, 2 * w)
        np.testing.assert_array_equal(d, up2_scalar(img))
        np.testing.assert_array_equal(d[0::2, 0::2], img)  # output pixel 2x sits on source pixel x
        # border replication: the last column / row repeats the one before it
        np.testing.assert_array_equal(d[:, -1], d[:, -2])
        np.testing.assert_array_equal(d[-1, :], d[-2, :])
    # the association matters in fp32: (a + b) + (c + d), not a + b + c + d
    a, b, c, e = np.float32(1e8), np.float32(1.0), np.float32(-1e8), np.float32(1.0)
    img = np.array([[a, b], [c, e]], np.float32)
    assert up2(img)[1, 1] == np.float32(0.25) * ((a + b) + (c + e))


def header_text(name="cusift_amd.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def test_header_library_and_binding_agree():
    from cusift_amd import capi

    text = header_text()
    flat = re.sub(r"\s+", " ", text)
    assert ("int cusift_scale_up(cusift_ctx *ctx, float *d_dst, int dst_pitch, size_t dst_stride, const float *d_src, "
            "int w, int h, int src_pitch, size_t src_stride, int n_images);") in flat
    assert hasattr(C.CDLL(capi.LIB_PATH), "cusift_scale_up")
    res, args = capi.SIGNATURES["cusift_scale_up"]
    assert res is C.c_int and args == [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                       C.c_size_t, C.c_int]
    assert callable(capi.Context.scale_up)
    # the new field is the struct's tail, in the header and in the binding, in the same order
    body = re.sub(r"/\*.*?\*/", "", text[text.index("typedef struct cusift_params {"):text.index("} cusift_params;")], flags=re.S)
    fields = re.findall(r"\b(?:int|float|double)\s+(\w+)\s*;", body)
    assert fields == [n for n, _ in capi.Params._fields_] and fields[-1] == "upsample" and fields[-2] == "concurrent_batches"
    assert capi.Params._fields_[-1] == ("upsample", C.c_int)
    assert capi.default_params().upsample == 0
    # the library itself writes the tail: a poisoned struct comes back with upsample == 0
    p = capi.Params()
    C.memset(C.byref(p), 0x55, C.sizeof(p))
    capi.lib().cusift_default_params(C.byref(p))
    assert p.upsample == 0 and p.concurrent_batches == 1 and p.root_sift == 0
    assert capi.default_params(upsample=1).upsample == 1
    # the header's own count of its entry points
    names = set(re.findall(r"\b(cusift_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    assert "cusift_scale_up" in names and len(names) <= 50
    assert "THIS FILE, %d)" % len(names) in text


def test_binding_rejects_bad_arguments_before_any_device_call():
    from cusift_amd import capi

    ctx = object.__new__(capi.Context)  # no device behind it: anything that reached the library would raise differently
    good = dict(d_dst=0x1000, dst_pitch=256, d_src=0x2000, w=100, h=50, src_pitch=128)
    assert capi.check_scale_up_args(**good) == (2 * 50 * 256, 50 * 128)
    bad = [
        dict(good, dst_pitch=199),            # dst_pitch < 2w
        dict(good, dst_pitch=0),
        dict(good, src_pitch=99),             # pitch < w
        dict(good, w=0),
        dict(good, h=0),
        dict(good, w=-3),
        dict(good, n_images=0),
        dict(good, n_images=70000),
        dict(good, d_dst=None),
        dict(good, d_src=0),
        dict(good, n_images=2, src_stride=50 * 128 - 1),
        dict(good, n_images=2, dst_stride=2 * 50 * 256 - 1),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            capi.check_scale_up_args(**kw)
        with pytest.raises(ValueError):
            capi.Context.scale_up(ctx, **kw)


def build_cpp():
    subprocess.check_call(["make", "-C", CPP, "all"], stdout=subprocess.DEVNULL)
    assert os.path.exists(BIN)


def test_cpp_header_compiles_with_plain_gxx_with_scale_up_used():
    if os.path.exists(BIN):
        os.remove(BIN)
    build_cpp()
    text = header_text("cuSIFT.h")
    assert "bool scaleUp;" in text and "scaleUp(false)" in text
    assert re.search(r"float subsampling = 1\.0f,\s*bool scaleUp = false\)", text)
    assert "p.upsample = scaleUp ? 1 : 0;" in text
    src = open(os.path.join(CPP, "upsample_dropin.cpp")).read()
    assert "1.0f, true)" in src and ".scaleUp = true" in src
    recipe = open(os.path.join(CPP, "Makefile")).read()
    assert "hipcc" not in recipe and "/opt/rocm" not in recipe


def test_kernel_has_no_scratch_and_16_byte_vector_stores():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_mix
    import kernel_regs

    asm = kernel_regs.assembly("sift_stencils.hip")
    ks = {k["name"]: k for k in kernel_regs.kernels(asm)}
    fast = next(v for n, v in ks.items() if "scale_up_fast_kernel" in n)
    generic = next(v for n, v in ks.items() if "scale_up_kernel" in n)
    for k in (fast, generic):
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
        assert k["group_segment_fixed_size"] == 0 and kernel_regs.waves_per_simd(k) == 8, k
    body = isa_mix.kernel_body(asm, "scale_up_fast_kernel")
    mnemonics = [line.split()[0] for line in body if line.startswith("\t") and line.split()]
    stores = [m for m in mnemonics if "store" in m]
    # both output rows of a source row: one 16-byte store each, and nothing narrower
    assert stores == ["buffer_store_dwordx4", "buffer_store_dwordx4"], stores
    assert any(m == "buffer_load_dwordx2" for m in mnemonics)
    assert sum(1 for line in body if "wave_shl:1" in line) >= 1  # the right neighbour comes from the next lane
    assert not [m for m in mnemonics if m.startswith(("scratch_", "ds_"))]
    # plain vector stores only: no scalar memory write of any kind (the prefixes are spelled in pieces on purpose)
    kinds = ("st" "ore", "buffer_" "st" "ore", "scratch_" "st" "ore", "at" "omic", "buffer_" "at" "omic", "dcache_" "wb")
    assert not [m for m in mnemonics if m.startswith(tuple("s_" + k for k in kinds))]
    # no multiply-add was formed from the formulas (the multipliers are powers of two, the file is built without contraction)
    assert not [m for m in mnemonics if m.startswith(("v_fma", "v_mad", "v_mac", "v_pk_fma"))]


# ------------------------------------------------------------------------------------------------------------------
# on the GPU
# ------------------------------------------------------------------------------------------------------------------
def rand_image(h, w, seed):
    rng = np.random.default_rng(seed)
    return (rng.random((h, w)) * 255.0).astype(np.float32)


def run_scale_up(ctx, imgs, src_pitch, offset_floats=0, src_stride=None, dst_stride=None):
    """imgs [n, h, w] -> [n, 2h, 2w] through cusift_scale_up, from a source laid out with the given pitch / stride /
    base offset; also checks that nothing outside the 2w x 2h images was written."""
    from cusift_amd import capi
    from cusift_amd.capi import DeviceBuffer

    n, h, w = imgs.shape
    src_stride = h * src_pitch if src_stride is None else src_stride
    dp = capi.ialign_up(2 * w, 128)
    dst_stride = 2 * h * dp if dst_stride is None else dst_stride
    src = np.full(offset_floats + n * src_stride + 8, -7.0, np.float32)
    for i in range(n):
        view = src[offset_floats + i * src_stride:offset_floats + i * src_stride + h * src_pitch].reshape(h, src_pitch)
        view[:, :w] = imgs[i]
    d_src = DeviceBuffer.from_numpy(ctx, src)
    sentinel = np.full(n * dst_stride, -3.0, np.float32)
    d_dst = DeviceBuffer.from_numpy(ctx, sentinel)
    ctx.scale_up(d_dst.ptr, dp, d_src.ptr + 4 * offset_floats, w, h, src_pitch, n_images=n, dst_stride=dst_stride,
                 src_stride=src_stride)
    ctx.synchronize()
    out = d_dst.to_numpy(np.float32, (n * dst_stride,))
    got = np.stack([out[i * dst_stride:i * dst_stride + 2 * h * dp].reshape(2 * h, dp) for i in range(n)])
    mask = np.ones(n * dst_stride, bool)
    for i in range(n):
        m = mask[i * dst_stride:i * dst_stride + 2 * h * dp].reshape(2 * h, dp)
        m[:, :2 * w] = False
    assert (out[mask] == -3.0).all(), "wrote outside the enlarged images"
    d_src.free()
    d_dst.free()
    return got[:, :, :2 * w]


SCALE_UP_CASES = {
    "640x480": dict(w=640, h=480),
    "1920x1080": dict(w=1920, h=1080),
    "641x479": dict(w=641, h=479),
    "127x3": dict(w=127, h=3),
    "1x1": dict(w=1, h=1),
    "pitch_not_128": dict(w=300, h=41, src_pitch=302),
    "pitch_odd": dict(w=300, h=41, src_pitch=301),
    "base_plus_4_bytes": dict(w=640, h=33, offset_floats=1),
    "batch_of_3_strided": dict(w=333, h=57, n=3, extra_stride=1000),
}


@pytest.mark.gpu
@pytest.mark.parametrize("generic", [0, 1])
@pytest.mark.parametrize("case", sorted(SCALE_UP_CASES))
def test_scale_up_bit_exact(case, generic):
    from cusift_amd import capi

    c = SCALE_UP_CASES[case]
    w, h, n = c["w"], c["h"], c.get("n", 1)
    pitch = c.get("src_pitch", capi.ialign_up(w, 128))
    imgs = np.stack([rand_image(h, w, 100 + i) for i in range(n)])
    src_stride = h * pitch + c.get("extra_stride", 0)
    dp = capi.ialign_up(2 * w, 128)
    dst_stride = 2 * h * dp + (4 * c["extra_stride"] if "extra_stride" in c else 0)
    with capi.Context(0) as ctx:
        ctx.set_policy(capi.POLICY_GENERIC_KERNELS, generic)
        got = run_scale_up(ctx, imgs, pitch, offset_floats=c.get("offset_floats", 0), src_stride=src_stride,
                           dst_stride=dst_stride)
    for i in range(n):
        want = up2(imgs[i])
        assert got[i].tobytes() == want.tobytes(), (case, i, int((got[i] != want).sum()))


@pytest.mark.gpu
def test_scale_up_refuses_bad_geometry(ctx):
    """The library's own checks (the binding's are bypassed): CUSIFT_ERR_INVALID, nothing enqueued."""
    from cusift_amd import capi
    from cusift_amd.capi import DeviceBuffer

    d = DeviceBuffer(ctx, 1 << 16)
    d.zero()
    L = capi.lib()
    for args in ((d.ptr, 127, 64 * 128, d.ptr, 64, 8, 128, 8 * 128, 1),   # dst_pitch < 2w
                 (d.ptr, 128, 64 * 128, d.ptr, 64, 8, 63, 8 * 128, 1),    # src_pitch < w
                 (d.ptr, 128, 64 * 128, d.ptr, 0, 8, 128, 8 * 128, 1),
                 (d.ptr, 128, 64 * 128, d.ptr, 64, 0, 128, 8 * 128, 1),
                 (d.ptr, 128, 64 * 128, d.ptr, 64, 8, 128, 8 * 128, 0),
                 (None, 128, 64 * 128, d.ptr, 64, 8, 128, 8 * 128, 1),
                 (d.ptr, 128, 16 * 128 - 1, d.ptr, 64, 8, 128, 8 * 128, 2)):
        assert L.cusift_scale_up(ctx.handle, *args) == -1, args
    ctx.synchronize()
    assert (d.to_numpy(np.float32, (1 << 14,)) == 0).all()
    d.free()


def compare_every_keypoint(want, got):
    """The project's every-keypoint bar: the same point set, header fields and orientation identical (NaN in the same
    places), every descriptor within 1e-4 L2.  No tolerated fraction."""
    assert len(want) == len(got), (len(want), len(got))
    a, b = canonical_order(want), canonical_order(got)
    for f in ("subsampling", "coords2D", "scale", "sharpness", "edgeness", "orientation"):
        np.testing.assert_array_equal(a[f], b[f], err_msg=f)
    fin = np.isfinite(a["data"]).all(axis=1)
    np.testing.assert_array_equal(np.isfinite(b["data"]).all(axis=1), fin)
    l2 = np.linalg.norm(a["data"][fin].astype(np.float64) - b["data"][fin].astype(np.float64), axis=1)
    print("descriptors: %d finite of %d, max L2 %.3e" % (int(fin.sum()), len(a), float(l2.max()) if len(l2) else 0.0))
    assert len(l2) == 0 or l2.max() < 1e-4, (float(l2.max()), int((l2 >= 1e-4).sum()))


def gpu_extract(ctx, img, **kw):
    from cusift_amd import capi
    from cusift_amd.capi import SIFT_POINT_DTYPE, DeviceBuffer

    prm = capi.default_params(**kw)
    d_pts = DeviceBuffer(ctx, prm.max_pts * 588)
    d_pts.zero()
    h_pts = np.zeros(prm.max_pts, dtype=SIFT_POINT_DTYPE)
    n = ctx.extract_host(img, prm, d_pts.ptr, h_pts)
    d_pts.free()
    return h_pts[:n].copy()


def oracle_upsampled(oracle, img, init_blur=0.0, subsampling=1.0, **kw):
    from cusift_amd.capi import SIFT_POINT_DTYPE

    kw.pop("root_sift", None)
    return oracle.extract(up2(img), init_blur=2.0 * init_blur, subsampling=0.5 * subsampling, **kw).view(SIFT_POINT_DTYPE)


EXTRACT_CASES = {
    # name: (image, params, the oracle's count as the issue states it or None)
    "gray1_0_0.1": ("gray1", dict(init_blur=0.0, peak_thresh=0.1, max_pts=65536), 41439),
    "gray1_0_1.0": ("gray1", dict(init_blur=0.0, peak_thresh=1.0, max_pts=8192), 1681),
    "gray1_0.5_3.0": ("gray1", dict(init_blur=0.5, peak_thresh=3.0, max_pts=4096), 384),
    "tile1080p_0.5": ("tile", dict(init_blur=0.5, peak_thresh=3.0, edge_thresh=10.0, max_pts=32768), None),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(EXTRACT_CASES))
def test_extract_upsample_equals_oracle_on_enlarged_image(ctx, oracle, gray1, case):
    from cusift_amd import synth

    which, kw, count = EXTRACT_CASES[case]
    img = gray1 if which == "gray1" else synth.tile(1000, 1920, 1080, preblur=0.5)
    kw = dict(kw, num_octaves=6)  # octaves -1 .. 4
    want = oracle_upsampled(oracle, img, **kw)
    print("%s: oracle %d points, %d at subsampling 0.5" % (case, len(want), int((want["subsampling"] == 0.5).sum())))
    assert len(want) < kw["max_pts"], (len(want), kw["max_pts"])  # nothing saturates
    if count is not None:
        assert len(want) == count
    assert (want["subsampling"] == 0.5).sum() > 0
    got = gpu_extract(ctx, img, upsample=1, **kw)
    print("%s: device %d points" % (case, len(got)))
    assert np.all(np.diff(got["subsampling"]) <= 0) and got["subsampling"][-1] == 0.5  # coarsest first, octave -1 last
    compare_every_keypoint(want, got)


@pytest.mark.gpu
def test_extract_upsample_root_sift(ctx, oracle, gray1):
    from cusift_amd.capi import SIFT_POINT_DTYPE

    kw = dict(num_octaves=6, init_blur=0.0, peak_thresh=1.0, max_pts=8192)
    want = oracle_upsampled(oracle, gray1, **kw).copy()
    assert len(want) == 1681 < kw["max_pts"]
    oracle.rootsift(want, len(want))
    got = gpu_extract(ctx, gray1, upsample=1, root_sift=1, **kw)
    compare_every_keypoint(want.view(SIFT_POINT_DTYPE), got)
    fin = np.isfinite(got["data"]).all(axis=1)
    np.testing.assert_allclose((got["data"][fin].astype(np.float64) ** 2).sum(axis=1), 1.0, atol=1e-5)


@pytest.mark.gpu
def test_extract_upsample_lowest_scale_skips_the_enlarged_octave(ctx, oracle, gray1):
    """lowest_scale = 1.0: octave -1 (2 * 0.5 = 1.0, not above it) is not searched, but it is still octave 0 of the plan --
    the other octaves come from it and their coordinates carry the 0.5."""
    kw = dict(num_octaves=6, init_blur=0.0, peak_thresh=1.0, max_pts=8192, lowest_scale=1.0)
    want = oracle_upsampled(oracle, gray1, **kw)
    assert 100 < len(want) < kw["max_pts"] and want["subsampling"].min() == 1.0
    got = gpu_extract(ctx, gray1, upsample=1, **kw)
    assert got["subsampling"].min() == 1.0
    compare_every_keypoint(want, got)


def sorted_records(pts):
    from cusift_amd import capi

    pts = np.ascontiguousarray(pts).copy()
    capi.sort_points(pts)
    return pts


def same_records(a, b):
    return len(a) == len(b) and all(np.array_equal(a[f], b[f], equal_nan=True) for f in FIELDS)


class Batch:
    """n frames on the device + output buffers, for the routes of one context."""

    def __init__(self, ctx, frames, max_pts):
        from cusift_amd import capi
        from cusift_amd.capi import DeviceBuffer

        self.ctx, self.n, (self.h, self.w) = ctx, len(frames), frames[0].shape
        self.p = capi.ialign_up(self.w, 128)
        self.max_pts = max_pts
        self.d_imgs = DeviceBuffer.from_numpy(ctx, np.stack([pitched(f) for f in frames]))
        self.d_pts = DeviceBuffer(ctx, self.n * max_pts * 588)
        self.d_cnt = DeviceBuffer(ctx, 4 * self.n)
        self.up_p = capi.ialign_up(2 * self.w, 128)
        self.d_up = DeviceBuffer(ctx, self.n * 2 * self.h * self.up_p * 4)

    def read(self):
        from cusift_amd.capi import SIFT_POINT_DTYPE

        self.ctx.synchronize()
        cnt = np.minimum(self.d_cnt.to_numpy(np.uint32, (self.n,)), self.max_pts)
        pts = self.d_pts.to_numpy(SIFT_POINT_DTYPE, (self.n, self.max_pts))
        return [sorted_records(pts[i, :cnt[i]]) for i in range(self.n)]

    def direct(self, prm):
        self.d_pts.zero()
        self.ctx.extract_batch(self.d_imgs.ptr, self.n, self.w, self.h, self.p, self.h * self.p, prm, self.d_pts.ptr,
                               self.d_cnt.ptr)
        return self.read()

    def staged(self, prm):
        """scale_up by hand, then the parent's code path on the enlarged image."""
        from cusift_amd import capi

        kw = {name: getattr(prm, name) for name, _ in capi.Params._fields_}
        kw.update(upsample=0, subsampling=prm.subsampling * 0.5, init_blur=2.0 * prm.init_blur)
        self.d_pts.zero()
        self.ctx.scale_up(self.d_up.ptr, self.up_p, self.d_imgs.ptr, self.w, self.h, self.p, n_images=self.n)
        self.ctx.extract_batch(self.d_up.ptr, self.n, 2 * self.w, 2 * self.h, self.up_p, 2 * self.h * self.up_p,
                               capi.default_params(**kw), self.d_pts.ptr, self.d_cnt.ptr)
        return self.read()

    def graph(self, prm, replays=2):
        g = self.ctx.record_graph(self.d_imgs.ptr, self.n, self.w, self.h, self.p, self.h * self.p, prm, self.d_pts.ptr,
                                  self.d_cnt.ptr)
        out = []
        for _ in range(replays):
            self.d_pts.zero()
            self.d_up.zero()
            g.launch()
            out.append(self.read())
        g.close()
        return out

    def free(self):
        for b in (self.d_imgs, self.d_pts, self.d_cnt, self.d_up):
            b.free()


def three_frames(gray1):
    return [gray1, np.roll(gray1, (13, 57), axis=(0, 1)), gray1[::-1, ::-1].copy()]


@pytest.mark.gpu
def test_entry_points_agree(gray1):
    """extract_batch(upsample=1) == scale_up + extract_batch(upsample=0, subsampling 0.5, init_blur doubled) == the graph
    replay == extract_host, as sorted records; the cusift_pipe_* route gives the same point sets."""
    from cusift_amd import capi

    frames = three_frames(gray1)
    kw = dict(num_octaves=6, init_blur=0.25, peak_thresh=1.0, max_pts=8192)
    prm = capi.default_params(upsample=1, **kw)
    with capi.Context(0) as ctx:
        b = Batch(ctx, frames, prm.max_pts)
        direct = b.direct(prm)
        assert all(500 < len(x) < prm.max_pts and x["subsampling"].min() == 0.5 for x in direct)
        staged = b.staged(prm)
        replays = b.graph(prm)
        b.free()
        for i in range(len(frames)):
            assert same_records(direct[i], staged[i]), i
            for r in replays:
                assert same_records(direct[i], r[i]), i
            host = sorted_records(gpu_extract(ctx, frames[i], upsample=1, **kw))
            assert same_records(direct[i], host), i
    # a context that reserved for the option first: the same records, and no growth of the arena by the call
    with capi.Context(0) as ctx:
        ctx.reserve(len(frames), gray1.shape[1], gray1.shape[0], prm)
        before = ctx.arena_bytes()
        plain = capi.default_params(**kw)
        with capi.Context(0) as other:
            other.reserve(len(frames), gray1.shape[1], gray1.shape[0], plain)
            assert before > other.arena_bytes()  # the enlarged images live in the arena
        b = Batch(ctx, frames, prm.max_pts)
        again = b.direct(prm)
        assert ctx.arena_bytes() == before
        b.free()
        assert all(same_records(x, y) for x, y in zip(direct, again))
    # host to host
    stack = np.ascontiguousarray(np.stack(frames), dtype=np.float32)
    with capi.Pipe(0, len(frames), gray1.shape[1], gray1.shape[0], prm, capi.PIPE_F32, depth=2) as pipe:
        def collect():
            rec, off = pipe.collect()
            assert len(off) == len(frames) + 1
            for i in range(len(frames)):
                assert same_records(direct[i], sorted_records(rec[off[i]:off[i + 1]])), i

        pipe.submit(stack)
        pipe.submit(stack)  # two batches in flight: the pipeline's extraction contexts alternate
        collect()
        pipe.submit(stack)
        collect()
        collect()


@pytest.mark.gpu
def test_launch_policies_do_not_change_the_records(gray1):
    from cusift_amd import capi

    frames = three_frames(gray1)
    kw = dict(num_octaves=6, init_blur=0.0, peak_thresh=1.0, max_pts=8192, upsample=1)
    with capi.Context(0) as ctx:
        b = Batch(ctx, frames, 8192)
        base = b.direct(capi.default_params(**kw))
        b.free()
    assert all(len(x) > 1000 for x in base)
    settings = [
        ({capi.POLICY_SIDE_STREAM: 3}, 1),
        ({capi.POLICY_OCTAVE_LISTS: 0}, 1),
        ({capi.POLICY_OCTAVE_LISTS: 1}, 1),
        ({capi.POLICY_PYRAMID_IN_DETECT: 0}, 1),
        ({capi.POLICY_PYRAMID_IN_DETECT: 2}, 1),
        ({capi.POLICY_PYRAMID_IN_DETECT: 2}, 4),
        ({}, 4),
        ({capi.POLICY_SIDE_STREAM: 3, capi.POLICY_OCTAVE_LISTS: 0}, 1),
        ({capi.POLICY_LAUNCH_PER_OCTAVE: 1, capi.POLICY_OCTAVE_LISTS: 1}, 1),
    ]
    for policy, concurrent in settings:
        with capi.Context(0) as ctx:
            for k, v in policy.items():
                ctx.set_policy(k, v)
            b = Batch(ctx, frames, 8192)
            got = b.direct(capi.default_params(concurrent_batches=concurrent, **kw))
            b.free()
        for i in range(len(frames)):
            assert same_records(base[i], got[i]), (policy, concurrent, i)
    # the per-octave stage sequence of the reference and the generic kernels too: the same points, descriptors within 1e-4
    for policy, extra in (({}, dict(fused_detect=0)), ({capi.POLICY_GENERIC_KERNELS: 1}, {})):
        with capi.Context(0) as ctx:
            for k, v in policy.items():
                ctx.set_policy(k, v)
            b = Batch(ctx, frames, 8192)
            got = b.direct(capi.default_params(**dict(kw, **extra)))
            b.free()
        for i in range(len(frames)):
            compare_every_keypoint(base[i], got[i])


@pytest.mark.gpu
def test_off_is_unchanged_and_tiling_refuses(gray1):
    from cusift_amd import capi

    frames = three_frames(gray1)
    kw = dict(num_octaves=5, init_blur=0.0, peak_thresh=1.0, max_pts=8192)
    untouched, off = capi.default_params(**kw), capi.default_params(upsample=0, **kw)
    assert bytes(untouched) == bytes(off)
    with capi.Context(0) as ctx:
        b = Batch(ctx, frames, 8192)
        first, second = b.direct(untouched), b.direct(off)
        b.free()
        for x, y in zip(first, second):
            assert x.tobytes() == y.tobytes() and x["subsampling"].min() == 1.0
        with pytest.raises(capi.CusiftError, match="upsample"):
            capi.Tiled(ctx, None, 0, 1, 640, 480, capi.default_params(upsample=1, **kw))
        t = capi.Tiled(ctx, None, 0, 1, 640, 480, off)  # and still accepts the option off
        t.close()


@pytest.mark.gpu
def test_cpp_program_reports_the_python_route_count(ctx, gray1):
    build_cpp()
    out = subprocess.run([BIN, PGM], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0 and "PASSED" in out.stdout, out.stdout + out.stderr
    m = re.search(r"scaleUp: (\d+) points, smallest subsampling (\S+),", out.stdout)
    got = gpu_extract(ctx, gray1, upsample=1, num_octaves=6, init_blur=0.0, peak_thresh=1.0, max_pts=8192)
    assert int(m.group(1)) == len(got) == 1681
    assert float(m.group(2)) == 0.5 == got["subsampling"].min()
