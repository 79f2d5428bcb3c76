"""Keep the K strongest keypoints per image, selected on the device: cusift_ctx_set_keep_strongest,
cusift_select_strongest (cusift_amd/csrc/sift_select.hip), SiftData::keepStrongest of include/cuSIFT.h.

The total order is restated here in numpy (`strongest`): larger key first (key = |sharpness| as its IEEE bit pattern, 0
when sharpness is not finite), then the coarser octave, then smaller y, x, scale.  The kept SET is a function of the image
alone, so every comparison below is every keypoint: the stage entry point against `strongest` on synthetic heads, the
drivers against `strongest` of the oracle's extraction and of their own unselected run, under every staged launch policy.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from cusift_amd import capi, synth
from cusift_amd.capi import SIFT_POINT_DTYPE, DeviceBuffer
from oracle_binding import Oracle, pitched
from parity_utils import canonical_order

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp_keep_strongest")
BIN = os.path.join(CPP, "keep_strongest_dropin")
GRAY1 = os.path.join(ROOT, "tests", "golden", "gray1.pgm")

# a staged keypoint: the first 16 floats of a SiftPoint
HEAD_DTYPE = np.dtype([(n, SIFT_POINT_DTYPE.fields[n][0]) for n in SIFT_POINT_DTYPE.names[:SIFT_POINT_DTYPE.names.index("data")]])
assert HEAD_DTYPE.itemsize == 64
WRITTEN = ("coords2D", "scale", "sharpness", "edgeness", "orientation", "subsampling", "data")
UNTOUCHED = ("score", "ambiguity", "match", "match_xpos", "match_ypos", "match_error", "empty", "coords3D")


# ------------------------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------------------------
def strength_key(sharpness):
    s = np.ascontiguousarray(sharpness, dtype=np.float32)
    bits = s.view(np.uint32) & np.uint32(0x7FFFFFFF)
    return np.where(np.isfinite(s), bits, np.uint32(0)).astype(np.int64)


def strongest_order(records):
    """Indices of `records` (anything with coords2D, scale, sharpness, subsampling) in the total order, strongest first."""
    xy = records["coords2D"].astype(np.float64)
    return np.lexsort((records["scale"].astype(np.float64), xy[:, 0], xy[:, 1], -records["subsampling"].astype(np.float64),
                       -strength_key(records["sharpness"])))


def strongest(records, k):
    return records[strongest_order(records)[:k]]


def heads(rows):
    """rows of (x, y, scale, sharpness, subsampling) -> HEAD_DTYPE array; edgeness numbers the rows."""
    out = np.zeros(len(rows), dtype=HEAD_DTYPE)
    for i, (x, y, scale, sharp, sub) in enumerate(rows):
        out[i]["coords2D"] = (x, y)
        out[i]["scale"], out[i]["sharpness"], out[i]["subsampling"], out[i]["edgeness"] = scale, sharp, sub, i
    return out


def kept_ids(records, k):
    return [int(e) for e in strongest(records, k)["edgeness"]]


def test_restatement_on_handcrafted_cases():
    # strength alone, by magnitude, sign ignored
    r = heads([(1, 1, 1, 0.5, 1), (2, 2, 1, -3.0, 1), (3, 3, 1, 2.0, 1), (4, 4, 1, -0.25, 1)])
    assert kept_ids(r, 4) == [1, 2, 0, 3] and kept_ids(r, 1) == [1] and kept_ids(r, 2) == [1, 2]
    assert kept_ids(r, 9) == [1, 2, 0, 3]  # K >= count: everything, still in order
    # ties on strength inside an octave: smaller y, then smaller x, then smaller scale
    r = heads([(5, 9, 1, 2.0, 1), (7, 3, 1, -2.0, 1), (2, 3, 2, 2.0, 1), (2, 3, 1.5, 2.0, 1), (0, 0, 1, 1.0, 1)])
    assert kept_ids(r, 5) == [3, 2, 1, 0, 4]
    # ties across octaves: the coarser octave (larger subsampling) wins whatever its position
    r = heads([(0, 0, 1, 2.0, 1), (99, 99, 9, 2.0, 4), (50, 50, 1, 2.0, 2), (1, 1, 1, 2.5, 0.5)])
    assert kept_ids(r, 4) == [3, 1, 2, 0]
    # a NaN, an inf and a -inf rank last (key 0), among themselves by the secondary order; 0.0 ties with them
    r = heads([(3, 3, 1, np.nan, 1), (2, 2, 1, np.inf, 1), (1, 1, 1, 1e-30, 1), (0, 0, 1, -np.inf, 2), (9, 0, 1, 0.0, 1)])
    assert kept_ids(r, 5) == [2, 3, 4, 1, 0] and kept_ids(r, 1) == [2]
    # the key is the bit pattern: denormals order like everything else
    r = heads([(0, 0, 1, 1e-45, 1), (0, 1, 1, 3e-45, 1), (0, 2, 1, 0.0, 1)])
    assert kept_ids(r, 3) == [1, 0, 2]
    assert len(strongest(r[:0], 3)) == 0


# ------------------------------------------------------------------------------------------------------------------
# surface, without a GPU
# ------------------------------------------------------------------------------------------------------------------
def header_text(name):
    return open(os.path.join(ROOT, "include", name)).read()


def test_headers_library_and_binding_agree():
    core, extras = header_text("cusift_amd.h"), header_text("cusift_amd_extras.h")
    assert "int cusift_ctx_set_keep_strongest(cusift_ctx *ctx, int k);" in re.sub(r"\s+", " ", core)
    assert ("int cusift_select_strongest(cusift_ctx *ctx, void *d_heads, int n_lists, int n_images, int capacity, "
            "unsigned int *d_counts, int keep, unsigned int *d_kept);") in re.sub(r"\s+", " ", extras)
    handle = C.CDLL(capi.LIB_PATH)
    assert hasattr(handle, "cusift_ctx_set_keep_strongest") and hasattr(handle, "cusift_select_strongest")
    assert capi.SIGNATURES["cusift_ctx_set_keep_strongest"] == (C.c_int, [C.c_void_p, C.c_int])
    assert capi.SIGNATURES["cusift_select_strongest"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                                                    C.c_void_p, C.c_int, C.c_void_p])
    assert callable(capi.Context.set_keep_strongest) and callable(capi.Context.select_strongest)
    # the core header's own count of its entry points
    names = set(re.findall(r"\b(cusift_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", core, flags=re.S)))
    assert len(names) == 48 and "THIS FILE, 48)" in core
    # cusift_params is what it was: the setting is the context's, not a field
    body = re.sub(r"/\*.*?\*/", "", core[core.index("typedef struct cusift_params {"):core.index("} cusift_params;")], flags=re.S)
    fields = re.findall(r"\b(?:int|float|double)\s+(\w+)\s*;", body)
    assert fields == [n for n, _ in capi.Params._fields_] and fields[-1] == "upsample" and len(fields) == 12
    # the header states when the result is defined
    assert "candidates beyond max_pts in one octave are lost" in re.sub(r"\s+\*?\s*", " ", core)
    import inspect
    from cusift_amd import batch
    assert "keep_strongest" in inspect.signature(batch.BatchExtractor.__init__).parameters


def test_binding_rejects_bad_arguments_before_any_device_call():
    ctx = object.__new__(capi.Context)  # no device behind it: anything that reached the library would raise differently
    assert capi.check_keep_strongest(0) == 0 and capi.check_keep_strongest(np.int32(7), 7) == 7
    for bad in (-1, 1.5, "3", None, True, 1 << 31):
        with pytest.raises(ValueError):
            capi.check_keep_strongest(bad)
        with pytest.raises(ValueError):
            capi.Context.set_keep_strongest(ctx, bad)
    with pytest.raises(ValueError):
        capi.check_keep_strongest(1025, 1024)
    good = dict(d_heads=0x1000, n_lists=3, n_images=5, capacity=100, d_counts=0x2000, keep=7, d_kept=0x3000)
    capi.check_select_strongest_args(**good)
    for kw in (dict(good, d_heads=None), dict(good, d_counts=0), dict(good, d_kept=None), dict(good, n_lists=0),
               dict(good, n_lists=17), dict(good, n_images=0), dict(good, n_images=65536), dict(good, capacity=0),
               dict(good, keep=0), dict(good, keep=-2), dict(good, n_lists=16, capacity=1 << 28)):
        with pytest.raises(ValueError):
            capi.check_select_strongest_args(**kw)
        with pytest.raises(ValueError):
            capi.Context.select_strongest(ctx, **kw)


def test_cpp_header_compiles_with_plain_gxx_with_keep_strongest_used():
    if os.path.exists(BIN):
        os.remove(BIN)
    subprocess.check_call(["make", "-C", CPP, "all"], stdout=subprocess.DEVNULL)
    assert os.path.exists(BIN)
    text = header_text("cuSIFT.h")
    assert "int keepStrongest;" in text and "keepStrongest(0)" in text
    assert re.search(r"bool scaleUp,\s*int keepStrongest\)", text)
    assert "cusift_ctx_set_keep_strongest(cusift_dropin::ctx(), keepStrongest)" in text
    src = open(os.path.join(CPP, "keep_strongest_dropin.cpp")).read()
    assert "1.0f, false, K)" in src and ".keepStrongest = K" in src
    recipe = open(os.path.join(CPP, "Makefile")).read()
    assert "hipcc" not in recipe and "/opt/rocm" not in recipe


# ------------------------------------------------------------------------------------------------------------------
# the expected sets: the oracle's extraction with ample max_pts, then `strongest`
# ------------------------------------------------------------------------------------------------------------------
def tie_image():
    """A 64 x 64 block of the fixture repeated 6 x 6: the keypoints of the inner blocks repeat with bit-equal sharpness."""
    g = synth.tile(4000, 640, 480, 0.0)
    return np.tile(g[100:164, 200:264], (6, 6)).copy()


# name -> (images, extraction parameters, the K of the GPU tests)
CASES = {
    "gray1": (lambda: [synth.fixture_image()], dict(num_octaves=6, init_blur=0.0, peak_thresh=0.1, max_pts=16384),
              (1, 100, 4096, 9507, 9508, 16384)),
    "333x257": (lambda: [synth.tile(4000, 333, 257, 0.0)], dict(num_octaves=6, init_blur=0.0, peak_thresh=0.5, max_pts=4096), (97,)),
    "128x96": (lambda: [synth.tile(4001, 128, 96, 0.5)], dict(num_octaves=3, init_blur=0.5, peak_thresh=0.2, max_pts=1024), (100,)),
    "batch": (lambda: [synth.tile(4000 + i, 320, 240, 1.0) for i in range(3)],
              dict(num_octaves=5, init_blur=1.0, peak_thresh=1.0, max_pts=4096), (150,)),
    "ties": (lambda: [tie_image()], dict(num_octaves=3, init_blur=0.0, peak_thresh=1.0, max_pts=8192), None),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(images, params dict, per image the oracle's records) -- computed once, shared, never written."""
    make, prm, _ = CASES[name]
    imgs = make()
    ora = Oracle()
    want = [ora.extract(i, **prm).view(SIFT_POINT_DTYPE).copy() for i in imgs]
    for w in want:
        w.setflags(write=False)
    return imgs, prm, want


def tie_cut(records):
    """A K that cuts a group of bit-equal sharpness: the first such cut past the 40 strongest."""
    key = strength_key(records["sharpness"])[strongest_order(records)]
    for k in range(40, len(key)):
        if key[k - 1] == key[k]:
            return k
    return None


def test_expected_sets_and_their_preconditions():
    for name, (_, prm, ks) in CASES.items():
        imgs, prm, want = case(name)
        for w in want:
            assert len(w) > 20, name
            # no octave reaches max_pts, so the lists hold every keypoint and the result is defined
            for sub in np.unique(w["subsampling"]):
                assert (w["subsampling"] == sub).sum() < prm["max_pts"], (name, sub)
            assert len(w) < prm["max_pts"]
        if name == "gray1":
            assert len(want[0]) == 9508
            assert [k for k in ks if k < 9508] == [1, 100, 4096, 9507]  # these cut; 9508 and 16384 keep everything
        elif ks:
            assert all(k < len(w) for k in ks for w in want), name  # every K actually cuts the list
    # the tie case: a group of bit-equal sharpness straddles the cut, and the cut is decided by the secondary order
    w = case("ties")[2][0]
    k = tie_cut(w)
    assert k is not None and k < len(w)
    order = strongest_order(w)
    key = strength_key(w["sharpness"])
    assert key[order[k - 1]] == key[order[k]]
    group = w[key == key[order[k]]]
    assert len(group) >= 2 and len(np.unique(group["coords2D"], axis=0)) == len(group)


# ------------------------------------------------------------------------------------------------------------------
# on the GPU
# ------------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu

MODES = {"fork": (3, 0), "lists": (0, 1), "lists, a launch per octave": (0, 1, True), "fork+lists": (3, 1),
         "pyramid in the detections": (0, 1, False, 2), "pyramid in octave 0's detection": (0, 1, False, 1),
         "pyramid in octave 0's detection, a launch per octave": (0, 1, True, 1)}


def context_with(overlap=0, stage_all=None, no_multi=False, pyramid=None, keep=0):
    c = capi.Context(0)
    c.set_policy(capi.POLICY_SIDE_STREAM, overlap)
    if stage_all is not None:
        c.set_policy(capi.POLICY_OCTAVE_LISTS, stage_all)
    if no_multi:
        c.set_policy(capi.POLICY_LAUNCH_PER_OCTAVE, 1)
    if pyramid is not None:
        c.set_policy(capi.POLICY_PYRAMID_IN_DETECT, pyramid)
    if keep:
        c.set_keep_strongest(keep)
    return c


@pytest.fixture
def kctx():
    """A context of this module's own (the setting is sticky: the session's shared context is never given one)."""
    c = capi.Context(0)
    yield c
    c.close()


def run_batch(ctx, imgs, prm, fill=0x5A):
    n = len(imgs)
    h, w = imgs[0].shape
    stack = np.stack([pitched(i) for i in imgs])
    p = stack.shape[2]
    d_imgs = DeviceBuffer.from_numpy(ctx, stack)
    d_pts = DeviceBuffer(ctx, n * prm.max_pts * 588)
    ctx.memset(d_pts.ptr, fill, n * prm.max_pts * 588)
    d_cnt = DeviceBuffer(ctx, 4 * n)
    try:
        ctx.extract_batch(d_imgs.ptr, n, w, h, p, h * p, prm, d_pts.ptr, d_cnt.ptr)
        ctx.synchronize()
        cnt = d_cnt.to_numpy(np.uint32, (n,)).copy()
        pts = d_pts.to_numpy(SIFT_POINT_DTYPE, (n, prm.max_pts)).copy()
    finally:
        for b in (d_imgs, d_pts, d_cnt):
            b.free()
    return cnt, pts


def assert_same_bits(got, want, fields=WRITTEN):
    assert len(got) == len(want), (len(got), len(want))
    a, b = canonical_order(got), canonical_order(want)
    for f in fields:
        assert np.ascontiguousarray(a[f]).tobytes() == np.ascontiguousarray(b[f]).tobytes(), f


def assert_matches_oracle(got, want):
    """The project's bar against the oracle: head fields and orientation bit for bit, descriptors < 1e-4 L2, every keypoint."""
    assert_same_bits(got, want, ("subsampling", "coords2D", "scale", "sharpness", "edgeness", "orientation"))
    a, b = canonical_order(got), canonical_order(want)
    fin = np.isfinite(b["data"]).all(axis=1)
    np.testing.assert_array_equal(np.isfinite(a["data"]).all(axis=1), fin)
    if fin.any():
        l2 = np.linalg.norm(a["data"][fin].astype(np.float64) - b["data"][fin].astype(np.float64), axis=1)
        assert l2.max() < 1e-4, (l2.max(), int((l2 >= 1e-4).sum()))


def assert_layout(cnt, pts, k, held):
    """Coarsest octave first, the counter is the kept count, nothing but the written fields and the kept records touched."""
    assert int(cnt) == min(k, held)
    got = pts[: int(cnt)]
    assert np.all(np.diff(got["subsampling"]) <= 0)
    for f in UNTOUCHED:
        assert np.all(np.ascontiguousarray(got[f]).view(np.uint8) == 0x5A), f
    assert np.all(pts[int(cnt):].view(np.uint8) == 0x5A)


# ---- the stage entry point on synthetic heads ----
CAPACITY = 2100  # more than two 1024-head passes of a workgroup
SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, CAPACITY)


def synthetic_heads(rng, n, levels=37, sub=1.0, nonfinite=False):
    """n heads with sharpness from a few values (ties everywhere), distinct positions, numbered in edgeness."""
    out = np.zeros(n, dtype=HEAD_DTYPE)
    sharp = rng.integers(0, levels, n).astype(np.float32) * np.float32(0.37) * rng.choice(np.float32([-1, 1]), n)
    if nonfinite:
        sharp[rng.random(n) < 0.2] = np.nan
        sharp[rng.random(n) < 0.1] = np.inf
        sharp[rng.random(n) < 0.1] = -np.inf
    out["sharpness"] = sharp
    pos = rng.permutation(4 * max(n, 1))[:n]  # distinct (y, x)
    out["coords2D"][:, 1] = (pos // 64).astype(np.float32) * np.float32(0.5)
    out["coords2D"][:, 0] = (pos % 64).astype(np.float32) * np.float32(1.25)
    out["scale"] = rng.random(n).astype(np.float32) + np.float32(1.0)
    out["subsampling"] = sub
    out["edgeness"] = rng.random(n).astype(np.float32)
    out["orientation"] = np.arange(n, dtype=np.float32)
    return out


def run_select(ctx, lists, keep, capacity=CAPACITY, counts=None):
    """lists[r][i]: HEAD_DTYPE arrays.  Returns (lists after the call, up to their new counts; new counts; kept totals)."""
    n_lists, n_images = len(lists), len(lists[0])
    buf = np.full((n_lists, n_images, capacity), 0, dtype=HEAD_DTYPE)
    buf.view(np.uint8)[:] = 0xA5
    cnt = np.zeros((n_lists, n_images), dtype=np.uint32)
    for r in range(n_lists):
        for i in range(n_images):
            buf[r, i, : len(lists[r][i])] = lists[r][i]
            cnt[r, i] = len(lists[r][i])
    if counts is not None:
        cnt = np.asarray(counts, dtype=np.uint32).reshape(n_lists, n_images)
    d_heads, d_cnt = DeviceBuffer.from_numpy(ctx, buf), DeviceBuffer.from_numpy(ctx, cnt)
    d_kept = DeviceBuffer(ctx, 4 * n_images)
    ctx.memset(d_kept.ptr, 0xEE, 4 * n_images)
    try:
        ctx.select_strongest(d_heads.ptr, n_lists, n_images, capacity, d_cnt.ptr, keep, d_kept.ptr)
        ctx.synchronize()
        out = d_heads.to_numpy(HEAD_DTYPE, (n_lists, n_images, capacity)).copy()
        new = d_cnt.to_numpy(np.uint32, (n_lists, n_images)).copy()
        kept = d_kept.to_numpy(np.uint32, (n_images,)).copy()
    finally:
        for b in (d_heads, d_cnt, d_kept):
            b.free()
    return out, new, kept


def check_select(ctx, lists, keep, capacity=CAPACITY, counts=None):
    n_lists, n_images = len(lists), len(lists[0])
    out, new, kept = run_select(ctx, lists, keep, capacity, counts)
    for i in range(n_images):
        held = np.concatenate([lists[r][i][:capacity] for r in range(n_lists)])
        want = strongest(held, keep)
        assert kept[i] == min(keep, len(held)) == len(want), (i, kept[i], keep, len(held))
        for r in range(n_lists):
            # list r keeps exactly its members of the expected set, bit for bit, compacted to its head
            mine = want[want["subsampling"] == lists[r][i]["subsampling"][0]] if len(lists[r][i]) else want[:0]
            assert new[r, i] == len(mine), (r, i, new[r, i], len(mine))
            got = out[r, i, : new[r, i]]
            assert sorted(g.tobytes() for g in got) == sorted(m.tobytes() for m in mine), (r, i)


def keeps_for(count):
    return sorted({k for k in (1, count - 1, count, count + 1, CAPACITY) if k >= 1})


@gpu
def test_select_one_list_one_image(kctx):
    rng = np.random.default_rng(11)
    for n in SIZES:
        lst = synthetic_heads(rng, n)
        for keep in keeps_for(n):
            check_select(kctx, [[lst]], keep)


@gpu
def test_select_three_lists_five_images(kctx):
    """Every list size in every list position; the octave of a list is its subsampling (4, 2, 1: coarsest first)."""
    rng = np.random.default_rng(12)
    for shift in range(0, len(SIZES), 2):
        lists = [[synthetic_heads(rng, SIZES[(shift + 5 * r + i) % len(SIZES)], sub=4.0 / (1 << r)) for i in range(5)]
                 for r in range(3)]
        count0 = sum(len(lists[r][0]) for r in range(3))
        for keep in keeps_for(count0) + [700]:
            check_select(kctx, lists, keep)


@gpu
@pytest.mark.parametrize("n_lists,n_images", [(1, 1), (3, 5)])
def test_select_ties_nonfinite_and_overflowing_counts(kctx, n_lists, n_images):
    rng = np.random.default_rng(13)
    subs = [4.0 / (1 << r) for r in range(n_lists)]

    def make(n, **kw):
        return [[synthetic_heads(rng, n, sub=subs[r], **kw) for _ in range(n_images)] for r in range(n_lists)]

    # keys that are all equal: the secondary order decides everything
    lists = make(1025, levels=1)
    for keep in (1, 64, 1024, 1025, 1026, 1025 * n_lists - 1, CAPACITY):
        check_select(kctx, lists, keep)
    lists = make(CAPACITY, levels=1)
    check_select(kctx, lists, CAPACITY - 1)
    # two tie groups around the cut: 300 heads of one strength, 300 of the next, the cut inside either and between them
    lists = make(600, levels=1)
    for r in range(n_lists):
        for i in range(n_images):
            lists[r][i]["sharpness"][:300] = 2.0
            lists[r][i]["sharpness"][300:] = -1.0
    for keep in (299 * n_lists, 300 * n_lists, 300 * n_lists + 1, 450 * n_lists, 600 * n_lists - 1):
        check_select(kctx, lists, keep)
    # non-finite sharpness ranks last, with key 0
    lists = make(700, nonfinite=True)
    for keep in (1, 350, 650 * n_lists, 700 * n_lists - 1):
        check_select(kctx, lists, keep)
    # a count above the capacity (the detection kept counting): clamped by the call
    lists = make(CAPACITY)
    over = np.full((n_lists, n_images), CAPACITY + 1000, dtype=np.uint32)
    check_select(kctx, lists, 1500, counts=over)
    check_select(kctx, lists, CAPACITY * n_lists, counts=over)


@gpu
def test_select_interchangeable_heads_fill_the_cut(kctx):
    """Heads equal in all five words of the order straddle the cut: as many are kept as the cut has room for, each one an
    input head, none twice (they differ in edgeness, which the order does not look at)."""
    rng = np.random.default_rng(14)
    lst = synthetic_heads(rng, 500)
    for f in ("coords2D", "scale", "sharpness"):
        lst[f][100:400] = lst[f][100]
    lst["sharpness"][100:400] = 5.0
    lst["sharpness"][:100] = 9.0
    lst["sharpness"][400:] = 1.0
    lst["edgeness"] = np.arange(500, dtype=np.float32)
    for keep in (101, 250, 399, 400, 450):
        out, new, kept = run_select(kctx, [[lst]], keep)
        assert new[0, 0] == keep == kept[0]
        ids = sorted(int(e) for e in out[0, 0, :keep]["edgeness"])
        assert len(set(ids)) == keep and ids[:100] == list(range(100))
        assert all(out[0, 0, j].tobytes() == lst[int(out[0, 0, j]["edgeness"])].tobytes() for j in range(keep))
        assert sum(100 <= e < 400 for e in ids) == min(keep - 100, 300) and sum(e >= 400 for e in ids) == max(0, keep - 400)


# ---- end to end against the oracle ----
def check_against_oracle(ctx, name, ks):
    imgs, prm_kw, want = case(name)
    prm = capi.default_params(**prm_kw)
    for k in ks:
        ctx.set_keep_strongest(k)
        cnt, pts = run_batch(ctx, imgs, prm)
        for i in range(len(imgs)):
            assert_layout(cnt[i], pts[i], k, len(want[i]))
            assert_matches_oracle(pts[i, : cnt[i]], strongest(want[i], k))


@gpu
@pytest.mark.parametrize("k", CASES["gray1"][2])
def test_fixture_keeps_the_oracles_strongest(kctx, k):
    check_against_oracle(kctx, "gray1", (k,))


@gpu
@pytest.mark.parametrize("name", ["333x257", "128x96", "batch"])
def test_small_images_and_a_batch_keep_the_oracles_strongest(kctx, name):
    check_against_oracle(kctx, name, CASES[name][2])


@gpu
def test_one_octave_and_unsearched_octaves(kctx):
    """One octave takes a list of its own under the setting; octaves below lowest_scale leave empty lists."""
    img = synth.tile(4002, 320, 240, 1.0)
    ora = Oracle()
    for kw in (dict(num_octaves=1, peak_thresh=2.0), dict(num_octaves=4, lowest_scale=2.0, peak_thresh=0.5)):
        base = dict(init_blur=1.0, max_pts=4096)
        base.update(kw)
        want = ora.extract(img, **base).view(SIFT_POINT_DTYPE)
        k = len(want) // 3
        assert k >= 5
        kctx.set_keep_strongest(k)
        cnt, pts = run_batch(kctx, [img], capi.default_params(**base))
        assert_layout(cnt[0], pts[0], k, len(want))
        assert_matches_oracle(pts[0, : cnt[0]], strongest(want, k))


# ---- against its own unselected run, under every staged launch policy ----
@gpu
@pytest.mark.parametrize("mode", sorted(MODES))
def test_every_launch_policy_keeps_the_same_records(mode):
    imgs, prm_kw, _ = case("batch")
    prm = capi.default_params(**prm_kw)
    with context_with(0, 0) as plain:
        cnt_all, pts_all = run_batch(plain, imgs, prm)
    k = 150
    with context_with(*MODES[mode], keep=k) as c:
        cnt, pts = run_batch(c, imgs, prm)
        assert c.forks() == (1 if "fork" in mode else 0)
    for i in range(len(imgs)):
        assert_layout(cnt[i], pts[i], k, int(cnt_all[i]))
        assert_same_bits(pts[i, : cnt[i]], strongest(pts_all[i, : cnt_all[i]], k))


# ---- the tie image ----
@gpu
def test_a_cut_through_equal_strengths_is_decided_by_position():
    imgs, prm_kw, want = case("ties")
    prm = capi.default_params(**prm_kw)
    k = tie_cut(want[0])
    expected = strongest(want[0], k)
    sets = []
    for mode in ("lists", "fork+lists"):
        with context_with(*MODES[mode], keep=k) as c:
            for _ in range(2):
                cnt, pts = run_batch(c, imgs, prm)
                assert cnt[0] == k
                assert_matches_oracle(pts[0, :k], expected)
                sets.append(canonical_order(pts[0, :k]))
    for s in sets[1:]:
        assert_same_bits(s, sets[0])


# ---- an input with far more keypoints than K ----
@gpu
def test_two_runs_keep_the_same_set():
    imgs = [synth.tile(4100 + i, 640, 480, 0.0) for i in range(2)]
    prm = capi.default_params(num_octaves=5, init_blur=0.0, peak_thresh=0.5, max_pts=16384)
    runs = []
    for policy in ((0, None), (3, 1), (0, None)):
        with context_with(*policy, keep=1024) as c:
            cnt, pts = run_batch(c, imgs, prm)
            assert list(cnt) == [1024, 1024]
            runs.append([canonical_order(pts[i, :1024]) for i in range(2)])
    for r in runs[1:]:
        for i in range(2):
            assert_same_bits(r[i], runs[0][i])
            assert strength_key(r[i]["sharpness"]).min() > 0


# ---- other paths ----
@gpu
def test_graph_replay_host_entry_point_and_reset(kctx):
    imgs, prm_kw, want = case("128x96")
    img = imgs[0]
    prm = capi.default_params(**prm_kw)
    k = 100
    expected = strongest(want[0], k)
    kctx.set_keep_strongest(k)
    cnt, pts = run_batch(kctx, [img], prm)
    eager = pts[0, : cnt[0]]
    # cusift_extract_host
    d_pts = DeviceBuffer(kctx, prm.max_pts * 588)
    h_pts = np.zeros(prm.max_pts, dtype=SIFT_POINT_DTYPE)
    n = kctx.extract_host(img, prm, d_pts.ptr, h_pts)
    assert n == k
    assert_same_bits(h_pts[:n], eager)
    assert_matches_oracle(h_pts[:n], expected)
    # a recorded graph uses the setting at recording time, whatever it is at replay
    src = pitched(img)
    h, w = img.shape
    p = src.shape[1]
    d_img = DeviceBuffer.from_numpy(kctx, src)
    d_cnt = DeviceBuffer(kctx, 4)
    g = kctx.record_graph(d_img.ptr, 1, w, h, p, h * p, prm, d_pts.ptr, d_cnt.ptr)
    kctx.set_keep_strongest(0)
    for _ in range(2):
        kctx.memset(d_pts.ptr, 0x5A, prm.max_pts * 588)
        g.launch()
        kctx.synchronize()
        n = int(d_cnt.to_numpy(np.uint32, (1,))[0])
        rec = d_pts.to_numpy(SIFT_POINT_DTYPE, (prm.max_pts,)).copy()
        assert_layout(n, rec, k, len(want[0]))
        assert_same_bits(rec[:n], eager)
    g.close()
    for b in (d_img, d_pts, d_cnt):
        b.free()
    # K set and reset to 0: the bits of a context that never had it
    cnt0, pts0 = run_batch(kctx, [img], prm)
    with capi.Context(0) as fresh:
        cnt1, pts1 = run_batch(fresh, [img], prm)
    assert cnt0[0] == cnt1[0] == len(want[0])
    assert canonical_order(pts0[0, : cnt0[0]]).tobytes() == canonical_order(pts1[0, : cnt1[0]]).tobytes()
    assert np.all(pts0[0, cnt0[0]:].view(np.uint8) == 0x5A)


@gpu
def test_what_cannot_be_selected_is_refused(kctx):
    imgs, kw, want = case("128x96")
    img = imgs[0]
    assert kw["max_pts"] == 1024 and len(want[0]) > 100  # K = 100 below cuts the list

    def refused(ctx, prm, word):
        with pytest.raises(capi.CusiftError) as e:
            run_batch(ctx, [img], prm)
        assert "cusift error -1:" in str(e.value) and word in str(e.value), str(e.value)

    kctx.set_keep_strongest(1025)
    refused(kctx, capi.default_params(**kw), "max_pts")
    with pytest.raises(capi.CusiftError) as e:  # K < 0, straight at the library
        capi.check(capi.lib().cusift_ctx_set_keep_strongest(kctx.handle, -1))
    assert "cusift error -1:" in str(e.value)
    kctx.set_keep_strongest(100)
    refused(kctx, capi.default_params(fused_detect=0, **kw), "fused_detect")
    kctx.set_policy(capi.POLICY_GENERIC_KERNELS, 1)
    refused(kctx, capi.default_params(**kw), "GENERIC_KERNELS")
    kctx.set_policy(capi.POLICY_GENERIC_KERNELS, 0)
    with pytest.raises(capi.CusiftError) as e:  # the tiled path
        capi.Tiled(kctx, None, 0, 1, 256, 768, capi.default_params(**kw))
    assert "cusift error -1:" in str(e.value) and "keep_strongest" in str(e.value)
    # ... and the setting still works afterwards
    cnt, _ = run_batch(kctx, [img], capi.default_params(**kw))
    assert cnt[0] == 100


@gpu
def test_cpp_dropin_keeps_the_strongest():
    subprocess.check_call(["make", "-C", CPP, "all"], stdout=subprocess.DEVNULL)
    out = subprocess.run([BIN, GRAY1], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "PASSED" in out.stdout, out.stdout + out.stderr
    m = re.search(r"kept (\d+) of (\d+): weakest kept (\S+), strongest dropped (\S+)", out.stdout)
    assert m and int(m.group(1)) == 500 and int(m.group(2)) > 500 and float(m.group(3)) >= float(m.group(4))
