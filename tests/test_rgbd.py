"""RGB-D pair registration on the device (cusift_amd/csrc/sift_rgbd.hip + the device-side point count of sift_rigid.hip):
cusift_lift_depth, cusift_select_matches, cusift_register_rgbd, include/rgbd.h.

The yardstick is the reference's own fixture chain for its (commented-out) RANSACTestImage, test/test.cpp:136-184:
the VLFeat keypoints of frames 1 and 2 (vlfeat_sift1/2.bin), their depth images (rgbd_depth.npz: the raw 16-bit samples
of depth1/2.png), INTRINSICS (rgbd_intrinsics.txt), MATLAB's matches with their 3-D points (match_indices1_2.bin,
rgbd_match1_2.bin) and MATLAB's Rt (rgbd_Rt1_2.bin) -- and a float32 numpy restatement of the lift written in this file,
which the non-GPU tests pin to that chain: z of all 652 fixture points bit-identical, x / y within 1e-6 m, and
340 ratio-test matches -> 330 with depth on both sides -> 326 within 0.05 m of Rt1_2, exactly MATLAB's index pairs.

Bounds (none fitted to what the kernels return):
  * lift: z bit-identical (one correctly rounded fp32 division of an integer); x, y within 1e-6 m: three fp32 roundings
    plus the restatement's own, coordinates below 4 m in this scene (max depth 2.867 m), 4 ulp(4 m) = 9.6e-7;
  * selection: the same fp32 comparisons as the numpy filter over the read-back records, so exact;
  * refit: the tolerance tests/test_rigid.py applies to a refit against its float64 anchor (beta_of the anchor's
    eigenvalues for R, beta |yc| + 1e-6 for t), imported from there;
  * inliers: every match below 0.03 m under Rt1_2 must be an inlier, the three at 0.195 m or more must not be; the two
    in between (0.0477 and 0.0501 m against the 0.05 m cut) may fall either way -- they sit within the distance by which
    any refit moves t.  (330 = 325 + 2 + 3: the restatement finds 325 matches below 0.03 m, all of them MATLAB inliers,
    where the feature request counted 324; asking for all 325 asks no less.)
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_binding import SIFT_POINT_DTYPE, read_match_indices, read_vlfeat_sift
from test_rigid import beta_of, horn, rot_dist, trans_dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CPP = os.path.join(ROOT, "tests", "cpp_rgbd")
BIN_RGBD = os.path.join(CPP, "rgbd_dropin")
W, H = 640, 480
THRESH2 = np.float32(0.05) * np.float32(0.05)
LOOPS = 1024
SEEDS = (1, 0xC0FFEE)


# ------------------------------------------------------------------------------------------------------------------
# fixtures and the float32 restatement
# ------------------------------------------------------------------------------------------------------------------
def intrinsics():
    K = np.array(open(os.path.join(GOLDEN, "rgbd_intrinsics.txt")).read().split(), np.float64).reshape(3, 3)
    return K[0, 0], K[1, 1], K[0, 2], K[1, 2]


def camera():
    from cusift_amd import capi

    fx, fy, cx, cy = intrinsics()
    return capi.Camera(fx, fy, cx, cy, origin=1.0, units_per_metre=1000.0, encoding=1)


def read_match_points():
    """rgbd_match1_2.bin (extras/debug.cpp:244-280): u32 n; n x {f64 xyz of frame 1, f64 xyz of frame 2}."""
    raw = open(os.path.join(GOLDEN, "rgbd_match1_2.bin"), "rb").read()
    n = int(np.frombuffer(raw[:4], "<u4")[0])
    assert len(raw) == 4 + 48 * n
    return np.frombuffer(raw[4:], "<f8").reshape(n, 6)


def read_rt():
    raw = open(os.path.join(GOLDEN, "rgbd_Rt1_2.bin"), "rb").read()
    assert len(raw) == 96
    return np.frombuffer(raw, "<f8").reshape(3, 4)


def roundf(x):
    """C roundf (half away from zero) of a float32 array, exactly: x - trunc(x) is exact in fp32."""
    x = np.asarray(x, np.float32)
    t = np.trunc(x)
    return (t + np.where(np.abs(x - t) >= np.float32(0.5), np.copysign(np.float32(1), x), np.float32(0))).astype(np.float32)


def lift(xy, raw, origin=1.0, units_per_metre=1000.0, encoding=1):
    """The convention documented at cusift_lift_depth, in float32 numpy: coords3D [n, 3] of coords2D xy [n, 2]."""
    fx, fy, cx, cy = (np.float32(v) for v in intrinsics())
    origin, upm = np.float32(origin), np.float32(units_per_metre)
    h, w = raw.shape
    x, y = np.asarray(xy[:, 0], np.float32), np.asarray(xy[:, 1], np.float32)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(x) & np.isfinite(y)
        u, v = roundf(np.where(ok, x, 0)), roundf(np.where(ok, y, 0))
        ok &= (u >= 0) & (u < np.float32(w)) & (v >= 0) & (v < np.float32(h))
    ui, vi = np.where(ok, u, 0).astype(np.int64), np.where(ok, v, 0).astype(np.int64)
    r = raw[vi, ui].astype(np.uint16)
    if encoding == 1:
        r = (r >> np.uint16(3)) | (r << np.uint16(13))
    z = r.astype(np.float32) / upm
    X = ((ui.astype(np.float32) + origin) - cx) * z / fx
    Y = ((vi.astype(np.float32) + origin) - cy) * z / fy
    assert X.dtype == np.float32 and z.dtype == np.float32
    ok &= r != 0
    out = np.zeros((len(x), 3), np.float32)
    out[ok] = np.stack([X, Y, z], 1)[ok]
    return out


@pytest.fixture(scope="module")
def pair():
    """(records of frame 1, of frame 2, raw depth 1, raw depth 2, restated coords3D 1, 2)."""
    s1 = read_vlfeat_sift(os.path.join(GOLDEN, "vlfeat_sift1.bin"))
    s2 = read_vlfeat_sift(os.path.join(GOLDEN, "vlfeat_sift2.bin"))
    z = np.load(os.path.join(GOLDEN, "rgbd_depth.npz"))
    d1, d2 = np.ascontiguousarray(z["depth1"]), np.ascontiguousarray(z["depth2"])
    assert d1.dtype == np.uint16 and d1.shape == (H, W) and d2.shape == (H, W)
    return s1, s2, d1, d2, lift(s1["coords2D"], d1), lift(s2["coords2D"], d2)


def select_numpy(t1, t2, score_threshold, ambiguity_threshold, three_d):
    """include/matching.h:43-58 over host records: (indices into t1, their partners)."""
    s2 = np.float32(score_threshold) * np.float32(score_threshold)
    a2 = np.float32(ambiguity_threshold) * np.float32(ambiguity_threshold)
    m = t1["match"]
    keep = (t1["score"] < s2) & (t1["ambiguity"] < a2) & (m >= 0) & (m < len(t2))
    if three_d:
        keep &= (t1["coords3D"][:, 2] != 0) & (t2["coords3D"][np.clip(m, 0, len(t2) - 1), 2] != 0)
    idx = np.nonzero(keep)[0]
    return idx.astype(np.int32), m[idx].astype(np.int32)


def residuals(rt, x1, x2):
    rt = np.asarray(rt, np.float64)
    return np.linalg.norm(x2.astype(np.float64) @ rt[:, :3].T + rt[:, 3] - x1.astype(np.float64), axis=1)


# ------------------------------------------------------------------------------------------------------------------
# without a GPU
# ------------------------------------------------------------------------------------------------------------------
def test_fixtures_are_small_and_numpy_reads_them(pair):
    for name in ("rgbd_depth.npz", "rgbd_intrinsics.txt", "rgbd_match1_2.bin", "rgbd_Rt1_2.bin"):
        assert os.path.getsize(os.path.join(GOLDEN, name)) < 466756, name
    _, _, d1, d2, _, _ = pair
    mm = (d1 >> np.uint16(3)) | (d1 << np.uint16(13))
    assert abs((mm == 0).mean() - 0.039) < 0.001 and mm.max() == 2867
    rt = read_rt()
    assert abs(np.linalg.det(rt[:, :3]) - 1) < 1e-5
    assert read_match_points().shape == (326, 6)


def test_restatement_reproduces_the_fixture_points(pair):
    """The anchor of the GPU tests: all 652 points of match1_2 from the VLFeat keypoints and the depth images."""
    s1, s2, _, _, c1, c2 = pair
    m = read_match_points()
    ii, jj = read_match_indices(os.path.join(GOLDEN, "match_indices1_2.bin"))
    a, b = c1[ii - 1], c2[jj - 1]
    assert np.array_equal(a[:, 2], m[:, 2].astype(np.float32)) and np.array_equal(b[:, 2], m[:, 5].astype(np.float32))
    dxy = max(np.abs(a[:, :2] - m[:, :2]).max(), np.abs(b[:, :2] - m[:, 3:5]).max())
    print("x, y against the fixture: max %.3g m" % dxy)
    assert dxy <= 1e-6
    assert (c1[:, 2] == 0).sum() == 29 and np.abs(np.r_[c1, c2]).max() < 4.0
    # no keypoint is closer than 7.6e-5 to a rounding tie: roundf pins the pixel
    xy = np.r_[s1["coords2D"], s2["coords2D"]].astype(np.float64)
    assert np.abs(np.abs(xy - np.trunc(xy)) - 0.5).min() > 7e-5
    # edge cases of the convention
    odd = np.array([[-3, 5], [1e9, 5], [np.nan, 5], [5, np.inf], [639.5, 5], [5, 479.5], [-0.4, -0.4]], np.float32)
    got = lift(odd, pair[2])
    assert (got[:6] == 0).all()
    assert np.array_equal(got[6], lift(np.zeros((1, 2), np.float32), pair[2])[0])


def test_restatement_reproduces_the_340_330_326_chain(oracle, pair):
    s1, s2, _, _, c1, c2 = pair
    t1, t2 = s1.copy(), s2.copy()
    t1["coords3D"], t2["coords3D"] = c1, c2
    oracle.match(t1, t2, 1)
    i2, _ = select_numpy(t1, t2, 1000.0, 0.6, False)
    i3, j3 = select_numpy(t1, t2, 1000.0, 0.6, True)
    assert len(i2) == 340 and len(i3) == 330
    assert np.abs(t1["ambiguity"] - np.float32(0.36)).min() > 1e-3
    res = residuals(read_rt(), c1[i3], c2[j3])
    inl = res < 0.05
    ii, jj = read_match_indices(os.path.join(GOLDEN, "match_indices1_2.bin"))
    assert inl.sum() == 326
    assert np.array_equal(i3[inl], ii - 1) and np.array_equal(j3[inl], jj - 1)  # the same pairs, the same order
    print("left out:", np.sort(res[~inl]), "closest inlier to the cut:", res[inl].max())
    assert (res < 0.03).sum() == 325 and (res >= 0.195).sum() == 3
    np.testing.assert_allclose(np.sort(res[(res >= 0.03) & (res < 0.195)]), [0.0477, 0.0501], atol=1e-4)
    fit, w, _ = horn(c1[i3[inl]], c2[j3[inl]])
    print("float64 Horn over the 326 against Rt1_2: R %.3g, t %.3g m" %
          (np.abs(fit - read_rt())[:, :3].max(), np.abs(fit - read_rt())[:, 3].max()))
    assert np.abs(fit - read_rt())[:, :3].max() < 5e-4 and np.abs(fit - read_rt())[:, 3].max() < 1e-3


def test_header_library_and_binding_agree():
    from cusift_amd import capi

    text = open(os.path.join(ROOT, "include", "cusift_amd_extras.h")).read()
    handle = C.CDLL(capi.LIB_PATH)
    for name, nargs in (("cusift_lift_depth", 11), ("cusift_select_matches", 11), ("cusift_register_rgbd", 23)):
        assert "int %s(cusift_ctx *ctx" % name in text, name
        assert hasattr(handle, name), name
        res, args = capi.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs, (name, len(args))
    assert "typedef struct cusift_camera" in text
    assert C.sizeof(capi.Camera) == 28 and [f[0] for f in capi.Camera._fields_] == [
        "fx", "fy", "cx", "cy", "origin", "units_per_metre", "encoding"]
    for m in ("lift_depth", "select_matches", "register_rgbd"):
        assert callable(getattr(capi.Context, m))
    assert "sift_rgbd" in open(os.path.join(ROOT, "Makefile")).read()


def test_rgbd_kernels_compile_for_gfx950_without_scratch_and_with_vector_stores_only():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs

    asm = kernel_regs.assembly("sift_rgbd.hip")
    assert "gfx950" in asm
    ks = {k["name"]: k for k in kernel_regs.kernels(asm)}
    assert len(ks) == 3 and all("rgbd_lift" in n or "match_select" in n for n in ks), sorted(ks)
    for n, k in ks.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
    # scalar memory writes and scalar atomics, by mnemonic prefix (the prefixes are spelled in pieces on purpose)
    kinds = ("st" "ore", "buffer_" "st" "ore", "scratch_" "st" "ore", "at" "omic", "buffer_" "at" "omic", "dcache_" "wb",
             "dcache_" "discard")
    prefixes = tuple("s_" + k for k in kinds)
    mnemonics = [line.split()[0] for line in asm.splitlines() if line.startswith("\t") and line.split()]
    assert not [m for m in mnemonics if m.startswith(prefixes)]
    assert not [m for m in mnemonics if "atomic" in m]  # the compaction's order comes from a scan, not from atomics
    assert any(m.startswith("v_mbcnt") for m in mnemonics)
    assert any(m.startswith("v_div_") or m.startswith("v_rcp") for m in mnemonics)  # z = r / units_per_metre


def build_cpp():
    subprocess.check_call(["make", "-C", CPP, "all"], stdout=subprocess.DEVNULL)
    assert os.path.exists(BIN_RGBD)


def test_cpp_header_compiles_and_links_with_plain_gxx():
    if os.path.exists(BIN_RGBD):
        os.remove(BIN_RGBD)
    build_cpp()
    text = open(os.path.join(ROOT, "include", "rgbd.h")).read()
    assert "LiftSiftData(" in text and "RegisterRGBD(" in text and "#include <hip" not in text
    recipe = open(os.path.join(CPP, "Makefile")).read()
    assert "hipcc" not in recipe and "/opt/rocm" not in recipe


# ------------------------------------------------------------------------------------------------------------------
# on the GPU
# ------------------------------------------------------------------------------------------------------------------
def upload(ctx, arr):
    from cusift_amd.capi import DeviceBuffer

    return DeviceBuffer.from_numpy(ctx, arr)


def other_bytes(recs):
    """Every byte of the records except coords3D (the last 12 of 588)."""
    return np.ascontiguousarray(recs).view(np.uint8).reshape(len(recs), 588)[:, :576]


def with_marks(s, extra_xy=()):
    """A copy of the records with a sentinel in coords3D and unrelated values in the match fields, plus appended
    records at the given coordinates."""
    out = np.zeros(len(s) + len(extra_xy), SIFT_POINT_DTYPE)
    out[:len(s)] = s
    for k, xy in enumerate(extra_xy):
        out[len(s) + k] = s[k]
        out["coords2D"][len(s) + k] = xy
    out["coords3D"] = 7.0
    out["score"], out["match"], out["empty"] = 0.25, -5, 3.0
    return out


@pytest.mark.gpu
def test_lift_matches_the_restatement_and_touches_nothing_else(ctx, pair):
    s1, s2, d1, d2, c1, c2 = pair
    cam = camera()
    odd = [(-3.0, 5.0), (1e9, 5.0), (np.nan, 5.0)]
    for s, d, c in ((s1, d1, c1), (s2, d2, c2)):
        src = with_marks(s, odd)
        buf, dep = upload(ctx, src), upload(ctx, d)
        ctx.lift_depth(buf.ptr, len(src), dep.ptr, W, H, cam)
        ctx.synchronize()
        got = buf.to_numpy(SIFT_POINT_DTYPE, (len(src),))
        n = len(s)
        assert np.array_equal(got["coords3D"][:n, 2], c[:, 2])
        dxy = np.abs(got["coords3D"][:n, :2] - c[:, :2]).max()
        print("x, y against the restatement: max %.3g m" % dxy)
        assert dxy <= 1e-6
        assert (got["coords3D"][n:] == 0).all()  # x = -3, 1e9, NaN
        holes = c[:, 2] == 0
        assert (got["coords3D"][:n][holes] == 0).all()
        assert np.array_equal(other_bytes(got), other_bytes(src))
    assert (c1[:, 2] == 0).sum() == 29


@pytest.mark.gpu
def test_lift_batch_equals_single_calls_and_honours_counters(ctx, pair):
    s1, s2, d1, d2, c1, c2 = pair
    cam = camera()
    max_pts = max(len(s1), len(s2)) + 5
    batch = np.zeros((2, max_pts), SIFT_POINT_DTYPE)
    batch["coords2D"] = 17.0  # valid pixels past the counts: a lift there would show
    batch[0, :len(s1)], batch[1, :len(s2)] = s1, s2
    batch["coords3D"] = 7.0
    counts = np.array([len(s1), len(s2) - 11], np.uint32)
    pitch = W + 16
    depth = np.zeros((2, H + 3, pitch), np.uint16)
    depth[0, :H, :W], depth[1, :H, :W] = d1, d2
    buf, dep, cnt = upload(ctx, batch), upload(ctx, depth), upload(ctx, counts)
    ctx.lift_depth(buf.ptr, max_pts, dep.ptr, W, H, cam, pitch=pitch, n_images=2, d_counters=cnt.ptr,
                   image_stride=(H + 3) * pitch)
    ctx.synchronize()
    got = buf.to_numpy(SIFT_POINT_DTYPE, (2, max_pts))
    for k, (s, d, n) in enumerate(((s1, d1, int(counts[0])), (s2, d2, int(counts[1])))):
        one = with_marks(s)
        b1, dd = upload(ctx, one), upload(ctx, d)
        ctx.lift_depth(b1.ptr, n, dd.ptr, W, H, cam)
        ctx.synchronize()
        single = b1.to_numpy(SIFT_POINT_DTYPE, (len(one),))
        assert got["coords3D"][k, :n].tobytes() == single["coords3D"][:n].tobytes()
        assert (got["coords3D"][k, n:] == 7.0).all() and (single["coords3D"][n:] == 7.0).all()  # past the count
        assert np.array_equal(other_bytes(got[k]), other_bytes(batch[k]))
    assert np.array_equal(got["coords3D"][0, :len(s1), 2], c1[:, 2])


def staged_select(ctx, pair, kind, depth2=None):
    """lift x 2, match, select on the device; returns (records 1, records 2, pairs, coord) as read back."""
    s1, s2, d1, d2, _, _ = pair
    cam = camera()
    b1, b2 = upload(ctx, s1), upload(ctx, s2)
    e1, e2 = upload(ctx, d1), upload(ctx, d2 if depth2 is None else depth2)
    n1, n2 = len(s1), len(s2)
    ctx.lift_depth(b1.ptr, n1, e1.ptr, W, H, cam)
    ctx.lift_depth(b2.ptr, n2, e2.ptr, W, H, cam)
    ctx.match(b1.ptr, n1, b2.ptr, n2, 1)
    pairs = upload(ctx, np.full((n1, 2), -1, np.int32))
    coord = upload(ctx, np.full((n1, 6), -1, np.float32))
    count = upload(ctx, np.full(1, -1, np.int32))
    ctx.select_matches(b1.ptr, n1, b2.ptr, n2, pairs.ptr, coord.ptr, count.ptr, 1000.0, 0.6, kind)
    ctx.synchronize()
    k = int(count.to_numpy(np.int32, (1,))[0])
    all_pairs, all_coord = pairs.to_numpy(np.int32, (n1, 2)), coord.to_numpy(np.float32, (n1, 6))
    assert 0 <= k <= n1 and (all_pairs[k:] == -1).all() and (all_coord[k:] == -1).all()  # rows past the count untouched
    return (b1.to_numpy(SIFT_POINT_DTYPE, (n1,)), b2.to_numpy(SIFT_POINT_DTYPE, (n2,)), all_pairs[:k].copy(),
            all_coord[:k].copy())


@pytest.mark.gpu
def test_select_is_the_host_filter_in_ascending_order(ctx, pair):
    t1, t2, p2, _ = staged_select(ctx, pair, "2d")
    assert len(p2) == 340
    u1, u2, p3, coord = staged_select(ctx, pair, "3d")
    assert len(p3) == 330
    assert u1.tobytes() == t1.tobytes() and u2.tobytes() == t2.tobytes()
    for p, three_d in ((p2, False), (p3, True)):
        assert (np.diff(p[:, 0]) > 0).all()
        i, j = select_numpy(t1, t2, 1000.0, 0.6, three_d)
        assert np.array_equal(p[:, 0], i) and np.array_equal(p[:, 1], j)
    ii, jj = read_match_indices(os.path.join(GOLDEN, "match_indices1_2.bin"))
    pos = np.searchsorted(p3[:, 0], ii - 1)
    assert np.array_equal(p3[pos, 0], ii - 1) and np.array_equal(p3[pos, 1], jj - 1)
    assert np.array_equal(coord[:, :3], t1["coords3D"][p3[:, 0]]) and np.array_equal(coord[:, 3:], t2["coords3D"][p3[:, 1]])
    assert np.array_equal(coord[:, :3][:, 2], pair[4][p3[:, 0], 2])


def fused(ctx, pair, seed, depth2=None, loops=LOOPS, kind="3d"):
    s1, s2, d1, d2, _, _ = pair
    b1, b2 = upload(ctx, s1), upload(ctx, s2)
    e1, e2 = upload(ctx, d1), upload(ctx, d2 if depth2 is None else depth2)
    out = ctx.register_rgbd(b1.ptr, len(s1), e1.ptr, b2.ptr, len(s2), e2.ptr, W, H, camera(), distance=1,
                            score_threshold=1000.0, ambiguity_threshold=0.6, loops=loops, thresh2=THRESH2, kind=kind,
                            seed=seed)
    return out + (b1.to_numpy(SIFT_POINT_DTYPE, (len(s1),)), b2.to_numpy(SIFT_POINT_DTYPE, (len(s2),)))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_registration_recovers_the_fixture_motion(ctx, pair, seed):
    _, _, _, _, c1, c2 = pair
    rt, pairs, flags, n_in, _, _ = fused(ctx, pair, seed)
    want = read_rt()
    assert len(pairs) == 330 and len(flags) == 330 and flags.sum() == n_in
    res = residuals(want, c1[pairs[:, 0]], c2[pairs[:, 1]])
    assert (res < 0.03).sum() == 325 and (res >= 0.195).sum() == 3
    print("seed %#x: %d inliers; undecided pair(s) %s -> %s" %
          (seed, n_in, res[(res >= 0.03) & (res < 0.195)], flags[(res >= 0.03) & (res < 0.195)]))
    assert flags[res < 0.03].all() and not flags[res >= 0.195].any()
    # the refit against a float64 Horn over the restated coordinates of the reported inliers
    fit, w, yc = horn(c1[pairs[flags, 0]], c2[pairs[flags, 1]])
    beta = beta_of(w)
    tol_t = beta * np.linalg.norm(yc) + 1e-6
    print("eigenvalues %s, beta %.3g; against the anchor |dR| %.3g, |dt| %.3g (bound %.3g)" %
          (w, beta, rot_dist(rt, fit), trans_dist(rt, fit), tol_t))
    assert rot_dist(rt, fit) <= beta
    assert trans_dist(rt, fit) <= tol_t
    # against MATLAB's Rt1_2: no further than the float64 anchor is, plus that tolerance
    d0_r, d0_t = rot_dist(fit, want), trans_dist(fit, want)
    print("anchor against Rt1_2: |dR| %.3g, |dt| %.3g (max entries %.3g / %.3g m); device %.3g, %.3g" %
          (d0_r, d0_t, np.abs(fit - want)[:, :3].max(), np.abs(fit - want)[:, 3].max(), rot_dist(rt, want),
           trans_dist(rt, want)))
    assert rot_dist(rt, want) <= d0_r + beta
    assert trans_dist(rt, want) <= d0_t + tol_t
    assert d0_r < 1e-3 and d0_t < 2e-3  # the anchor itself is MATLAB's answer (2.7e-4 / 5.4e-4 m per entry for the 326)
    assert abs(np.linalg.det(rt[:, :3].astype(np.float64)) - 1) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_fused_equals_staged_bit_for_bit(ctx, pair, seed):
    rt, pairs, flags, n_in, f1, f2 = fused(ctx, pair, seed)
    t1, t2, p3, coord = staged_select(ctx, pair, "3d")
    srt, sn, _, sflags = ctx.estimate_rigid(coord, None, loops=LOOPS, thresh2=THRESH2, kind="3d", seed=seed)
    assert rt.tobytes() == srt.tobytes() and n_in == sn
    assert np.array_equal(pairs, p3) and np.array_equal(flags, sflags)
    assert f1.tobytes() == t1.tobytes() and f2.tobytes() == t2.tobytes()  # the records end up the same too
    again = fused(ctx, pair, seed)
    for u, v in zip((rt, pairs, flags, n_in), again[:4]):
        assert np.asarray(u).tobytes() == np.asarray(v).tobytes()


@pytest.mark.gpu
def test_planar_type_and_small_counts(ctx, pair):
    """rigid_type 0 through the fused call equals the staged route too; fewer selected pairs than a sample needs give
    the identity."""
    rt, pairs, flags, n_in, _, _ = fused(ctx, pair, 5, kind="2d")
    _, _, p3, coord = staged_select(ctx, pair, "3d")
    srt, sn, _, sflags = ctx.estimate_rigid(coord, None, loops=LOOPS, thresh2=THRESH2, kind="2d", seed=5)
    assert rt.tobytes() == srt.tobytes() and n_in == sn and np.array_equal(flags, sflags) and np.array_equal(pairs, p3)
    # a frame-2 depth with two valid pixels under two matched keypoints: 2 selected pairs, below the 3-D sample size
    s1, s2, d1, d2, c1, c2 = pair
    keep = p3[[10, 200], 1]
    sparse = np.zeros_like(d2)
    for j in keep:
        u, v = int(roundf(s2["coords2D"][j, 0])), int(roundf(s2["coords2D"][j, 1]))
        sparse[v, u] = d2[v, u]
    rt, pairs, flags, n_in, _, _ = fused(ctx, pair, 5, depth2=sparse)
    assert np.array_equal(pairs, p3[[10, 200]])
    assert n_in == 0 and not flags.any() and np.array_equal(rt, np.eye(3, 4, dtype=np.float32))
    # two pairs are enough for the planar type: it runs (the third drawn index is never read)
    rt, pairs, flags, n_in, _, _ = fused(ctx, pair, 5, depth2=sparse, kind="2d")
    assert np.array_equal(pairs, p3[[10, 200]]) and 0 <= n_in <= 2 and flags.sum() == n_in


@pytest.mark.gpu
def test_edge_cases_and_refusals(ctx, pair):
    from cusift_amd import capi

    s1, s2, d1, d2, _, _ = pair
    rt, pairs, flags, n_in, _, f2 = fused(ctx, pair, 3, depth2=np.zeros_like(d2))
    assert len(pairs) == 0 and n_in == 0 and np.array_equal(rt, np.eye(3, 4, dtype=np.float32))
    assert (f2["coords3D"] == 0).all()
    b1, b2, e1, e2 = upload(ctx, s1), upload(ctx, s2), upload(ctx, d1), upload(ctx, d2)
    cam = camera()
    out = ctx.register_rgbd(b1.ptr, 0, e1.ptr, b2.ptr, len(s2), e2.ptr, W, H, cam, loops=64)
    assert len(out[1]) == 0 and out[3] == 0 and np.array_equal(out[0], np.eye(3, 4, dtype=np.float32))
    out = ctx.register_rgbd(b1.ptr, len(s1), e1.ptr, b2.ptr, 0, e2.ptr, W, H, cam, loops=64)
    assert len(out[1]) == 0 and out[3] == 0 and np.array_equal(out[0], np.eye(3, 4, dtype=np.float32))
    # select with n1 == 0 writes a zero count
    count = upload(ctx, np.full(1, -1, np.int32))
    ctx.select_matches(b1.ptr, 0, b2.ptr, len(s2), None, None, count.ptr)
    ctx.synchronize()
    assert count.to_numpy(np.int32, (1,))[0] == 0

    rt = np.full(12, 9.0, np.float32)
    nm, ni = C.c_int(-7), C.c_int(-7)

    def call(cam=cam, out=rt, pnm=C.byref(nm), pni=C.byref(ni), loops=64, th=0.0025, kind=1, dist=1, pitch=W, dep=e1.ptr):
        return capi.lib().cusift_register_rgbd(ctx.handle, b1.ptr, len(s1), dep, b2.ptr, len(s2), e2.ptr, W, H, pitch,
                                               C.byref(cam) if cam is not None else None, dist, 1000.0, 0.6, loops, th,
                                               kind, 1, out.ctypes.data if out is not None else None, pnm, pni, None,
                                               None)

    fx0 = camera()
    fx0.fx = 0.0
    upm0 = camera()
    upm0.units_per_metre = 0.0
    enc = camera()
    enc.encoding = 2
    for kw in (dict(cam=fx0), dict(cam=upm0), dict(cam=enc), dict(cam=None), dict(out=None), dict(pnm=None),
               dict(pni=None), dict(loops=0), dict(th=0.0), dict(th=float("nan")), dict(kind=2), dict(dist=3),
               dict(pitch=W - 1), dict(dep=None)):
        assert call(**kw) == -1, kw  # CUSIFT_ERR_INVALID
        assert (rt == 9.0).all() and nm.value == -7 and ni.value == -7, kw  # nothing of the caller's written
    with pytest.raises(capi.CusiftError):
        ctx.lift_depth(b1.ptr, len(s1), e1.ptr, W, H, fx0)
    with pytest.raises(capi.CusiftError):
        ctx.lift_depth(b1.ptr, len(s1), None, W, H, cam)
    with pytest.raises(capi.CusiftError):
        ctx.select_matches(b1.ptr, len(s1), b2.ptr, len(s2), None, None, None)
    assert call(loops=LOOPS) == 0 and nm.value == 330 and 325 <= ni.value <= 327


@pytest.mark.gpu
def test_cpp_program_passes_on_gpu(tmp_path, pair):
    """tests/cpp_rgbd/rgbd_dropin.cpp: the reference's RANSACTestImage shape through LiftSiftData + the unchanged
    MatchSiftData / EstimateRigidTransform headers, and through RegisterRGBD."""
    build_cpp()
    _, _, d1, d2, _, _ = pair
    d1.astype("<u2").tofile(str(tmp_path / "depth1.u16"))
    d2.astype("<u2").tofile(str(tmp_path / "depth2.u16"))
    cmd = [BIN_RGBD, os.path.join(GOLDEN, "vlfeat_sift1.bin"), os.path.join(GOLDEN, "vlfeat_sift2.bin"),
           str(tmp_path / "depth1.u16"), str(tmp_path / "depth2.u16"), os.path.join(GOLDEN, "rgbd_intrinsics.txt"),
           os.path.join(GOLDEN, "rgbd_Rt1_2.bin")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout
    assert "staged: matches 330, inliers " in out.stdout and "fused: matches 330, inliers " in out.stdout
