"""RANSAC rigid transform (cusift_estimate_rigid, cusift_amd/csrc/sift_rigid.hip): EstimateRigidTransformH of the
reference, extras/rigidTransform.cu:388-520.

The yardstick is a float64 numpy restatement of the algorithm written in this file (Horn's quaternion estimate per sample
triple, the strict `<` inlier test, the LAST maximum, the refit over the winner's inliers; the closed-form 2-D estimate;
the documented integer generator), anchored on the one fixture the reference pins this estimator with:

    tests/golden/rigid_ransac.bin is the reference's test/data/RigidTransform_RANSAC.bin, byte for byte (3,056 bytes,
    data only; written by its authors' DEBUG_ransactfitRt.m): u32 nMatch = 120, nLoops = 10; f32[120][3] reference-frame
    points; f32[120][3] moving-frame points; i32[10][3] 1-based sample triples; f32[12] MATLAB's resulting Rt.

The device is never compared with itself alone.  Bounds (none of them fitted to what the kernels return):
  * rotation: |R_dev - R_f64|_F / sqrt(2) <= 32 * 2^-24 / g, with g = (lambda2 - lambda1) / lambda4 the relative gap of
    the 4x4 matrix B whose lowest eigenvector is the quaternion (an fp32 LAPACK solve reaches 1.2-1.6 in these units);
    compared only where g >= 1e-3, and at most 1 % of the hypotheses may be left out;
  * translation: t = xc - R yc inherits beta * |yc| (+ 1e-6 for its own fp32 rounding);
  * scoring: exact outside a band of 64 * 2^-24 * M / sqrt(thresh2) (relative) around thresh2 -- 12 fp32 products of
    magnitude <= M carry a few ulps each into an error of size sqrt(thresh2); at most 0.1 % of all tests may fall in it;
  * 2-D: every entry within 16 * 2^-24 * M / d of float64, d the sample's x-z separation (the smaller of the two frames').
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "rigid_ransac.bin")
CPP = os.path.join(ROOT, "tests", "cpp_rigid")
BIN_RIGID = os.path.join(CPP, "rigid_dropin")
U = 2.0 ** -24
FIXTURE_COUNTS = [114, 102, 38, 57, 114, 114, 114, 0, 113, 103]
THRESH2 = np.float32(0.05) * np.float32(0.05)


# ------------------------------------------------------------------------------------------------------------------
# the float64 restatement
# ------------------------------------------------------------------------------------------------------------------
def read_fixture():
    raw = open(FIXTURE, "rb").read()
    n, loops = np.frombuffer(raw, "<u4", 2)
    n, loops = int(n), int(loops)
    off = 8
    ci = np.frombuffer(raw, "<f4", 3 * n, off).reshape(n, 3)
    off += 12 * n
    cj = np.frombuffer(raw, "<f4", 3 * n, off).reshape(n, 3)
    off += 12 * n
    idx = np.frombuffer(raw, "<i4", 3 * loops, off).reshape(loops, 3) - 1
    off += 12 * loops
    rt = np.frombuffer(raw, "<f4", 12, off).reshape(3, 4)
    assert off + 48 == len(raw) == 3056
    return np.ascontiguousarray(np.hstack([ci, cj])), np.ascontiguousarray(idx.astype(np.int32)), rt.astype(np.float64)


def horn(x, y):
    """Batched: x, y [..., K, 3] float64 -> Rt [..., 3, 4], eigenvalues [..., 4] of B (ascending), moving centroid."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)
    xc, yc = x.mean(-2), y.mean(-2)
    x, y = x - xc[..., None, :], y - yc[..., None, :]
    d, s = y - x, y + x
    A = np.zeros(x.shape[:-1] + (4, 4))
    A[..., 0, 1:] = d
    A[..., 1:, 0] = -d
    A[..., 1, 2], A[..., 1, 3] = -s[..., 2], s[..., 1]
    A[..., 2, 1], A[..., 2, 3] = s[..., 2], -s[..., 0]
    A[..., 3, 1], A[..., 3, 2] = -s[..., 1], s[..., 0]
    B = np.einsum("...kij,...klj->...il", A, A)
    w, V = np.linalg.eigh(B)
    q = V[..., :, 0]
    q0, q1, q2, q3 = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.stack([1 - 2 * (q2 * q2 + q3 * q3), 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2),
                  2 * (q1 * q2 + q0 * q3), 1 - 2 * (q1 * q1 + q3 * q3), 2 * (q2 * q3 - q0 * q1),
                  2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), 1 - 2 * (q1 * q1 + q2 * q2)], -1)
    R = R.reshape(R.shape[:-1] + (3, 3))
    t = xc - np.einsum("...ij,...j->...i", R, yc)
    return np.concatenate([R, t[..., None]], -1), w, yc


def solve2d(a, b):
    """Batched extras/rigidTransform.cu:222-290 in float64: a, b [..., 6] -> Rt [..., 3, 4]."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        dxw, dzw = a[..., 0] - b[..., 0], a[..., 2] - b[..., 2]
        dxc, dzc = a[..., 3] - b[..., 3], a[..., 5] - b[..., 5]
        lw, lc = np.sqrt(dxw * dxw + dzw * dzw), np.sqrt(dxc * dxc + dzc * dzc)
        cs = (dxw / lw) * (dxc / lc) + (dzw / lw) * (dzc / lc)
        sn = (dzw / lw) * (dxc / lc) - (dxw / lw) * (dzc / lc)
        sxw, szw, sxc, szc = a[..., 0] + b[..., 0], a[..., 2] + b[..., 2], a[..., 3] + b[..., 3], a[..., 5] + b[..., 5]
        rt = np.zeros(cs.shape + (3, 4))
        rt[..., 0, 0], rt[..., 0, 2], rt[..., 0, 3] = cs, -sn, (sxw - cs * sxc + sn * szc) / 2
        rt[..., 1, 1] = 1.0
        rt[..., 2, 0], rt[..., 2, 2], rt[..., 2, 3] = sn, cs, (szw - sn * sxc - cs * szc) / 2
    return rt, np.minimum(lw, lc)


def errors2(rt, coord):
    """|R y + t - x|^2 in float64 for hypotheses rt [L, 3, 4] and points coord [N, 6] -> ([L, N], largest magnitude)."""
    rt = np.asarray(rt, np.float64)
    x, y = coord[:, :3].astype(np.float64), coord[:, 3:].astype(np.float64)
    with np.errstate(invalid="ignore"):
        p = np.einsum("lij,nj->lni", rt[:, :, :3], y) + rt[:, None, :, 3]
        big = max(np.abs(x).max(), np.abs(y).max(), np.nanmax(np.abs(p), initial=0.0))
        return ((p - x[None]) ** 2).sum(-1), big


def hypotheses(coord, idx, kind):
    s = coord[idx].astype(np.float64)  # [L, 3, 6]
    if kind == "3d":
        rt, w, _ = horn(s[:, :, :3], s[:, :, 3:])
        return rt, w
    rt, d = solve2d(s[:, 0], s[:, 1])
    return rt, d


def ransac64(coord, idx, thresh2, kind="3d"):
    """The whole estimator in float64: (Rt, count, best loop, flags, all Rt, all counts, refit eigenvalues or None)."""
    all_rt, _ = hypotheses(coord, idx, kind)
    with np.errstate(invalid="ignore"):
        inl = np.vstack([errors2(all_rt[a:a + 256], coord)[0] < float(thresh2) for a in range(0, len(idx), 256)])
    counts = inl.sum(1)
    best = len(counts) - 1 - int(np.argmax(counts[::-1]))  # the last maximum, rigidTransform.cu:450
    flags = inl[best]
    rt, w = all_rt[best], None
    if kind == "3d" and counts[best] >= 3:
        rt, w, _ = horn(coord[flags, :3], coord[flags, 3:])
    return rt, int(counts[best]), best, flags, all_rt, counts, w


M64 = (1 << 64) - 1


def mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def draw_samples(seed, loops, num_pts):
    """The generator documented in include/cusift_amd_extras.h, in Python integers."""
    out = np.zeros((loops, 3), np.int32)
    for l in range(loops):
        def draw(k):
            return (mix((seed & M64) ^ mix((l << 32) | k)) >> 32) % num_pts
        p1, p2, p3, k = draw(0), draw(1), draw(2), 3
        tries = 0
        while p2 == p1 and tries < 64:
            p2, k, tries = draw(k), k + 1, tries + 1
        if p2 == p1:
            p2 = min(i for i in range(num_pts) if i != p1)
        tries = 0
        while p3 in (p1, p2) and tries < 64:
            p3, k, tries = draw(k), k + 1, tries + 1
        if p3 in (p1, p2):
            p3 = min(i for i in range(num_pts) if i not in (p1, p2))
        out[l] = p1, p2, p3
    return out


def cross(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def planted(axis=(0.2, 0.9, 0.1), angle=0.35, t=(0.12, -0.03, 0.2)):
    ax = np.asarray(axis, np.float64)
    K = cross(ax / np.linalg.norm(ax))
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K, np.asarray(t, np.float64)


def scene(n_in, n_out, seed, noise=0.004, R=None, t=None):
    """Points in a 1.8 x 1.2 x 2.7 m volume at 0.8-3.5 m, moved by a planted rigid motion, 4 mm Gaussian noise; outliers
    uniform in the volume.  Returns coord float32 [n, 6] (reference xyz, moving xyz), shuffled."""
    r = np.random.default_rng(seed)
    n = n_in + n_out
    if R is None:
        R, t = planted()

    def volume(m):
        return np.c_[r.uniform(-0.9, 0.9, m), r.uniform(-0.6, 0.6, m), r.uniform(0.8, 3.5, m)]

    y = volume(n)
    x = y @ R.T + t + r.normal(0, noise, (n, 3))
    x[n_in:] = volume(n_out)
    p = r.permutation(n)
    return np.ascontiguousarray(np.hstack([x[p], y[p]]).astype(np.float32))


def triples(n, loops, seed):
    r = np.random.default_rng(seed)
    return np.ascontiguousarray(np.array([r.choice(n, 3, replace=False) for _ in range(loops)], np.int32))


def rot_dist(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64)[:, :3] - np.asarray(b, np.float64)[:, :3]) / np.sqrt(2))


def trans_dist(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64)[:, 3] - np.asarray(b, np.float64)[:, 3]))


def beta_of(w):
    return 32 * U / ((w[1] - w[0]) / w[3])


def check_scoring(coord, all_rt, all_counts, thresh2):
    """Item 2: every device count lies in [sure, sure + borderline] of a float64 recount with the device's own Rt."""
    th = float(thresh2)
    total_border = 0
    for a in range(0, len(all_rt), 256):
        e, big = errors2(all_rt[a:a + 256], coord)
        band = 64 * U * big / np.sqrt(th)
        with np.errstate(invalid="ignore"):
            border = np.abs(e - th) <= band * th
            sure = (e < th) & ~border
        lo, hi = sure.sum(1), sure.sum(1) + border.sum(1)
        got = all_counts[a:a + 256]
        bad = np.nonzero((got < lo) | (got > hi))[0]
        assert len(bad) == 0, (a + bad[:5], got[bad[:5]], lo[bad[:5]], hi[bad[:5]])
        total_border += int(border.sum())
    share = total_border / (len(all_rt) * len(coord))
    print("borderline tests: %d of %d (%.4f %%)" % (total_border, len(all_rt) * len(coord), 100 * share))
    assert share <= 1e-3, share


def check_flags(coord, rt, flags, thresh2):
    e, big = errors2(np.asarray(rt, np.float64)[None], coord)
    th = float(thresh2)
    with np.errstate(invalid="ignore"):
        border = np.abs(e[0] - th) <= 64 * U * big / np.sqrt(th) * th
        want = e[0] < th
    assert np.array_equal(flags[~border], want[~border]), np.nonzero(flags != want)[0][:10]


# ------------------------------------------------------------------------------------------------------------------
# without a GPU
# ------------------------------------------------------------------------------------------------------------------
def test_fixture_is_the_reference_file():
    assert os.path.getsize(FIXTURE) == 3056
    coord, idx, rt = read_fixture()
    assert coord.shape == (120, 6) and idx.shape == (10, 3) and idx.min() >= 0 and idx.max() < 120
    assert abs(np.linalg.det(rt[:, :3]) - 1) < 1e-5


def test_numpy_restatement_reproduces_the_fixture():
    """The test of the test: Horn per triple, strict threshold, last maximum, refit == MATLAB's Rt."""
    coord, idx, want = read_fixture()
    rt, n, best, flags, all_rt, counts, w = ransac64(coord, idx, THRESH2)
    assert counts.tolist() == FIXTURE_COUNTS
    assert best == 6 and n == 114 and flags.sum() == 114
    print("max |Rt - fixture| = %.3g, refit eigenvalues %s" % (np.abs(rt - want).max(), w))
    assert np.abs(rt - want).max() <= 2e-7
    # no point of any hypothesis closer to the threshold than 1.9 % of thresh2 => the counts are exact in fp32 too
    e = errors2(all_rt, coord)[0]
    assert np.abs(e - float(THRESH2)).min() / float(THRESH2) > 0.018
    # the FIRST maximum (hypothesis 0) would be 6.2e-3 away: the tie rule is pinned
    first = int(np.argmax(counts))
    other = horn(coord[e[first] < float(THRESH2), :3], coord[e[first] < float(THRESH2), 3:])[0]
    assert first == 0 and np.abs(other - want).max() > 1e-3


def test_generator_restatement_draws_distinct_triples():
    for n in (3, 4, 120):
        s = draw_samples(12345, 200, n)
        assert s.min() >= 0 and s.max() < n
        assert (s[:, 0] != s[:, 1]).all() and (s[:, 0] != s[:, 2]).all() and (s[:, 1] != s[:, 2]).all()
    assert not np.array_equal(draw_samples(1, 50, 120), draw_samples(2, 50, 120))
    assert mix(0) == 0xE220A8397B1DCDAF  # splitmix64's first output for seed 0


def test_library_header_and_binding_agree_on_estimate_rigid():
    from cusift_amd import capi

    text = open(os.path.join(ROOT, "include", "cusift_amd_extras.h")).read()
    assert "int cusift_estimate_rigid(cusift_ctx *ctx, const float *h_coord" in text and "uint64_t seed" in text
    assert "const int *h_indices" in text
    assert hasattr(C.CDLL(capi.LIB_PATH), "cusift_estimate_rigid")
    res, args = capi.SIGNATURES["cusift_estimate_rigid"]
    assert res is C.c_int and len(args) == 15 and args[7] is C.c_uint64
    assert os.path.exists(os.path.join(ROOT, "cusift_amd", "csrc", "sift_rigid.hip"))
    assert "sift_rigid" in open(os.path.join(ROOT, "Makefile")).read()


def test_binding_rejects_bad_arguments_before_any_device_call():
    from cusift_amd import capi

    ctx = object.__new__(capi.Context)  # no device behind it: anything that reached the library would raise differently
    coord = scene(20, 0, 1)
    idx = triples(20, 8, 2)
    bad = [
        dict(coord=coord.astype(np.float64), indices=idx),
        dict(coord=coord[:, :5], indices=idx),
        dict(coord=coord.reshape(-1), indices=idx),
        dict(coord=coord, indices=idx.astype(np.int64)),
        dict(coord=coord, indices=idx[:, :2]),
        dict(coord=coord, indices=idx.reshape(-1)),
        dict(coord=coord, indices=idx[:0]),
        dict(coord=coord, indices=idx, loops=9),
        dict(coord=coord[:2], indices=np.zeros((4, 3), np.int32)),
        dict(coord=coord[:2], loops=16),
        dict(coord=coord[:2], loops=16, kind="2d"),
        dict(coord=coord[:1], indices=np.zeros((4, 3), np.int32), kind="2d"),
        dict(coord=coord, indices=np.full((4, 3), 20, np.int32)),
        dict(coord=coord, indices=np.full((4, 3), -1, np.int32)),
        dict(coord=coord),
        dict(coord=coord, loops=0),
        dict(coord=coord, indices=idx, thresh2=0.0),
        dict(coord=coord, indices=idx, thresh2=float("nan")),
        dict(coord=coord, indices=idx, kind="4d"),
    ]
    for kw in bad:
        with pytest.raises((ValueError, capi.CusiftError)):
            capi.Context.estimate_rigid(ctx, **kw)
        with pytest.raises(ValueError):
            capi.check_rigid_args(**kw)
    c, i, loops, rtype = capi.check_rigid_args(coord, idx)
    assert c.shape == (20, 6) and i.shape == (8, 3) and loops == 8 and rtype == 1
    # the 2-D estimate reads two samples: two points and a free third index are legal
    assert capi.check_rigid_args(coord[:2], np.array([[0, 1, 7]], np.int32), kind="2d")[3] == 0


def build_cpp():
    subprocess.check_call(["make", "-C", CPP, "all"], stdout=subprocess.DEVNULL)
    assert os.path.exists(BIN_RIGID)


def test_cpp_headers_compile_and_link_with_plain_gxx():
    """include/rigidTransform.h + ReadMATLABRANSAC of include/debug.h: plain C++ over the C ABI, no HIP include path."""
    if os.path.exists(BIN_RIGID):
        os.remove(BIN_RIGID)
    build_cpp()
    text = open(os.path.join(ROOT, "include", "rigidTransform.h")).read()
    for needle in ("RigidTransformType", "EstimateRigidTransformH(", "EstimateRigidTransform(", "RigidTransformType2D",
                   "RigidTransformType3D"):
        assert needle in text, needle
    assert "#include <hip" not in text and "curand" not in text.replace("cuRAND", "")
    assert "ReadMATLABRANSAC(" in open(os.path.join(ROOT, "include", "debug.h")).read()
    recipe = open(os.path.join(CPP, "Makefile")).read()
    assert "hipcc" not in recipe and "/opt/rocm" not in recipe


def test_rigid_kernels_use_no_scratch_and_only_vector_stores():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs

    asm = kernel_regs.assembly("sift_rigid.hip")
    ks = {k["name"]: k for k in kernel_regs.kernels(asm)}
    assert len(ks) == 5 and all("rigid_" in n for n in ks), sorted(ks)  # solve x 2, score, select x 2
    for n, k in ks.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
        assert kernel_regs.waves_per_simd(k) >= 4, (n, k)
    # scalar memory writes and scalar atomics, by mnemonic prefix (the prefixes are spelled in pieces on purpose)
    kinds = ("st" "ore", "buffer_" "st" "ore", "scratch_" "st" "ore", "at" "omic", "buffer_" "at" "omic", "dcache_" "wb",
             "dcache_" "discard")
    prefixes = tuple("s_" + k for k in kinds)
    mnemonics = [line.split()[0] for line in asm.splitlines() if line.startswith("\t") and line.split()]
    assert any(m.startswith("v_fma_f32") for m in mnemonics) and any(m.startswith("v_fma_f64") for m in mnemonics)
    hits = [m for m in mnemonics if m.startswith(prefixes)]
    assert not hits, sorted(set(hits))
    assert any(m.startswith("global_atomic_add") for m in mnemonics)  # the splits' partial counts


# ------------------------------------------------------------------------------------------------------------------
# on the GPU
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fixture_with_given_indices(ctx):
    """Item 1: the reference's fixture through the device -- counts, winner, flags, and MATLAB's Rt."""
    coord, idx, want = read_fixture()
    rt64, n64, best64, flags64, _, _, w = ransac64(coord, idx, THRESH2)
    before = idx.copy()
    rt, n, best, flags, all_rt, all_c, drawn = ctx.estimate_rigid(coord, idx, thresh2=THRESH2, kind="3d", want_all=True)
    assert all_c.tolist() == FIXTURE_COUNTS
    assert best == 6 and n == 114
    assert np.array_equal(flags, flags64) and flags.sum() == 114
    assert np.array_equal(idx, before) and np.array_equal(drawn, idx)
    beta = beta_of(w)
    ynorm = np.linalg.norm(coord[flags, 3:].astype(np.float64).mean(0))
    print("eigenvalues %s, beta %.3g; |dR| %.3g, |dt| %.3g (bound %.3g); vs float64 |dR| %.3g" %
          (w, beta, rot_dist(rt, want), trans_dist(rt, want), beta * ynorm + 1e-6, rot_dist(rt, rt64)))
    assert 0.25 < (w[1] - w[0]) / w[3] < 0.33  # g = 0.29, beta about 7e-6
    assert rot_dist(rt, want) <= beta
    assert trans_dist(rt, want) <= beta * ynorm + 1e-6


SCENES = [(114, 6, 4096), (1500, 2500, 4096), (3, 0, 1), (700, 333, 1000)]


@pytest.mark.gpu
@pytest.mark.parametrize("n_in,n_out,loops", SCENES)
def test_scenes_scoring_solve_selection_and_refit(ctx, n_in, n_out, loops):
    """Items 2, 3, 4 and 7: 4000 and 1033 points are no multiple of the 256-point tile, 1000 loops no multiple of 64.  On a
    part with 256 CUs the 4000 points are scored in 16 splits of 250, so every workgroup still sees ONE partial tile; splits
    of several tiles, whole and ragged, are tests/test_ransac_sizes.py's."""
    coord = scene(n_in, n_out, seed=n_in + loops)
    n_pts = len(coord)
    idx = triples(n_pts, loops, seed=n_out + 7)
    before = idx.copy()
    rt, n, best, flags, all_rt, all_c, drawn = ctx.estimate_rigid(coord, idx, thresh2=THRESH2, kind="3d", want_all=True)
    assert np.array_equal(idx, before) and np.array_equal(drawn, idx)
    assert np.isfinite(all_rt).all()
    # item 2: scoring is exact up to borderline points, judged with the device's own hypotheses
    check_scoring(coord, all_rt, all_c, THRESH2)
    # item 3: the solve is as accurate as fp32 allows
    rt64, w = hypotheses(coord, idx, "3d")
    g = (w[:, 1] - w[:, 0]) / w[:, 3]
    keep = g >= 1e-3
    dist = np.linalg.norm((all_rt.astype(np.float64) - rt64)[:, :, :3], axis=(1, 2)) / np.sqrt(2)
    ratio = dist[keep] / (U / g[keep])
    print("solve: %d of %d left out (g < 1e-3); |dR| / (2^-24 / g): median %.3g, max %.3g (bound 32)" %
          ((~keep).sum(), loops, np.median(ratio), ratio.max()))
    assert (~keep).mean() <= 0.01
    assert ratio.max() <= 32
    # item 4: selection, flags, refit
    assert best == len(all_c) - 1 - int(np.argmax(all_c[::-1]))
    assert n == all_c[best] == flags.sum()
    check_flags(coord, all_rt[best], flags, THRESH2)
    if n >= 3:
        fit, wf, yc = horn(coord[flags, :3], coord[flags, 3:])
    else:
        fit, wf, yc = rt64[best], w[best], coord[idx[best], 3:].astype(np.float64).mean(0)
    beta = beta_of(wf)
    assert rot_dist(rt, fit) <= beta, (rot_dist(rt, fit), beta)
    assert trans_dist(rt, fit) <= beta * np.linalg.norm(yc) + 1e-6
    # the planted motion is recovered as well as the float64 estimator recovers it from the same samples
    R, t = planted()
    truth = np.c_[R, t]
    ref = ransac64(coord, idx, THRESH2)
    print("planted motion: float64 RANSAC |dR| %.3g |dt| %.3g (%d inliers, loop %d); device |dR| %.3g |dt| %.3g "
          "(%d inliers, loop %d)" % (rot_dist(ref[0], truth), trans_dist(ref[0], truth), ref[1], ref[2],
                                     rot_dist(rt, truth), trans_dist(rt, truth), n, best))
    assert n >= min(n_in, 3)
    assert rot_dist(rt, truth) <= rot_dist(ref[0], truth) + beta
    assert trans_dist(rt, truth) <= trans_dist(ref[0], truth) + beta * np.linalg.norm(yc)


@pytest.mark.gpu
def test_device_sampling_follows_the_documented_generator(ctx):
    """Item 5."""
    coord = scene(114, 6, seed=3)
    loops, seed = 1000, 0x1234_5678_9ABC_DEF0
    a = ctx.estimate_rigid(coord, None, loops=loops, thresh2=THRESH2, seed=seed, want_all=True)
    b = ctx.estimate_rigid(coord, None, loops=loops, thresh2=THRESH2, seed=seed, want_all=True)
    c = ctx.estimate_rigid(coord, None, loops=loops, thresh2=THRESH2, seed=seed + 1, want_all=True)
    drawn = a[6]
    assert np.array_equal(drawn, draw_samples(seed, loops, len(coord)))
    assert drawn.min() >= 0 and drawn.max() < len(coord)
    assert (drawn[:, 0] != drawn[:, 1]).all() and (drawn[:, 0] != drawn[:, 2]).all() and (drawn[:, 1] != drawn[:, 2]).all()
    for u, v in zip(a, b):
        assert np.asarray(u).tobytes() == np.asarray(v).tobytes()
    assert not np.array_equal(c[6], drawn) and np.array_equal(c[6], draw_samples(seed + 1, loops, len(coord)))
    # the drawn samples are what was solved: given back as indices they give the same answer
    d = ctx.estimate_rigid(coord, drawn, thresh2=THRESH2, want_all=True)
    for u, v in zip(a, d):
        assert np.asarray(u).tobytes() == np.asarray(v).tobytes()
    check_scoring(coord, a[4], a[5], THRESH2)
    # three points: every draw collides often, the triples still come out distinct and as documented
    tiny = ctx.estimate_rigid(coord[:3], None, loops=257, thresh2=THRESH2, seed=9, want_all=True)
    assert np.array_equal(tiny[6], draw_samples(9, 257, 3)) and (np.sort(tiny[6], 1) == [0, 1, 2]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("y_mode", ["consistent", "arbitrary"])
def test_two_point_planar_type(ctx, y_mode):
    """Item 6: rotation about y plus an x-z translation.  `consistent`: y is an arbitrary value per point, the same in
    both frames up to the noise (what a rotation about y leaves alone), so the scene has inliers.  `arbitrary`: the
    moving frame's y is replaced by unrelated values -- the estimate must not move (it never reads y), the counts drop."""
    R, t = planted(axis=(0, 1, 0), angle=0.35, t=(0.12, 0.0, 0.2))
    coord = scene(600, 400, seed=11, R=R, t=t)
    r = np.random.default_rng(5)
    if y_mode == "arbitrary":
        coord[:, 4] = r.uniform(-0.6, 0.6, len(coord)).astype(np.float32)
    loops = 4096
    idx = triples(len(coord), loops, seed=13)
    idx[7] = (5, 5, 9)  # coincident samples: NaN hypothesis, no inlier, no error
    idx[100, 2] = 10 ** 6  # the third sample is never read
    rt, n, best, flags, all_rt, all_c, drawn = ctx.estimate_rigid(coord, idx, thresh2=THRESH2, kind="2d", want_all=True)
    assert np.array_equal(drawn, idx)
    assert np.isnan(all_rt[7][[0, 0, 2, 2, 0, 2], [0, 2, 0, 2, 3, 3]]).all() and all_c[7] == 0
    # the form [c 0 -s; 0 1 0; s 0 c], t_y = 0, with exact zeros and one
    assert (all_rt[:, 0, 1] == 0).all() and (all_rt[:, 1, 0] == 0).all() and (all_rt[:, 1, 2] == 0).all()
    assert (all_rt[:, 2, 1] == 0).all() and (all_rt[:, 1, 1] == 1).all() and (all_rt[:, 1, 3] == 0).all()
    ok = np.arange(loops) != 7
    assert np.array_equal(all_rt[ok, 0, 0], all_rt[ok, 2, 2]) and np.array_equal(all_rt[ok, 0, 2], -all_rt[ok, 2, 0])
    rt64, d = hypotheses(coord, idx[:, [0, 1, 1]], "2d")
    big = errors2(rt64[ok], coord)[1]
    keep = ok & (d >= 1e-3 * big)
    diff = np.abs(all_rt.astype(np.float64) - rt64).max(axis=(1, 2))
    ratio = diff[keep] / (U * big / d[keep])
    print("2-D: M = %.3g, %d of %d left out; |dRt| / (2^-24 M / d): median %.3g, max %.3g (bound 16)" %
          (big, (~keep).sum(), loops, np.median(ratio), ratio.max()))
    assert (~keep).mean() <= 0.01 and ratio.max() <= 16
    check_scoring(coord, all_rt, all_c, THRESH2)
    # no refit: the winner is returned as it is
    assert best == len(all_c) - 1 - int(np.argmax(all_c[::-1])) and n == all_c[best] == flags.sum()
    assert rt.tobytes() == all_rt[best].tobytes()
    check_flags(coord, all_rt[best], flags, THRESH2)
    if y_mode == "consistent":
        truth = np.c_[R, t]
        print("2-D winner: %d inliers, |dR| %.3g |dt| %.3g from the planted motion" %
              (n, rot_dist(rt, truth), trans_dist(rt, truth)))
        assert n >= 300 and rot_dist(rt, truth) < 0.02 and trans_dist(rt, truth) < 0.05


@pytest.mark.gpu
def test_library_refuses_what_the_header_says_it_refuses(ctx):
    from cusift_amd import capi

    coord = scene(20, 0, 1)
    idx = triples(20, 8, 2)
    rt = np.zeros(12, np.float32)
    n = C.c_int(0)

    def call(c=coord, npts=20, i=idx, loops=8, th=0.0025, kind=1, out=rt):
        return capi.lib().cusift_estimate_rigid(ctx.handle, c.ctypes.data if c is not None else None, npts,
                                                i.ctypes.data if i is not None else None, loops, th, kind, 0,
                                                out.ctypes.data if out is not None else None, C.byref(n), None, None,
                                                None, None, None)

    assert call() == 0 and 3 <= n.value <= 20
    bad_idx = idx.copy()
    bad_idx[3, 2] = 20
    for kw in (dict(npts=2), dict(npts=2, i=None), dict(npts=1, kind=0), dict(loops=0), dict(th=0.0), dict(th=-1.0),
               dict(th=float("nan")), dict(i=bad_idx), dict(kind=2), dict(out=None), dict(c=None)):
        assert call(**kw) == -1, kw  # CUSIFT_ERR_INVALID
    assert call(i=bad_idx, kind=0) == 0  # the 2-D estimate does not read the third sample
    assert call(npts=2, kind=0, i=np.array([[0, 1, 0]] * 8, np.int32)) == 0


@pytest.mark.gpu
def test_cpp_program_passes_on_gpu():
    """Item 8: the reference's RANSACWithIndices / RANSACWithRandom (test/test.cpp:62-134) against
    include/rigidTransform.h, asserting instead of printing."""
    build_cpp()
    out = subprocess.run([BIN_RIGID, FIXTURE], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout and "RANSACWithIndices: inliers / total: 114 / 120" in out.stdout
    assert "RANSACWithRandom" in out.stdout
