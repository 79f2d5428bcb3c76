"""Epipolar registration on the device (cusift_amd/csrc/sift_epipolar.hip): cusift_estimate_fundamental,
cusift_register_epipolar, include/epipolar.h's EstimateFundamental / RegisterEpipolar.

The reference has no fundamental-matrix code, so the yardstick is a float64 numpy model written in this file, none of it
fitted to what the kernels return:
  * samples: a pure-integer restatement of the eight-slot recipe (sample8);
  * hypotheses: the normalised 8-point algorithm with numpy's SVD for the null vector and for the rank-2 step (the device
    uses Gaussian elimination and a 3 x 3 Jacobi).  Bound 1e-6 max-abs on the unit-norm F for the loops whose normalised
    8 x 9 matrix has sigma8 / sigma1 >= 1e-3: the fp64 null vector is good to about eps * (sigma1 / sigma8)^2 ~ 1e-10,
    denormalisation multiplies by up to ~1e3, an fp32 solve measured 3e-4.  The filter may drop at most 15 % of a scene's
    loops (the model alone drops up to 12.5 % of the 12-point scene and 3 % of the larger ones, asserted on the CPU);
  * counts, flags, num_fit: the pinned inlier test in float64 with the device's OWN matrices -- exactly, every loop;
  * refit: the model's rounds started from the device's winner: F within 1e-6, num_fit exactly, match_error within 1e-5
    relative.  A seed is skipped when, in the model, some candidate lies within a relative 1e-9 of the threshold in any
    round (at most one of the listed seeds);
  * planted inliers: at least 99 % have match_error < refine_thresh.  The model alone is asserted at 99.5 % on the CPU: on
    the committed 400-point scene it reaches 99.75 % (399 of 400: at 0.3 px of noise, 1 px is 3.3 sigma and one point
    beyond it is the expectation), 100 % on the two smaller ones.
SCENE_SEEDS, the generator's seed per scene size, were picked with the model alone so that the scenes serve -- 100 loops over
60 % inliers draw an all-inlier sample with probability 0.82 only -- and the CPU test rechecks them.
"""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle_binding import SIFT_POINT_DTYPE, read_vlfeat_sift
from test_planar import RULE_ARGS, candidates, draw, subset_scores, upload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SCENES = [(12, 0, 64), (60, 40, 100), (400, 250, 512)]  # (planted inliers, outliers, loops)
SEEDS = (1, 0xC0FFEE, 2 ** 64 - 3)
THRESH = 1.0
REFINE_LOOPS = 5
NEW_KERNELS = ("epipolar_solve_kernel", "epipolar_score_kernel", "epipolar_select_kernel")


# ------------------------------------------------------------------------------------------------------------------
# the scene
# ------------------------------------------------------------------------------------------------------------------
F_PIX, CX, CY, ANGLE, BASELINE = 1000.0, 640.0, 480.0, 0.15, 0.8
# The generator's seed per scene size, chosen with the float64 model alone (test_model_meets_the_caps_... rechecks it): a
# RANSAC of 100 loops over 60 % inliers draws an all-inlier sample with probability 0.82 only, so not every scene serves.
SCENE_SEEDS = {12: 2, 60: 10, 400: 0}


def cameras():
    """(R, t, F): X2 = R X1 + t for a second camera at (BASELINE, 0, 0) turned ANGLE about y; F = K^-T [t]x R K^-1."""
    c, s = np.cos(ANGLE), np.sin(ANGLE)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    t = -R @ np.array([BASELINE, 0.0, 0.0])
    K = np.array([[F_PIX, 0, CX], [0, F_PIX, CY], [0, 0, 1.0]])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    return R, t, Ki.T @ tx @ R @ Ki


@functools.lru_cache(maxsize=None)
def scene(n_in, n_out, seed=None):
    """Matched keypoints of two 1280 x 960 views of a NON-PLANAR scene plus gross outliers: (records, planted mask).
    3-D points with x in [-3, 3], y in [-2, 2], z in [3, 12] that both cameras see, 0.3 px of noise in both images."""
    rng = np.random.default_rng(SCENE_SEEDS.get(n_in, n_in) if seed is None else seed)
    R, t, _ = cameras()
    p1, p2 = np.zeros((0, 2)), np.zeros((0, 2))
    while len(p1) < n_in:
        X = rng.uniform([-3, -2, 3], [3, 2, 12], size=(4 * n_in, 3))
        X2 = X @ R.T + t
        a = F_PIX * X[:, :2] / X[:, 2:] + [CX, CY]
        b = F_PIX * X2[:, :2] / X2[:, 2:] + [CX, CY]
        ok = ((a >= 0) & (a < [1280, 960]) & (b >= 0) & (b < [1280, 960])).all(axis=1)
        p1, p2 = np.r_[p1, a[ok]], np.r_[p2, b[ok]]
    p1 = p1[:n_in] + rng.normal(0, 0.3, size=(n_in, 2))
    p2 = p2[:n_in] + rng.normal(0, 0.3, size=(n_in, 2))
    p1 = np.r_[p1, rng.uniform([0, 0], [1280, 960], size=(n_out, 2))]
    p2 = np.r_[p2, rng.uniform([0, 0], [1280, 960], size=(n_out, 2))]
    n = n_in + n_out
    perm = rng.permutation(n)
    pts = np.zeros(n, dtype=SIFT_POINT_DTYPE)
    pts["coords2D"] = p1[perm].astype(np.float32)
    pts["match_xpos"], pts["match_ypos"] = p2[perm, 0].astype(np.float32), p2[perm, 1].astype(np.float32)
    pts["score"], pts["ambiguity"] = 0.9, 0.5  # pass rule 0 at lo = 0.85, hi = 0.95
    pts["match"] = rng.integers(0, 500, n).astype(np.int32)
    pts["match_error"] = 7.0
    planted = np.zeros(n, dtype=bool)
    planted[:n_in] = True
    pts.setflags(write=False)
    return pts, planted[perm]


def coords(pts, idx=None):
    """float64 (x1, y1, x2, y2) of the records idx, widened from the records' floats as the kernels widen them."""
    sub = pts if idx is None else pts[idx]
    return (sub["coords2D"][:, 0].astype(np.float64), sub["coords2D"][:, 1].astype(np.float64),
            sub["match_xpos"].astype(np.float64), sub["match_ypos"].astype(np.float64))


# ------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------
def sample_loop8(seed, loop, n):
    """Positions in the candidate list of the eight samples of one hypothesis, and the redraws each of p2..p8 took."""
    p = [draw(seed, loop, s, n) for s in range(8)]
    k = 8
    redraws = [0] * 7
    for s in range(1, 8):
        while p[s] in p[:s] and redraws[s - 1] < 64:
            p[s] = draw(seed, loop, k, n)
            k += 1
            redraws[s - 1] += 1
        if p[s] in p[:s]:
            p[s] = min(v for v in range(n) if v not in p[:s])
    return p, redraws


def sample8(seed, n, loops):
    return np.array([sample_loop8(seed, l, n)[0] for l in range(loops)], dtype=np.int32).T.copy()  # [8, loops]


def hartley(x, y):
    cx, cy = x.mean(), y.mean()
    return cx, cy, np.sqrt(2.0) / np.sqrt((x - cx) ** 2 + (y - cy) ** 2).mean()


def system(x1, y1, x2, y2):
    """(A [n, 9], T1, T2) of the normalised correspondences."""
    c1, c2 = hartley(x1, y1), hartley(x2, y2)
    u1, v1, u2, v2 = (x1 - c1[0]) * c1[2], (y1 - c1[1]) * c1[2], (x2 - c2[0]) * c2[2], (y2 - c2[1]) * c2[2]
    A = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], axis=1)
    T = [np.array([[c[2], 0, -c[2] * c[0]], [0, c[2], -c[2] * c[1]], [0, 0, 1.0]]) for c in (c1, c2)]
    return A, T[0], T[1]


def unit(F):
    """Frobenius norm 1, the largest-magnitude entry (the first in row-major order among equals) positive; nine zeros
    for a result that is not finite or all zero."""
    f = np.asarray(F, dtype=np.float64).ravel()
    norm = np.sqrt((f * f).sum())
    if not (np.isfinite(norm) and norm > 0):
        return np.zeros(9)
    f = f / norm
    return -f if f[np.argmax(np.abs(f))] < 0 else f


def solve(x1, y1, x2, y2):
    """(F [9], sigma8 / sigma1 of the normalised system): null vector and rank-2 projection by SVD."""
    with np.errstate(all="ignore"):
        A, T1, T2 = system(x1, y1, x2, y2)
        if not np.isfinite(A).all():
            return np.zeros(9), 0.0
        _, sv, vt = np.linalg.svd(A)
        U, S, Vt = np.linalg.svd(vt[-1].reshape(3, 3))
        S[2] = 0.0
        return unit(T2.T @ (U * S) @ Vt @ T1), float(sv[7] / sv[0]) if sv[0] > 0 else 0.0


def sampson(F, x1, y1, x2, y2):
    """(e * e, den) of the pinned expressions, in float64 operation for operation."""
    l0 = (F[0] * x1 + F[1] * y1) + F[2]
    l1 = (F[3] * x1 + F[4] * y1) + F[5]
    l2 = (F[6] * x1 + F[7] * y1) + F[8]
    m0 = (F[0] * x2 + F[3] * y2) + F[6]
    m1 = (F[1] * x2 + F[4] * y2) + F[7]
    e = (x2 * l0 + y2 * l1) + l2
    den = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1
    return e * e, den


def inliers(F, xy, thresh):
    t2 = float(np.float32(thresh)) * float(np.float32(thresh))
    with np.errstate(all="ignore"):
        e2, den = sampson(F, *xy)
        return e2 < t2 * den


def near_threshold(F, xy, thresh):
    t2 = float(np.float32(thresh)) * float(np.float32(thresh))
    with np.errstate(all="ignore"):
        e2, den = sampson(F, *xy)
        return bool((np.abs(e2 - t2 * den) <= 1e-9 * t2 * den).any())


def refit(F0, xy, rounds, thresh):
    """(F, a candidate came within a relative 1e-9 of the threshold in some round or in the final count)."""
    F, near = np.asarray(F0, dtype=np.float64), False
    for _ in range(rounds):
        near |= near_threshold(F, xy, thresh)
        S = inliers(F, xy, thresh)
        if S.sum() < 8:
            break
        new, _ = solve(*(c[S] for c in xy))
        if not new.any():
            break
        F = new
    return F, near | near_threshold(F, xy, thresh)


def match_error(F, xy):
    with np.errstate(all="ignore"):
        e2, den = sampson(F, *xy)
        return np.sqrt(e2 / den)


def conditioned(pts, drawn):
    """(model F [9, L], well-conditioned mask [L]) of the samples drawn [8, L] (record indices)."""
    out, ok = np.zeros((9, drawn.shape[1])), np.zeros(drawn.shape[1], dtype=bool)
    for l in range(drawn.shape[1]):
        out[:, l], ratio = solve(*coords(pts, drawn[:, l]))
        ok[l] = ratio >= 1e-3
    return out, ok


def eight_of(pts, good):
    """A copy in which only eight records, spread over the set, stay candidates under RULE_ARGS[0]."""
    out = pts.copy()
    out["score"] = 0.3
    out["score"][good] = 0.9
    return out


# ------------------------------------------------------------------------------------------------------------------
# without a GPU
# ------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_recipes_agree():
    from cusift_amd import batch, capi

    extras = open(os.path.join(ROOT, "include", "cusift_amd_extras.h")).read()
    front = open(os.path.join(ROOT, "include", "cusift_amd.h")).read()
    handle = C.CDLL(capi.LIB_PATH)
    for name, nargs in (("cusift_estimate_fundamental", 22), ("cusift_register_epipolar", 24)):
        assert "int %s(cusift_ctx *ctx" % name in extras, name
        assert "int %s(" % name not in front, name
        assert hasattr(handle, name), name
        res, args = capi.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs and C.c_uint64 in args, (name, len(args))
    for m in ("estimate_fundamental", "register_epipolar"):
        assert callable(getattr(capi.Context, m))
    assert callable(batch.BatchExtractor.register_epipolar)
    make = open(os.path.join(ROOT, "Makefile")).read()
    assert "sift_epipolar" in make.split("SOURCES :=")[1].split("HEADERS")[0] and "cpp_epipolar" in make
    assert "tests/cpp_epipolar/epipolar_dropin.cpp" in open(os.path.join(ROOT, "CMakeLists.txt")).read()
    assert "tests/cpp_epipolar/epipolar_dropin" in open(os.path.join(ROOT, ".gitignore")).read()
    head = open(os.path.join(ROOT, "include", "epipolar.h")).read()
    assert "RegisterEpipolar(SiftData &data1, SiftData &data2" in head and "EstimateFundamental(SiftData &data" in head
    # the pinned expressions stand in the header as they stand in the kernel
    for expr in ("l0 = (F0*x1 + F1*y1) + F2", "den = ((l0*l0 + l1*l1) + m0*m0) + m1*m1", "e*e < t2*den"):
        assert expr in extras, expr


@pytest.mark.parametrize("seed,n,loops", [(0, 8, 300), (1, 9, 300), (0xC0FFEE, 12, 300), (7, 650, 512),
                                          (2 ** 64 - 1, 32768, 1000)])
def test_sampler_gives_eight_distinct_indices(seed, n, loops):
    s = sample8(seed, n, loops)
    assert s.shape == (8, loops) and s.min() >= 0 and s.max() < n
    assert all(len(set(s[:, l])) == 8 for l in range(loops))
    if n >= 650:
        assert len(np.unique(s)) > min(n, 8 * loops) // 4 and not np.array_equal(s[0], s[1])
    assert not np.array_equal(s, sample8(seed ^ 1, n, loops))


def test_sampler_fallback_after_64_redraws():
    """With eight candidates the last slot has one free value and misses it with probability 7 / 8 per redraw, so all 64
    redraws miss in about 1 loop of 5000 (0.875^64): among the first 40 000 loops of seed 0 some take the fallback."""
    hits = 0
    for l in range(40000):
        if draw(0, l, 7, 8) not in [draw(0, l, s, 8) for s in range(7)]:
            continue  # slot 8 was free at once: the common case, cheaply skipped
        p, redraws = sample_loop8(0, l, 8)
        k = 8 + sum(redraws[:6])
        if redraws[6] == 64 and all(draw(0, l, k + t, 8) in p[:7] for t in range(64)):  # every redraw was refused
            hits += 1
            assert sorted(p) == list(range(8)) and p[7] == min(set(range(8)) - set(p[:7]))
    assert hits, "no loop of 40 000 reached the fallback"
    assert all(sorted(sample_loop8(5, l, 8)[0]) == list(range(8)) for l in range(500))


@pytest.mark.parametrize("n_in,n_out,loops", SCENES)
def test_model_meets_the_caps_and_recalls_the_gpu_tests_rely_on(n_in, n_out, loops):
    pts, planted = scene(n_in, n_out)
    assert len(pts) == n_in + n_out and planted.sum() == n_in
    _, _, truth = cameras()
    clean = match_error(unit(truth), coords(pts))[planted]
    assert np.percentile(clean, 90) < 1.0  # the planted geometry is the records' geometry
    cand = candidates(pts, 0, 0.85, 0.95)
    assert len(cand) == len(pts)
    xy = coords(pts, cand)
    skipped = 0
    for seed in SEEDS:
        drawn = cand[sample8(seed, len(cand), loops)]
        F, ok = conditioned(pts, drawn)
        dropped = 1.0 - ok.mean()
        counts = np.array([inliers(F[:, l], xy, THRESH).sum() for l in range(loops)])
        best = int(np.argmax(counts))
        fit, near = refit(F[:, best], xy, REFINE_LOOPS, THRESH)
        recall = float((match_error(fit, coords(pts))[planted] < THRESH).mean())
        nz = F[:, F.any(axis=0)]
        dets = np.abs([np.linalg.det(nz[:, l].reshape(3, 3)) for l in range(nz.shape[1])])
        print("scene %s seed %#x: %.1f %% of the loops dropped, winner %d of %d candidates, recall %.4f, near %s, "
              "|det| <= %.2g" % ((n_in, n_out), seed, 100 * dropped, counts[best], len(cand), recall, near, dets.max()))
        assert dropped <= (0.125 if n_in == 12 else 0.03)
        assert recall >= 0.995  # the GPU tests ask for 0.99: one planted point of 400 beyond 1 px (3.3 sigma) is expected
        assert np.abs(np.sqrt((nz * nz).sum(axis=0)) - 1).max() <= 1e-12 and dets.max() <= 1e-12
        skipped += near
    assert skipped <= 1


def test_epipolar_kernels_compile_for_gfx950_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs

    asm = kernel_regs.assembly("sift_epipolar.hip")
    assert "gfx950" in asm
    ks = {k["name"]: k for k in kernel_regs.kernels(asm)}
    assert len(ks) == 3 and all(any(w in n for n in ks) for w in NEW_KERNELS), sorted(ks)
    for n, k in ks.items():
        print("%s: %d VGPRs, %d AGPRs, %d bytes of scratch, %d bytes of LDS" %
              (n[:40], k["vgpr_count"], k["agpr_count"], k["private_segment_fixed_size"], k["group_segment_fixed_size"]))
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
    mnemonics = [line.split()[0] for line in asm.splitlines() if line.startswith("\t") and line.split()]
    atomics = [m for m in mnemonics if "atomic" in m]
    assert atomics and all(m.startswith("global_atomic_add") and "_f" not in m for m in atomics), atomics
    assert any(m.startswith("v_mul_f64") for m in mnemonics) and any(m.startswith("v_sqrt_f64") or
                                                                     m.startswith("v_rsq_f64") for m in mnemonics)
    text = open(os.path.join(ROOT, "cusift_amd", "csrc", "sift_epipolar.hip")).read()
    assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", text, flags=re.M)


# ------------------------------------------------------------------------------------------------------------------
# on the GPU
# ------------------------------------------------------------------------------------------------------------------
def run(ctx, pts, n2=-1, **kw):
    """estimate_fundamental on a fresh upload; returns (result, the records afterwards)."""
    buf = upload(ctx, np.ascontiguousarray(pts))
    kw.setdefault("want_all", True)
    kw.setdefault("thresh", THRESH)
    kw.setdefault("refine_thresh", THRESH)
    kw.setdefault("refine_loops", REFINE_LOOPS)
    res = ctx.estimate_fundamental(buf.ptr, len(pts), n2, **kw)
    after = buf.to_numpy(SIFT_POINT_DTYPE, (len(pts),))
    buf.free()
    return res, after


RESULTS = {}


def scene_run(ctx, n_in, n_out, loops, seed):
    """One device run per (scene, seed), shared by the tests below."""
    key = (n_in, n_out, loops, seed)
    if key not in RESULTS:
        RESULTS[key] = run(ctx, scene(n_in, n_out)[0], loops=loops, seed=seed, **RULE_ARGS[0])
    return RESULTS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("seed", SEEDS)
def test_samples_and_candidates_equal_the_restatement(ctx, rule, seed):
    pts = subset_scores(scene(400, 250)[0], rule, seed & 0xFFFF)
    n2 = 500 if rule == 1 else -1
    want = candidates(pts, rule, RULE_ARGS[rule]["lo"], RULE_ARGS[rule]["hi"], n2)
    assert 8 <= len(want) < len(pts)
    res, _ = run(ctx, pts, n2, loops=512, seed=seed, **RULE_ARGS[rule])
    assert res.num_candidates == len(want)
    assert np.array_equal(res.drawn, want[sample8(seed, len(want), 512)])
    assert set(np.unique(res.drawn)) == set(want.tolist())  # 4096 draws from ~350: every candidate is drawn somewhere


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_eight_candidates_among_300_records(ctx, seed):
    """Every loop is a permutation of the same eight records: the redraws and, in some loops, the fallback decide it."""
    base = scene(200, 100)[0]
    good = np.array([3, 41, 77, 120, 166, 201, 250, 299])
    pts = eight_of(base, good)
    res, after = run(ctx, pts, loops=512, seed=seed, **RULE_ARGS[0])
    assert res.num_candidates == 8
    assert np.array_equal(res.drawn, good[sample8(seed, 8, 512)].astype(np.int32))
    assert (np.sort(res.drawn, axis=0) == good[:, None]).all()
    xy = coords(pts, good)
    counts = np.array([inliers(res.all_fundamentals[:, l], xy, THRESH).sum() for l in range(512)])
    assert np.array_equal(res.all_counts, counts) and res.all_counts.max() <= 8
    assert not res.inliers[np.setdiff1d(np.arange(300), good)].any()  # a record that is no candidate is no inlier


@pytest.mark.gpu
@pytest.mark.parametrize("n_in,n_out,loops", SCENES)
@pytest.mark.parametrize("seed", SEEDS)
def test_counts_flags_and_winner_equal_the_pinned_test_on_the_devices_own_matrices(ctx, n_in, n_out, loops, seed):
    pts, _ = scene(n_in, n_out)
    res, _ = scene_run(ctx, n_in, n_out, loops, seed)
    cand = candidates(pts, 0, 0.85, 0.95)
    assert res.num_candidates == len(cand) and np.array_equal(res.drawn, cand[sample8(seed, len(cand), loops)])
    xy = coords(pts, cand)
    counts = np.array([inliers(res.all_fundamentals[:, l], xy, THRESH).sum() for l in range(loops)], dtype=np.int32)
    assert np.array_equal(res.all_counts, counts)  # every loop, exactly: another expression order moves some count
    assert res.best_loop == int(np.argmax(counts)) and res.num_matches == counts.max()
    assert res.ransac.tobytes() == res.all_fundamentals[:, res.best_loop].tobytes()
    flags = np.zeros(len(pts), dtype=bool)
    flags[cand] = inliers(res.ransac, xy, THRESH)
    assert np.array_equal(res.inliers, flags) and res.inliers.sum() == res.num_matches
    assert res.num_matches >= 8 and res.num_matches >= 0.5 * n_in


@pytest.mark.gpu
@pytest.mark.parametrize("n_in,n_out,loops", SCENES)
def test_hypotheses_equal_the_svd_model(ctx, n_in, n_out, loops):
    pts, _ = scene(n_in, n_out)
    worst = 0.0
    for seed in SEEDS:
        res, _ = scene_run(ctx, n_in, n_out, loops, seed)
        want, ok = conditioned(pts, res.drawn)
        assert 1.0 - ok.mean() <= 0.15, (seed, 1.0 - ok.mean())
        diff = np.abs(res.all_fundamentals - want).max(axis=0)
        worst = max(worst, float(diff[ok].max()))
        nz = res.all_fundamentals[:, res.all_fundamentals.any(axis=0)]
        assert np.isfinite(res.all_fundamentals).all() and nz.shape[1] >= ok.sum()
        norms = np.sqrt((nz * nz).sum(axis=0))
        dets = np.abs([np.linalg.det(nz[:, l].reshape(3, 3)) for l in range(nz.shape[1])])
        print("scene %s seed %#x: %d of %d loops compared, largest difference %.3g; | |F| - 1 | <= %.3g, |det| <= %.3g" %
              ((n_in, n_out), seed, ok.sum(), loops, diff[ok].max(), np.abs(norms - 1).max(), dets.max()))
        assert np.abs(norms - 1).max() <= 1e-12 and dets.max() <= 1e-12
    print("scene %s: largest difference over the seeds %.3g" % ((n_in, n_out), worst))
    assert worst <= 1e-6, worst


@pytest.mark.gpu
@pytest.mark.parametrize("n_in,n_out,loops", SCENES)
def test_refit_equals_the_model_from_the_devices_winner(ctx, n_in, n_out, loops):
    pts, planted = scene(n_in, n_out)
    cand = candidates(pts, 0, 0.85, 0.95)
    xy, skipped = coords(pts, cand), 0
    for seed in SEEDS:
        res, after = scene_run(ctx, n_in, n_out, loops, seed)
        want, near = refit(res.ransac, xy, REFINE_LOOPS, THRESH)
        if near:
            skipped += 1
            continue
        diff = float(np.abs(res.fundamental - want).max())
        err = match_error(res.fundamental, coords(pts))
        rel = float((np.abs(after["match_error"].astype(np.float64) - err) / err).max())
        recall = float((after["match_error"][planted] < THRESH).mean())
        print("scene %s seed %#x: refit differs by %.3g, match_error by %.3g relative, num_fit %d, recall %.4f" %
              ((n_in, n_out), seed, diff, rel, res.num_fit, recall))
        assert diff <= 1e-6, diff
        assert res.num_fit == inliers(res.fundamental, xy, THRESH).sum() == inliers(want, xy, THRESH).sum()
        assert rel <= 1e-5
        assert recall >= 0.99
        rest = after.copy()
        rest["match_error"] = pts["match_error"]
        assert rest.tobytes() == pts.tobytes()  # nothing else of the records moved
    assert skipped <= 1


@pytest.mark.gpu
def test_same_seed_same_bytes_other_seed_other_samples_and_no_refit(ctx):
    pts, _ = scene(400, 250)
    kw = dict(loops=512, **RULE_ARGS[0])
    a, rec_a = run(ctx, pts, seed=5, **kw)
    b, rec_b = run(ctx, pts, seed=5, **kw)
    for u, v in zip(a, b):
        assert np.asarray(u).tobytes() == np.asarray(v).tobytes()
    assert rec_a.tobytes() == rec_b.tobytes()
    c, _ = run(ctx, pts, seed=6, **kw)
    assert not np.array_equal(a.drawn, c.drawn)
    d, rec_d = run(ctx, pts, seed=5, refine_loops=0, **kw)
    assert d.fundamental.tobytes() == d.ransac.tobytes() == a.ransac.tobytes() and d.num_matches == a.num_matches
    assert d.num_fit == d.num_matches  # the same test at the same threshold with the same matrix
    assert a.fundamental.tobytes() != a.ransac.tobytes()


@pytest.mark.gpu
def test_edges_and_refusals(ctx):
    from cusift_amd import capi

    pts = scene(60, 40)[0].copy()
    # seven candidates: zeros, zero counts, CUSIFT_OK, the records untouched
    seven = eight_of(pts, np.array([1, 5, 9, 13, 20, 30, 44]))
    res, after = run(ctx, seven, loops=64, seed=3, **RULE_ARGS[0])
    assert res.num_candidates == 7 and res.num_matches == 0 and res.num_fit == 0 and res.best_loop == 0
    assert not res.fundamental.any() and not res.ransac.any() and not res.inliers.any()
    assert not res.all_counts.any() and not res.drawn.any() and not res.all_fundamentals.any()
    assert after.tobytes() == seven.tobytes()
    # seven records
    res, after = run(ctx, pts[:7], loops=64, seed=3, **RULE_ARGS[0])
    assert res.num_candidates == 0 and res.num_matches == 0 and not res.fundamental.any() and not res.ransac.any()
    assert after.tobytes() == pts[:7].tobytes()

    # refusals: nothing enqueued, nothing written
    buf = upload(ctx, pts)
    fun, ran = np.full(9, 9.0), np.full(9, 9.0)
    ints = [C.c_int(-7) for _ in range(4)]
    extra = np.full(8 * 64, -7, np.int32)

    def call(rule=0, lo=0.0, hi=0.8, loops=64, th=1.0, rl=5, rth=1.0, h=fun, r=ran, pc=0, pm=1, pf=2, data=buf.ptr):
        p = [C.byref(v) for v in ints]
        return capi.lib().cusift_estimate_fundamental(
            ctx.handle, data, len(pts), -1, rule, lo, hi, loops, th, rl, rth, 1, h.ctypes.data if h is not None else None,
            r.ctypes.data if r is not None else None, p[pc] if pc is not None else None, p[pm] if pm is not None else None,
            p[pf] if pf is not None else None, p[3], None, extra.ctypes.data, None, None)

    nan = float("nan")
    for kw in (dict(h=None), dict(r=None), dict(pc=None), dict(pm=None), dict(pf=None), dict(loops=0), dict(loops=-3),
               dict(th=0.0), dict(th=-1.0), dict(th=nan), dict(rth=0.0), dict(rth=nan), dict(lo=nan), dict(hi=nan),
               dict(rule=2), dict(rule=-1), dict(rl=-1), dict(data=None)):
        assert call(**kw) == -1, kw  # CUSIFT_ERR_INVALID
        assert (fun == 9.0).all() and (ran == 9.0).all() and all(v.value == -7 for v in ints) and (extra == -7).all(), kw
        assert buf.to_numpy(SIFT_POINT_DTYPE, (len(pts),)).tobytes() == pts.tobytes(), kw
    assert call(loops=17) == 0 and ints[0].value == len(pts) and ints[1].value >= 8  # any num_loops >= 1 is accepted; a hypothesis fits its own samples
    # the fused call: its own refusals on top, the records of both frames untouched
    other = upload(ctx, pts)
    p = [C.byref(v) for v in ints]
    fun[:], ran[:] = 9.0, 9.0
    for v in ints:
        v.value = -7

    def fused(d2=other.ptr, n2=len(pts), distance=0, loops=64):
        return capi.lib().cusift_register_epipolar(ctx.handle, buf.ptr, len(pts), d2, n2, distance, 0, 0.0, 0.8, loops, 1.0,
                                                   5, 1.0, 1, fun.ctypes.data, ran.ctypes.data, p[0], p[1], p[2], p[3], None,
                                                   None, None, None)

    before = buf.to_numpy(SIFT_POINT_DTYPE, (len(pts),)).tobytes()
    for kw in (dict(distance=2), dict(distance=-1), dict(d2=None), dict(n2=-1), dict(loops=0)):
        assert fused(**kw) == -1, kw
        assert (fun == 9.0).all() and (ran == 9.0).all() and all(v.value == -7 for v in ints), kw
        assert buf.to_numpy(SIFT_POINT_DTYPE, (len(pts),)).tobytes() == before, kw


@pytest.mark.gpu
@pytest.mark.parametrize("distance,rule_args", [(1, dict(rule=1, lo=999.0, hi=0.8)), (0, dict(rule=0, lo=0.0, hi=0.95)),
                                                (1, dict(rule=1, lo=999.0, hi=0.8, thresh=2.0, refine_thresh=0.75)),
                                                (0, dict(rule=0, lo=0.0, hi=0.95, thresh=2.0, refine_thresh=0.75))])
def test_fused_equals_staged_byte_for_byte(ctx, distance, rule_args):
    """The last two sets carry thresholds of their own, thresh and refine_thresh apart; the others run both at THRESH."""
    s1 = read_vlfeat_sift(os.path.join(GOLDEN, "vlfeat_sift1.bin"))
    s2 = read_vlfeat_sift(os.path.join(GOLDEN, "vlfeat_sift2.bin"))
    kw = dict(loops=512, thresh=THRESH, refine_loops=REFINE_LOOPS, refine_thresh=THRESH, seed=9, want_all=True)
    kw.update(rule_args)
    b1, b2 = upload(ctx, s1), upload(ctx, s2)
    fused = ctx.register_epipolar(b1.ptr, len(s1), b2.ptr, len(s2), distance=distance, **kw)
    f1 = b1.to_numpy(SIFT_POINT_DTYPE, (len(s1),))
    c1, c2 = upload(ctx, s1), upload(ctx, s2)
    ctx.match(c1.ptr, len(s1), c2.ptr, len(s2), distance)
    staged = ctx.estimate_fundamental(c1.ptr, len(s1), len(s2), **kw)
    t1 = c1.to_numpy(SIFT_POINT_DTYPE, (len(s1),))
    print("distance %d: %d candidates, %d inliers, %d fit" % (distance, fused.num_candidates, fused.num_matches, fused.num_fit))
    assert 8 <= fused.num_candidates < len(s1) and fused.num_matches >= 8
    for u, v in zip(fused, staged):
        assert np.asarray(u).tobytes() == np.asarray(v).tobytes()
    assert f1.tobytes() == t1.tobytes() and b2.to_numpy(SIFT_POINT_DTYPE, (len(s2),)).tobytes() == s2.tobytes()
    cand = candidates(t1, rule_args["rule"], rule_args["lo"], rule_args["hi"], len(s2))
    assert np.array_equal(cand[sample8(9, fused.num_candidates, 512)], fused.drawn)
    for b in (b1, b2, c1, c2):
        b.free()


@pytest.mark.gpu
@pytest.mark.parametrize("distance,rule_args", [(1, dict(rule=1, lo=999.0, hi=0.8)), (0, dict(rule=0, lo=0.0, hi=0.95))])
def test_cross_check_keeps_the_mutual_candidates_and_writes_frame_2(distance, rule_args):
    """A context of this test's own, so that the session's shared context is never switched."""
    from cusift_amd import capi
    from test_match_mutual import column_model
    from test_matching_exact import score_matrix

    if capi.device_count() < 1:
        pytest.fail("gpu test selected but no HIP device is visible")
    s1 = read_vlfeat_sift(os.path.join(GOLDEN, "vlfeat_sift1.bin"))
    s2 = read_vlfeat_sift(os.path.join(GOLDEN, "vlfeat_sift2.bin"))
    kw = dict(loops=256, thresh=THRESH, refine_loops=REFINE_LOOPS, refine_thresh=THRESH, seed=4, want_all=True, **rule_args)
    with capi.Context(0) as own:
        b1, b2 = upload(own, s1), upload(own, s2)
        off = own.register_epipolar(b1.ptr, len(s1), b2.ptr, len(s2), distance=distance, **kw)
        assert b2.to_numpy(SIFT_POINT_DTYPE, (len(s2),)).tobytes() == s2.tobytes()
        own.set_cross_check(True)
        c1, c2 = upload(own, s1), upload(own, s2)
        on = own.register_epipolar(c1.ptr, len(s1), c2.ptr, len(s2), distance=distance, **kw)
        f1, f2 = c1.to_numpy(SIFT_POINT_DTYPE, (len(s1),)), c2.to_numpy(SIFT_POINT_DTYPE, (len(s2),))
        # the staged route: cusift_match_mutual, then the estimate told about frame 2 -- which takes no cross-check, so
        # the comparison is of the matcher's bytes
        m1, m2 = upload(own, s1), upload(own, s2)
        own.match_mutual(m1.ptr, len(s1), m2.ptr, len(s2), distance)
        g1, g2 = m1.to_numpy(SIFT_POINT_DTYPE, (len(s1),)), m2.to_numpy(SIFT_POINT_DTYPE, (len(s2),))
        assert f2.tobytes() == g2.tobytes() and f2.tobytes() != s2.tobytes()
        same = f1.copy()
        same["match_error"] = g1["match_error"]
        assert same.tobytes() == g1.tobytes()
        # overlapping ranges are refused before anything is written
        with pytest.raises(capi.CusiftError):
            own.register_epipolar(c1.ptr, len(s1), c1.ptr, len(s1), distance=distance, **kw)
        assert c1.to_numpy(SIFT_POINT_DTYPE, (len(s1),)).tobytes() == f1.tobytes()
        own.set_cross_check(False)
        again = own.register_epipolar(b1.ptr, len(s1), b2.ptr, len(s2), distance=distance, **kw)
        for u, v in zip(off, again):
            assert np.asarray(u).tobytes() == np.asarray(v).tobytes()
    # the documented column side: the best record of frame 1 for every record of frame 2, the lowest on exact ties
    back = column_model(score_matrix(s1["data"], s2["data"], distance, exact=False), distance)[2]
    m = f1["match"]
    ok = (m >= 0) & (m < len(s2))
    mutual = ok & (back[np.where(ok, m, 0)] == np.arange(len(s1)))
    assert np.array_equal(mutual, ok & (f2["match"][np.where(ok, m, 0)] == np.arange(len(s1))))
    by_rule = candidates(f1, rule_args["rule"], rule_args["lo"], rule_args["hi"], len(s2))
    cand = by_rule[mutual[by_rule]]
    print("distance %d: %d candidates by the rule, %d of them mutual" % (distance, len(by_rule), len(cand)))
    assert 8 <= len(cand) < len(by_rule) == off.num_candidates
    assert on.num_candidates == len(cand) and np.array_equal(on.drawn, cand[sample8(4, len(cand), 256)])
    assert not on.inliers[~mutual].any()


def ground_truth_pair():
    """(F of the fixture pair from its intrinsics and MATLAB's Rt, MATLAB's matches as pixel coordinates).  Rt maps frame
    2 into frame 1, X1 = R X2 + t, so X2 = R^T X1 - R^T t; the intrinsics are 1-based (pixel u sits at u + 1)."""
    from test_rgbd import intrinsics, read_match_points, read_rt

    fx, fy, cx, cy = intrinsics()
    K = np.array([[fx, 0, cx - 1.0], [0, fy, cy - 1.0], [0, 0, 1.0]])
    Rt = read_rt()
    R, t = Rt[:, :3].T, -Rt[:, :3].T @ Rt[:, 3]
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    P = read_match_points()
    a = P[:, :2] / P[:, 2:3] * [fx, fy] + [cx - 1.0, cy - 1.0]
    b = P[:, 3:5] / P[:, 5:6] * [fx, fy] + [cx - 1.0, cy - 1.0]
    return unit(Ki.T @ tx @ R @ Ki), (a[:, 0], a[:, 1], b[:, 0], b[:, 1])


def test_ground_truth_of_the_real_pair_fits_its_matches():
    F, xy = ground_truth_pair()
    err = match_error(F, xy)
    print("MATLAB's %d matches under the ground-truth F: median Sampson distance %.3f px, 90 %% below %.3f px" %
          (len(err), np.median(err), np.percentile(err, 90)))
    assert np.median(err) < 2.0


@pytest.mark.gpu
def test_real_pair_stays_close_to_the_ground_truth(ctx):
    """register_epipolar on the VLFeat fixture pair: over MATLAB's matches the device's F keeps the median Sampson
    distance within twice the ground truth's own median or 1 px, whichever is larger."""
    F, xy = ground_truth_pair()
    truth = float(np.median(match_error(F, xy)))
    s1 = read_vlfeat_sift(os.path.join(GOLDEN, "vlfeat_sift1.bin"))
    s2 = read_vlfeat_sift(os.path.join(GOLDEN, "vlfeat_sift2.bin"))
    b1, b2 = upload(ctx, s1), upload(ctx, s2)
    res = ctx.register_epipolar(b1.ptr, len(s1), b2.ptr, len(s2), distance=1, loops=2000, thresh=THRESH,
                                refine_loops=REFINE_LOOPS, refine_thresh=THRESH, seed=21)
    b1.free()
    b2.free()
    got = float(np.median(match_error(res.fundamental, xy)))
    print("median Sampson distance over MATLAB's matches: ground truth %.3f px, device %.3f px (%d candidates, %d fit)" %
          (truth, got, res.num_candidates, res.num_fit))
    assert got <= max(2.0 * truth, 1.0), (got, truth)
