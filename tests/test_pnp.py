"""Absolute pose on the device (cusift_amd/csrc/sift_pnp.hip): cusift_estimate_pnp, cusift_register_pnp,
BatchExtractor.register_pnp.  tests/test_pnp_sizes.py runs the same comparison where a scoring split holds several tiles,
tests/test_pnp_dropin.py runs include/pnp.h's EstimatePnP / RegisterPnP.

The yardstick is `pnp_model`, a float64 numpy restatement of the definition in include/cusift_amd_extras.h, written in
this file and fitted to nothing the kernels return: the sampler, the 11 x 12 system and its elimination with complete
pivoting in the kernel's order, numpy.linalg.eigh where the header says Jacobi, the pinned inlier test, the Gauss-Newton
rounds with numpy.linalg.solve where the header says Cholesky.
  * DEVICE = MODEL.  h_drawn equals the model's samples exactly.  Recounted with the pinned test from the device's own
    h_all_rt, every entry of h_all_counts, num_matches, best_loop and the flags are exactly equal; from the device's own
    h_rt, num_fit and match_error of every record (the model's float) are exactly equal.  The model's refit, run from the
    device's winner, reproduces h_rt within 1e-9 max-abs (the pose tests' bound: fp64 eps times the condition of a 6 x 6
    normal matrix in pixel units).  A seed is skipped only when, in the model, a candidate lies within a relative 1e-9 of
    the refit's threshold in some round; at most one per scene.  The winning hypothesis itself equals the model's within
    1e-6: the same operations in the same order up to the eigen-solver.
    Measured on an MI355X over the five geometries, the fixture and tests/test_pnp_sizes.py: the winning hypothesis within
    1.0e-15 of the model's, [R | t] within 3.2e-16 of the model's refit; no seed skipped.
  * TRUTH.  ROT_BOUND and TRANS_BOUND are twice the worst error the model makes from its own RANSAC over the GPU tests'
    scenes, seeds and loop counts (test_model_stays_inside_the_truth_bounds prints every figure and holds the model
    to them): worst rotation error 0.03252 degrees, worst translation error 0.334 % of |t|, both on `shallow`.
  * CHAIN.  Three planted views: register_pose(1, 0) writes coords3D at the scale of the first baseline, register_pnp(1,
    2) then returns |t| in that unit.  CHAIN_BOUND is twice the model chain's worst relative error of the ratio (0.000069).
"""
import collections
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

from oracle_binding import SIFT_POINT_DTYPE, read_vlfeat_sift
from test_planar import candidates, draw, upload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW_KERNELS = ("pnp_mark_kernel", "pnp_solve_kernel", "pnp_score_kernel", "pnp_select_kernel")
LOOPS, SEEDS = 2048, (1, 0xC0FFEE)
THRESH, REFINE_THRESH, REFINE_LOOPS = 3.0, 2.0, 5
RULE = dict(rule=0, lo=0.85, hi=0.95)
# the model's worst over GEOMETRIES x SEEDS (test_model_stays_inside_the_truth_bounds), rounded up: degrees, share of |t|
MODEL_ROT, MODEL_TRANS = 0.0326, 0.00334
ROT_BOUND, TRANS_BOUND = 2 * MODEL_ROT, 2 * MODEL_TRANS
# the model chain's worst relative error of |t_pnp| against the planted ratio (test_model_chain_keeps_the_scale), rounded up
MODEL_CHAIN = 0.00007
CHAIN_BOUND = 2 * MODEL_CHAIN
IDENT = np.hstack([np.eye(3), np.zeros((3, 1))])


# ------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------
def sample_loop6(seed, loop, n):
    """Positions in the candidate list of the six samples of one hypothesis (the homography recipe with six slots)."""
    p = [draw(seed, loop, s, n) for s in range(6)]
    k = 6
    for s in range(1, 6):
        redraws = 0
        while p[s] in p[:s] and redraws < 64:
            p[s] = draw(seed, loop, k, n)
            k += 1
            redraws += 1
        if p[s] in p[:s]:
            p[s] = min(v for v in range(n) if v not in p[:s])
    return p


def sample6(seed, n, loops):
    return np.array([sample_loop6(seed, l, n) for l in range(loops)], dtype=np.int32).T.copy()  # [6, loops]


def pnp_candidates(pts, rule, lo, hi, n2=-1):
    cand = candidates(pts, rule, lo, hi, n2)
    c3 = pts["coords3D"][cand]
    return cand[np.isfinite(c3).all(axis=1) & (c3[:, 2] != 0)]


def cam_of(cam):
    """(fx, fy, px, py) in float64 from a (fx, fy, cx, cy, origin) whose floats are widened first."""
    fx, fy, cx, cy, origin = (float(np.float32(v)) for v in cam)
    return fx, fy, cx - origin, cy - origin


def coords5(pts, idx=None):
    """float64 (X, Y, Z, x2, y2) of the records idx, widened from the records' floats as the kernels widen them."""
    sub = pts if idx is None else pts[idx]
    c3 = sub["coords3D"].astype(np.float64)
    return c3[:, 0], c3[:, 1], c3[:, 2], sub["match_xpos"].astype(np.float64), sub["match_ypos"].astype(np.float64)


def terms(rt, k, c5):
    """(a, b, c, e2, den) of the pinned test; rt [12] or [12, L] against points [n] -> [n] or [n, L]."""
    fx, fy, px, py = k
    X, Y, Z, x2, y2 = c5
    rt = np.asarray(rt, dtype=np.float64)
    if rt.ndim == 2:
        X, Y, Z, x2, y2 = (v[:, None] for v in (X, Y, Z, x2, y2))
    with np.errstate(all="ignore"):
        dx, dy, dz = X - rt[3], Y - rt[7], Z - rt[11]
        a = (rt[0] * dx + rt[4] * dy) + rt[8] * dz
        b = (rt[1] * dx + rt[5] * dy) + rt[9] * dz
        c = (rt[2] * dx + rt[6] * dy) + rt[10] * dz
        ex = fx * a - (x2 - px) * c
        ey = fy * b - (y2 - py) * c
        return a, b, c, ex * ex + ey * ey, c * c


def pnp_inliers(rt, k, c5, thresh):
    t2 = float(np.float32(thresh)) * float(np.float32(thresh))
    _, _, c, e2, den = terms(rt, k, c5)
    with np.errstate(all="ignore"):
        return (c > 0) & (e2 < t2 * den)


def near_threshold(rt, k, c5, thresh):
    t2 = float(np.float32(thresh)) * float(np.float32(thresh))
    _, _, c, e2, den = terms(rt, k, c5)
    with np.errstate(all="ignore"):
        return bool(((c > 0) & (np.abs(e2 - t2 * den) <= 1e-9 * t2 * den)).any() or (np.abs(c) <= 1e-9 * np.abs(c5[2])).any())


def match_error(rt, k, c5):
    _, _, c, e2, den = terms(rt, k, c5)
    with np.errstate(all="ignore"):
        return np.where(c > 0, np.sqrt(e2 / den), np.nan).astype(np.float32)


def solve6(k, X, Y, Z, x2, y2):
    """The hypotheses of L sextuples ([L, 6] each) as [12, L]: the header's HYPOTHESIS, in the kernel's order."""
    fx, fy, px, py = k
    L = X.shape[0]
    with np.errstate(all="ignore"):
        u, v = (x2 - px) / fx, (y2 - py) / fy
        cx, cy, cz = (np.add.reduce(w, axis=1) / 6.0 for w in (X, Y, Z))  # add.reduce over 6 sums left to right
        ax, ay, az = X - cx[:, None], Y - cy[:, None], Z - cz[:, None]
        d = np.zeros(L)
        for i in range(6):
            d = d + np.sqrt((ax[:, i] * ax[:, i] + ay[:, i] * ay[:, i]) + az[:, i] * az[:, i])
        s = np.sqrt(3.0) / (d / 6.0)
        xn, yn, zn = ax * s[:, None], ay * s[:, None], az * s[:, None]
        M = np.zeros((L, 12, 12))
        one = np.ones(L)
        for i in range(6):
            M[:, 2 * i, 0:4] = np.stack([xn[:, i], yn[:, i], zn[:, i], one], axis=1)
            M[:, 2 * i, 8:12] = np.stack([-(u[:, i] * xn[:, i]), -(u[:, i] * yn[:, i]), -(u[:, i] * zn[:, i]), -u[:, i]], axis=1)
            M[:, 2 * i + 1, 4:8] = np.stack([xn[:, i], yn[:, i], zn[:, i], one], axis=1)
            M[:, 2 * i + 1, 8:12] = np.stack([-(v[:, i] * xn[:, i]), -(v[:, i] * yn[:, i]), -(v[:, i] * zn[:, i]), -v[:, i]], axis=1)
        M = M[:, :11].copy()
        col = np.tile(np.arange(12), (L, 1))
        rows = np.arange(L)
        for kk in range(11):
            sub = np.abs(M[:, kk:, kk:])
            sub = np.where(np.isnan(sub), -1.0, sub).reshape(L, -1)
            flat = np.argmax(sub, axis=1)  # the first of the largest, row by row
            pi, pj = kk + flat // (12 - kk), kk + flat % (12 - kk)
            a, b = M[rows, kk].copy(), M[rows, pi].copy()
            M[rows, kk], M[rows, pi] = b, a
            a, b = M[rows, :, kk].copy(), M[rows, :, pj].copy()
            M[rows, :, kk], M[rows, :, pj] = b, a
            a, b = col[rows, kk].copy(), col[rows, pj].copy()
            col[rows, kk], col[rows, pj] = b, a
            f = M[:, kk + 1:, kk] / M[:, kk, kk][:, None]
            M[:, kk + 1:, kk + 1:] -= f[:, :, None] * M[:, kk, kk + 1:][:, None, :]
        x = np.zeros((L, 12))
        x[:, 11] = 1.0
        for kk in range(10, -1, -1):
            acc = np.zeros(L)
            for j in range(kk + 1, 12):
                acc = acc + M[:, kk, j] * x[:, j]
            x[:, kk] = -acc / M[:, kk, kk]
        ph = np.zeros((L, 12))
        ph[rows[:, None], col] = x
        ph = ph.reshape(L, 3, 4)
        tx, ty, tz = -(s * cx), -(s * cy), -(s * cz)
        P = np.zeros((L, 3, 4))
        P[:, :, :3] = ph[:, :, :3] * s[:, None, None]
        P[:, :, 3] = ((ph[:, :, 0] * tx[:, None] + ph[:, :, 1] * ty[:, None]) + ph[:, :, 2] * tz[:, None]) + ph[:, :, 3]
        det = (P[:, 0, 0] * (P[:, 1, 1] * P[:, 2, 2] - P[:, 1, 2] * P[:, 2, 1]) -
               P[:, 0, 1] * (P[:, 1, 0] * P[:, 2, 2] - P[:, 1, 2] * P[:, 2, 0])) + \
            P[:, 0, 2] * (P[:, 1, 0] * P[:, 2, 1] - P[:, 1, 1] * P[:, 2, 0])
        P = np.where((det < 0)[:, None, None], -P, P)
        out = np.zeros((12, L))
        Mm = P[:, :, :3]
        ok = np.isfinite(P).all(axis=(1, 2))
        G = np.where(ok[:, None, None], np.einsum("lki,lkj->lij", Mm, Mm), np.eye(3))
        lam, V = np.linalg.eigh(G)  # ascending
        v1, v2 = V[:, :, 2], V[:, :, 1]
        s1, s2 = np.sqrt(np.maximum(lam[:, 2], 0.0)), np.sqrt(np.maximum(lam[:, 1], 0.0))
        v3 = np.cross(v1, v2)
        u1 = np.einsum("lij,lj->li", Mm, v1) / s1[:, None]
        w = np.einsum("lij,lj->li", Mm, v2)
        w = w - (w * u1).sum(axis=1)[:, None] * u1
        u2 = w / np.sqrt((w * w).sum(axis=1))[:, None]
        u3 = np.cross(u1, u2)
        s3 = np.abs((u3 * np.einsum("lij,lj->li", Mm, v3)).sum(axis=1))
        R21 = u1[:, :, None] * v1[:, None, :] + u2[:, :, None] * v2[:, None, :] + u3[:, :, None] * v3[:, None, :]
        scale = ((s1 + s2) + s3) / 3.0
        t21 = P[:, :, 3] / scale[:, None]
        rt = np.zeros((L, 3, 4))
        rt[:, :, :3] = np.transpose(R21, (0, 2, 1))
        rt[:, :, 3] = -np.einsum("lji,lj->li", R21, t21)
        good = ok & (scale > 0) & np.isfinite(rt).all(axis=(1, 2))
        out[:, good] = rt[good].reshape(-1, 12).T
        return out


def gn_round(rt, k, c5, thresh):
    """One Gauss-Newton round of the header's REFIT: (the new pose or None where the refit ends, |S|)."""
    fx, fy, px, py = k
    member = pnp_inliers(rt, k, c5, thresh)
    if member.sum() < 6:
        return None, int(member.sum())
    X, Y, Z, x2, y2 = (v[member] for v in c5)
    a, b, c, _, _ = terms(rt, k, (X, Y, Z, x2, y2))
    xs, ys = x2 - px, y2 - py
    ic = 1.0 / c
    ua, vb = a * ic, b * ic
    g0 = fx * ic
    g2 = -(g0 * ua)
    h1 = fy * ic
    h2 = -(h1 * vb)
    ru, rv = fx * ua - xs, fy * vb - ys
    zero = np.zeros_like(a)
    Ju = np.stack([g2 * b, g0 * c - g2 * a, -(g0 * b), g0, zero, g2], axis=1)
    Jv = np.stack([h2 * b - h1 * c, -(h2 * a), h1 * a, zero, h1, h2], axis=1)
    A = Ju.T @ Ju + Jv.T @ Jv
    g = Ju.T @ ru + Jv.T @ rv
    with np.errstate(all="ignore"):
        try:
            np.linalg.cholesky(A)  # a pivot that is not > 0 ends the refit
            p = np.linalg.solve(A, -g)
        except np.linalg.LinAlgError:
            return None, int(member.sum())
    if not np.isfinite(p).all():
        return None, int(member.sum())
    w, d = p[:3], p[3:]
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = np.sqrt(th2)
    Ac, Bc = (1.0, 0.5) if th2 < 1e-20 else (np.sin(th) / th, (1.0 - np.cos(th)) / th2)
    Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    E = np.eye(3) + Ac * Wx + Bc * (Wx @ Wx)
    R = np.asarray(rt, dtype=np.float64).reshape(3, 4)
    Rn = R[:, :3] @ E.T
    out = np.hstack([Rn, (R[:, 3] - Rn @ d)[:, None]]).ravel()
    return (out if np.isfinite(out).all() else None), int(member.sum())


def refit(rt0, k, c5, rounds, thresh):
    """(the refined pose [12], whether a candidate came within a relative 1e-9 of the threshold in some round)."""
    rt, near = np.asarray(rt0, dtype=np.float64).ravel().copy(), False
    for _ in range(rounds):
        near |= near_threshold(rt, k, c5, thresh)
        new, _ = gn_round(rt, k, c5, thresh)
        if new is None:
            break
        rt = new
    return rt, near | near_threshold(rt, k, c5, thresh)


Model = collections.namedtuple("Model", "rt ransac num_candidates num_matches num_fit best_loop inliers drawn all_rt "
                                        "all_counts match_error near")


def pnp_model(pts, cam, loops, seed, thresh=THRESH, refine_loops=REFINE_LOOPS, refine_thresh=REFINE_THRESH, rule=0,
              lo=0.85, hi=0.95, n2=-1, start=None):
    """The whole call.  start = (all_rt [12, L], best loop): the hypotheses of a device run in place of the model's own."""
    n, k = len(pts), cam_of(cam)
    cand = pnp_candidates(pts, rule, lo, hi, n2) if n >= 6 else np.zeros(0, np.int32)
    nothing = Model(IDENT.copy(), IDENT.copy(), len(cand), 0, 0, 0, np.zeros(n, bool), np.zeros((6, loops), np.int32),
                    np.zeros((12, loops)), np.zeros(loops, np.int32), None, False)
    if len(cand) < 6:
        return nothing
    drawn = cand[sample6(seed, len(cand), loops)]
    c5 = coords5(pts, cand)
    if start is None:
        all_rt = solve6(k, *(np.stack([v[drawn[i]] for i in range(6)], axis=1) for v in coords5(pts)))
    else:
        all_rt = np.asarray(start, dtype=np.float64)
    counts = np.concatenate([pnp_inliers(all_rt[:, l:l + 256], k, c5, thresh).sum(axis=0)  # 256 loops at a time: memory
                             for l in range(0, loops, 256)]).astype(np.int32)
    best = int(np.argmax(counts))  # among equals the first
    if counts[best] == 0:
        return nothing
    flags = np.zeros(n, bool)
    flags[cand] = pnp_inliers(all_rt[:, best], k, c5, thresh)
    rt, near = refit(all_rt[:, best], k, c5, refine_loops, refine_thresh)
    fit = int(pnp_inliers(rt, k, c5, refine_thresh).sum())
    return Model(rt.reshape(3, 4), all_rt[:, best].reshape(3, 4).copy(), len(cand), int(counts[best]), fit, best, flags,
                 drawn, all_rt, counts, match_error(rt, k, coords5(pts)), near)


def rot_err(Ra, Rb):
    """The angle between two rotations in degrees, 2 asin(|Ra - Rb|_F / (2 sqrt 2)): unlike the arccos of the trace it
    resolves angles below 1e-8."""
    return float(np.degrees(2.0 * np.arcsin(min(1.0, np.sqrt(((Ra - Rb) ** 2).sum()) / (2.0 * np.sqrt(2.0))))))


def truth_errors(rt, R21, t21):
    """(rotation error in degrees, translation error relative to |t|) against the planted pose, in the call's direction."""
    rt = np.asarray(rt).reshape(3, 4)
    t = -R21.T @ t21
    return rot_err(rt[:, :3], R21.T), float(np.sqrt(((rt[:, 3] - t) ** 2).sum()) / np.sqrt(t @ t))


# ------------------------------------------------------------------------------------------------------------------
# the scenes: 400 records in a 640 x 480 view -- 240 planted (depths 2 to 6, 0.3 px of noise in the second image, 40 of
# them with coords3D = 0) and 160 gross outliers
# ------------------------------------------------------------------------------------------------------------------
def about_y(angle):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


CAM = (500.0, 500.0, 320.0, 240.0, 0.0)
# name: (R21, the second camera's centre in frame 1, camera2, (nearest, farthest depth), generator seed)
GEOMETRIES = {
    "forward": (np.eye(3), (0.02, -0.01, 0.5), CAM, (2.0, 6.0), 0),
    "sideways": (about_y(0.03), (0.5, 0.05, 0.0), CAM, (2.0, 6.0), 1),
    "rot20": (about_y(np.radians(20.0)), (1.2, 0.0, 0.1), CAM, (2.0, 6.0), 2),
    "fxfy": (about_y(-0.1) @ about_y(0.02).T, (-0.4, 0.1, 0.15), (520.0, 470.0, 321.0, 241.0, 1.0), (2.0, 6.0), 3),
    "shallow": (about_y(0.08), (0.4, -0.05, 0.05), CAM, (2.0, 2.5), 4),
}
N_IN, N_NODEPTH, N_OUT, W, H = 240, 40, 160, 640, 480
Case = collections.namedtuple("Case", "pts planted cam2 R21 t21")


def project(X, cam):
    fx, fy, px, py = cam_of(cam)
    return np.stack([fx * X[:, 0] / X[:, 2] + px, fy * X[:, 1] / X[:, 2] + py], axis=1)


def frustum(rng, n, depth, cam=CAM):
    fx, fy, px, py = cam_of(cam)
    z = rng.uniform(depth[0], depth[1], n)
    u, v = rng.uniform(0, W, n), rng.uniform(0, H, n)
    return np.stack([(u - px) / fx * z, (v - py) / fy * z, z], axis=1)


@functools.lru_cache(maxsize=None)
def case(name):
    R21, centre, cam2, depth, gen = GEOMETRIES[name]
    t21 = -R21 @ np.array(centre)
    rng = np.random.default_rng(gen)
    X1, x2 = np.zeros((0, 3)), np.zeros((0, 2))
    while len(X1) < N_IN:
        X = frustum(rng, 4 * N_IN, depth)
        X2 = X @ R21.T + t21
        b = project(X2, cam2)
        ok = (X2[:, 2] > 0.1) & ((b >= 0) & (b < [W, H])).all(axis=1)
        X1, x2 = np.r_[X1, X[ok]], np.r_[x2, b[ok]]
    X1, x2 = X1[:N_IN], x2[:N_IN] + rng.normal(0, 0.3, size=(N_IN, 2))
    X1[:N_NODEPTH] = 0.0  # the "no depth" mark: no candidates
    X1 = np.r_[X1, frustum(rng, N_OUT, depth)]
    x2 = np.r_[x2, rng.uniform([0, 0], [W, H], size=(N_OUT, 2))]
    n = N_IN + N_OUT
    perm = rng.permutation(n)
    pts = np.zeros(n, dtype=SIFT_POINT_DTYPE)
    pts["coords3D"] = X1[perm].astype(np.float32)
    pts["coords2D"] = rng.uniform([0, 0], [W, H], size=(n, 2)).astype(np.float32)
    pts["match_xpos"], pts["match_ypos"] = x2[perm, 0].astype(np.float32), x2[perm, 1].astype(np.float32)
    pts["score"], pts["ambiguity"] = 0.9, 0.5
    pts["match"] = rng.integers(0, 500, n).astype(np.int32)
    pts["match_error"] = 7.0
    planted = np.zeros(n, dtype=bool)
    planted[N_NODEPTH:N_IN] = True
    pts.setflags(write=False)
    return Case(pts, planted[perm], cam2, R21, t21)


MODEL = {}


def model_of(name, seed):
    if (name, seed) not in MODEL:
        c = case(name)
        MODEL[name, seed] = pnp_model(c.pts, c.cam2, LOOPS, seed, **RULE)
    return MODEL[name, seed]


# ---- the chain: three planted views, descriptors that make the matcher's answer known in advance ----
CHAIN_CENTRES = ((-0.45, 0.03, 0.02), (0.7, -0.05, 0.1))  # of view 0 and of view 2, in frame 1
CHAIN_ROT = (about_y(-0.04), about_y(0.06))


@functools.lru_cache(maxsize=None)
def chain_scene():
    """(records of view 1, of view 0, of view 2, planted mask): 300 points of the 2-to-6 frustum that all three views see,
    0.3 px of noise in every image, 100 records whose partners are unrelated points.  Record i of every view carries the
    same descriptor, distinct from all others, so the matcher pairs i with i."""
    rng = np.random.default_rng(7)
    n_in, n_out = 300, 100
    poses = [(R, -R @ np.array(c)) for R, c in zip(CHAIN_ROT, CHAIN_CENTRES)]
    X = np.zeros((0, 3))
    while len(X) < n_in:
        Y = frustum(rng, 4 * n_in, (2.0, 6.0))
        ok = np.ones(len(Y), bool)
        for R, t in poses:
            Z = Y @ R.T + t
            b = project(Z, CAM)
            ok &= (Z[:, 2] > 0.1) & ((b >= 0) & (b < [W, H])).all(axis=1)
        X = np.r_[X, Y[ok]]
    X = X[:n_in]
    n = n_in + n_out
    views = []
    for R, t in [(np.eye(3), np.zeros(3))] + poses:
        p = project(X @ R.T + t, CAM) + rng.normal(0, 0.3, size=(n_in, 2))
        views.append(np.r_[p, rng.uniform([0, 0], [W, H], size=(n_out, 2))])
    desc = rng.uniform(0, 1, size=(n, 128)) ** 4
    desc = (desc / np.sqrt((desc * desc).sum(axis=1))[:, None]).astype(np.float32)
    perm = rng.permutation(n)
    out = []
    for p in views:
        pts = np.zeros(n, dtype=SIFT_POINT_DTYPE)
        pts["coords2D"] = p[perm].astype(np.float32)
        pts["data"] = desc[perm]
        pts["scale"], pts["match"], pts["match_error"] = 2.0, -1, 7.0
        pts.setflags(write=False)
        out.append(pts)
    planted = np.zeros(n, bool)
    planted[:n_in] = True
    return out[0], out[1], out[2], planted[perm]


def chain_ratio():
    a, b = (np.array(c) for c in CHAIN_CENTRES)
    return float(np.sqrt(b @ b) / np.sqrt(a @ a))


def matched(one, other):
    """`one` as the matcher leaves it when record i's partner is record i of `other` (scores: any that pass RULE)."""
    pts = one.copy()
    pts["match"] = np.arange(len(one))
    pts["match_xpos"], pts["match_ypos"] = other["coords2D"][:, 0], other["coords2D"][:, 1]
    pts["score"], pts["ambiguity"] = 0.9, 0.5
    return pts


# ------------------------------------------------------------------------------------------------------------------
# without a GPU
# ------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_carry_the_pnp_calls():
    from cusift_amd import batch, capi

    extras = open(os.path.join(ROOT, "include", "cusift_amd_extras.h")).read()
    front = open(os.path.join(ROOT, "include", "cusift_amd.h")).read()
    handle = C.CDLL(capi.LIB_PATH)
    for name, nargs in (("cusift_estimate_pnp", 23), ("cusift_register_pnp", 25)):
        assert "int %s(cusift_ctx *ctx" % name in extras, name
        assert "int %s(" % name not in front, name
        assert hasattr(handle, name), name
        res, args = capi.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs and args.count(C.POINTER(capi.Camera)) == 1, (name, len(args))
        assert C.c_uint64 in args
    for m in ("estimate_pnp", "register_pnp"):
        assert callable(getattr(capi.Context, m))
    assert callable(batch.BatchExtractor.register_pnp)
    assert capi.PnPResult._fields == ("rt", "ransac", "num_candidates", "num_matches", "num_fit", "best_loop", "inliers",
                                      "drawn", "all_rt", "all_counts")
    make = open(os.path.join(ROOT, "Makefile")).read()
    assert "sift_pnp" in make.split("SOURCES :=")[1].split("HEADERS")[0] and "cpp_pnp" in make
    assert "tests/cpp_pnp/pnp_dropin.cpp" in open(os.path.join(ROOT, "CMakeLists.txt")).read()
    assert "tests/cpp_pnp/pnp_dropin" in open(os.path.join(ROOT, ".gitignore")).read()
    head = open(os.path.join(ROOT, "include", "pnp.h")).read()
    assert "RegisterPnP(SiftData &data1, SiftData &data2, const cusift_camera *camera2, double *Rt, int *numMatches," in head
    assert "EstimatePnP(SiftData &data" in head and "#include <hip" not in head
    # the pinned expressions stand in the header as they stand in the kernels
    for expr in ("ex = fx*a - (x2 - px)*c", "ey = fy*b - (y2 - py)*c", "c > 0 && ex*ex + ey*ey < t2 * (c*c)",
                 "a = (rt[0]*dx + rt[4]*dy) + rt[8]*dz", "c = (rt[2]*dx + rt[6]*dy) + rt[10]*dz",
                 "match_error = (float)sqrt((ex*ex + ey*ey) / (c*c))", "scale = ((s1 + s2) + s3) / 3",
                 "R21[i][j] = (u1[i]*v1[j] + u2[i]*v2[j]) + u3[i]*v3[j]", "g2 = -(g0*ua)", "h2 = -(h1*vb)",
                 "Ju = [g2*b, g0*c - g2*a, -(g0*b), g0, 0, g2]", "Jv = [h2*b - h1*c, -(h2*a), h1*a, 0, h1, h2]"):
        assert expr in extras, expr
    kernels = open(os.path.join(ROOT, "cusift_amd", "csrc", "sift_pnp.hip")).read()
    for expr in ("const double ex = k.fx * a - xs * c;", "const double ey = k.fy * b - ys * c;",
                 "return c > 0.0 && err < t2 * den;", "const double a = (rt[0] * dx + rt[4] * dy) + rt[8] * dz;",
                 "const double c = (rt[2] * dx + rt[6] * dy) + rt[10] * dz;", "const double scale = ((s1 + s2) + s3) / 3.0;",
                 "R21[3 * i + j] = (u1[i] * v1[j] + u2[i] * v2[j]) + u3[i] * v3[j];",
                 "const double ju[6] = {g2 * b, g0 * c - g2 * a, -(g0 * b), g0, 0.0, g2};",
                 "const double jv[6] = {h2 * b - h1 * c, -(h2 * a), h1 * a, 0.0, h1, h2};",
                 "draw_and_gather<6, 5>(", "ransac_winner<true>(counts, num_loops, s_key, best, best_count);",
                 "wave_tree_sum<kPnPSums>(s, s_part, s_sum, tx);"):
        assert expr in kernels, expr
    # the six samples are drawn in the solve front that the PnP and the epipolar chain share
    chain = open(os.path.join(ROOT, "cusift_amd", "csrc", "sift_ransac_chain.h")).read()
    assert "ransac_sample<N>(seed, idx, n, p);" in chain and "template <int N, int kRows>" in chain
    # the scoring grid that tests/test_pnp_sizes.py plans for; tests/test_register_source.py pins the planner and its call
    # (one grid layer per pair); the launch itself, not a comment about it
    host = open(os.path.join(ROOT, "cusift_amd", "csrc", "sift_register.hip")).read()
    host = "\n".join(line.split("//")[0] for line in host.splitlines())
    assert "hipLaunchKernelGGL(pnp_score_kernel, dim3(loop_blocks, splits, n_pairs), dim3(64)" in host


def exact_scene(name, n=60):
    """n records whose match positions are the exact float64 projections of the planted pose (kept as float32 pixels:
    1e-5 px), all candidates."""
    R21, centre, cam2, depth, gen = GEOMETRIES[name]
    t21 = -R21 @ np.array(centre)
    rng = np.random.default_rng(100 + gen)
    X = np.zeros((0, 3))
    while len(X) < n:
        Y = frustum(rng, 4 * n, depth).astype(np.float32).astype(np.float64)
        b = project(Y @ R21.T + t21, cam2)
        X = np.r_[X, Y[((b >= 0) & (b < [W, H])).all(axis=1)]]
    X = X[:n]
    return X, project(X @ R21.T + t21, cam2), R21, t21, cam2


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_model_recovers_a_planted_pose_from_exact_projections(name):
    """From exact data -- float64 pixels, handed to the model's stages directly -- the model (64 hypotheses, the winner, two
    Gauss-Newton rounds) returns the planted pose: rotation (radians) and translation (relative to |t|) within 1e-9, every
    planted record counted at a thousandth of a pixel, [R | t] orthonormal to 1e-12, det(R) > 0.999.  Every single
    hypothesis is a rotation and lies within 1e-6 (a minimal sample's conditioning times fp64 eps; 5e-8 at worst here).
    Two rounds from a pose 2 degrees and 5 % off need two more to return to it."""
    X, x2, R21, t21, cam2 = exact_scene(name)
    k = cam_of(cam2)
    c5 = (X[:, 0], X[:, 1], X[:, 2], x2[:, 0], x2[:, 1])
    drawn = sample6(3, len(X), 64)
    all_rt = solve6(k, *(np.stack([v[drawn[i]] for i in range(6)], axis=1) for v in c5))
    worst_r = worst_t = 0.0
    for l in range(all_rt.shape[1]):
        r, t = truth_errors(all_rt[:, l], R21, t21)
        worst_r, worst_t = max(worst_r, np.radians(r)), max(worst_t, t)
        R = all_rt[:, l].reshape(3, 4)[:, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and np.linalg.det(R) > 0.999
    counts = pnp_inliers(all_rt, k, c5, 0.001).sum(axis=0)
    best = int(np.argmax(counts))
    rt, _ = refit(all_rt[:, best], k, c5, 2, 0.001)
    r, t = truth_errors(rt, R21, t21)
    R = rt.reshape(3, 4)[:, :3]
    print("%s: worst hypothesis %.3g rad, %.3g of |t| from the planted pose; counts %d..%d of %d; the model's answer %.3g rad, "
          "%.3g of |t|" % (name, worst_r, worst_t, counts.min(), counts.max(), len(X), np.radians(r), t))
    assert worst_r <= 1e-6 and worst_t <= 1e-6
    assert counts[best] == len(X) and int(pnp_inliers(rt, k, c5, 0.001).sum()) == len(X)
    assert np.radians(r) <= 1e-9 and t <= 1e-9, (r, t)
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and np.linalg.det(R) > 0.999
    truth = np.hstack([R21.T, (-R21.T @ t21)[:, None]])
    off = np.hstack([truth[:, :3] @ about_y(np.radians(2.0)), (truth[:, 3] * 1.05)[:, None]]).ravel()
    for _ in range(4):
        off, size = gn_round(off, k, c5, 1e6)
        assert size == len(X)
    r, t = truth_errors(off, R21, t21)
    assert np.radians(r) <= 1e-9 and t <= 1e-9, (r, t)


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_model_stays_inside_the_truth_bounds(name):
    """CPU twin of the truth test: the model from its own RANSAC over the GPU tests' scenes, seeds and loop counts.  The
    bounds are twice the worst value measured here over all five geometries and both seeds (the two seeds end in the same
    optimum, so one figure each):
        forward   0.01748 degrees, 0.00245 of |t|      sideways  0.00626 degrees, 0.00224 of |t|
        rot20     0.01129 degrees, 0.00070 of |t|      fxfy      0.00459 degrees, 0.00076 of |t|
        shallow   0.03252 degrees, 0.00334 of |t|
    so MODEL_ROT = 0.0326 degrees, MODEL_TRANS = 0.00334, and the bounds are twice these.  This test holds the model to the
    measured values themselves; the winners before the refit lie 0.11 to 0.22 degrees and 0.4 to 8.9 % off."""
    c = case(name)
    for seed in SEEDS:
        m = model_of(name, seed)
        r, t = truth_errors(m.rt, c.R21, c.t21)
        r0, t0 = truth_errors(m.ransac, c.R21, c.t21)
        print("%s seed %#x: %d candidates, winner %d inliers at %.4f degrees / %.4f of |t|; refined %d fit at %.4f degrees / "
              "%.4f of |t|" % (name, seed, m.num_candidates, m.num_matches, r0, t0, m.num_fit, r, t))
        assert m.num_candidates == N_IN - N_NODEPTH + N_OUT
        assert r <= MODEL_ROT and t <= MODEL_TRANS, (r, t)
        assert m.num_fit >= 0.97 * c.planted.sum() and not m.inliers[~c.planted].sum() > 5
        R = m.rt[:, :3]
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and np.linalg.det(R) > 0.999


def test_dropping_the_origin_or_swapping_the_focal_lengths_moves_the_pose():
    """The camera handling is visible to DEVICE = MODEL at 1e-9: a dropped origin or swapped fx / fy moves [R | t] by more
    than 1e-4."""
    c = case("fxfy")
    right = model_of("fxfy", SEEDS[0])
    fx, fy, cx, cy, origin = c.cam2
    for what, cam in (("origin dropped", (fx, fy, cx, cy, 0.0)), ("fx and fy swapped", (fy, fx, cx, cy, origin))):
        wrong = pnp_model(c.pts, cam, LOOPS, SEEDS[0], **RULE)
        moved = float(np.abs(wrong.rt - right.rt).max())
        print("%s: [R | t] moved by %.3g" % (what, moved))
        assert moved > 1e-4, what


def chain_model(seed):
    """The model chain: the epipolar model and the pose model of tests/test_pose.py write coords3D of view 1, then the
    PnP model registers view 2.  (|t| of the PnP pose, the Model)."""
    from test_epipolar import REFINE_LOOPS as EPI_ROUNDS, refit as epi_refit
    from test_epipolar_edges import model_run
    from test_pose import pose_model

    v1, v0, v2, _ = chain_scene()
    first = matched(v1, v0)
    _, xy, F, _, best = model_run(first, 512, seed)
    fit, _ = epi_refit(F[:, best], xy, EPI_ROUNDS, 1.0)
    pose = pose_model(fit, first, CAM, CAM, thresh=1.0)
    second = matched(v1, v2)
    second["coords3D"] = pose.coords3D
    m = pnp_model(second, CAM, LOOPS, seed, **RULE)
    return float(np.sqrt(m.rt[:, 3] @ m.rt[:, 3])), m


def test_model_chain_keeps_the_scale():
    """CPU twin of the chain test.  Measured: |t| / planted ratio - 1 = 0.000069 for both seeds, so MODEL_CHAIN = 0.00007
    and CHAIN_BOUND is twice that."""
    for seed in SEEDS:
        length, m = chain_model(seed)
        rel = length / chain_ratio() - 1.0
        print("seed %#x: |t| = %.5f against the planted ratio %.5f (%.4f relative), %d candidates, %d fit" %
              (seed, length, chain_ratio(), rel, m.num_candidates, m.num_fit))
        assert abs(rel) <= MODEL_CHAIN and m.num_fit >= 250


def test_pnp_kernels_compile_for_gfx950_without_scratch():
    """The four kernels of sift_pnp.hip and planar_compact_kernel, the fifth of the chain: no scratch, no spills; the solve
    kernel's LDS stays at or below 72 KB."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs

    asm = kernel_regs.assembly("sift_pnp.hip")
    assert "gfx950" in asm
    ks = {k["name"]: k for k in kernel_regs.kernels(asm)}
    assert len(ks) == 4 and all(any(w in n for n in ks) for w in NEW_KERNELS), sorted(ks)
    ks.update({k["name"]: k for k in kernel_regs.kernels(kernel_regs.assembly("sift_planar.hip"))
               if "planar_compact_kernel" in k["name"]})
    assert len(ks) == 5
    for n, k in ks.items():
        print("%s: %d VGPRs, %d AGPRs, %d bytes of scratch, %d bytes of LDS" %
              (n[:40], k["vgpr_count"], k["agpr_count"], k["private_segment_fixed_size"], k["group_segment_fixed_size"]))
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
        if "pnp_solve_kernel" in n:
            assert 11 * 12 * 64 * 8 <= k["group_segment_fixed_size"] <= 72 * 1024
    text = open(os.path.join(ROOT, "cusift_amd", "csrc", "sift_pnp.hip")).read()
    assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", text, flags=re.M)
    assert "__launch_bounds__(kPnPThreads)" in text and "constexpr int kPnPTile = 64;" in text


# ------------------------------------------------------------------------------------------------------------------
# on the GPU
# ------------------------------------------------------------------------------------------------------------------
def camera(cam):
    """capi.Camera of a (fx, fy, cx, cy, origin); units_per_metre and encoding hold what the depth lift would refuse."""
    from cusift_amd import capi

    return capi.Camera(cam[0], cam[1], cam[2], cam[3], cam[4], 0.0, 7)


def run(ctx, pts, cam, n2=-1, **kw):
    """estimate_pnp on a fresh upload; returns (result, the records afterwards)."""
    buf = upload(ctx, pts)
    kw.setdefault("want_all", True)
    kw.setdefault("thresh", THRESH)
    kw.setdefault("refine_thresh", REFINE_THRESH)
    kw.setdefault("refine_loops", REFINE_LOOPS)
    res = ctx.estimate_pnp(buf.ptr, len(pts), camera(cam), n2, **kw)
    after = buf.to_numpy(SIFT_POINT_DTYPE, (len(pts),))
    buf.free()
    return res, after


DEVICE = {}


def device_of(ctx, name, seed):
    if (name, seed) not in DEVICE:
        c = case(name)
        DEVICE[name, seed] = run(ctx, c.pts, c.cam2, loops=LOOPS, seed=seed, **RULE)
    return DEVICE[name, seed]


def check_device_equals_model(res, after, pts, cam, loops, seed, label, thresh=THRESH, refine_thresh=REFINE_THRESH,
                              refine_loops=REFINE_LOOPS, rule=RULE):
    """The assertions of DEVICE = MODEL.  False: the seed is skipped (a candidate on the refit's threshold)."""
    k = cam_of(cam)
    cand = pnp_candidates(pts, rule["rule"], rule["lo"], rule["hi"])
    assert res.num_candidates == len(cand)
    assert np.array_equal(res.drawn, cand[sample6(seed, len(cand), loops)])
    c5 = coords5(pts, cand)
    # recounted from the device's own hypotheses
    want = pnp_model(pts, cam, loops, seed, thresh, refine_loops, refine_thresh, start=res.all_rt, **rule)
    assert np.array_equal(res.all_counts, want.all_counts)
    assert (res.num_matches, res.best_loop) == (want.num_matches, want.best_loop)
    assert np.array_equal(res.inliers, want.inliers)
    assert res.ransac.tobytes() == np.ascontiguousarray(res.all_rt[:, res.best_loop]).tobytes()
    # from the device's own refined pose
    assert res.num_fit == int(pnp_inliers(res.rt.ravel(), k, c5, refine_thresh).sum())
    err = match_error(res.rt.ravel(), k, coords5(pts))
    assert np.array_equal(after["match_error"], err, equal_nan=True)
    rest = after.copy()
    rest["match_error"] = pts["match_error"]
    assert rest.tobytes() == pts.tobytes()  # no other byte of any record moved, coords3D included
    # the winning hypothesis against the model's own solve of the same samples
    own = solve6(k, *(np.stack([v[res.drawn[i, res.best_loop:res.best_loop + 1]] for i in range(6)], axis=1)
                      for v in coords5(pts)))[:, 0]
    d_hyp = float(np.abs(own - res.ransac.ravel()).max())
    d_rt = float(np.abs(want.rt - res.rt).max())
    R = res.rt[:, :3]
    print("%s: %d candidates, winner loop %d with %d inliers, %d fit; winning hypothesis differs from the model's by %.3g, "
          "[R | t] from the model's refit of the device's winner by %.3g%s" %
          (label, len(cand), res.best_loop, res.num_matches, res.num_fit, d_hyp, d_rt, " (near: skipped)" if want.near else ""))
    assert d_hyp <= 1e-6, d_hyp
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and np.linalg.det(R) > 0.999
    if want.near:
        return False
    assert d_rt <= 1e-9, d_rt
    return True


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_device_equals_the_model(ctx, name):
    c = case(name)
    done = 0
    for seed in SEEDS:
        res, after = device_of(ctx, name, seed)
        done += check_device_equals_model(res, after, c.pts, c.cam2, LOOPS, seed, "%s seed %#x" % (name, seed))
    assert done >= len(SEEDS) - 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_pose_is_close_to_the_planted_one(ctx, name):
    c = case(name)
    for seed in SEEDS:
        res, _ = device_of(ctx, name, seed)
        r, t = truth_errors(res.rt, c.R21, c.t21)
        print("%s seed %#x: rotation %.4f degrees, translation %.4f of |t|" % (name, seed, r, t))
        assert r <= ROT_BOUND and t <= TRANS_BOUND, (r, t)


@pytest.mark.gpu
def test_same_seed_same_bytes_and_no_refit(ctx):
    c = case("sideways")
    a, rec_a = run(ctx, c.pts, c.cam2, loops=512, seed=5, **RULE)
    b, rec_b = run(ctx, c.pts, c.cam2, loops=512, seed=5, **RULE)
    for u, v in zip(a, b):
        assert np.asarray(u).tobytes() == np.asarray(v).tobytes()
    assert rec_a.tobytes() == rec_b.tobytes()
    other, _ = run(ctx, c.pts, c.cam2, loops=512, seed=6, **RULE)
    assert not np.array_equal(a.drawn, other.drawn)
    d, _ = run(ctx, c.pts, c.cam2, loops=512, seed=5, refine_loops=0, refine_thresh=THRESH, **RULE)
    assert d.rt.tobytes() == d.ransac.tobytes() == a.ransac.tobytes() and d.num_fit == d.num_matches == a.num_matches
    assert a.rt.tobytes() != a.ransac.tobytes()


def descriptors_make_the_match(pts):
    return np.array_equal(pts["match"], np.arange(len(pts)))


@pytest.mark.gpu
def test_chain_gives_the_third_view_in_units_of_the_first_baseline(ctx):
    """register_pose(1, 0) writes coords3D of view 1 with the first baseline as the unit; register_pnp(1, 2) returns view
    2's pose in that unit, so |t| is the ratio of the two planted baselines.  A two-view pose returns |t| = 1 whatever the
    ratio is (here 1.57) and cannot pass."""
    v1, v0, v2, planted = chain_scene()
    for seed in SEEDS:
        b1, b0, b2 = upload(ctx, v1), upload(ctx, v0), upload(ctx, v2)
        first = ctx.register_pose(b1.ptr, len(v1), b0.ptr, len(v0), camera(CAM), None, distance=0, loops=512, seed=seed,
                                  thresh=1.0, refine_thresh=1.0, **RULE)
        lifted = b1.to_numpy(SIFT_POINT_DTYPE, (len(v1),))
        assert descriptors_make_the_match(lifted) and abs(np.sqrt(first.rt[:, 3] @ first.rt[:, 3]) - 1.0) <= 1e-12
        res = ctx.register_pnp(b1.ptr, len(v1), b2.ptr, len(v2), camera(CAM), distance=0, loops=LOOPS, seed=seed,
                               thresh=THRESH, refine_thresh=REFINE_THRESH, refine_loops=REFINE_LOOPS, **RULE)
        after = b1.to_numpy(SIFT_POINT_DTYPE, (len(v1),))
        for b in (b1, b0, b2):
            b.free()
        assert descriptors_make_the_match(after)
        assert after["coords3D"].tobytes() == lifted["coords3D"].tobytes()  # the matcher and the call leave them alone
        length = float(np.sqrt(res.rt[:, 3] @ res.rt[:, 3]))
        rel = length / chain_ratio() - 1.0
        r = rot_err(res.rt[:, :3], CHAIN_ROT[1].T)
        print("seed %#x: %d of %d records carry a point, %d candidates, %d fit, |t| = %.5f against %.5f (%.4f relative), "
              "rotation %.4f degrees" % (seed, (lifted["coords3D"][:, 2] > 0).sum(), len(v1), res.num_candidates, res.num_fit,
                                         length, chain_ratio(), rel, r))
        assert res.num_candidates == int((lifted["coords3D"][:, 2] > 0).sum()) and res.num_fit >= 250
        assert abs(rel) <= CHAIN_BOUND, rel
        assert abs(length - 1.0) > 0.5  # not a two-view pose's unit baseline


def lifted_pair():
    """The golden pair with coords3D of frame 1 from its depth image (the restated lift) and the camera of frame 2."""
    from test_rgbd import intrinsics, lift

    s1 = read_vlfeat_sift(os.path.join(GOLDEN, "vlfeat_sift1.bin")).copy()
    s2 = read_vlfeat_sift(os.path.join(GOLDEN, "vlfeat_sift2.bin"))
    z = np.load(os.path.join(GOLDEN, "rgbd_depth.npz"))
    s1["coords3D"] = lift(s1["coords2D"], np.ascontiguousarray(z["depth1"]))
    fx, fy, cx, cy = intrinsics()
    return s1, s2, (fx, fy, cx, cy, 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("distance,rule_args", [(1, dict(rule=1, lo=999.0, hi=0.8)), (0, dict(rule=0, lo=0.0, hi=0.95))])
@pytest.mark.parametrize("cross", (False, True))
def test_fused_equals_staged_byte_for_byte(distance, rule_args, cross):
    """register_pnp against match (match_mutual under the cross-check) followed by estimate_pnp, on the golden pair with
    frame 1 lifted from its depth image.  A context of this test's own, so that the shared one is never switched."""
    from cusift_amd import capi

    if capi.device_count() < 1:
        pytest.fail("gpu test selected but no HIP device is visible")
    s1, s2, cam = lifted_pair()
    kw = dict(loops=512, thresh=THRESH, refine_loops=REFINE_LOOPS, refine_thresh=REFINE_THRESH, seed=9, want_all=True)
    kw.update(rule_args)
    with capi.Context(0) as own:
        own.set_cross_check(cross)
        b1, b2 = upload(own, s1), upload(own, s2)
        fused = own.register_pnp(b1.ptr, len(s1), b2.ptr, len(s2), camera(cam), distance=distance, **kw)
        f1, f2 = b1.to_numpy(SIFT_POINT_DTYPE, (len(s1),)), b2.to_numpy(SIFT_POINT_DTYPE, (len(s2),))
        c1, c2 = upload(own, s1), upload(own, s2)
        (own.match_mutual if cross else own.match)(c1.ptr, len(s1), c2.ptr, len(s2), distance)
        m1, m2 = c1.to_numpy(SIFT_POINT_DTYPE, (len(s1),)), c2.to_numpy(SIFT_POINT_DTYPE, (len(s2),))
        if cross:  # the staged estimate takes no cross-check: the comparison is then of the matcher's bytes and the marks
            with pytest.raises(capi.CusiftError):
                own.register_pnp(b1.ptr, len(s1), b1.ptr, len(s1), camera(cam), distance=distance, **kw)
            assert b1.to_numpy(SIFT_POINT_DTYPE, (len(s1),)).tobytes() == f1.tobytes()
            same = f1.copy()
            same["match_error"] = m1["match_error"]
            assert same.tobytes() == m1.tobytes() and f2.tobytes() == m2.tobytes() and f2.tobytes() != s2.tobytes()
            m = f1["match"]
            ok = (m >= 0) & (m < len(s2))
            mutual = ok & (f2["match"][np.where(ok, m, 0)] == np.arange(len(s1)))
            by_rule = pnp_candidates(m1, rule_args["rule"], rule_args["lo"], rule_args["hi"], len(s2))
            cand = by_rule[mutual[by_rule]]
            assert 6 <= len(cand) < len(by_rule) and fused.num_candidates == len(cand)
            assert np.array_equal(fused.drawn, cand[sample6(9, len(cand), 512)]) and not fused.inliers[~mutual].any()
        else:
            staged = own.estimate_pnp(c1.ptr, len(s1), camera(cam), len(s2), **kw)
            t1 = c1.to_numpy(SIFT_POINT_DTYPE, (len(s1),))
            for u, v in zip(fused, staged):
                assert np.asarray(u).tobytes() == np.asarray(v).tobytes()
            assert f1.tobytes() == t1.tobytes() and f2.tobytes() == s2.tobytes()  # d_sift2 is untouched
            cand = pnp_candidates(t1, rule_args["rule"], rule_args["lo"], rule_args["hi"], len(s2))
            assert np.array_equal(cand[sample6(9, fused.num_candidates, 512)], fused.drawn)
        assert f1["coords3D"].tobytes() == s1["coords3D"].tobytes() and f2["coords3D"].tobytes() == s2["coords3D"].tobytes()
        print("distance %d, cross-check %s: %d candidates, %d inliers, %d fit, t = %s" %
              (distance, cross, fused.num_candidates, fused.num_matches, fused.num_fit, fused.rt[:, 3]))
        assert 6 <= fused.num_candidates < len(s1) and fused.num_matches >= 6
        for b in (b1, b2, c1, c2):
            b.free()


def coplanar_scene(thickness=0.0):
    """`sideways` with every point moved along its own ray onto the plane z = 4 (thickness 0), or into a slab of that
    thickness behind it; the planted records' match positions are the exact projections."""
    c = case("sideways")
    pts = c.pts.copy()
    X = pts["coords3D"].astype(np.float64)
    has = X[:, 2] != 0
    depth = 4.0 + thickness * np.random.default_rng(9).uniform(0, 1, has.sum())
    X[has] *= (depth / X[has, 2])[:, None]
    pts["coords3D"] = X.astype(np.float32)
    sel = np.flatnonzero(has & c.planted)
    b = project(pts["coords3D"][sel].astype(np.float64) @ c.R21.T + c.t21, c.cam2)
    pts["match_xpos"][sel], pts["match_ypos"][sel] = b[:, 0].astype(np.float32), b[:, 1].astype(np.float32)
    return pts, c.cam2


@pytest.mark.gpu
def test_degenerate_answers(ctx):
    c = case("sideways")
    cand = pnp_candidates(c.pts, **RULE)
    # five candidates: every other record loses its depth
    five = c.pts.copy()
    five["coords3D"][np.setdiff1d(np.arange(len(five)), cand[[1, 5, 9, 13, 20]])] = 0.0
    for pts, n_cand in ((five, 5), (c.pts[:5], 0), (c.pts[:0], 0)):
        res, after = run(ctx, pts, c.cam2, loops=64, seed=3, **RULE) if len(pts) else (None, None)
        if res is None:
            res = ctx.estimate_pnp(None, 0, camera(c.cam2), loops=64, seed=3, want_all=True, **RULE)
        else:
            assert after.tobytes() == pts.tobytes()  # the records are untouched
        assert (res.num_candidates, res.num_matches, res.num_fit, res.best_loop) == (n_cand, 0, 0, 0)
        assert np.array_equal(res.rt, IDENT) and np.array_equal(res.ransac, IDENT) and not res.inliers.any()
        assert not res.all_counts.any() and not res.drawn.any() and not res.all_rt.any()
    # all coords3D zero
    flat = c.pts.copy()
    flat["coords3D"] = 0.0
    res, after = run(ctx, flat, c.cam2, loops=64, seed=3, **RULE)
    assert res.num_candidates == 0 and np.array_equal(res.rt, IDENT) and after.tobytes() == flat.tobytes()
    # no solvable hypothesis: every candidate is the same point
    same = c.pts.copy()
    same["coords3D"][cand] = same["coords3D"][cand[0]]
    res, after = run(ctx, same, c.cam2, loops=64, seed=3, **RULE)
    assert res.num_candidates == len(cand) and (res.num_matches, res.num_fit, res.best_loop) == (0, 0, 0)
    assert np.array_equal(res.rt, IDENT) and np.array_equal(res.ransac, IDENT) and not res.all_rt.any()
    assert after.tobytes() == same.tobytes()
    # a coplanar scene, and one 1 % thick: CUSIFT_OK, finite outputs, an orthonormal rotation; no promise about the pose
    for thickness in (0.0, 0.04):
        pts, cam = coplanar_scene(thickness)
        res, after = run(ctx, pts, cam, loops=256, seed=3, **RULE)
        R = res.rt[:, :3]
        print("coplanar, thickness %.2f: %d candidates, %d inliers, %d fit, |R R^T - I| = %.3g" %
              (thickness, res.num_candidates, res.num_matches, res.num_fit, np.abs(R @ R.T - np.eye(3)).max()))
        assert np.isfinite(res.rt).all() and np.isfinite(res.ransac).all() and np.isfinite(res.all_rt).all()
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and np.linalg.det(R) > 0.999
        assert res.num_candidates == N_IN - N_NODEPTH + N_OUT and 0 <= res.num_fit <= res.num_candidates


@pytest.mark.gpu
def test_refusals_write_nothing(ctx):
    from cusift_amd import capi

    c = case("sideways")
    pts = c.pts
    buf = upload(ctx, pts)
    rt, ran = np.full(12, 9.0), np.full(12, 9.0)
    ints = [C.c_int(-7) for _ in range(4)]
    extra = np.full(6 * 64, -7, np.int32)
    good = camera(c.cam2)

    def cam_with(**kw):
        v = dict(fx=c.cam2[0], fy=c.cam2[1], cx=c.cam2[2], cy=c.cam2[3], origin=c.cam2[4])
        v.update(kw)
        return capi.Camera(v["fx"], v["fy"], v["cx"], v["cy"], v["origin"], 0.0, 7)

    def call(rule=0, lo=0.0, hi=0.8, loops=64, th=1.0, rl=5, rth=1.0, h=rt, r=ran, pc=0, pm=1, pf=2, data=buf.ptr, cam=good,
             n=len(pts)):
        p = [C.byref(v) for v in ints]
        return capi.lib().cusift_estimate_pnp(
            ctx.handle, data, n, -1, rule, lo, hi, C.byref(cam) if cam is not None else None, loops, th, rl, rth, 1,
            h.ctypes.data if h is not None else None, r.ctypes.data if r is not None else None,
            p[pc] if pc is not None else None, p[pm] if pm is not None else None, p[pf] if pf is not None else None, p[3], None,
            extra.ctypes.data, None, None)

    nan, inf = float("nan"), float("inf")
    for kw in (dict(h=None), dict(r=None), dict(pc=None), dict(pm=None), dict(pf=None), dict(loops=0), dict(loops=-3),
               dict(th=0.0), dict(th=-1.0), dict(th=nan), dict(rth=0.0), dict(rth=nan), dict(lo=nan), dict(hi=nan),
               dict(rule=2), dict(rule=-1), dict(rl=-1), dict(data=None), dict(n=-1), dict(cam=None),
               dict(cam=cam_with(fx=0.0)), dict(cam=cam_with(fy=nan)), dict(cam=cam_with(fx=inf)), dict(cam=cam_with(cx=nan)),
               dict(cam=cam_with(cy=inf)), dict(cam=cam_with(origin=nan))):
        assert call(**kw) == -1, kw  # CUSIFT_ERR_INVALID
        assert (rt == 9.0).all() and (ran == 9.0).all() and all(v.value == -7 for v in ints) and (extra == -7).all(), kw
        assert buf.to_numpy(SIFT_POINT_DTYPE, (len(pts),)).tobytes() == pts.tobytes(), kw
    assert call(loops=17) == 0 and ints[0].value == N_IN - N_NODEPTH + N_OUT  # any num_loops >= 1 is accepted
    # the fused call: its own refusals on top, the records of both frames untouched
    other = upload(ctx, pts)
    p = [C.byref(v) for v in ints]
    rt[:], ran[:] = 9.0, 9.0
    for v in ints:
        v.value = -7

    def fused(d2=other.ptr, n2=len(pts), distance=0, loops=64, cam=good):
        return capi.lib().cusift_register_pnp(ctx.handle, buf.ptr, len(pts), d2, n2, distance, 0, 0.0, 0.8,
                                              C.byref(cam) if cam is not None else None, loops, 1.0, 5, 1.0, 1,
                                              rt.ctypes.data, ran.ctypes.data, p[0], p[1], p[2], p[3], None, None, None, None)

    before = buf.to_numpy(SIFT_POINT_DTYPE, (len(pts),)).tobytes()
    for kw in (dict(distance=2), dict(distance=-1), dict(d2=None), dict(n2=-1), dict(loops=0), dict(cam=None)):
        assert fused(**kw) == -1, kw
        assert (rt == 9.0).all() and (ran == 9.0).all() and all(v.value == -7 for v in ints), kw
        assert buf.to_numpy(SIFT_POINT_DTYPE, (len(pts),)).tobytes() == before, kw
        assert other.to_numpy(SIFT_POINT_DTYPE, (len(pts),)).tobytes() == pts.tobytes(), kw
    buf.free()
    other.free()


@pytest.mark.gpu
def test_batch_extractor_register_pnp_equals_the_context_call(ctx):
    """BatchExtractor.register_pnp hands its slots' records and clamped counts to Context.register_pnp: the same result as
    the context call on copies of those records, and the same bytes in frame i's records afterwards."""
    import torch

    from cusift_amd import batch, capi

    s1, s2, cam = lifted_pair()
    n, cap = min(len(s1), len(s2)), max(len(s1), len(s2))
    stub = batch.BatchExtractor.__new__(batch.BatchExtractor)
    recs = np.zeros((2, cap), dtype=SIFT_POINT_DTYPE)
    recs[0, :len(s1)], recs[1, :len(s2)] = s1, s2
    points = torch.from_numpy(recs.view(np.uint8).reshape(2, cap, 588).copy()).to("cuda")
    counts = torch.tensor([len(s1), len(s2) + 1000], dtype=torch.int32, device="cuda")  # the second is clamped at max_pts
    stub.ctx, stub.max_pts, stub.n, stub.slots = ctx, cap, 2, [(points, counts)]
    kw = dict(distance=1, loops=256, seed=11, want_all=True, thresh=THRESH, refine_thresh=REFINE_THRESH)
    got = stub.register_pnp(0, 1, camera(cam), **kw)
    torch.cuda.synchronize()
    after = points[0].cpu().numpy().reshape(-1).view(SIFT_POINT_DTYPE)[:len(s1)]
    full2 = np.zeros(cap, dtype=SIFT_POINT_DTYPE)
    full2[:len(s2)] = s2
    b1, b2 = upload(ctx, s1), upload(ctx, full2)
    want = ctx.register_pnp(b1.ptr, len(s1), b2.ptr, cap, camera(cam), **kw)
    assert b1.to_numpy(SIFT_POINT_DTYPE, (len(s1),)).tobytes() == after.tobytes()
    for u, v in zip(got, want):
        assert np.asarray(u).tobytes() == np.asarray(v).tobytes()
    assert got.num_candidates >= 6 and n > 0
    b1.free()
    b2.free()


def fixture_records():
    """Records from rgbd_match1_2.bin: frame 1's points as coords3D, frame 2's points projected with rgbd_intrinsics.txt
    (1-based) as the match pixels.  (records, the camera, the fixture's [R | t])."""
    from test_rgbd import intrinsics, read_match_points, read_rt

    m = read_match_points()
    fx, fy, cx, cy = intrinsics()
    cam = (fx, fy, cx, cy, 1.0)
    pts = np.zeros(len(m), dtype=SIFT_POINT_DTYPE)
    pts["coords3D"] = m[:, :3].astype(np.float32)
    b = project(m[:, 3:], cam)
    pts["match_xpos"], pts["match_ypos"] = b[:, 0].astype(np.float32), b[:, 1].astype(np.float32)
    pts["coords2D"] = project(m[:, :3], cam).astype(np.float32)
    pts["score"], pts["ambiguity"], pts["match"], pts["match_error"] = 0.9, 0.5, np.arange(len(m)), 7.0
    return pts, cam, read_rt()


FIXTURE_LOOPS, FIXTURE_SEED = 1024, 1


def fixture_distance(rt, truth):
    return rot_err(rt[:, :3], truth[:, :3]), float(np.sqrt(((rt[:, 3] - truth[:, 3]) ** 2).sum()))


def test_model_on_the_rgbd_fixture():
    """The model's side of the fixture test: 316 of the 326 records fit at 3 px; its distance from rgbd_Rt1_2.bin is
    measured here (0.01980 degrees, 0.725 mm) and doubled for the device's bound."""
    pts, cam, truth = fixture_records()
    m = pnp_model(pts, cam, FIXTURE_LOOPS, FIXTURE_SEED, thresh=3.0, refine_thresh=3.0, **RULE)
    r, t = fixture_distance(m.rt, truth)
    print("fixture: %d records, %d fit at 3 px, %.4f degrees and %.5f m from rgbd_Rt1_2.bin" % (len(pts), m.num_fit, r, t))
    assert len(pts) == 326 and m.num_fit == 316
    assert r <= MODEL_FIXTURE_ROT and t <= MODEL_FIXTURE_T


MODEL_FIXTURE_ROT, MODEL_FIXTURE_T = 0.0199, 0.00073  # the model's distance (degrees, metres), rounded up
FIXTURE_ROT, FIXTURE_T = 2 * MODEL_FIXTURE_ROT, 2 * MODEL_FIXTURE_T


@pytest.mark.gpu
def test_rgbd_fixture_fits(ctx):
    """A plumbing check, not an accuracy test: the fixture's motion is 0.04 degrees and 2 mm, so the identity nearly
    passes.  What it shows is that real 3-D points and real intrinsics (1-based) go through the call: at 3 px at least
    300 of the 326 records fit (the numpy model counts 316), and h_rt stays within twice the model's own distance from
    rgbd_Rt1_2.bin."""
    pts, cam, truth = fixture_records()
    res, after = run(ctx, pts, cam, loops=FIXTURE_LOOPS, seed=FIXTURE_SEED, thresh=3.0, refine_thresh=3.0, **RULE)
    r, t = fixture_distance(res.rt, truth)
    print("fixture: %d candidates, %d inliers, %d fit, %.4f degrees and %.5f m from rgbd_Rt1_2.bin" %
          (res.num_candidates, res.num_matches, res.num_fit, r, t))
    assert res.num_candidates == 326 and res.num_fit >= 300
    assert r <= FIXTURE_ROT and t <= FIXTURE_T
    check_device_equals_model(res, after, pts, cam, FIXTURE_LOOPS, FIXTURE_SEED, "fixture", thresh=3.0, refine_thresh=3.0)
