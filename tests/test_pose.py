"""Calibrated two-view pose on the device (cusift_amd/csrc/sift_pose.hip): cusift_estimate_pose, cusift_register_pose,
BatchExtractor.register_pose.  tests/test_pose_dropin.py runs include/pose.h's EstimatePose / RegisterPose.

The yardstick is a float64 numpy restatement of the definition in include/cusift_amd_extras.h, written in this file and
fitted to nothing the kernels return: E = K2^T (F K1), numpy.linalg.svd for the decomposition (the device runs a 3 x 3
Jacobi on E^T E), U and V completed to proper rotations, the four candidates, the least-squares depths, the vote.  The
scene generators and the fundamental-matrix model are imported from tests/test_epipolar.py and test_epipolar_edges.py.
  * DEVICE = MODEL, from the device's own F: h_rt within 1e-9 max-abs -- fp64 eps times a condition of at most ~1e6 from
    the pixel-scale K; an fp32 restatement would sit near 1e-4 -- sigma within 1e-9 of sigma_1 (sigma_3 of a rank-2 F is
    rounding noise, so the scale is the largest singular value), votes as a sorted multiset (the SVD's sign choices permute
    the candidates), num_front and the zero pattern of coords3D exactly, its values within 1e-5 relative (they are floats).
    A seed is skipped only when, in the model, a record of the fit set lies within a relative 1e-9 of the Sampson
    threshold or of a zero depth; at most one per scene.
    Measured on an MI355X over all ten scenes: [R | t] within 2.2e-15, sigma within 4.2e-16 of sigma_1, coords3D identical.
  * TRUTH: rotation within 0.25 degrees, translation direction within 1.5 degrees -- about 3 x what the model measures
    from the refit of the true F (0.085 / 0.59 degrees at worst over these scenes) -- on the scenes whose geometry fixes
    the pose: two planted scenes, `sideways`, `forward`, `large`, and TWOCAM, a scene seen by two different cameras (f =
    1000, origin 0 against fx = 1400, fy = 1380, another principal point, origin 1), which one shared K cannot replace:
    the CPU twin shows that swapping K1 and K2 breaks the bounds on it (a missed origin, one pixel, is left to DEVICE =
    MODEL).  At least 99 % of the
    planted records carry a point and at least 90 % of those lie within 5 % of the planted 3-D point once scaled by the
    planted baseline; the CPU twin asserts 95 % of the model alone.
The model's own RANSAC route (test_model_meets_the_truth_bounds, these tests' loop counts and seeds) stays inside both
bounds, so they stand as the issue states them.
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
from test_epipolar import REFINE_LOOPS, SCENES, SEEDS, THRESH, cameras, coords, inliers, near_threshold, refit, run, scene
from test_epipolar_edges import GEO_LOOPS, GEO_SEEDS, GEOMETRIES, N_IN, N_OUT, model_run, view_scene
from test_planar import RULE_ARGS, candidates, upload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW_KERNELS = ("pose_vote_kernel", "pose_write_kernel")
ROT_BOUND, DIR_BOUND = 0.25, 1.5  # degrees
STALE = -5.0                      # coords3D before a call: every record is owed an answer


# ------------------------------------------------------------------------------------------------------------------
# the scenes: records, cameras (fx, fy, cx, cy, origin), the planted pose X2 = R21 X1 + t21 and the planted 3-D points
# ------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "pts planted cam1 cam2 loops seeds R21 t21 world")
TWOCAM = ((1000.0, 1000.0, 640.0, 480.0, 0.0), (1400.0, 1380.0, 661.0, 501.0, 1.0))
PLANTED = ("s100", "s650")
GOOD = PLANTED + ("sideways", "forward", "large", "twocam")
ALL = ("s12",) + GOOD + ("cluster", "planar", "rotation")


def kmat(cam):
    fx, fy, cx, cy, origin = (float(np.float32(v)) for v in cam)
    return np.array([[fx, 0, cx - origin], [0, fy, cy - origin], [0, 0, 1.0]])


def replay(seed, n_in, n_out, R, t, f, centre, size, lo, hi, depth_check):
    """The generators of scene() and view_scene() once more, keeping what they drop: (coords2D float32 [n, 2], the
    planted 3-D point of every record in frame-1 coordinates, NaN for an outlier)."""
    rng = np.random.default_rng(seed)
    p1, p2, world = np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 3))
    while len(p1) < n_in:
        X = rng.uniform(lo, hi, size=(4 * n_in, 3))
        X2 = X @ R.T + t
        a = f * X[:, :2] / X[:, 2:] + centre
        b = f * X2[:, :2] / X2[:, 2:] + centre
        ok = ((a >= 0) & (a < size) & (b >= 0) & (b < size)).all(axis=1)
        if depth_check:
            ok &= X2[:, 2] > 0
        p1, p2, world = np.r_[p1, a[ok]], np.r_[p2, b[ok]], np.r_[world, X[ok]]
    p1 = p1[:n_in] + rng.normal(0, 0.3, size=(n_in, 2))
    rng.normal(0, 0.3, size=(n_in, 2))
    p1 = np.r_[p1, rng.uniform([0, 0], size, size=(n_out, 2))]
    rng.uniform([0, 0], size, size=(n_out, 2))
    perm = rng.permutation(n_in + n_out)
    return p1[perm].astype(np.float32), np.r_[world[:n_in], np.full((n_out, 3), np.nan)][perm]


@functools.lru_cache(maxsize=None)
def twocam_scene():
    """300 planted points seen by the two cameras of TWOCAM (both images 1280 x 960) + 150 outliers, 0.3 px of noise."""
    rng = np.random.default_rng(1)
    c, s = np.cos(0.15), np.sin(0.15)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    t = -R @ np.array([0.8, 0.0, 0.0])
    K1, K2 = kmat(TWOCAM[0]), kmat(TWOCAM[1])
    p1, p2, world = np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 3))
    while len(p1) < N_IN:
        X = rng.uniform([-3, -2, 3], [3, 2, 12], size=(4 * N_IN, 3))
        X2 = X @ R.T + t
        a, b = X @ K1.T, X2 @ K2.T
        a, b = a[:, :2] / a[:, 2:], b[:, :2] / b[:, 2:]
        ok = ((a >= 0) & (a < [1280, 960]) & (b >= 0) & (b < [1280, 960])).all(axis=1) & (X2[:, 2] > 0)
        p1, p2, world = np.r_[p1, a[ok]], np.r_[p2, b[ok]], np.r_[world, X[ok]]
    p1 = np.r_[p1[:N_IN] + rng.normal(0, 0.3, size=(N_IN, 2)), rng.uniform([0, 0], [1280, 960], size=(N_OUT, 2))]
    p2 = np.r_[p2[:N_IN] + rng.normal(0, 0.3, size=(N_IN, 2)), rng.uniform([0, 0], [1280, 960], size=(N_OUT, 2))]
    n = N_IN + N_OUT
    perm = rng.permutation(n)
    pts = np.zeros(n, dtype=SIFT_POINT_DTYPE)
    pts["coords2D"] = p1[perm].astype(np.float32)
    pts["match_xpos"], pts["match_ypos"] = p2[perm, 0].astype(np.float32), p2[perm, 1].astype(np.float32)
    pts["score"], pts["ambiguity"] = 0.9, 0.5
    pts["match"] = rng.integers(0, 500, n).astype(np.int32)
    pts["match_error"] = 7.0
    planted = np.zeros(n, dtype=bool)
    planted[:N_IN] = True
    pts.setflags(write=False)
    return pts, planted[perm], R, t, np.r_[world[:N_IN], np.full((N_OUT, 3), np.nan)][perm]


@functools.lru_cache(maxsize=None)
def case(name):
    from test_epipolar import CX, CY, F_PIX, SCENE_SEEDS

    if name == "twocam":
        pts, planted, R, t, world = twocam_scene()
        return Case(pts, planted, TWOCAM[0], TWOCAM[1], GEO_LOOPS, GEO_SEEDS, R, t, world)
    if name in GEOMETRIES:
        (R, t), f, (w, h), (lo, hi), gen = GEOMETRIES[name]
        pts, planted = view_scene(name)
        cam = (f, f, w / 2.0, h / 2.0, 0.0)
        again, world = replay(gen, N_IN, N_OUT, R, t, f, [w / 2.0, h / 2.0], [w, h], lo, hi, True)
        loops, seeds = GEO_LOOPS, GEO_SEEDS
    else:
        n_in, n_out, loops = SCENES[("s12", "s100", "s650").index(name)]
        R, t, _ = cameras()
        pts, planted = scene(n_in, n_out)
        cam, seeds = (F_PIX, F_PIX, CX, CY, 0.0), SEEDS
        again, world = replay(SCENE_SEEDS[n_in], n_in, n_out, R, t, F_PIX, [CX, CY], [1280, 960], [-3, -2, 3], [3, 2, 12],
                              False)
    assert np.array_equal(again, pts["coords2D"]) and np.array_equal(np.isfinite(world[:, 0]), planted), name
    return Case(pts, planted, cam, cam, loops, seeds, R, t, world)


# ------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------
Pose = collections.namedtuple("Pose", "rt sigma votes num_front coords3D near fit front")
IDENT = np.hstack([np.eye(3), np.zeros((3, 1))])


def decompose(F, K1, K2):
    """(the four candidates [(R21, t21)] or None for a degenerate answer, sigma [3])."""
    F = np.asarray(F, dtype=np.float64).reshape(3, 3)
    if not np.isfinite(F).all() or not F.any():
        return None, np.zeros(3)
    with np.errstate(all="ignore"):
        E = K2.T @ (F @ K1)
        U, S, Vt = np.linalg.svd(E)
        if not S[1] > 0:
            return None, S
        v1, v2 = Vt[0], Vt[1]
        v3 = np.cross(v1, v2)
        u1 = E @ v1 / S[0]
        w = E @ v2
        w = w - (w @ u1) * u1
        u2 = w / np.sqrt(w @ w)
        u3 = np.cross(u1, u2)
        Ra = np.outer(u2, v1) - np.outer(u1, v2) + np.outer(u3, v3)
        Rb = np.outer(u1, v2) - np.outer(u2, v1) + np.outer(u3, v3)
    if not (np.isfinite(Ra).all() and np.isfinite(Rb).all() and np.isfinite(u3).all() and np.isfinite(S).all()):
        return None, S
    return [(Ra, u3), (Ra, -u3), (Rb, u3), (Rb, -u3)], S


def depths(R, t, K1, K2, xy):
    """(z1, z2, d1 [n, 3], a numerator within a relative 1e-9 of zero) of the records xy under one candidate."""
    x1, y1, x2, y2 = xy
    d1 = np.stack([(x1 - K1[0, 2]) / K1[0, 0], (y1 - K1[1, 2]) / K1[1, 1], np.ones_like(x1)], axis=1)
    d2 = np.stack([(x2 - K2[0, 2]) / K2[0, 0], (y2 - K2[1, 2]) / K2[1, 1], np.ones_like(x2)], axis=1)
    a = d1 @ R.T
    aa, bb, ab = (a * a).sum(axis=1), (d2 * d2).sum(axis=1), (a * d2).sum(axis=1)
    at, bt = a @ t, d2 @ t
    with np.errstate(all="ignore"):
        det = aa * bb - ab * ab
        n1, n2 = ab * bt - bb * at, aa * bt - ab * at
        near = (np.abs(n1) <= 1e-9 * (np.abs(ab * bt) + np.abs(bb * at))) | (np.abs(n2) <= 1e-9 * (np.abs(aa * bt) +
                                                                                                  np.abs(ab * at)))
        return n1 / det, n2 / det, d1, near


def pose_model(F, pts, cam1, cam2, thresh=THRESH, rule=0, lo=0.85, hi=0.95, n2=-1):
    n = len(pts)
    K1, K2 = kmat(cam1), kmat(cam2)
    cand = candidates(pts, rule, lo, hi, n2)
    xy = coords(pts, cand)
    F = np.asarray(F, dtype=np.float64).ravel()
    fit = np.zeros(n, dtype=bool)
    fit[cand] = inliers(F, xy, thresh)
    four, sigma = decompose(F, K1, K2)
    nothing = Pose(IDENT.copy(), sigma, np.zeros(4, np.int32), 0, np.zeros((n, 3), np.float32), False, fit,
                   np.zeros(n, dtype=bool))
    if four is None:
        return nothing
    xy = coords(pts, np.flatnonzero(fit))
    near = bool(near_threshold(F, coords(pts, cand), thresh)) if len(cand) else False
    z = []
    for R, t in four:
        z1, z2, d1, nz = depths(R, t, K1, K2, xy)
        z.append((z1, z2))
        near |= bool(nz.any())
    votes = np.array([int(((z1 > 0) & (z2 > 0)).sum()) for z1, z2 in z], dtype=np.int32)
    win = int(np.argmax(votes))  # among equals the first
    if votes[win] == 0:
        return nothing._replace(near=near)
    R21, t21 = four[win]
    z1, z2 = z[win]
    with np.errstate(all="ignore"):
        P = (z1[:, None] * d1).astype(np.float32)
    keep = (z1 > 0) & (z2 > 0) & np.isfinite(P).all(axis=1) & (P[:, 2] > 0)
    out = np.zeros((n, 3), np.float32)
    out[np.flatnonzero(fit)[keep]] = P[keep]
    front = np.zeros(n, dtype=bool)
    front[np.flatnonzero(fit)] = (z1 > 0) & (z2 > 0)
    return Pose(np.hstack([R21.T, (-R21.T @ t21)[:, None]]), sigma, votes, int(votes[win]), out, near, fit, front)


def rot_err(Ra, Rb):
    return float(np.degrees(np.arccos(np.clip((np.trace(Ra.T @ Rb) - 1.0) / 2.0, -1.0, 1.0))))


def dir_err(a, b):
    return float(np.degrees(np.arccos(np.clip(a @ b / np.sqrt((a @ a) * (b @ b)), -1.0, 1.0))))


def truth_errors(rt, c):
    """(rotation error, translation-direction error) in degrees against the planted pose, in the call's direction."""
    return rot_err(rt[:, :3], c.R21.T), dir_err(rt[:, 3], -c.R21.T @ c.t21)


def lifted_shares(coords3D, c):
    """(share of the planted records that carry a point, share of those within 5 % of the planted 3-D point)."""
    has = c.planted & (coords3D[:, 2] > 0)
    P = coords3D[has].astype(np.float64) * np.sqrt(c.t21 @ c.t21)
    d = np.sqrt(((P - c.world[has]) ** 2).sum(axis=1)) / np.sqrt((c.world[has] ** 2).sum(axis=1))
    return float(has.sum() / c.planted.sum()), float((d <= 0.05).mean())


def check_against_model(dev, after, want, pts, label):
    """The assertions of DEVICE = MODEL; `dev` is a capi.PoseResult, `after` the records as the call left them."""
    d_rt = float(np.abs(dev.rt - want.rt).max())
    d_sigma = float(np.abs(dev.sigma - want.sigma).max() / max(want.sigma[0], 1e-300))
    got = after["coords3D"]
    nz, want_nz = got.any(axis=1), want.coords3D.any(axis=1)
    rel = float((np.abs(got[nz & want_nz].astype(np.float64) - want.coords3D[nz & want_nz]) /
                 np.abs(want.coords3D[nz & want_nz])).max()) if (nz & want_nz).any() else 0.0
    print("%s: [R | t] differs by %.3g, sigma by %.3g of sigma_1, sigma2 / sigma1 = %.4f, votes %s (model %s), %d points, "
          "coords3D by %.3g relative" % (label, d_rt, d_sigma, want.sigma[1] / max(want.sigma[0], 1e-300),
                                         dev.votes.tolist(), want.votes.tolist(), nz.sum(), rel))
    assert d_rt <= 1e-9, d_rt
    assert d_sigma <= 1e-9, d_sigma
    assert sorted(dev.votes.tolist()) == sorted(want.votes.tolist()) and dev.num_front == want.num_front == dev.votes.max()
    assert np.array_equal(nz, want_nz) and nz.sum() <= dev.num_front
    assert rel <= 1e-5, rel
    assert (got[nz][:, 2] > 0).all()
    rest = after.copy()
    rest["coords3D"] = pts["coords3D"]
    assert rest.tobytes() == pts.tobytes()  # no other byte of any record moved


def camera(cam):
    """capi.Camera of a (fx, fy, cx, cy, origin); units_per_metre and encoding hold what the depth lift would refuse."""
    from cusift_amd import capi

    return capi.Camera(cam[0], cam[1], cam[2], cam[3], cam[4], 0.0, 7)


def stale(pts):
    out = pts.copy()
    out["coords3D"] = STALE
    return out


# ------------------------------------------------------------------------------------------------------------------
# without a GPU
# ------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_carry_the_pose_calls():
    from cusift_amd import batch, capi

    extras = open(os.path.join(ROOT, "include", "cusift_amd_extras.h")).read()
    front = open(os.path.join(ROOT, "include", "cusift_amd.h")).read()
    handle = C.CDLL(capi.LIB_PATH)
    for name, nargs in (("cusift_estimate_pose", 15), ("cusift_register_pose", 30)):
        assert "int %s(cusift_ctx *ctx" % name in extras, name
        assert "int %s(" % name not in front, name
        assert hasattr(handle, name), name
        res, args = capi.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs and args.count(C.POINTER(capi.Camera)) == 2, (name, len(args))
    assert C.c_uint64 in capi.SIGNATURES["cusift_register_pose"][1]
    for m in ("estimate_pose", "register_pose"):
        assert callable(getattr(capi.Context, m))
    assert callable(batch.BatchExtractor.register_pose)
    assert capi.RegisterPoseResult._fields == capi.EpipolarResult._fields + ("rt", "num_front", "votes", "sigma")
    make = open(os.path.join(ROOT, "Makefile")).read()
    assert "sift_pose" in make.split("SOURCES :=")[1].split("HEADERS")[0] and "cpp_pose" in make
    assert "tests/cpp_pose/pose_dropin.cpp" in open(os.path.join(ROOT, "CMakeLists.txt")).read()
    assert "tests/cpp_pose/pose_dropin" in open(os.path.join(ROOT, ".gitignore")).read()
    head = open(os.path.join(ROOT, "include", "pose.h")).read()
    assert "RegisterPose(SiftData &data1, SiftData &data2" in head and "EstimatePose(SiftData &data" in head
    assert "#include <hip" not in head
    # the pinned expressions stand in the header as they stand in the kernels
    for expr in ("det = aa*bb - ab*ab", "z1 = (ab*bt - bb*at) / det", "z2 = (aa*bt - ab*at) / det",
                 "Ra[i][j] = (u2[i]*v1[j] - u1[i]*v2[j]) + u3[i]*v3[j]", "E[2][j] = (px2*A[0][j] + py2*A[1][j]) + A[2][j]"):
        assert expr in extras, expr
    kernels = open(os.path.join(ROOT, "cusift_amd", "csrc", "sift_pose.hip")).read()
    for expr in ("det = aa * bb - ab * ab", "z1 = (ab * bt - bb * at) / det", "z2 = (aa * bt - ab * at) / det"):
        assert expr in kernels, expr


def test_model_decomposes_a_planted_essential_matrix():
    """The restatement itself: from the exact F of a planted pose the winner is that pose to rounding, the votes are all
    for one candidate, every depth is the planted depth over the baseline, and the other three candidates lose."""
    c = case("twocam")
    K1, K2 = kmat(c.cam1), kmat(c.cam2)
    tx = np.array([[0, -c.t21[2], c.t21[1]], [c.t21[2], 0, -c.t21[0]], [-c.t21[1], c.t21[0], 0]])
    F = np.linalg.inv(K2).T @ tx @ c.R21 @ np.linalg.inv(K1)
    F = F.ravel() / np.sqrt((F * F).sum())
    X = c.world[c.planted]
    a, b = X @ K1.T, (X @ c.R21.T + c.t21) @ K2.T
    pts = np.zeros(len(X), dtype=SIFT_POINT_DTYPE)
    pts["coords2D"] = (a[:, :2] / a[:, 2:]).astype(np.float32)
    pts["match_xpos"], pts["match_ypos"] = (b[:, :2] / b[:, 2:]).astype(np.float32).T
    pts["score"], pts["ambiguity"] = 0.9, 0.5
    got = pose_model(F, pts, c.cam1, c.cam2)
    r, d = truth_errors(got.rt, c)
    assert r <= 1e-6 and d <= 1e-6 and abs(np.sqrt(got.rt[:, 3] @ got.rt[:, 3]) - 1.0) <= 1e-12
    assert sorted(got.votes.tolist()) == [0, 0, 0, len(X)] and got.num_front == len(X)
    scaled = got.coords3D.astype(np.float64) * np.sqrt(c.t21 @ c.t21)
    assert (np.abs(scaled - X).max(axis=1) / np.abs(X).max(axis=1)).max() <= 1e-3  # float pixels: ~1e-4 px of a pixel
    assert abs(got.sigma[1] / got.sigma[0] - 1.0) <= 1e-6 and got.sigma[2] <= 1e-9 * got.sigma[0]


MODEL = {}


def model_pose(name, seed):
    """The model alone on one scene and seed: its own RANSAC, its refit, its pose.  Shared by the tests below."""
    if (name, seed) not in MODEL:
        c = case(name)
        cand, xy, F, counts, best = model_run(c.pts, c.loops, seed)
        fit, near = refit(F[:, best], xy, REFINE_LOOPS, THRESH)
        MODEL[name, seed] = (fit, near, pose_model(fit, c.pts, c.cam1, c.cam2))
    return MODEL[name, seed]


@pytest.mark.parametrize("name", GOOD)
def test_model_meets_the_truth_bounds(name):
    """CPU twin of the truth test: the model, run from its own RANSAC with these tests' loop counts and seeds, stays within
    0.25 degrees of the planted rotation and 1.5 degrees of the planted translation direction, so the bounds stand as
    stated.  Every planted record of the fit set lies in front of both cameras, no depth of the fit set comes within a
    relative 1e-9 of zero, 99 % of the planted records carry a point and 95 % of those lie within 5 % of the planted
    3-D point."""
    c = case(name)
    for seed in c.seeds:
        F, near, pose = model_pose(name, seed)
        r, d = truth_errors(pose.rt, c)
        has, close = lifted_shares(pose.coords3D, c)
        print("%s seed %#x: rotation %.4f, direction %.4f degrees, sigma2 / sigma1 = %.4f, votes %s, %d fit, %.4f of the "
              "planted carry a point, %.4f of those within 5 %%, near %s" %
              (name, seed, r, d, pose.sigma[1] / pose.sigma[0], pose.votes.tolist(), pose.fit.sum(), has, close, pose.near))
        assert r <= ROT_BOUND and d <= DIR_BOUND, (r, d)
        assert (pose.front | ~pose.fit | ~c.planted).all()  # a planted record of the fit set is in front
        K1, K2 = kmat(c.cam1), kmat(c.cam2)
        four, _ = decompose(F, K1, K2)
        xy = coords(c.pts, np.flatnonzero(pose.fit))
        assert not any(depths(R, t, K1, K2, xy)[3].any() for R, t in four)
        assert has >= 0.99 and close >= 0.95, (has, close)
        assert abs(np.sqrt(pose.rt[:, 3] @ pose.rt[:, 3]) - 1.0) <= 1e-12
        assert np.abs(pose.rt[:, :3] @ pose.rt[:, :3].T - np.eye(3)).max() <= 1e-12
        assert np.linalg.det(pose.rt[:, :3]) > 0.999


def test_two_cameras_cannot_be_replaced_by_one_or_swapped():
    """TWOCAM's twin: with the right F, the model under swapped cameras and under camera 1 for both views misses the truth
    bounds, so a device that confused them would fail the truth test.  A dropped origin moves the principal point by one
    pixel only and stays inside them; it moves [R | t] by more than 1e-4, which DEVICE = MODEL catches at 1e-9."""
    c = case("twocam")
    F, _, right = model_pose("twocam", c.seeds[0])
    no_origin = c.cam2[:4] + (0.0,)
    for what, cams in (("swapped", (c.cam2, c.cam1)), ("camera 1 twice", (c.cam1, c.cam1)),
                       ("origin dropped", (c.cam1, no_origin))):
        wrong = pose_model(F, c.pts, *cams)
        r, d = truth_errors(wrong.rt, c)
        moved = float(np.abs(wrong.rt - right.rt).max())
        print("%s: rotation %.3f, direction %.3f degrees, sigma2 / sigma1 = %.4f, [R | t] moved by %.3g" %
              (what, r, d, wrong.sigma[1] / wrong.sigma[0], moved))
        assert moved > 1e-4, what
        if what != "origin dropped":
            assert r > ROT_BOUND or d > DIR_BOUND, what


def test_pose_kernels_compile_for_gfx950_without_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs

    asm = kernel_regs.assembly("sift_pose.hip")
    assert "gfx950" in asm
    ks = {k["name"]: k for k in kernel_regs.kernels(asm)}
    assert len(ks) == 2 and all(any(w in n for n in ks) for w in NEW_KERNELS), sorted(ks)
    for n, k in ks.items():
        print("%s: %d VGPRs, %d AGPRs, %d bytes of scratch, %d bytes of LDS" %
              (n[:40], k["vgpr_count"], k["agpr_count"], k["private_segment_fixed_size"], k["group_segment_fixed_size"]))
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
        assert k["group_segment_fixed_size"] <= 64  # the block sum and nothing else
    text = open(os.path.join(ROOT, "cusift_amd", "csrc", "sift_pose.hip")).read()
    assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", text, flags=re.M)
    assert "__launch_bounds__(kPoseThreads)" in text and "constexpr int kPoseThreads = 256;" in text


# ------------------------------------------------------------------------------------------------------------------
# on the GPU
# ------------------------------------------------------------------------------------------------------------------
DEVICE = {}


def device_pose(ctx, name, seed):
    """The staged route on one scene and seed, once: estimate_fundamental, then estimate_pose with the returned F on a
    fresh upload whose coords3D are stale.  (EpipolarResult, PoseResult, the records afterwards)."""
    if (name, seed) not in DEVICE:
        c = case(name)
        epi, _ = run(ctx, c.pts, loops=c.loops, seed=seed, **RULE_ARGS[0])
        buf = upload(ctx, stale(c.pts))
        pose = ctx.estimate_pose(buf.ptr, len(c.pts), epi.fundamental, camera(c.cam1), camera(c.cam2), thresh=THRESH,
                                 **RULE_ARGS[0])
        DEVICE[name, seed] = (epi, pose, buf.to_numpy(SIFT_POINT_DTYPE, (len(c.pts),)))
        buf.free()
    return DEVICE[name, seed]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_device_equals_the_model_from_the_devices_own_f(ctx, name):
    c = case(name)
    skipped = 0
    for seed in c.seeds:
        epi, pose, after = device_pose(ctx, name, seed)
        want = pose_model(epi.fundamental, c.pts, c.cam1, c.cam2)
        if want.near:
            skipped += 1
            continue
        check_against_model(pose, after, want, stale(c.pts), "%s seed %#x" % (name, seed))
        assert pose.num_front <= epi.num_fit  # the fit set at the same threshold
    assert skipped <= 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", GOOD)
def test_pose_and_points_are_close_to_the_planted_ones(ctx, name):
    c = case(name)
    for seed in c.seeds:
        _, pose, after = device_pose(ctx, name, seed)
        r, d = truth_errors(pose.rt, c)
        has, close = lifted_shares(after["coords3D"], c)
        print("%s seed %#x: rotation %.4f, direction %.4f degrees, %.4f of the planted carry a point, %.4f of those within "
              "5 %%" % (name, seed, r, d, has, close))
        assert r <= ROT_BOUND and d <= DIR_BOUND, (r, d)
        assert has >= 0.99 and close >= 0.90, (has, close)
        assert abs(np.sqrt(pose.rt[:, 3] @ pose.rt[:, 3]) - 1.0) <= 1e-12


@pytest.mark.gpu
def test_swapped_roles_give_the_inverse_pose(ctx):
    """TWOCAM registered 2 -> 1: the records' two positions and the two cameras change places."""
    c = case("twocam")
    back = c.pts.copy()
    back["coords2D"][:, 0], back["coords2D"][:, 1] = c.pts["match_xpos"], c.pts["match_ypos"]
    back["match_xpos"], back["match_ypos"] = c.pts["coords2D"][:, 0], c.pts["coords2D"][:, 1]
    for seed in c.seeds:
        _, fwd, _ = device_pose(ctx, "twocam", seed)
        epi, _ = run(ctx, back, loops=c.loops, seed=seed, **RULE_ARGS[0])
        buf = upload(ctx, stale(back))
        inv = ctx.estimate_pose(buf.ptr, len(back), epi.fundamental, camera(c.cam2), camera(c.cam1), thresh=THRESH,
                                **RULE_ARGS[0])
        buf.free()
        R, t = fwd.rt[:, :3], fwd.rt[:, 3]
        r, d = rot_err(inv.rt[:, :3], R.T), dir_err(inv.rt[:, 3], -R.T @ t)
        print("seed %#x: the 2 -> 1 pose against the inverse of 1 -> 2: rotation %.4f, direction %.4f degrees" % (seed, r, d))
        assert r <= ROT_BOUND and d <= DIR_BOUND, (r, d)
        assert inv.num_front >= 0.99 * c.planted.sum()


def paired_frames(pts, paired=None, seed=3):
    """Two frames for the matcher out of records that carry match positions: frame 2's record (7 i + 3) mod n sits at the
    match position of record i of frame 1 and shares its descriptor, a random unit vector with entries >= 0, so the dot
    product pairs them with score 1 and an ambiguity of about 0.8.  paired: only these records of frame 1 find their
    partner; the others hold a one-hot descriptor in the lower half and their partners one in the upper half (scores of
    0.1 at most)."""
    n = len(pts)
    rng = np.random.default_rng(seed)
    step = next(s for s in (7, 11, 13, 17) if np.gcd(s, n) == 1)
    f1, f2 = pts.copy(), np.zeros(n, dtype=SIFT_POINT_DTYPE)
    desc = rng.random((n, 128)).astype(np.float32)
    desc /= np.sqrt((desc.astype(np.float64) ** 2).sum(axis=1))[:, None].astype(np.float32)
    other = desc.copy()
    if paired is not None:
        lone = np.setdiff1d(np.arange(n), paired)
        desc[lone], other[lone] = 0, 0
        desc[lone, lone % 64], other[lone, 64 + lone % 64] = 1, 1
    j = (step * np.arange(n) + 3) % n
    f1["data"], f2["data"][j] = desc, other
    f2["coords2D"][j, 0], f2["coords2D"][j, 1] = pts["match_xpos"], pts["match_ypos"]
    for f in ("score", "ambiguity", "match", "match_xpos", "match_ypos", "match_error"):
        f1[f] = 0
    return stale(f1), stale(f2)


@pytest.mark.gpu
@pytest.mark.parametrize("distance,rule_args", [(1, dict(rule=1, lo=999.0, hi=0.8)), (0, dict(rule=0, lo=0.0, hi=0.95)),
                                                (1, dict(rule=1, lo=999.0, hi=0.8, thresh=2.0, refine_thresh=0.75))])
def test_fused_equals_staged_byte_for_byte(ctx, distance, rule_args):
    """register_pose against register_epipolar followed by estimate_pose at refine_thresh, on the VLFeat fixture pair with
    its own intrinsics (1-based): every output and the whole record arrays of both frames, guard rows behind num_pts
    included.  (MATLAB's baseline for this pair is 1.9 mm, so its pose is printed, not judged.)"""
    from test_rgbd import intrinsics

    s1 = read_vlfeat_sift(os.path.join(GOLDEN, "vlfeat_sift1.bin"))
    s2 = read_vlfeat_sift(os.path.join(GOLDEN, "vlfeat_sift2.bin"))
    guard = np.zeros(5, dtype=SIFT_POINT_DTYPE)
    guard["coords3D"], guard["match_error"], guard["score"] = 77.0, 77.0, 77.0
    a1, a2 = np.concatenate([stale(s1), guard]), np.concatenate([stale(s2), guard])
    cam = camera(intrinsics() + (1.0,))
    kw = dict(loops=512, thresh=THRESH, refine_loops=REFINE_LOOPS, refine_thresh=THRESH, seed=9, want_all=True)
    kw.update(rule_args)
    b1, b2 = upload(ctx, a1), upload(ctx, a2)
    fused = ctx.register_pose(b1.ptr, len(s1), b2.ptr, len(s2), cam, distance=distance, **kw)
    f1, f2 = b1.to_numpy(SIFT_POINT_DTYPE, (len(a1),)), b2.to_numpy(SIFT_POINT_DTYPE, (len(a2),))
    c1, c2 = upload(ctx, a1), upload(ctx, a2)
    epi = ctx.register_epipolar(c1.ptr, len(s1), c2.ptr, len(s2), distance=distance, **kw)
    mid = c1.to_numpy(SIFT_POINT_DTYPE, (len(a1),))
    pose = ctx.estimate_pose(c1.ptr, len(s1), epi.fundamental, cam, None, num_pts2=len(s2), rule=kw["rule"], lo=kw["lo"],
                             hi=kw["hi"], thresh=kw["refine_thresh"])
    t1, t2 = c1.to_numpy(SIFT_POINT_DTYPE, (len(a1),)), c2.to_numpy(SIFT_POINT_DTYPE, (len(a2),))
    print("distance %d: %d candidates, %d fit, %d in front, votes %s, sigma2 / sigma1 = %.4f, |t| = %.6f" %
          (distance, fused.num_candidates, fused.num_fit, fused.num_front, fused.votes.tolist(),
           fused.sigma[1] / fused.sigma[0], np.sqrt(fused.rt[:, 3] @ fused.rt[:, 3])))
    assert 8 <= fused.num_candidates < len(s1) and fused.num_fit >= 8 and 0 < fused.num_front <= fused.num_fit
    for u, v in zip(fused, tuple(epi) + tuple(pose)):
        assert np.asarray(u).tobytes() == np.asarray(v).tobytes()
    assert f1.tobytes() == t1.tobytes() and f2.tobytes() == t2.tobytes() == a2.tobytes()
    assert f1[len(s1):].tobytes() == guard.tobytes()
    # the epipolar call's bytes: only coords3D lies between the fused records and register_epipolar's
    same = f1.copy()
    same["coords3D"] = mid["coords3D"]
    assert same.tobytes() == mid.tobytes() and (mid["coords3D"][:len(s1)] == STALE).all()
    assert (f1["coords3D"][:len(s1), 2] > 0).sum() == fused.num_front and not (f1["coords3D"][:len(s1)] == STALE).any()
    for b in (b1, b2, c1, c2):
        b.free()


@pytest.mark.gpu
def test_degenerate_answers(ctx):
    """Eight candidates among 300 records work; seven give F = 0 and with it [I | 0], zero votes and all-zero coords3D,
    staged and fused; so do an F of zeros, an F of NaNs, an F that is not rank 2 in a way no camera explains (sigma_2 =
    0), and a fit set with nobody in front.  The same call twice gives the same bytes."""
    c = case("s650")
    base = c.pts[:300]
    good = np.flatnonzero(c.planted[:300])[np.array([3, 21, 40, 66, 90, 111, 130, 150])]
    cam = camera(c.cam1)

    def only(idx):
        out = stale(base)
        out["score"] = 0.3
        out["score"][idx] = 0.9
        return out

    def pose_of(pts, F, **kw):
        buf = upload(ctx, pts)
        args = dict(thresh=THRESH, **RULE_ARGS[0])
        args.update(kw)
        res = ctx.estimate_pose(buf.ptr, len(pts), F, cam, **args)
        after = buf.to_numpy(SIFT_POINT_DTYPE, (len(pts),))
        buf.free()
        return res, after

    def nothing(res, after, what):
        assert np.array_equal(res.rt, IDENT) and res.num_front == 0 and not res.votes.any(), what
        assert not after["coords3D"].any(), what

    eight = only(good)
    epi, _ = run(ctx, eight, loops=64, seed=3, **RULE_ARGS[0])
    assert epi.num_candidates == 8 and epi.num_fit == 8
    res, after = pose_of(eight, epi.fundamental)
    want = pose_model(epi.fundamental, eight, c.cam1, c.cam1)
    assert not want.near
    check_against_model(res, after, want, eight, "eight candidates")
    assert res.num_front == 8 and set(np.flatnonzero(after["coords3D"].any(axis=1))) == set(good.tolist())
    again, after2 = pose_of(eight, epi.fundamental)
    assert all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(res, again))
    assert after.tobytes() == after2.tobytes()

    seven = only(good[:7])
    epi7, _ = run(ctx, seven, loops=64, seed=3, **RULE_ARGS[0])
    assert epi7.num_candidates == 7 and not epi7.fundamental.any()
    nothing(*pose_of(seven, epi7.fundamental), what="seven candidates, staged")
    f1, f2 = paired_frames(seven, good[:7])
    b1, b2 = upload(ctx, f1), upload(ctx, f2)
    fused = ctx.register_pose(b1.ptr, len(f1), b2.ptr, len(f2), cam, distance=0, loops=64, seed=3, **RULE_ARGS[0])
    assert fused.num_candidates == 7 and not fused.fundamental.any() and not fused.sigma.any()
    nothing(fused, b1.to_numpy(SIFT_POINT_DTYPE, (len(f1),)), "seven candidates, fused")
    few = ctx.register_pose(b1.ptr, 5, b2.ptr, len(f2), cam, distance=0, loops=64, seed=3, **RULE_ARGS[0])
    rec = b1.to_numpy(SIFT_POINT_DTYPE, (len(f1),))
    nothing(few, rec[:5], "five records, fused")
    b1.free()
    b2.free()

    nothing(*pose_of(eight, np.zeros(9)), what="F of zeros")
    nothing(*pose_of(eight, np.full(9, np.nan)), what="F of NaNs")
    bad = epi.fundamental.copy()
    bad[4] = np.inf
    nothing(*pose_of(eight, bad), what="F with an infinite entry")
    rank1 = np.zeros(9)
    rank1[8] = 1.0  # E = e3 e3^T: sigma = (1, 0, 0)
    res, after = pose_of(eight, rank1, thresh=1e9)
    nothing(res, after, "sigma_2 = 0")
    assert res.sigma[0] == 1.0 and res.sigma[1] == 0.0
    none = only([])
    res, after = pose_of(none, epi.fundamental)
    nothing(res, after, "an empty fit set")
    assert res.sigma[1] > 0  # sigma is what was computed
    buf = upload(ctx, eight)
    res = ctx.estimate_pose(buf.ptr, 0, epi.fundamental, cam, thresh=THRESH, **RULE_ARGS[0])  # no record at all
    assert np.array_equal(res.rt, IDENT) and res.num_front == 0 and not res.votes.any() and res.sigma[1] > 0
    assert buf.to_numpy(SIFT_POINT_DTYPE, (len(eight),)).tobytes() == eight.tobytes()
    buf.free()


@pytest.mark.gpu
def test_refusals_leave_everything_untouched(ctx):
    from cusift_amd import capi

    c = case("s100")
    pts = stale(c.pts)
    buf = upload(ctx, pts)
    F = np.ascontiguousarray(cameras()[2].ravel() / np.sqrt((cameras()[2] ** 2).sum()))
    rt, sigma, votes, front = np.full(12, 9.0), np.full(3, 9.0), np.full(4, -7, np.int32), C.c_int(-7)
    nan, inf = float("nan"), float("inf")

    def cam_of(**kw):
        v = dict(fx=1000.0, fy=1000.0, cx=640.0, cy=480.0, origin=0.0)
        v.update(kw)
        return capi.Camera(v["fx"], v["fy"], v["cx"], v["cy"], v["origin"], 1000.0, 0)

    def untouched(what):
        assert (rt == 9.0).all() and (sigma == 9.0).all() and (votes == -7).all() and front.value == -7, what
        assert buf.to_numpy(SIFT_POINT_DTYPE, (len(pts),)).tobytes() == pts.tobytes(), what

    def call(c1=cam_of(), c2=None, rule=0, lo=0.85, hi=0.95, th=1.0, f=F, out=rt, nf=front, data=buf.ptr, n=len(pts)):
        return capi.lib().cusift_estimate_pose(
            ctx.handle, data, n, -1, rule, lo, hi, f.ctypes.data if f is not None else None, th,
            C.byref(c1) if c1 is not None else None, C.byref(c2) if c2 is not None else None,
            out.ctypes.data if out is not None else None, C.byref(nf) if nf is not None else None, votes.ctypes.data,
            sigma.ctypes.data)

    cases = [dict(c1=None), dict(out=None), dict(nf=None), dict(f=None), dict(th=0.0), dict(th=-1.0), dict(th=nan),
             dict(rule=2), dict(rule=-1), dict(lo=nan), dict(hi=nan), dict(data=None), dict(n=-1)]
    for field, values in (("fx", (0.0, nan, inf)), ("fy", (0.0, nan, -inf)), ("cx", (nan, inf)), ("cy", (nan, inf)),
                          ("origin", (nan, inf))):
        for v in values:
            cases += [dict(c1=cam_of(**{field: v})), dict(c2=cam_of(**{field: v}))]
    for kw in cases:
        assert call(**kw) == -1, kw  # CUSIFT_ERR_INVALID
        untouched(kw)
    assert call() == 0 and front.value >= 0.9 * c.planted.sum() and abs(np.sqrt(rt[[3, 7, 11]] @ rt[[3, 7, 11]]) - 1) <= 1e-12

    # the fused call: the cameras' and the pose outputs' refusals on top of cusift_register_epipolar's
    other = upload(ctx, pts)
    buf2 = upload(ctx, pts)
    fun, ran = np.full(9, 9.0), np.full(9, 9.0)
    ints = [C.c_int(-7) for _ in range(4)]
    rt[:], sigma[:], votes[:], front.value = 9.0, 9.0, -7, -7

    def fused(c1=cam_of(), c2=None, d2=other.ptr, n2=len(pts), distance=0, loops=64, out=rt, nf=front, rth=1.0):
        p = [C.byref(v) for v in ints]
        return capi.lib().cusift_register_pose(
            ctx.handle, buf2.ptr, len(pts), d2, n2, distance, 0, 0.0, 0.8, loops, 1.0, 5, rth, 1,
            C.byref(c1) if c1 is not None else None, C.byref(c2) if c2 is not None else None, fun.ctypes.data,
            ran.ctypes.data, p[0], p[1], p[2], p[3], None, None, None, None, out.ctypes.data if out is not None else None,
            C.byref(nf) if nf is not None else None, votes.ctypes.data, sigma.ctypes.data)

    for kw in (dict(c1=None), dict(out=None), dict(nf=None), dict(c1=cam_of(fx=0.0)), dict(c2=cam_of(origin=nan)),
               dict(distance=2), dict(d2=None), dict(n2=-1), dict(loops=0), dict(rth=0.0)):
        assert fused(**kw) == -1, kw
        assert (rt == 9.0).all() and (sigma == 9.0).all() and (votes == -7).all() and front.value == -7, kw
        assert (fun == 9.0).all() and (ran == 9.0).all() and all(v.value == -7 for v in ints), kw
        assert buf2.to_numpy(SIFT_POINT_DTYPE, (len(pts),)).tobytes() == pts.tobytes(), kw
        assert other.to_numpy(SIFT_POINT_DTYPE, (len(pts),)).tobytes() == pts.tobytes(), kw
    for b in (buf, buf2, other):
        b.free()


@pytest.mark.gpu
def test_batch_extractor_register_pose_equals_the_context_call(ctx):
    """Two synthetic frames written into a BatchExtractor's slot: register_pose(0, 1, camera) gives the bytes of
    Context.register_pose on copies of the same records, and the same bytes when asked twice."""
    import torch
    from cusift_amd.batch import BatchExtractor

    c = case("s100")
    f1, f2 = paired_frames(c.pts)
    n = len(f1)
    kw = dict(distance=0, loops=100, seed=7, want_all=True, **RULE_ARGS[0])
    cam = camera(c.cam1)
    ex = BatchExtractor(2, 160, 120, num_octaves=3, max_pts=128)
    try:
        def fill():
            for k, f in enumerate((f1, f2)):
                raw = torch.from_numpy(f.view(np.uint8).reshape(n, -1).copy()).to(ex.device)
                ex.points[k, :n] = raw
            ex.counts[:] = n
            torch.cuda.synchronize()

        fill()
        got = ex.register_pose(0, 1, cam, **kw)
        recs = ex.to_host()
        fill()
        again = ex.register_pose(0, 1, cam, **kw)
        b1, b2 = upload(ctx, f1), upload(ctx, f2)
        want = ctx.register_pose(b1.ptr, n, b2.ptr, n, cam, **kw)
        for u, v, w in zip(got, want, again):
            assert np.asarray(u).tobytes() == np.asarray(v).tobytes() == np.asarray(w).tobytes()
        assert recs[0].tobytes() == b1.to_numpy(SIFT_POINT_DTYPE, (n,)).tobytes()
        assert recs[1].tobytes() == b2.to_numpy(SIFT_POINT_DTYPE, (n,)).tobytes() == f2.tobytes()
        assert ex.to_host()[0].tobytes() == recs[0].tobytes()
        r, d = truth_errors(got.rt, c)
        print("%d candidates, %d fit, %d in front; rotation %.4f, direction %.4f degrees" %
              (got.num_candidates, got.num_fit, got.num_front, r, d))
        assert got.num_candidates == n and got.num_front >= 0.99 * c.planted.sum()
        assert r <= ROT_BOUND and d <= DIR_BOUND
        b1.free()
        b2.free()
    finally:
        ex.close()
