"""tests/bundle_model.py, the numpy restatement of cusift_bundle_adjust (include/cusift_amd_extras.h), checked by
itself: it reaches the planted configuration's cost on Scene A from the default and from a far start, its history is
monotone, an independent solver (scipy) finds no lower cost, and every special case of the contract -- a four-zero row,
a NaN pixel, the entry gate, Huber weights, fixed frames -- comes out as the header defines it.  No GPU."""
import os
import re

import numpy as np
import pytest

import bundle_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# Scene A from 0.01 rad / 0.02 units: the model is below the planted cost after its 5th iteration (2.148e-7 against
# C* = 3.646e-7), so 5 are enqueued.  From 0.05 rad / 0.2 units at lambda = 1e-9: 7 rejections, then 6 accepted steps
# reach it; 13 are enqueued.
ITERS_DEFAULT, ITERS_FAR = 5, 13


def scene(far=False):
    return bm.scene_a_far() if far else bm.scene_a()


def project(sc, poses, X):
    """Plain numpy, no pinned order: (c2, err) of every observation slot."""
    nodes = sc["obs"].astype(np.int64)
    tracks = np.repeat(np.arange(len(sc["offsets"]) - 1), np.diff(sc["offsets"]))
    fx, fy, cx, cy = sc["cam"]
    P = poses[nodes // sc["max_pts"]]
    c = np.einsum("nji,nj->ni", P[:, :, :3], X[tracks] - P[:, :, 3])
    uv = np.stack([fx * c[:, 0] / c[:, 2] + cx, fy * c[:, 1] / c[:, 2] + cy], axis=1)
    return c[:, 2], np.linalg.norm(uv - sc["xy"].reshape(-1, 2)[nodes].astype(np.float64), axis=1), tracks


def test_exports_are_declared_and_bound():
    from cusift_amd import capi

    header = open(os.path.join(ROOT, "include", "cusift_amd_extras.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ("cusift_bundle_adjust", "cusift_bundle_default_params"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in capi.SIGNATURES, name
    assert "typedef struct cusift_bundle_params" in code
    assert [f for f, _ in capi.BundleParams._fields_] == ["iterations", "lambda_", "lambda_min", "lambda_max", "huber",
                                                          "max_error", "min_decrease"]
    assert callable(capi.Context.bundle_adjust)


def test_scene_a_turns_every_strided_loop_twice():
    sc = scene()
    r = bm.run_model(sc, iterations=1)
    assert sc["n"] == 7 and sc["max_pts"] == 808
    assert r["summary"][4] == 800 > 256 and r["summary"][6] == 5
    per_frame = np.bincount(sc["obs"][r["used_obs"]] // sc["max_pts"], minlength=7)
    assert per_frame.max() > 512 and per_frame[6] == 0
    assert set(np.diff(sc["offsets"]).tolist()) == {2, 3, 4, 5, 6}
    assert r["held"].tolist() == [True, False, False, False, False, False, True]  # frame 0 by default, 6 has nothing


def test_default_start_reaches_the_planted_cost():
    sc = scene()
    c_star = bm.planted_cost(sc)
    r = bm.run_model(sc, iterations=ITERS_DEFAULT)
    h = r["history"]
    print("Scene A: C* = %.4g, entry %.4g, final %.4g, flags %s" % (c_star, r["summary"][0], r["summary"][1],
                                                                    h[:, 3].astype(int).tolist()))
    assert 0 < c_star < 1e-6
    assert r["summary"][1] <= c_star
    ran = h[h[:, 3] != 2]
    assert (ran[1:, 0] <= ran[:-1, 0]).all() and (ran[ran[:, 3] == 1, 1] < ran[ran[:, 3] == 1, 0]).all()
    assert (ran[1:, 0] == np.where(ran[:-1, 3] == 1, ran[:-1, 1], ran[:-1, 0])).all()
    assert r["summary"][1] == (ran[-1, 1] if ran[-1, 3] == 1 else ran[-1, 0])
    assert r["summary"][2] == (h[:, 3] == 1).sum() and r["summary"][3] == len(ran)
    # the largest reprojection error of the output rows is the cost's scale: sub-millipixel
    assert 0 < r["points3d"][:, 3].max() < 1e-3


def test_far_start_is_rejected_first_and_still_arrives():
    sc = scene(far=True)
    c_star = bm.planted_cost(sc)
    r = bm.run_model(sc, iterations=ITERS_FAR, lam=1e-9)
    flags = r["history"][:, 3].astype(int).tolist()
    print("far start: flags %s, final %.4g (C* %.4g)" % (flags, r["summary"][1], c_star))
    assert flags[0] == 0, "the far start must exercise the reject path"
    assert np.isinf(r["history"][0, 1])  # a used observation lands behind its camera
    lam = r["history"][:, 2]
    rejected = flags.index(1)
    assert rejected >= 1 and np.allclose(lam[1:rejected + 1] / lam[:rejected], 10.0, rtol=1e-12)
    assert r["summary"][1] <= c_star
    assert (np.diff(r["history"][:, 0]) <= 0).all()


def test_an_independent_solver_finds_no_lower_cost():
    """scipy.optimize.least_squares (trf, 3-point finite differences on a sparse pattern, ftol = xtol = gtol = 1e-15) on
    the same residuals from the same start.  Measured: model 2.14764e-07, scipy 2.14766e-07, model / scipy - 1 =
    -5.75e-06 -- the model ends BELOW scipy, whose finite-difference Jacobian stalls at a cost that is float32 pixel
    rounding.  The margin allowed above scipy is 1e-6 relative, a fifth of the distance measured in the other direction."""
    pytest.importorskip("scipy")
    from scipy.optimize import least_squares
    from scipy.sparse import lil_matrix

    sc = scene()
    r = bm.run_model(sc, iterations=ITERS_DEFAULT)
    nodes = sc["obs"].astype(np.int64)
    tracks = np.repeat(np.arange(800), np.diff(sc["offsets"]))
    frames = nodes // sc["max_pts"]
    fx, fy, cx, cy = sc["cam"]
    pix = sc["xy"].reshape(-1, 2)[nodes].astype(np.float64)
    start = sc["poses"]

    def unpack(p):
        poses = start.copy()
        for f in range(1, 6):
            w, dt = p[6 * (f - 1):6 * (f - 1) + 3], p[6 * (f - 1) + 3:6 * f]
            poses[f, :, :3], poses[f, :, 3] = start[f, :, :3] @ bm.rodrigues(w), start[f, :, 3] + dt
        return poses, p[30:].reshape(800, 3)

    def residuals(p):
        poses, X = unpack(p)
        P = poses[frames]
        c = np.einsum("nji,nj->ni", P[:, :, :3], X[tracks] - P[:, :, 3])
        return np.stack([fx * c[:, 0] / c[:, 2] + cx - pix[:, 0], fy * c[:, 1] / c[:, 2] + cy - pix[:, 1]], axis=1).ravel()

    pattern = lil_matrix((2 * len(nodes), 30 + 2400), dtype=int)
    for k, (f, t) in enumerate(zip(frames, tracks)):
        for row in (2 * k, 2 * k + 1):
            if 1 <= f <= 5:
                pattern[row, 6 * (f - 1):6 * f] = 1
            pattern[row, 30 + 3 * t:30 + 3 * t + 3] = 1
    p0 = np.concatenate([np.zeros(30), sc["points"][:, :3].ravel()])
    assert abs((residuals(p0) ** 2).sum() / r["summary"][0] - 1.0) < 1e-9  # the same problem
    sol = least_squares(residuals, p0, jac="3-point", jac_sparsity=pattern, method="trf", ftol=1e-15, xtol=1e-15,
                        gtol=1e-15, max_nfev=60)
    scipy_cost = 2.0 * sol.cost
    print("model %.6g, scipy %.6g, model / scipy - 1 = %.3g" % (r["summary"][1], scipy_cost,
                                                               r["summary"][1] / scipy_cost - 1.0))
    assert r["summary"][1] <= scipy_cost * (1.0 + 1e-6)


def test_unused_tracks_and_the_entry_gate():
    base = scene()
    views = np.diff(base["offsets"])
    sc, who = bm.scene_a_gated()
    zero_t, nan_t, gate3, gate2, cut3, cut2 = (who[k] for k in ("zero", "nan", "gate3", "gate2", "cut3", "cut2"))
    r = bm.run_model(sc, iterations=ITERS_DEFAULT, max_error=20.0)
    # the definition, with plain numpy: the gate at entry, then two used observations a track
    c2, err, tracks = project(sc, sc["poses"], sc["points"][:, :3])
    with np.errstate(invalid="ignore"):
        ok = (c2 > 0) & (err <= 20.0)
    assert not ok[cut3] and not ok[cut2]
    for t in range(800):
        s = slice(sc["offsets"][t], sc["offsets"][t + 1])
        if t in (zero_t, nan_t) or ok[s].sum() < 2:
            ok[s] = False
    np.testing.assert_array_equal(r["used_obs"], ok)
    assert r["used"].sum() == 797 and not r["used"][[zero_t, nan_t, gate2]].any() and r["used"][gate3]
    assert r["used_obs"][sc["offsets"][gate3]:sc["offsets"][gate3 + 1]].sum() == views[gate3] - 1
    assert r["summary"][4] == 797 and r["summary"][5] == ok.sum()
    # unused rows are the input rows, bit for bit; used ones moved
    for t in (zero_t, nan_t, gate2):
        assert r["points3d"][t].tobytes() == sc["points"][t].tobytes()
    assert (r["points3d"][zero_t] == 0).all()
    assert (r["points3d"][r["used"], :3] != sc["points"][r["used"], :3]).any(axis=1).all()
    # the cut observation does not pull: the gated track ends at its planted point like every other
    assert np.linalg.norm(r["points3d"][gate3, :3] - base["planted"][gate3]) < 0.05
    assert r["points3d"][r["used"], 3].max() < 1e-3  # over the USED observations only


def test_huber_weights_hold_an_outlier_back():
    base = scene()
    t = int(np.where(np.diff(base["offsets"]) >= 4)[0][0])
    sc = dict(base, xy=base["xy"].copy())
    sc["xy"].reshape(-1, 2)[base["obs"][base["offsets"][t] + 1]] += (50.0, 0.0)
    plain = bm.run_model(sc, iterations=10)
    robust = bm.run_model(sc, iterations=10, huber=1.0)
    d_plain = np.linalg.norm(plain["points3d"][t, :3] - base["planted"][t])
    d_robust = np.linalg.norm(robust["points3d"][t, :3] - base["planted"][t])
    print("outlier track: %.4g from its planted point without weights, %.4g with huber = 1" % (d_plain, d_robust))
    assert d_robust < 0.25 * d_plain
    # Huber's cost of the entry state: err2 inside, 2 h err - h^2 outside
    _, err, _ = project(sc, sc["poses"], sc["points"][:, :3])
    want = np.where(err <= 1.0, err * err, 2.0 * err - 1.0).sum()
    assert abs(robust["summary"][0] / want - 1.0) < 1e-12
    assert (np.diff(robust["history"][robust["history"][:, 3] != 2, 0]) <= 0).all()


def test_all_frames_fixed_is_structure_only():
    sc = scene()
    r = bm.run_model(sc, iterations=4, fixed=np.ones(7, bool))
    assert r["poses"].tobytes() == sc["poses"].tobytes()
    assert r["summary"][6] == 0 and r["held"].all()
    # the entry points are the midpoint triangulation under these very poses: little is left to gain, but some
    assert r["summary"][1] < r["summary"][0] and r["summary"][2] >= 1
    assert (r["points3d"][:, :3] != sc["points"][:, :3]).any(axis=1).all()


def test_two_fixed_frames_pin_the_scale():
    sc = scene()
    fixed = np.zeros(7, bool)
    fixed[[0, 3]] = True
    r = bm.run_model(sc, iterations=ITERS_DEFAULT, fixed=fixed)
    for f in (0, 3, 6):  # fixed, fixed, nothing observed
        assert r["poses"][f].tobytes() == sc["poses"][f].tobytes()
    for f in (1, 2, 4, 5):
        assert (r["poses"][f] != sc["poses"][f]).any()
        assert np.abs(r["poses"][f, :, :3].T @ r["poses"][f, :, :3] - np.eye(3)).max() < 1e-12
    assert r["summary"][6] == 4
    assert r["summary"][1] < r["summary"][0] and (np.diff(r["history"][:, 0]) <= 0).all()


def check_state_machine(r, lam, lambda_min, lambda_max, min_decrease):
    """The rows of a history against the contract's transitions, walked from the definition: row k + 1 starts at
    max(lambda_k / 10, lambda_min) and the trial cost after an accepted row, at 10 lambda_k and the same cost after a
    rejected one; the run stops after an accepted row whose gain is at most min_decrease or a rejected one whose next
    lambda exceeds lambda_max, and every later row is (cost, cost, lambda, 2).  Returns the number of rows that ran."""
    h, s = r["history"], r["summary"]
    cost, stopped, ran, accepted = s[0], s[4] == 0, 0, 0
    for row in h:
        if stopped:
            assert row.tolist() == [cost, cost, lam, 2.0]
            continue
        ran += 1
        assert row[0] == cost and row[2] == lam and row[3] in (0.0, 1.0)
        assert (row[3] == 1.0) == (row[1] < row[0])
        if row[3] == 1.0:
            accepted += 1
            stopped = (cost - row[1]) / cost <= min_decrease
            cost, lam = row[1], max(lam / 10.0, lambda_min)
        else:
            lam = 10.0 * lam
            stopped = lam > lambda_max
    assert s[1] == cost and s[2] == accepted and s[7] == lam
    assert s[3] == ran == (h[:, 3] != 2).sum() == len(r["causes"])
    return ran


def test_every_history_follows_the_state_machine():
    """The runs the other tests make, and the stops of tests/test_bundle.py, under check_state_machine."""
    d = bm.DEFAULTS
    runs = [(bm.run_model(scene(), iterations=ITERS_DEFAULT), {}),
            (bm.run_model(scene(far=True), iterations=ITERS_FAR, lam=1e-9), dict(lam=1e-9)),
            (bm.run_model(bm.scene_small(), iterations=4, min_decrease=0.9995), dict(min_decrease=0.9995)),
            (bm.run_model(bm.scene_small(), iterations=3, lambda_min=5e-4), dict(lambda_min=5e-4)),
            (bm.run_model(scene(far=True), iterations=3, lam=1e-9, lambda_max=5e-9), dict(lam=1e-9, lambda_max=5e-9))]
    for r, kw in runs:
        p = dict(d, **kw)
        check_state_machine(r, p["lam"], p["lambda_min"], p["lambda_max"], p["min_decrease"])


def test_min_decrease_stops_after_the_accepted_step():
    sc = bm.scene_small()
    free = bm.run_model(sc, iterations=1)
    r = bm.run_model(sc, iterations=4, min_decrease=0.9995)
    h = r["history"]
    print("small scene: first gain %.6f against min_decrease 0.9995" % ((h[0, 0] - h[0, 1]) / h[0, 0]))
    assert check_state_machine(r, 1e-3, 1e-9, 1e6, 0.9995) == 1
    assert abs((h[0, 0] - h[0, 1]) / h[0, 0] - 0.99903) < 1e-5  # 4e-4 under the threshold: no rounding decides this
    # the outputs are those of the one accepted step, not the entry state: the same as one iteration without the stop
    for k in ("poses", "points3d"):
        assert r[k].tobytes() == free[k].tobytes()
    assert (r["poses"][1:] != sc["poses"][1:]).any(axis=(1, 2)).all()
    assert h[1:].tolist() == [[h[0, 1], h[0, 1], 1e-4, 2.0]] * 3 and r["summary"][2] == r["summary"][3] == 1


def test_lambda_max_stops_after_the_rejected_step():
    sc = scene(far=True)
    r = bm.run_model(sc, iterations=3, lam=1e-9, lambda_max=5e-9)
    assert check_state_machine(r, 1e-9, 1e-9, 5e-9, 1e-12) == 1
    cause = r["causes"][0]
    assert cause["behind"] > 0 and cause["vfail"] == 0 and not cause["sfail"]  # points behind cameras, nothing else
    entry = r["summary"][0]
    assert np.isinf(r["history"][0, 1]) and r["summary"].tolist() == [entry, entry, 0, 1, 800, 3308, 5, 1e-8]
    assert r["history"][1:].tolist() == [[entry, entry, 1e-8, 2.0]] * 2
    # nothing was accepted: the input poses and points, and in column 3 each track's worst error at entry
    assert r["poses"].tobytes() == sc["poses"].tobytes()
    assert r["points3d"][:, :3].tobytes() == sc["points"][:, :3].tobytes()
    _, err, tracks = project(sc, sc["poses"], sc["points"][:, :3])
    worst = np.zeros(800)
    np.maximum.at(worst, tracks, err)
    assert np.abs(r["points3d"][:, 3] - worst).max() <= 1e-10
    # entry cost: the squared errors of all 3308 observations
    assert abs(entry / (err * err).sum() - 1.0) < 1e-12


def test_lambda_min_clamps_the_damping():
    r = bm.run_model(bm.scene_small(), iterations=3, lambda_min=5e-4)
    assert check_state_machine(r, 1e-3, 5e-4, 1e6, 1e-12) == 3
    assert r["history"][:, 2].tolist() == [1e-3, 5e-4, 5e-4] and r["summary"][7] == 5e-4
    assert (r["history"][:, 3] == 1).all()
    # without the clamp the second row would run at 1e-4
    assert bm.run_model(bm.scene_small(), iterations=2)["history"][1, 2] == 1e-4


def test_no_fixed_frame_leaves_the_gauge_to_the_damping():
    """fixed given and all zero: only the frame nothing observes is held; NULL would hold frame 0 as well."""
    sc = scene()
    r = bm.run_model(sc, iterations=4, fixed=np.zeros(7, bool))
    assert r["held"].tolist() == [False] * 6 + [True] and r["summary"][6] == 6
    assert check_state_machine(r, 1e-3, 1e-9, 1e6, 1e-12) == 4
    assert (r["history"][:, 1] < 0.1 * r["history"][:, 0]).all()  # accepted by large margins
    assert (r["poses"][0] != sc["poses"][0]).any() and r["poses"][6].tobytes() == sc["poses"][6].tobytes()
    assert not any(c["sfail"] or c["vfail"] or c["behind"] for c in r["causes"])


@pytest.mark.parametrize("frames_held", [True, False])
def test_a_point_far_out_fails_its_track_pivot(frames_held):
    """Track FAR_TRACK at 1e170 times its distance: used at entry, V_t exactly zero.  With its frames held the reduced
    system never sees it (vfail alone); with them free its 0 / 0 makes a Cholesky pivot NaN as well."""
    base = bm.scene_small()
    sc, frames = bm.scene_small_far_point()
    assert len(frames) == 2 and np.isfinite(sc["points"]).all()
    fixed = None
    if frames_held:
        fixed = np.zeros(5, bool)
        fixed[[0] + list(frames)] = True
    r = bm.run_model(sc, iterations=5, lambda_max=0.5, fixed=fixed)
    assert check_state_machine(r, 1e-3, 1e-9, 0.5, 1e-12) == 3
    # from the definition: the track is in front of both cameras with a finite error, and a product of two of its JX
    # entries (at most (|fx| + |fy|) / c2 each) is below the smallest subnormal by orders of magnitude
    c2, err, tracks = project(sc, sc["poses"], sc["points"][:, :3])
    mine = tracks == bm.FAR_TRACK
    assert (c2[mine] > 1e169).all() and np.isfinite(err[mine]).all() and r["used"][bm.FAR_TRACK]
    fx, fy, cx, cy = sc["cam"]
    pix = sc["xy"].reshape(-1, 2)[sc["obs"][mine]].astype(np.float64)
    q_max = ((np.abs(pix - (cx, cy)).max() + err[mine].max()) / min(fx, fy))  # |q| <= (|pixel - centre| + error) / f
    jx_max = (fx + fy) * (1.0 + q_max) / c2[mine].min()
    print("far point: c2 >= %.3g, |q| <= %.3g, |JX| <= %.3g: a product is below 1e%.1f" % (c2[mine].min(), q_max, jx_max,
                                                                                         2.0 * np.log10(jx_max)))
    assert 2.0 * np.log10(jx_max) < np.log10(5e-324) - 5.0  # five orders below the smallest subnormal: exactly 0
    assert r["summary"][4] == 60 and r["summary"][6] == (2 if frames_held else 4)
    for c in r["causes"]:
        assert c["vfail"] == 1 and c["behind"] == 0 and c["sfail"] == (not frames_held)
        if not frames_held:
            assert np.isnan(c["pivot"][1])  # not a sign that rounding could turn
    assert np.isinf(r["history"][:3, 1]).all() and r["history"][:, 2].tolist() == [1e-3, 1e-2, 1e-1, 1.0, 1.0]
    assert r["poses"].tobytes() == sc["poses"].tobytes()
    assert r["points3d"][:, :3].tobytes() == sc["points"][:, :3].tobytes()
    worst = np.zeros(60)
    np.maximum.at(worst, tracks, err)
    assert np.abs(r["points3d"][:, 3] - worst).max() <= 1e-10  # column 3: the worst error at entry
    # the scene without the far point is an ordinary one: its first step is accepted
    assert bm.run_model(base, iterations=1)["history"][0, 3] == 1


def test_the_size_scenes_keep_their_conditions():
    """tests/test_bundle_sizes.py's conditions at 170, 171 and 256 frames, without a GPU (the model: about 20 s)."""
    import test_bundle_sizes as sizes

    assert sorted(6 * v[0] for v in sizes.SIZES.values()) == [1020, 1026, 1026, 1536]
    for name, (n_cams, _, _, _, held) in sizes.SIZES.items():
        sc, model = sizes.check_size_conditions(name)
        per_frame = np.bincount(sc["obs"][model["used_obs"]] // sc["max_pts"], minlength=n_cams)
        print("%s: frame %d held, %d .. %d observations a frame, history %s" % (name, held, per_frame.min(),
                                                                              per_frame.max(),
                                                                              model["history"][:, :2].tolist()))
        assert per_frame.min() >= 2 and model["held"].sum() == 1


def test_strided_tree_sum_is_the_stated_order():
    rng = np.random.default_rng(0)
    v = rng.normal(size=700) * 10.0 ** rng.integers(-8, 8, size=700)
    part = [0.0] * 256
    for i, x in enumerate(v.tolist()):
        part[i % 256] += x
    h = 128
    while h >= 1:
        for k in range(h):
            part[k] += part[k + h]
        h //= 2
    assert bm.strided_tree_sum(v) == part[0]
    assert bm.strided_tree_sum(np.zeros((0, 3))).tolist() == [0.0, 0.0, 0.0]


def test_the_origin_is_visible_to_the_model():
    """px = cx - origin.  Origin 1 with (cx + 1, cy + 1) is origin 0 with (cx, cy) to the bit (320 and 240 are exact in
    float32).  On pixels generated for origin 0.5 (bm.with_origin) the model called with 0.5 sees the small scene's
    geometry; with the origin dropped or flipped it ends far from it -- far more than the 1e-9 of the device test
    (tests/test_bundle.py::test_origin_half_equals_the_model), so that test can tell `cx + origin` from `cx - origin`."""
    base = bm.scene_small()
    fx, fy, cx, cy = base["cam"]
    zero = bm.run_model(base, iterations=3)
    one = bm.run_model(dict(base, cam=(fx, fy, cx + 1.0, cy + 1.0), origin=1.0), iterations=3)
    for k in ("poses", "points3d", "history", "summary"):
        assert one[k].tobytes() == zero[k].tobytes(), k
    sc = bm.with_origin(base, 0.5)
    assert sc["origin"] == 0.5 and np.abs(sc["xy"][:5, :60] - (base["xy"][:5, :60] - 0.5)).max() < 1e-4
    half = bm.run_model(sc, iterations=3)
    assert check_state_machine(half, 1e-3, 1e-9, 1e6, 1e-12) == 3 and (half["history"][:, 3] == 1).all()
    # the scene's own run, to the float32 rounding of the moved pixels
    assert np.abs(half["poses"] - zero["poses"]).max() < 1e-4 and abs(half["summary"][0] / zero["summary"][0] - 1.0) < 1e-3
    for what, origin in (("dropped", 0.0), ("flipped", -0.5)):
        other = bm.run_model(sc, origin=origin, iterations=3)
        d_pose = np.abs(other["poses"] - half["poses"]).max()
        d_cost = abs(other["summary"][0] - half["summary"][0]) / half["summary"][0]
        print("origin %s: poses move by %.3g, entry cost by %.3g of itself (bar 1e-9)" % (what, d_pose, d_cost))
        assert d_pose > 1e-5 and d_cost > 1e-5
