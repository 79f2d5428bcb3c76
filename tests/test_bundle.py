"""cusift_bundle_adjust (cusift_amd/csrc/sift_bundle.hip) against tests/bundle_model.py's restatement in numpy, through
capi.Context.bundle_adjust: Scene A (800 tracks, seven frames, every strided loop turning twice) from the default start,
from a far start that is rejected first, with Huber weights and the entry gate over every kind of unused track, with all
frames, with frames {0, 3} and with no frame fixed; Scene B for the factorisation at 198 and 390 unknowns (1020 to 1536:
tests/test_bundle_sizes.py); the exits of the state machine -- the min_decrease and lambda_max stops, the lambda_min
clamp, a failed track pivot without and with a failed Cholesky pivot; the refusals; the edges.

Measured on an MI355X, largest deviation of the cases added with the stops: fixed_none 7.65e-13, min_decrease 2.79e-14,
lambda_min 8.99e-14; lambda_max, track_pivot and cholesky_pivot 0 (nothing is accepted: every output is an entry value).

The pixel origin (px = cx - origin): Scene A's default case through a camera (cx + 1, cy + 1, origin 1) must give the
bytes of (cx, cy, origin 0), and the small scene on pixels generated for origin 0.5 (bundle_model.with_origin) must equal
the model called with 0.5 -- measured 1.76e-13 --, which tests/test_bundle_model.py shows to end 4e-3 in the poses away
from the model with the origin dropped.  Tried once in a scratch build that was never committed, `cx + origin` in
cusift_bundle_adjust: both origin tests fail (deviations 0.29 and 0.084 from the model), and so does
tests/test_bundle_batch.py on the bytes of its origin-1 call; every other case of this file and of
tests/test_bundle_sizes.py stays green (origin 0 throughout).

The bar for fp64 against a numpy restatement is the project's: 1e-9 * max(1, |value|) on every pose entry, point row and
cost.  Flags are compared on the iterations where the model's own relative cost change exceeds 1e-6 -- below that the
decision can rest on rounding -- and the iteration counts stop before the tail where the model's own decisions are
rounding noise (tests/test_bundle_model.py prints the histories)."""
import ctypes as C
import functools

import numpy as np
import pytest

import bundle_model as bm
from bundle_model import FILL

pytestmark = pytest.mark.gpu
BAR = 1e-9


def fixed_mask(n, frames):
    m = np.zeros(n, bool)
    m[list(frames)] = True
    return m


# name -> (scene, keywords of the call); the iteration counts: tests/test_bundle_model.py and the histories printed there
CASES = {
    "default": (lambda: bm.scene_a(), dict(iterations=5)),
    "far": (lambda: bm.scene_a_far(), dict(iterations=13, lam=1e-9)),
    "huber_gate": (lambda: bm.scene_a_gated()[0], dict(iterations=5, huber=1.0, max_error=20.0)),
    "all_fixed": (lambda: bm.scene_a(), dict(iterations=2, fixed=fixed_mask(7, range(7)))),
    "fixed_0_3": (lambda: bm.scene_a(), dict(iterations=4, fixed=fixed_mask(7, (0, 3)))),
    # h_fixed given and all zero: no frame fixed by the caller (NULL would hold frame 0), frame 6 held as unobserved
    "fixed_none": (lambda: bm.scene_a(), dict(iterations=4, fixed=fixed_mask(7, ()))),
}


@functools.lru_cache(maxsize=None)
def model_of(name):
    make, kw = CASES[name]
    return bm.run_model(make(), **kw)


def deviation(got, want):
    want = np.asarray(want, dtype=np.float64)
    both_inf = np.isinf(want) & (got == want)
    with np.errstate(invalid="ignore"):
        d = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    return float(np.where(both_inf, 0.0, d).max()) if d.size else 0.0


def compare(out, model, sc, iterations, n_tracks=None, rows_in=None):
    """Every output of a device run against the model's; returns the largest deviation.  rows_in: what d_points3d held
    before the call where that is more than the scene's rows and FILL behind them."""
    T = len(sc["offsets"]) - 1 if n_tracks is None else n_tracks
    h, mh = out["history"][:iterations], model["history"]
    worst = max(deviation(out["poses"], model["poses"]), deviation(out["points3d"][:T], model["points3d"]),
                deviation(h[:, :3], mh[:, :3]), deviation(out["summary"][[0, 1, 7]], model["summary"][[0, 1, 7]]))
    assert worst <= BAR, worst
    with np.errstate(invalid="ignore", divide="ignore"):
        decided = ~(np.abs(mh[:, 0] - mh[:, 1]) / mh[:, 0] <= 1e-6) | (mh[:, 3] == 2)
    np.testing.assert_array_equal(h[decided, 3], mh[decided, 3])
    np.testing.assert_array_equal(out["summary"][2:7], model["summary"][2:7])
    # unused tracks and held frames: the input bytes
    unused = ~model["used"]
    assert out["points3d"][:T][unused].tobytes() == np.ascontiguousarray(sc["points"][:T][unused]).tobytes()
    held = model["held"]
    assert out["poses"][held].tobytes() == np.ascontiguousarray(sc["poses"][held]).tobytes()
    # nothing past the track count, nothing past the enqueued iterations
    if rows_in is None:
        assert (out["points3d"][len(sc["offsets"]) - 1:] == FILL).all()
    assert out["points3d"][T:].tobytes() == (out["points3d"] if rows_in is None else rows_in)[T:].tobytes()
    assert (out["history"][iterations:] == FILL).all()
    return worst, int(decided.sum())


@pytest.mark.parametrize("name", list(CASES))
def test_scene_a_equals_the_model(ctx, name):
    make, kw = CASES[name]
    sc, model = make(), model_of(name)
    if name == "fixed_none":  # on the model: the gauge is free, and the steps are still accepted by large margins
        assert model["held"].tolist() == [False] * 6 + [True] and model["summary"][6] == 6
        assert (model["history"][:, 3] == 1).all() and (model["history"][:, 1] < 0.1 * model["history"][:, 0]).all()
        assert not any(c["sfail"] or c["vfail"] or c["behind"] for c in model["causes"])
    dev = bm.DeviceBundle(ctx, sc)
    try:
        out = dev.run(**kw)
        worst, decided = compare(out, model, sc, kw["iterations"])
        print("bundle_adjust %s against the numpy model: largest deviation %.3g (bar 1e-9), %d of %d flags decided above "
              "1e-6, final cost %.6g" % (name, worst, decided, kw["iterations"], out["summary"][1]))
        assert dev.records_back().tobytes() == dev.recs.tobytes()  # d_points is read, never written
        again = dev.run(**kw)
        for k in ("points3d", "poses", "history", "summary"):
            assert again[k].tobytes() == out[k].tobytes(), k  # the same bytes on every run
        if name == "far":
            assert out["history"][0, 3] == 0 and np.isinf(out["history"][0, 1])
        if name in ("default", "far"):
            assert out["summary"][1] <= bm.planted_cost(sc)
    finally:
        dev.close()


def test_origin_one_is_origin_zero_to_the_byte(ctx):
    """px = cx - origin: Scene A's 320 and 240 plus 1 are exact in float32, so a camera (cx + 1, cy + 1, origin 1) is the
    camera (cx, cy, origin 0) and every output byte of the default case must be the same."""
    sc, kw = bm.scene_a(), CASES["default"][1]
    fx, fy, cx, cy = sc["cam"]
    assert np.float32(cx + 1.0) - np.float32(1.0) == np.float32(cx) and np.float32(cy + 1.0) - np.float32(1.0) == np.float32(cy)
    one = dict(sc, cam=(fx, fy, cx + 1.0, cy + 1.0), origin=1.0)
    outs = []
    for s in (sc, one):
        dev = bm.DeviceBundle(ctx, s)
        try:
            assert dev.camera().origin == s.get("origin", 0.0) and dev.camera().cx == s["cam"][2]
            outs.append(dev.run(**kw))
        finally:
            dev.close()
    compare(outs[1], model_of("default"), sc, kw["iterations"])
    assert outs[0]["summary"][2] >= 1  # steps were accepted: the outputs are no entry values
    for k in ("points3d", "poses", "history", "summary"):
        assert outs[1][k].tobytes() == outs[0][k].tobytes(), k


ORIGIN_KW = dict(iterations=3)


def test_origin_half_equals_the_model(ctx):
    """The stop tests' scene on pixels generated for origin 0.5, against the model called with 0.5.  The model with the
    origin dropped or flipped is far away (asserted here and, without a GPU, in tests/test_bundle_model.py)."""
    sc = bm.with_origin(bm.scene_small(), 0.5)
    model = bm.run_model(sc, **ORIGIN_KW)
    assert (model["history"][:, 3] == 1).all() and model["summary"][4] == 60
    for origin in (0.0, -0.5):
        other = bm.run_model(sc, origin=origin, **ORIGIN_KW)
        assert deviation(other["poses"], model["poses"]) > 1e4 * BAR and deviation(other["summary"][:2], model["summary"][:2]) > 1e4 * BAR
    dev = bm.DeviceBundle(ctx, sc)
    try:
        assert dev.camera().origin == 0.5
        out = dev.run(**ORIGIN_KW)
        worst, decided = compare(out, model, sc, ORIGIN_KW["iterations"])
        print("bundle_adjust, origin 0.5, against the numpy model: largest deviation %.3g (bar 1e-9), %d of %d flags "
              "decided" % (worst, decided, ORIGIN_KW["iterations"]))
        assert decided == ORIGIN_KW["iterations"]
    finally:
        dev.close()


@pytest.mark.parametrize("n_tracks,n_cams", [(120, 33), (60, 65)])
def test_scene_b_factorisation_sizes(ctx, n_tracks, n_cams):
    """33 frames: 561 Schur blocks, 198 unknowns; 65 frames: 390 unknowns.  33 and 65 passes of six columns, and
    neither 198 nor 390 is a multiple of the eight the factorisation's and the back-substitution's loops step by."""
    sc = bm.planted_scene(n_tracks, n_cams, 8, 0, 3, 0.01, 0.02)
    assert set(np.diff(sc["offsets"]).tolist()) == set(range(2, 9))
    model = bm.run_model(sc, iterations=2)
    assert model["summary"][6] == n_cams - 1 and model["summary"][2] >= 1
    dev = bm.DeviceBundle(ctx, sc)
    try:
        out = dev.run(iterations=2)
        worst, _ = compare(out, model, sc, 2)
        print("bundle_adjust %d frames x %d tracks: largest deviation %.3g (bar 1e-9)" % (n_cams, n_tracks, worst))
    finally:
        dev.close()


def far_point_fixed():
    """The frames of the far point's track and frame 0 held: the track's 0 / 0 never enters the reduced system."""
    return fixed_mask(5, (0,) + bm.scene_small_far_point()[1])


# The exits of the Levenberg-Marquardt state machine; tests/test_bundle_model.py states each from the definition.
# name -> (scene, keywords of the call; a callable is called for its value when the case runs)
STOPS = {
    # the first gain is 0.99903 <= 0.9995: accepted, then stopped (the margin, 4e-4, is far above rounding)
    "min_decrease": (lambda: bm.scene_small(), dict(iterations=4, min_decrease=0.9995)),
    # the first trial throws points behind cameras; 10 * 1e-9 exceeds lambda_max
    "lambda_max": (lambda: bm.scene_a_far(), dict(iterations=3, lam=1e-9, lambda_max=5e-9)),
    # three accepted steps: lambda 1e-3 -> max(1e-4, 5e-4) -> 5e-4
    "lambda_min": (lambda: bm.scene_small(), dict(iterations=3, lambda_min=5e-4)),
    # V_t exactly zero for one used track whose frames are held: vfail alone, three rejections up to lambda_max
    "track_pivot": (lambda: bm.scene_small_far_point()[0], dict(iterations=5, lambda_max=0.5, fixed=far_point_fixed)),
    # the same track with its frames free: its 0 / 0 reaches S, the Cholesky pivot of column 18 is NaN -- vfail AND sfail
    "cholesky_pivot": (lambda: bm.scene_small_far_point()[0], dict(iterations=5, lambda_max=0.5)),
}


def stop_case(name):
    make, kw = STOPS[name]
    return make(), {k: v() if callable(v) else v for k, v in kw.items()}


@functools.lru_cache(maxsize=None)
def stop_model(name):
    sc, kw = stop_case(name)
    return bm.run_model(sc, **kw)


def worst_entry_error(sc, model):
    """Column 3 of the rows a run that never accepts writes: each used track's largest reprojection error at entry, in
    plain numpy (no pinned order; the maximum and the square root are exact to an ulp or two)."""
    nodes = sc["obs"].astype(np.int64)
    tracks = np.repeat(np.arange(len(sc["offsets"]) - 1), np.diff(sc["offsets"]))
    fx, fy, cx, cy = (np.float64(np.float32(v)) for v in sc["cam"])
    P = sc["poses"][nodes // sc["max_pts"]]
    c = np.einsum("nji,nj->ni", P[:, :, :3], sc["points"][tracks, :3] - P[:, :, 3])
    uv = np.stack([fx * c[:, 0] / c[:, 2] + cx, fy * c[:, 1] / c[:, 2] + cy], axis=1)
    err = np.linalg.norm(uv - sc["xy"].reshape(-1, 2)[nodes].astype(np.float64), axis=1)
    worst = np.zeros(len(sc["offsets"]) - 1)
    np.maximum.at(worst, tracks[model["used_obs"]], err[model["used_obs"]])
    return worst


@pytest.mark.parametrize("name", list(STOPS))
def test_stops_and_failed_pivots(ctx, name):
    """Each case first asserts on the model that it takes the branch it is named for, then compares the device.

    cholesky_pivot: sfail is reached together with vfail only.  S is positive definite for every lambda > 0 in exact
    arithmetic, so a pivot fails by a margin only through a value that is not finite; NaN pixels and poses are refused
    or unused at entry, an overflow in U_f is an overflow in V_t of the same observation, and V_t^-1 enters S only
    through the tracks, so what poisons S has failed its track first.  For the same reason no case has a failed
    iteration followed by an accepted one (which would pin bundle_decide_kernel's reset of sfail): a rejection changes
    lambda alone, lambda enters as 1 + lambda, and a failure that ten times lambda cures is one of rounding (lambda
    below 1e-16) or of subnormal products -- nothing a test may rest on."""
    (sc, kw), model = stop_case(name), stop_model(name)
    n_it = kw["iterations"]
    h, s, causes = model["history"], model["summary"], model["causes"]
    entry_x, entry_p = np.ascontiguousarray(sc["points"][:, :3]), np.ascontiguousarray(sc["poses"])
    # ---- the model takes the branch
    if name == "min_decrease":
        gain = (h[0, 0] - h[0, 1]) / h[0, 0]
        assert h[0, 3] == 1 and 0.9985 < gain < 0.9995 - 1e-4
        assert s[2] == 1 and s[3] == 1 and s[7] == 1e-4
    elif name == "lambda_max":
        assert len(causes) == 1 and causes[0]["behind"] > 0 and not causes[0]["sfail"] and causes[0]["vfail"] == 0
        assert h[0, 3] == 0 and np.isinf(h[0, 1])
        np.testing.assert_array_equal(s, [h[0, 0], h[0, 0], 0, 1, 800, 3308, 5, 1e-8])
    elif name == "lambda_min":
        assert (h[:, 3] == 1).all() and ((h[:, 0] - h[:, 1]) / h[:, 0] > 0.5).all() and s[3] == 3
    else:
        assert model["used"][bm.FAR_TRACK] and s[4] == 60  # finite input, and the track is used
        assert len(causes) == 3 and all(c["vfail"] == 1 and c["behind"] == 0 for c in causes)
        if name == "track_pivot":
            assert not any(c["sfail"] for c in causes) and s[6] == 2
        else:
            assert all(c["sfail"] and np.isnan(c["pivot"][1]) for c in causes) and s[6] == 4
        assert np.isfinite(s[0]) and np.isinf(h[:3, 1]).all() and (h[:3, 3] == 0).all()
        np.testing.assert_array_equal(h[:, 2], [1e-3, 1e-2, 1e-1, 1.0, 1.0])
        assert s[2] == 0 and s[3] == 3 and s[7] == 1.0
    dev = bm.DeviceBundle(ctx, sc)
    try:
        out = dev.run(**kw)
        print("bundle_adjust stop %s: history\n%s\nsummary %s" % (name, out["history"][:n_it], out["summary"]))
        worst, decided = compare(out, model, sc, n_it)
        print("bundle_adjust stop %s against the numpy model: largest deviation %.3g (bar 1e-9), %d of %d flags decided"
              % (name, worst, decided, n_it))
        assert decided == n_it
        oh, os_ = out["history"], out["summary"]
        T = len(sc["offsets"]) - 1
        if name == "min_decrease":
            # rows 1 .. 3: (cost, cost, lambda, 2) of the accepted step; the outputs are that step's, not the entry's
            np.testing.assert_array_equal(oh[1:4], [[oh[0, 1], oh[0, 1], 1e-4, 2.0]] * 3)
            assert os_[2] == 1 and os_[3] == 1 and os_[1] == oh[0, 1] and os_[7] == 1e-4
            assert (out["poses"][1:] != entry_p[1:]).any(axis=(1, 2)).all()
            assert (out["points3d"][:T, :3] != entry_x).any(axis=1).all()
        elif name == "lambda_min":
            assert (oh[1:3, 2] == 5e-4).all() and os_[7] == 5e-4  # exactly
        else:
            # never accepted: the poses and the points are the input bytes, column 3 the worst error at entry
            assert out["poses"].tobytes() == entry_p.tobytes()
            assert np.ascontiguousarray(out["points3d"][:T, :3]).tobytes() == entry_x.tobytes()
            want = worst_entry_error(sc, model)
            # pixel coordinates are of the order 1e3, an ulp there is 2e-13: 1e-10 px is a few hundred ulps
            assert np.abs(out["points3d"][:T, 3] - want)[model["used"]].max() <= 1e-10
            ran = 1 if name == "lambda_max" else 3
            assert (oh[:ran, 3] == 0).all() and np.isinf(oh[:ran, 1]).all() and (oh[:ran, 0] == os_[0]).all()
            np.testing.assert_array_equal(oh[1:ran, 2], 10.0 * oh[:ran - 1, 2])  # tenfold a row
            np.testing.assert_array_equal(oh[ran:n_it], [[os_[0], os_[0], 10.0 * oh[ran - 1, 2], 2.0]] * (n_it - ran))
            np.testing.assert_array_equal(os_[1:4], [os_[0], 0, ran])
            assert os_[7] == 10.0 * oh[ran - 1, 2] > kw["lambda_max"]
            if name == "lambda_max":
                np.testing.assert_array_equal(os_[2:], [0, 1, 800, 3308, 5, 1e-8])
        assert dev.records_back().tobytes() == dev.recs.tobytes()
        again = dev.run(**kw)
        for k in ("points3d", "poses", "history", "summary"):
            assert again[k].tobytes() == out[k].tobytes(), k  # the same bytes on every run
    finally:
        dev.close()


def test_refusals(ctx):
    from cusift_amd import capi

    sc = bm.scene_a()
    dev = bm.DeviceBundle(ctx, sc)
    try:
        host = [dev.points_in(), np.full((sc["n"], 12), FILL), np.full((100, 4), FILL), np.full(8, FILL)]
        for p, a in zip(dev.outs, host):
            ctx.h2d(p, a)
        ctx.synchronize()
        fx, fy, cx, cy = sc["cam"]
        flat = np.ascontiguousarray(sc["poses"].reshape(sc["n"], 12))
        many = np.tile(flat[:1], (257, 1))
        bad = [flat.copy() for _ in range(2)]
        bad[0][3, 7], bad[1][6, 0] = np.nan, np.inf
        d_recs, d_offsets, d_obs, d_stats = dev.ptrs
        d_x, d_poses, d_hist, d_sum = dev.outs
        good = dict(recs=d_recs, n=sc["n"], max_pts=sc["max_pts"], offsets=d_offsets, obs=d_obs, stats=d_stats,
                    cap=dev.cap, poses=flat.ctypes.data, fixed=None, cam=capi.Camera(fx, fy, cx, cy), par={}, x=d_x,
                    out=d_poses, hist=d_hist, summ=d_sum)
        cases = [dict(recs=None), dict(offsets=None), dict(obs=None), dict(stats=None), dict(poses=None), dict(cam=None),
                 dict(par=None), dict(x=None), dict(out=None), dict(hist=None), dict(summ=None),
                 dict(poses=bad[0].ctypes.data), dict(poses=bad[1].ctypes.data),
                 dict(cam=capi.Camera(0.0, fy, cx, cy)), dict(cam=capi.Camera(fx, np.inf, cx, cy)),
                 dict(cam=capi.Camera(fx, fy, np.nan, cy)), dict(cam=capi.Camera(fx, fy, cx, np.inf)),
                 dict(cam=capi.Camera(fx, fy, cx, cy, origin=np.nan)), dict(cap=-1), dict(n=4096, max_pts=1 << 20),
                 dict(n=-1), dict(n=65536), dict(max_pts=-1), dict(max_pts=(1 << 20) + 1),
                 dict(n=257, max_pts=4, poses=many.ctypes.data),
                 dict(par=dict(iterations=0)), dict(par=dict(iterations=101)), dict(par=dict(lam=0.0)),
                 dict(par=dict(lam=np.nan)), dict(par=dict(lam=np.inf)), dict(par=dict(lambda_min=0.0)),
                 dict(par=dict(lambda_min=np.nan)), dict(par=dict(lambda_max=-1.0)), dict(par=dict(lambda_max=np.nan)),
                 dict(par=dict(huber=-1.0)), dict(par=dict(huber=np.nan)), dict(par=dict(max_error=-1.0)),
                 dict(par=dict(max_error=np.nan)), dict(par=dict(min_decrease=-1e-30)),
                 dict(par=dict(min_decrease=np.nan))]
        for case in cases:
            a = dict(good, **case)
            par = None if a["par"] is None else capi.BundleParams(**a["par"])
            rc = capi.lib().cusift_bundle_adjust(ctx.handle, a["recs"], a["n"], a["max_pts"], a["offsets"], a["obs"],
                                                 a["stats"], a["cap"], a["poses"], a["fixed"],
                                                 C.byref(a["cam"]) if a["cam"] is not None else None,
                                                 C.byref(par) if par is not None else None, a["x"], a["out"], a["hist"],
                                                 a["summ"])
            assert rc == -1, (case, rc)  # CUSIFT_ERR_INVALID
        ctx.synchronize()
        for p, a in zip(dev.outs, host):
            back = np.empty_like(a)
            ctx.d2h(back, p)
            assert back.tobytes() == a.tobytes()  # nothing was enqueued
        # 256 frames are not refused (one record each, no track: every frame held, the poses come back)
        par = capi.BundleParams(iterations=1)
        d_many = ctx.malloc(8 * 12 * 256)
        try:
            rc = capi.lib().cusift_bundle_adjust(ctx.handle, d_recs, 256, 4, d_offsets, d_obs, d_stats, 0,
                                                 many.ctypes.data, None, C.byref(good["cam"]), C.byref(par), d_x, d_many,
                                                 d_hist, d_sum)
            assert rc == 0
            ctx.synchronize()
            back = np.empty((256, 12))
            ctx.d2h(back, d_many)
            assert back.tobytes() == many[:256].tobytes()
        finally:
            ctx.free(d_many)
    finally:
        dev.close()


def test_edges(ctx):
    sc = bm.scene_a()
    dev = bm.DeviceBundle(ctx, sc)
    try:
        # max_tracks below the track count clamps it: the first 300 tracks are the problem
        model = bm.run_model(sc, iterations=3, n_tracks=300)
        out = dev.run(max_tracks=300, iterations=3)
        compare(out, model, sc, 3, n_tracks=300, rows_in=dev.points_in())  # rows 300 .. 799 keep the scene's rows
        assert out["summary"][4] == 300
        # max_tracks == 0: the poses copied, zeros in the summary, no iteration run
        out = dev.run(max_tracks=0, iterations=3, lam=0.5)
        assert out["poses"].tobytes() == np.ascontiguousarray(sc["poses"]).tobytes()
        assert (out["summary"] == 0).all()
        np.testing.assert_array_equal(out["history"][:3], [[0, 0, 0.5, 2]] * 3)
        assert (out["history"][3:] == FILL).all() and out["points3d"].tobytes() == dev.points_in().tobytes()
    finally:
        dev.close()
    # d_stats[0] == 0 with room for tracks: nothing is used, every frame is held, stopped at entry
    dev = bm.DeviceBundle(ctx, sc, n_tracks=0)
    try:
        out = dev.run(iterations=2)
        assert out["poses"].tobytes() == np.ascontiguousarray(sc["poses"]).tobytes()
        np.testing.assert_array_equal(out["summary"], [0, 0, 0, 0, 0, 0, 0, 1e-3])
        np.testing.assert_array_equal(out["history"][:2], [[0, 0, 1e-3, 2]] * 2)
        assert out["points3d"].tobytes() == dev.points_in().tobytes()
        model = bm.run_model(sc, iterations=2, n_tracks=0)
        np.testing.assert_array_equal(model["summary"], out["summary"])
    finally:
        dev.close()
    # one frame: it is frame 0, held; the tracks' observations in it are fewer than two each, so nothing is used
    one = dict(sc, n=1, poses=sc["poses"][:1], xy=sc["xy"][:1])
    offsets, obs = [0], []
    for t in range(20):
        obs.append(t)
        offsets.append(len(obs))
    one["offsets"], one["obs"], one["points"] = np.asarray(offsets, np.int32), np.asarray(obs, np.int32), sc["points"][:20]
    dev = bm.DeviceBundle(ctx, one)
    try:
        out = dev.run(iterations=2)
        model = bm.run_model(one, iterations=2)
        compare(out, model, one, 2)
        assert out["summary"][4] == 0 and out["summary"][6] == 0 and (out["history"][:2, 3] == 2).all()
    finally:
        dev.close()
