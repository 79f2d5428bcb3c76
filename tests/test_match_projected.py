"""Matching by projection (cusift_match_projected, cusift_match_batch_projected; cusift_amd/csrc/sift_match_project.hip:
GuideP) held to zero tolerance: every field of every row.

The expectation is the matcher's model of tests/test_matching_exact.py applied to np.where(mask, S, INIT), as in
tests/test_match_guided.py.  `project_mask` restates the definition of include/cusift_amd_extras.h in numpy -- float64 per
row, float32 per pair, the same parenthesisation -- so the mask is the kernel's bit for bit; the descriptors are the exact
families of that file, so the scores are too.  The one tolerance in this file is the derived margin of
test_gpu_matches_lie_within_the_radius_by_the_pnp_test, which compares two different formulations.
"""
import numpy as np
import pytest

from oracle_binding import SIFT_POINT_DTYPE
from test_match_guided import SENTINEL, fields_of, guided_fields, nothing_fields, same_fields, scattered_pair
from test_matching_exact import assert_same_fields, auto_candidates, cols_per_split, exact_descriptors, records

REC = SIFT_POINT_DTYPE.itemsize
FIELDS = ("score", "ambiguity", "match", "match_xpos", "match_ypos")
CAM = (120.0, 115.0, 50.5, 49.5, 1.0)  # fx, fy, cx, cy, origin
RADIUS = 27.0
SHAPES = [(1, 1), (17, 33), (64, 31), (65, 257), (129, 160)]


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.sqrt(w @ w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def pose(p=0):
    """[R | t] row-major, 12 doubles; pair p's translation moves by 0.1 p along x.  (A step of 0.02 p moves a prediction
    by 0.5 to 2.4 pixels at these depths and changes 0.4 to 1 % of a mask's entries, by test_batch_poses_tell_the_pairs_apart's
    count: too little for that test's condition of 2 %, which is what lets the batch test tell one pair's pose from
    another's.  0.1 p gives 2.6 % at the least.)"""
    return np.hstack([rodrigues((0.02, -0.03, 0.015)), np.array([[0.05 + 0.1 * p], [-0.03], [0.04]])]).reshape(12)


RT = pose()


# ----------------------------------------------------------------------------------------------------------------------
# the definition, restated
# ----------------------------------------------------------------------------------------------------------------------
def intrinsics(cam):
    """(fx, fy, px, py) in float64 of a (fx, fy, cx, cy, origin) whose floats are widened first."""
    fx, fy, cx, cy, origin = (np.float64(np.float32(v)) for v in cam)
    return fx, fy, cx - origin, cy - origin


def predicted(rt, cam, X1):
    """(qx, qy) float32 [n1] and usable bool [n1]: the per-row half of the definition."""
    rt = np.asarray(rt, np.float64).reshape(12)
    fx, fy, px, py = intrinsics(cam)
    X1 = np.asarray(X1, np.float32).astype(np.float64)
    X, Y, Z = X1[:, 0], X1[:, 1], X1[:, 2]
    with np.errstate(all="ignore"):
        dx, dy, dz = X - rt[3], Y - rt[7], Z - rt[11]
        a = (rt[0] * dx + rt[4] * dy) + rt[8] * dz
        b = (rt[1] * dx + rt[5] * dy) + rt[9] * dz
        c = (rt[2] * dx + rt[6] * dy) + rt[10] * dz
        usable = (Z != 0) & (c > 0)
        qx = np.where(usable, (fx * a) / c + px, np.nan).astype(np.float32)
        qy = np.where(usable, (fy * b) / c + py, np.nan).astype(np.float32)
    return qx, qy, usable


def project_mask(rt, cam, X1, xy2, radius):
    """bool [n1, n2]: does column j pass the test against row i.  X1: float32 [n1, 3] coords3D, xy2: float32 [n2, 2]."""
    qx, qy, _ = predicted(rt, cam, X1)
    xy2 = np.asarray(xy2, np.float32)
    r2 = np.float32(radius) * np.float32(radius)
    with np.errstate(all="ignore"):
        ex, ey = xy2[None, :, 0] - qx[:, None], xy2[None, :, 1] - qy[:, None]
        out = ex * ex + ey * ey < r2
    assert out.dtype == bool and out.shape == (len(qx), len(xy2))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the inputs
# ----------------------------------------------------------------------------------------------------------------------
def lift(s1, rng, holes=True):
    """coords3D of every record: its own pixel back-projected at a depth of 1 to 4.75 in quarters; with holes, rows
    i % 7 == 3 have no depth (Z = 0) and rows i % 7 == 5 lie behind the camera (Z negated)."""
    fx, fy, px, py = intrinsics(CAM)
    z = rng.integers(4, 20, len(s1)) / 4.0
    xy = s1["coords2D"].astype(np.float64)
    X = np.stack([(xy[:, 0] - px) / fx * z, (xy[:, 1] - py) / fy * z, z], axis=1)
    i = np.arange(len(s1))
    if holes:
        X[i % 7 == 3, 2] = 0.0
        X[i % 7 == 5, 2] *= -1.0
    s1["coords3D"] = X.astype(np.float32)
    return s1


def unusable_rows(n):
    i = np.arange(n)
    return (i % 7 == 3) | (i % 7 == 5)


def projected_pair(n1, n2, family, holes=True, seed=3):
    s1, s2 = scattered_pair(n1, n2, family, seed)
    lift(s1, np.random.default_rng(1000 + seed), holes)
    if (n1, n2) == (1, 1):  # one pair cannot pass by a fifth: it passes
        s2["coords2D"][0] = s1["coords2D"][0]
    return s1, s2


# ----------------------------------------------------------------------------------------------------------------------
# without a GPU: the restatement on hand-made cases, and the conditions on the GPU tests' inputs
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ("sparse16", "ties"))
@pytest.mark.parametrize("n1,n2", SHAPES)
def test_a_tenth_to_a_third_pass_and_unusable_rows_pass_nothing(n1, n2, family):
    s1, s2 = projected_pair(n1, n2, family)
    mask = project_mask(RT, CAM, s1["coords3D"], s2["coords2D"], RADIUS)
    bad = unusable_rows(n1)
    print("(%d, %d): %.1f %% of the pairs pass, %.1f %% of the usable rows'" %
          (n1, n2, 100 * mask.mean(), 100 * mask[~bad].mean()))
    if n1 * n2 > 1:
        assert 0.10 <= mask.mean() <= 0.30, mask.mean()
        assert bad.any()
    else:
        assert mask.all()
    assert not mask[bad].any()
    assert np.array_equal(predicted(RT, CAM, s1["coords3D"])[2], ~bad)
    assert not project_mask(RT, CAM, s1["coords3D"], s2["coords2D"], np.inf)[bad].any()


def test_nan_and_infinite_rows_pass_nothing():
    s1, s2 = projected_pair(17, 33, "sparse16", holes=False)
    X = s1["coords3D"].copy()
    X[0, 0], X[1, 1], X[2, 2], X[4, 0], X[5, 2], X[6] = np.nan, np.nan, np.nan, np.inf, np.inf, -np.inf
    for radius in (RADIUS, 1e6, np.inf):
        mask = project_mask(RT, CAM, X, s2["coords2D"], radius)
        assert not mask[[0, 1, 2, 4, 5, 6]].any()
        assert mask[[3, 7, 8]].any(axis=1).all()


def test_radius_is_strict():
    ident = np.hstack([np.eye(3), np.zeros((3, 1))])
    cam = (100.0, 100.0, 0.0, 0.0, 0.0)
    X1, x2 = np.array([[0.2, 0.4, 2.0]], np.float32), np.array([[13, 24]], np.float32)  # projects to (10, 20)
    assert predicted(ident, cam, X1)[0][0] == 10 and predicted(ident, cam, X1)[1][0] == 20
    assert not project_mask(ident, cam, X1, x2, 5.0)[0, 0]  # 25 < 25 is false
    assert project_mask(ident, cam, X1, x2, np.nextafter(np.float32(5), np.float32(np.inf)))[0, 0]
    assert project_mask(ident, cam, X1, x2, np.inf)[0, 0]


def test_zero_nan_and_infinite_poses_pass_nothing():
    s1, s2 = projected_pair(17, 33, "sparse16", holes=False)
    for rt in (np.zeros(12), np.full(12, np.nan), np.r_[RT[:11], np.nan], np.full(12, np.inf), np.r_[np.nan, RT[1:]]):
        for radius in (1.0, 1e6, np.inf):
            assert not project_mask(rt, CAM, s1["coords3D"], s2["coords2D"], radius).any()


def test_a_point_on_the_principal_plane_passes_nothing():
    rt = np.hstack([np.eye(3), np.array([[0.0], [0.0], [1.5]])])  # c = Z - 1.5
    X1 = np.array([[0.1, 0.2, 1.5], [0.0, 0.0, 1.5], [0.1, 0.2, 1.25], [0.0, 0.0, 2.5]], np.float32)
    x2 = np.array([[49.5, 48.5], [0, 0], [1e30, 1e30]], np.float32)
    for radius in (1.0, 1e6, np.inf):
        got = project_mask(rt, CAM, X1, x2, radius)
        assert not got[:3].any()  # c == 0 twice, c < 0 once
        assert got[3, 0]  # the principal point


BATCH_MAX = 160
BATCH_COUNTERS = np.array([95, 160, 33], np.uint32)
BATCH_PAIRS = np.array([(0, 1), (1, 0), (2, 2), (0, 2)], np.int32)


def batch_scene():
    rng = np.random.default_rng(11)
    frames = []
    for _ in range(3):
        p = records(exact_descriptors(rng, BATCH_MAX, "ties"))
        p["coords2D"] = (rng.integers(0, 400, (BATCH_MAX, 2)) / 4.0).astype(np.float32)
        frames.append(lift(p, rng))
    points = np.stack(frames)
    rts = np.stack([pose(p) for p in range(len(BATCH_PAIRS))])

    def mask_of(p, rt):
        a, b = BATCH_PAIRS[p]
        return project_mask(rt, CAM, points[a, :BATCH_COUNTERS[a]]["coords3D"], points[b, :BATCH_COUNTERS[b]]["coords2D"],
                            RADIUS)

    return points, rts, mask_of


def test_batch_poses_tell_the_pairs_apart():
    _, rts, mask_of = batch_scene()
    masks = [mask_of(p, rts[p]) for p in range(len(BATCH_PAIRS))]
    assert all(0.10 <= m.mean() <= 0.30 for m in masks), [m.mean() for m in masks]
    for p in range(len(BATCH_PAIRS)):  # another pair's pose would show
        other = [(masks[p] != mask_of(p, rts[o])).mean() for o in range(len(BATCH_PAIRS)) if o != p]
        assert min(other) > 0.02, (p, other)


# ----------------------------------------------------------------------------------------------------------------------
# on the GPU
# ----------------------------------------------------------------------------------------------------------------------
def gpu_projected(ctx, s1, s2, distance, rt, radius, splits=0, lead2=0, n1=None, n2=None, both=False, cam=CAM):
    """cusift_match_projected with POLICY_MATCH_SPLITS = splits over uploads of the whole arrays, as gpu_guided of
    test_match_guided.py.  Returns all of s1 read back (both=True: and all of s2)."""
    from cusift_amd import capi
    from cusift_amd.capi import DeviceBuffer

    n1 = len(s1) if n1 is None else n1
    n2 = len(s2) - lead2 if n2 is None else n2
    d1, d2 = DeviceBuffer.from_numpy(ctx, s1), DeviceBuffer.from_numpy(ctx, s2)
    try:
        ctx.set_policy(capi.POLICY_MATCH_SPLITS, splits)
        ctx.match_projected(d1.ptr, n1, d2.ptr + lead2 * REC, n2, rt, capi.Camera(*cam), radius, distance)
        ctx.synchronize()
        out1, out2 = d1.to_numpy(SIFT_POINT_DTYPE, (len(s1),)), d2.to_numpy(SIFT_POINT_DTYPE, (len(s2),))
    finally:
        ctx.set_policy(capi.POLICY_MATCH_SPLITS, 0)
        d1.free()
        d2.free()
    return (out1, out2) if both else out1


def match_field_mask():
    mask = np.zeros(REC, bool)
    for f in FIELDS:
        off = SIFT_POINT_DTYPE.fields[f][1]
        mask[off:off + 4] = True
    assert mask.sum() == 20
    return mask


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
@pytest.mark.parametrize("family", ("sparse16", "ties"))
@pytest.mark.parametrize("n1,n2", SHAPES)
def test_gpu_every_field_every_row(ctx, n1, n2, family, distance):
    s1, s2 = projected_pair(n1, n2, family)
    mask = project_mask(RT, CAM, s1["coords3D"], s2["coords2D"], RADIUS)
    assert (0.10 <= mask.mean() <= 0.30) if n1 * n2 > 1 else mask.all()
    bad = unusable_rows(n1)
    nothing = nothing_fields(n1, distance, s2)
    before1, before2 = s1.copy().view(np.uint8).reshape(-1, REC), s2.copy()
    outside = ~match_field_mask()
    models = {}

    def want(cps):
        if cps not in models:
            models[cps] = guided_fields(s1, s2, distance, cps, mask)
        return models[cps]

    def check(got, got2, what):
        for f in FIELDS:  # every unusable row is the "nothing passes" row
            assert np.ascontiguousarray(got[f][bad]).tobytes() == nothing[f][bad].tobytes(), (what, f)
        assert np.array_equal(got.view(np.uint8).reshape(-1, REC)[:, outside], before1[:, outside]), what
        assert got2.tobytes() == before2.tobytes(), what

    for k in (1, 2, 3, 1000):
        what = "(%d, %d) %s d%d, %d splits asked" % (n1, n2, family, distance, k)
        got, got2 = gpu_projected(ctx, s1, s2, distance, RT, RADIUS, k, both=True)
        assert_same_fields(fields_of(got), want(cols_per_split(n2, k)), what)
        check(got, got2, what)
    got, got2 = gpu_projected(ctx, s1, s2, distance, RT, RADIUS, 0, both=True)
    cands = auto_candidates(n2)
    if not any(same_fields(fields_of(got), want(c)) for c in cands):
        assert_same_fields(fields_of(got), want(cands[-1]), "automatic splits (none of %s columns per split fits)" % cands)
    check(got, got2, "automatic splits")


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
@pytest.mark.parametrize("n1,n2", [(1, 1), (65, 257)])
def test_gpu_radius_1e6_equals_cusift_match(ctx, n1, n2, distance):
    from test_matching_exact import gpu_match

    for family in ("sparse16", "ties"):
        s1, s2 = projected_pair(n1, n2, family, holes=False)
        assert project_mask(RT, CAM, s1["coords3D"], s2["coords2D"], 1e6).all()
        for k in (1, 2, 0):
            plain = gpu_match(ctx, s1, s2, distance, k)
            got = gpu_projected(ctx, s1, s2, distance, RT, 1e6, k)
            assert_same_fields(fields_of(got), fields_of(plain), "%s, %d splits" % (family, k))
            assert got.tobytes() == plain.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("lead2", (1, 3))
def test_gpu_record_offset_of_image_2(ctx, lead2):
    """d_sift2 starts `lead2` records into its buffer, in front of and behind records that would win every row and lie
    where every row projects if the staging used the allocation's base; image 1's records end in front of sentinel
    bytes."""
    n1, n2 = 70, 95
    s1, s2 = projected_pair(n1, n2, "sparse16", seed=lead2)
    rng = np.random.default_rng(lead2)
    buf2 = records(np.full((lead2 + n2 + 40, 128), 64.0, np.float32))
    buf2["coords2D"] = (rng.integers(0, 400, (len(buf2), 2)) / 4.0).astype(np.float32)
    buf2[lead2:lead2 + n2] = s2
    raw1 = np.full((n1 + 70, REC), SENTINEL, np.uint8)
    buf1 = raw1.view(SIFT_POINT_DTYPE).reshape(-1)
    buf1[:n1] = s1
    before1, before2 = buf1.copy().view(np.uint8).reshape(-1, REC), buf2.copy()
    mask = project_mask(RT, CAM, s1["coords3D"], s2["coords2D"], RADIUS)
    assert 0.10 <= mask.mean() <= 0.30
    for distance in (1, 0):
        for k in (1, 2):
            what = "lead %d, d%d, %d splits" % (lead2, distance, k)
            got, got2 = gpu_projected(ctx, buf1, buf2, distance, RT, RADIUS, k, lead2=lead2, n1=n1, n2=n2, both=True)
            assert_same_fields(fields_of(got[:n1]), guided_fields(s1, s2, distance, cols_per_split(n2, k), mask), what)
            assert np.array_equal(got.view(np.uint8).reshape(-1, REC)[n1:], before1[n1:]), what
            assert got2.tobytes() == before2.tobytes(), what


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
def test_gpu_batch_rows_equal_the_pair_call(ctx, distance):
    """Three frames of 95, 160 and 33 records in 160-record slots, four pairs, a pose of its own per pair: pair p's rows
    are the fields the pair call writes under pose p (and the numpy model's), rows past frame 1's count keep their bytes,
    the records are not written."""
    from cusift_amd import capi
    from cusift_amd.capi import DeviceBuffer

    points, rts, mask_of = batch_scene()
    masks = [mask_of(p, rts[p]) for p in range(len(BATCH_PAIRS))]
    for k in (1, 2):
        d_pts, d_cnt = DeviceBuffer.from_numpy(ctx, points), DeviceBuffer.from_numpy(ctx, BATCH_COUNTERS)
        d_rows = DeviceBuffer.from_numpy(ctx, np.full((len(BATCH_PAIRS), BATCH_MAX, 16), SENTINEL, np.uint8))
        try:
            ctx.set_policy(capi.POLICY_MATCH_SPLITS, k)
            ctx.match_batch_projected(d_pts.ptr, d_cnt.ptr, 3, BATCH_MAX, BATCH_PAIRS, rts, capi.Camera(*CAM), RADIUS,
                                      d_rows.ptr, distance)
            ctx.synchronize()
        finally:
            ctx.set_policy(capi.POLICY_MATCH_SPLITS, 0)
        assert d_pts.to_numpy(SIFT_POINT_DTYPE, points.shape).tobytes() == points.tobytes()
        rows = d_rows.to_numpy(capi.MatchRow, (len(BATCH_PAIRS), BATCH_MAX))
        for d in (d_pts, d_cnt, d_rows):
            d.free()
        cps = cols_per_split(BATCH_MAX, k)  # the batch sizes its splits from max_pts
        for p, (a, b) in enumerate(BATCH_PAIRS):
            na, nb = int(BATCH_COUNTERS[a]), int(BATCH_COUNTERS[b])
            s1, s2 = points[a, :na].copy(), points[b, :nb].copy()
            what = "pair %d (%d, %d), %d splits" % (p, a, b, k)
            want = guided_fields(s1, s2, distance, cps, masks[p])
            for f in ("score", "ambiguity", "match"):
                assert rows[f][p, :na].tobytes() == want[f].tobytes(), (what, f)
            assert (rows["reserved"][p, :na] == 0).all(), what
            assert (rows[p, na:].view(np.uint8) == SENTINEL).all(), what
            if cols_per_split(nb, k) == cps or k == 1:  # the pair call sizes its splits from n2: the same scan
                pair = gpu_projected(ctx, s1, s2, distance, rts[p], RADIUS, k)
                for f in ("score", "ambiguity", "match"):
                    assert rows[f][p, :na].tobytes() == np.ascontiguousarray(pair[f]).tobytes(), (what, f)


@pytest.mark.gpu
def test_gpu_refusals_write_nothing(ctx):
    from cusift_amd import capi
    from cusift_amd.capi import DeviceBuffer

    s1, s2 = projected_pair(70, 95, "sparse16")
    d1, d2 = DeviceBuffer.from_numpy(ctx, s1), DeviceBuffer.from_numpy(ctx, s2)
    pts = np.stack([lift(s2.copy(), np.random.default_rng(0)), s2])
    d_pts = DeviceBuffer.from_numpy(ctx, pts)
    d_rows = DeviceBuffer.from_numpy(ctx, np.full((1, 95, 16), SENTINEL, np.uint8))
    good = capi.Camera(*CAM)
    nan, inf = float("nan"), float("inf")
    cams = [None] + [capi.Camera(*c) for c in (
        (0.0, 115.0, 50.5, 49.5, 1.0), (120.0, 0.0, 50.5, 49.5, 1.0), (nan, 115.0, 50.5, 49.5, 1.0),
        (120.0, inf, 50.5, 49.5, 1.0), (120.0, 115.0, nan, 49.5, 1.0), (120.0, 115.0, 50.5, -inf, 1.0),
        (120.0, 115.0, 50.5, 49.5, nan))]
    bad = [(RT, cam, 5.0) for cam in cams] + [(None, good, 5.0), (RT, good, 0.0), (RT, good, -1.0), (RT, good, nan)]
    for rt, cam, radius in bad:
        with pytest.raises(capi.CusiftError):
            ctx.match_projected(d1.ptr, 70, d2.ptr, 95, rt, cam, radius, 1)
        with pytest.raises(capi.CusiftError):
            ctx.match_batch_projected(d_pts.ptr, None, 2, 95, [(0, 1)], rt, cam, radius, d_rows.ptr, 1)
    # what cusift_match and cusift_match_batch refuse
    for call in (lambda: ctx.match_projected(d1.ptr, 70, d2.ptr, 95, RT, good, 5.0, 2),
                 lambda: ctx.match_projected(None, 70, d2.ptr, 95, RT, good, 5.0, 1),
                 lambda: ctx.match_projected(d1.ptr, 70, None, 95, RT, good, 5.0, 1),
                 lambda: ctx.match_batch_projected(d_pts.ptr, None, 2, 95, [(0, 1)], RT, good, 5.0, d_rows.ptr, 2),
                 lambda: ctx.match_batch_projected(d_pts.ptr, None, 2, 95, [(0, 2)], RT, good, 5.0, d_rows.ptr, 1),
                 lambda: ctx.match_batch_projected(None, None, 2, 95, [(0, 1)], RT, good, 5.0, d_rows.ptr, 1),
                 lambda: ctx.match_batch_projected(d_pts.ptr, None, 2, 95, [(0, 1)], RT, good, 5.0, None, 1)):
        with pytest.raises(capi.CusiftError):
            call()
    ctx.synchronize()
    assert d1.to_numpy(SIFT_POINT_DTYPE, (70,)).tobytes() == s1.tobytes()
    assert d2.to_numpy(SIFT_POINT_DTYPE, (95,)).tobytes() == s2.tobytes()
    assert d_pts.to_numpy(SIFT_POINT_DTYPE, pts.shape).tobytes() == pts.tobytes()
    assert (d_rows.to_numpy(np.uint8, (1, 95, 16)) == SENTINEL).all()
    # counts <= 0: fine, and nothing happens -- whatever the geometry says
    ctx.match_projected(d1.ptr, 0, d2.ptr, 95, None, None, -1.0, 1)
    ctx.match_projected(d1.ptr, 70, d2.ptr, 0, None, None, -1.0, 1)
    ctx.synchronize()
    assert d1.to_numpy(SIFT_POINT_DTYPE, (70,)).tobytes() == s1.tobytes()
    # an infinite radius is legal, and so is a pose that is not finite: it passes nothing
    ctx.match_projected(d1.ptr, 70, d2.ptr, 95, np.full(12, np.nan), good, np.inf, 1)
    ctx.synchronize()
    got = d1.to_numpy(SIFT_POINT_DTYPE, (70,))
    assert_same_fields(fields_of(got), nothing_fields(70, 1, s2), "a NaN pose at an infinite radius")
    assert d2.to_numpy(SIFT_POINT_DTYPE, (95,)).tobytes() == s2.tobytes()
    for d in (d1, d2, d_pts, d_rows):
        d.free()


@pytest.mark.gpu
@pytest.mark.parametrize("radius", (RADIUS, 5.0))
def test_gpu_matches_lie_within_the_radius_by_the_pnp_test(ctx, radius):
    """Every row that found a match has, by the reprojection error of cusift_estimate_pnp (tests/test_pnp.py:
    match_error, fp64 and without the division per row), an error below radius + 2e-3 px.  The margin is the float32
    rounding of a pixel coordinate below 4,096 -- half an ulp is 2.4e-4 -- once for qx and once for the difference, with
    a factor of four to spare: derived, not measured."""
    from test_pnp import cam_of, coords5, match_error

    s1, s2 = projected_pair(129, 160, "sparse16")
    got = gpu_projected(ctx, s1, s2, 1, RT, radius)
    found = got["match"] >= 0
    assert found.sum() >= 30 and not found[unusable_rows(129)].any()
    err = match_error(RT, cam_of(CAM), coords5(got))[found]
    print("radius %g: %d rows matched, largest reprojection error %.6f px, largest excess over the radius %.3g px" %
          (radius, found.sum(), err.max(), (err - radius).max()))
    assert np.isfinite(err).all() and (err < radius + 2e-3).all()
