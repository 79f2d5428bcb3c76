"""cusift_ctx_set_match_bits: the registrations' matcher front on the 8-bit path (cusift_amd/csrc/sift_register.hip:
match_enqueue and match_batch_launch; the tables in the context's scratch, sift_match8.hip).

YARDSTICKS.  Every equality is bit for bit, against a staged route of existing calls: quantize_descriptors on both record
sets, match8 (cross-check on: match8_mutual, then the host applies the mutual rule), then the staged estimate_* (RGB-D:
select_matches / select_mutual + estimate_rigid); the pair-list forms against the pair calls at seed + p.  The planted
frames are test_cross_check's many-to-one frames at about 300 records: frame 1 holds exact descriptor copies of some of
its records, so the mutual rule removes candidates.  The CPU test asserts from match8_model and the candidate rule alone
that the structure survives quantisation (at least 8 candidates with the cross-check on, strictly more with it off), so
no equality below is satisfied by the degenerate "no model" answer.  No tolerance appears in this file except the
end-to-end test's, which is test_cross_check's.
"""
import numpy as np
import pytest

import test_planar
from match8_model import match8_model, quantize_model
from oracle_binding import SIFT_POINT_DTYPE
from test_cross_check import MASK64, ONE_RECORD, PLANAR, SELECT, many_to_one, upload
from test_planar import candidates, corner_distance, improve, r32_of, warp
from test_rgbd import H, THRESH2, W, camera, intrinsics

MAX_PTS = 1024
LOOPS = 496
SEED = 0xBEEF
# (true records, exact copies, records of frame 2) of the planted pairs (0, 1) and (2, 3): frame 1 crosses the 8-bit
# matcher's 256-row block
PLANTED = {0: (250, 50, 280), 2: (230, 40, 300)}
KINDS = ("planar", "epipolar", "pose", "pnp", "rgbd")
MODEL_FIELD = {"planar": "homography", "epipolar": "fundamental", "pose": "fundamental", "pnp": "rt"}
EST = {"planar": dict(thresh=5.0, refine_loops=5, refine_thresh=3.0), "epipolar": dict(thresh=1.0, refine_loops=5, refine_thresh=1.0),
       "pose": dict(thresh=1.0, refine_loops=5, refine_thresh=1.0), "pnp": dict(thresh=2.0, refine_loops=5, refine_thresh=2.0)}


def with_xyz(f, metres=2.0):
    """coords3D of every record from its pixel at one depth, as a lift would give: PnP reads them from frame 1."""
    fx, fy, cx, cy = intrinsics()
    f = f.copy()
    x, y = f["coords2D"][:, 0].astype(np.float64), f["coords2D"][:, 1].astype(np.float64)
    f["coords3D"] = np.c_[(x - cx) / fx * metres, (y - cy) / fy * metres, np.full(len(f), metres)].astype(np.float32)
    return f


class Frames:
    """Six frames in 1024-record slots: planted pairs (0, 1) and (2, 3), 4 is empty, 5 holds 5 records."""

    def __init__(self):
        f1a, f2a, d1a, d2a, pa = many_to_one(*PLANTED[0], seed=41)
        f1b, f2b, d1b, d2b, pb = many_to_one(*PLANTED[2], seed=42)
        frames = [with_xyz(f) for f in (f1a, f2a, f1b, f2b, f2a[:0], f2b[:5])]
        self.partner = {0: pa, 2: pb}
        self.points = np.zeros((6, MAX_PTS), SIFT_POINT_DTYPE)
        self.points[:] = np.resize(frames[3], MAX_PTS)  # records past a count: live-looking
        for k, f in enumerate(frames):
            self.points[k, :len(f)] = f
        self.n = np.array([len(f) for f in frames])
        self.counters = self.n.astype(np.uint32)
        self.depth = np.stack([d1a, d2a, d1b, d2b, np.zeros_like(d1a), d2b])

    def frame(self, k):
        return self.points[k, :self.n[k]].copy()


@pytest.fixture(scope="module")
def frames():
    return Frames()


# every planted pair, frames on both sides, an empty frame on either side, 5 records, unrelated frames
PAIRS = np.array([(0, 1), (2, 3), (1, 3), (4, 1), (0, 4), (5, 3), (2, 1)], np.int32)


def rule_mask(m, distance, n2):
    """The candidate rule of PLANAR[distance] on match fields, restated."""
    a = PLANAR[distance]
    ok = (m["match"] >= 0) & (m["match"] < n2)
    if a["rule"] == 0:
        return ok & (m["score"] > np.float32(a["lo"])) & (m["ambiguity"] < np.float32(a["hi"]))
    return ok & (m["score"] < np.float32(a["lo"]) ** 2) & (m["ambiguity"] < np.float32(a["hi"]) ** 2)


# ------------------------------------------------------------------------------------------------------------------
# without a GPU
# ------------------------------------------------------------------------------------------------------------------
def test_planted_structure_survives_quantisation(frames):
    for a, (n_true, n_extra, n2) in PLANTED.items():
        f1, f2 = frames.frame(a), frames.frame(a + 1)
        q1, q2 = quantize_model(f1["data"]), quantize_model(f2["data"])
        assert q1[n_true:].tobytes() == q1[3 * np.arange(n_extra)].tobytes()  # a copy stays a copy
        for distance in (1, 0):
            fwd = match8_model(q1, q2, distance, f2["coords2D"])
            bwd = match8_model(q2, q1, distance, f1["coords2D"])
            keep = rule_mask(fwd, distance, n2)
            mutual = bwd["match"][fwd["match"]] == np.arange(len(f1))
            off, on = int(keep.sum()), int((keep & mutual).sum())
            print("pair (%d, %d) d%d: %d candidates, %d mutual" % (a, a + 1, distance, off, on))
            assert on >= 8 and off > on
            assert (off, on) == (n_true + n_extra, n_true)
            assert np.array_equal(fwd["match"][:n_true], frames.partner[a])


def test_setting_is_declared_exported_bound_and_checked():
    import ctypes as C
    import inspect
    import os

    from cusift_amd import batch, capi

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    extras = open(os.path.join(root, "include", "cusift_amd_extras.h")).read()
    assert "int cusift_ctx_set_match_bits(cusift_ctx *ctx, int bits);" in extras
    assert hasattr(C.CDLL(capi.LIB_PATH), "cusift_ctx_set_match_bits")
    res, args = capi.SIGNATURES["cusift_ctx_set_match_bits"]
    assert res is C.c_int and len(args) == 2
    assert capi.lib().cusift_ctx_set_match_bits(None, 8) == -1  # CUSIFT_ERR_INVALID: no context
    for bad in (7, 0, 16, -8, 8.0, "8", None, True):
        with pytest.raises(ValueError):
            capi.check_match_bits(bad)
    assert [capi.check_match_bits(v) for v in (32, 8, np.int32(8))] == [32, 8, 8]
    assert inspect.signature(batch.BatchExtractor.__init__).parameters["match_bits"].default == 32
    head = open(os.path.join(root, "include", "matching.h")).read()
    assert "inline void SetMatchBits(int bits)" in head and "MatchSiftData8Mutual(" in head


# ------------------------------------------------------------------------------------------------------------------
# on the GPU
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def own():
    """A context of this test's own: the session's shared context is never switched."""
    from cusift_amd import capi

    if capi.device_count() < 1:
        pytest.fail("gpu test selected but no HIP device is visible")
    c = capi.Context(0)
    yield c
    c.close()


def blob(x):
    """Every byte of a result: named tuples, lists, arrays, scalars, None."""
    if x is None:
        return b"none"
    if isinstance(x, (tuple, list)):
        return b"|".join(blob(v) for v in x)
    return np.ascontiguousarray(x).tobytes()


def same(x, y):
    """A pair-list form's entry against the pair call's value: scalars by value, arrays byte for byte."""
    if np.ndim(x) == 0:
        return np.ndim(y) == 0 and np.asarray(x).item() == np.asarray(y).item()
    return np.asarray(x).dtype == np.asarray(y).dtype and blob(x) == blob(y)


def estimate(ctx, kind, d1, n1, n2, distance, seed, **kw):
    args = dict(loops=LOOPS, seed=seed & MASK64, want_all=True, **EST[kind])
    args.update(PLANAR[distance])
    args.update(kw)
    if kind == "planar":
        return ctx.estimate_homography(d1, n1, n2, **args)
    if kind == "pnp":
        return ctx.estimate_pnp(d1, n1, camera(), n2, **args)
    epi = ctx.estimate_fundamental(d1, n1, n2, **args)
    if kind == "epipolar":
        return epi
    pose = ctx.estimate_pose(d1, n1, epi.fundamental, camera(), None, n2, rule=args["rule"], lo=args["lo"], hi=args["hi"],
                             thresh=args["refine_thresh"])
    return tuple(epi) + tuple(pose)


def register(ctx, kind, d1, n1, d2, n2, distance, seed, **kw):
    args = dict(loops=LOOPS, seed=seed & MASK64, want_all=True, distance=distance, **EST[kind])
    args.update(PLANAR[distance])
    args.update(kw)
    if kind == "planar":
        return ctx.register_planar(d1, n1, d2, n2, **args)
    if kind == "epipolar":
        return ctx.register_epipolar(d1, n1, d2, n2, **args)
    if kind == "pose":
        return ctx.register_pose(d1, n1, d2, n2, camera(), **args)
    return ctx.register_pnp(d1, n1, d2, n2, camera(), **args)


def fused_pair(ctx, kind, fr, a, b, distance, seed, **kw):
    """The registration `kind` of frames (a, b) on fresh uploads: (result, frame a afterwards, frame b afterwards)."""
    f1, f2 = fr.frame(a), fr.frame(b)
    b1, b2 = upload(ctx, f1 if len(f1) else ONE_RECORD), upload(ctx, f2 if len(f2) else ONE_RECORD)
    bufs = [b1, b2]
    try:
        if kind == "rgbd":
            e1, e2 = upload(ctx, fr.depth[a]), upload(ctx, fr.depth[b])
            bufs += [e1, e2]
            res = ctx.register_rgbd(b1.ptr, len(f1), e1.ptr, b2.ptr, len(f2), e2.ptr, W, H, camera(), distance=distance,
                                    loops=LOOPS, thresh2=THRESH2, kind="3d", seed=seed & MASK64, **SELECT)
        else:
            res = register(ctx, kind, b1.ptr, len(f1), b2.ptr, len(f2), distance, seed, **kw)
        return (res, b1.to_numpy(SIFT_POINT_DTYPE, (max(len(f1), 1),))[:len(f1)],
                b2.to_numpy(SIFT_POINT_DTYPE, (max(len(f2), 1),))[:len(f2)])
    finally:
        for x in bufs:
            x.free()


class Staged:
    """Frames (a, b) uploaded, quantised with cusift_quantize_descriptors and matched with match8 / match8_mutual."""

    def __init__(self, ctx, fr, a, b, distance, mutual, lift=False):
        from cusift_amd.capi import DeviceBuffer

        self.ctx, self.f1, self.f2 = ctx, fr.frame(a), fr.frame(b)
        self.n1, self.n2 = len(self.f1), len(self.f2)
        self.b1, self.b2 = upload(ctx, self.f1), upload(ctx, self.f2)
        self.bufs = [self.b1, self.b2]
        if lift:
            e1, e2 = upload(ctx, fr.depth[a]), upload(ctx, fr.depth[b])
            self.bufs += [e1, e2]
            ctx.lift_depth(self.b1.ptr, self.n1, e1.ptr, W, H, camera())
            ctx.lift_depth(self.b2.ptr, self.n2, e2.ptr, W, H, camera())
        t = [DeviceBuffer(ctx, n * k) for n in (self.n1, self.n2) for k in (128, 8)]
        self.bufs += t
        ctx.quantize_descriptors(self.b1.ptr, self.n1, t[0].ptr, t[1].ptr)
        ctx.quantize_descriptors(self.b2.ptr, self.n2, t[2].ptr, t[3].ptr)
        call = ctx.match8_mutual if mutual else ctx.match8
        call(self.b1.ptr, self.n1, t[0].ptr, t[1].ptr, self.b2.ptr, self.n2, t[2].ptr, t[3].ptr, distance)
        ctx.synchronize()
        self.m1 = self.b1.to_numpy(SIFT_POINT_DTYPE, (self.n1,))
        self.m2 = self.b2.to_numpy(SIFT_POINT_DTYPE, (self.n2,))

    def mutual_mask(self):
        ok = (self.m1["match"] >= 0) & (self.m1["match"] < self.n2)
        return ok & (self.m2["match"][np.where(ok, self.m1["match"], 0)] == np.arange(self.n1))

    def rigid(self, mutual, seed):
        ctx, n1 = self.ctx, self.n1
        out = [upload(ctx, np.full((n1, 2), -9, np.int32)), upload(ctx, np.full((n1, 6), -9.0, np.float32)),
               upload(ctx, np.full(1, -9, np.int32))]
        self.bufs += out
        select = ctx.select_mutual if mutual else ctx.select_matches
        select(self.b1.ptr, n1, self.b2.ptr, self.n2, out[0].ptr, out[1].ptr, out[2].ptr, kind="3d", **SELECT)
        ctx.synchronize()
        count = int(out[2].to_numpy(np.int32, (1,))[0])
        pairs, coord = out[0].to_numpy(np.int32, (n1, 2))[:count], out[1].to_numpy(np.float32, (n1, 6))[:count]
        rt, n_in, _, flags = ctx.estimate_rigid(coord, loops=LOOPS, thresh2=THRESH2, kind="3d", seed=seed)
        return rt, pairs, flags, n_in

    def free(self):
        for x in self.bufs:
            x.free()


def same_rgbd(fused, staged):
    (g_rt, g_pairs, g_flags, g_in), (rt, pairs, flags, n_in) = fused, staged
    return (g_rt.tobytes() == rt.tobytes() and g_in == n_in and g_pairs.tobytes() == pairs.tobytes() and
            np.array_equal(g_flags, flags))


# ---- 1. pair calls, cross-check off -------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
@pytest.mark.parametrize("kind", KINDS)
def test_pair_call_equals_the_staged_route(own, frames, kind, distance):
    a, b = 0, 1
    s = Staged(own, frames, a, b, distance, mutual=False, lift=kind == "rgbd")
    try:
        assert int(rule_mask(s.m1, distance, s.n2).sum()) == sum(PLANTED[a][:2])
        if kind == "rgbd":
            staged = s.rigid(False, SEED)
        else:
            staged = estimate(own, kind, s.b1.ptr, s.n1, s.n2, distance, SEED)
        after = s.b1.to_numpy(SIFT_POINT_DTYPE, (s.n1,))
        own.set_match_bits(8)
        fused, g1, g2 = fused_pair(own, kind, frames, a, b, distance, SEED)
        if kind == "rgbd":
            assert same_rgbd(fused, staged) and len(fused[1]) == sum(PLANTED[a][:2])
            assert g2["coords3D"].tobytes() == s.m2["coords3D"].tobytes()
            g2 = g2.copy()
            g2["coords3D"] = frames.frame(b)["coords3D"]
        else:
            assert blob(fused) == blob(staged), kind
            assert fused.num_candidates == sum(PLANTED[a][:2])
        assert g1.tobytes() == after.tobytes()  # the records of frame 1: the staged route's
        assert g2.tobytes() == frames.frame(b).tobytes()  # off: frame 2 is not written
    finally:
        s.free()


# ---- 2. pair calls, cross-check on --------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
@pytest.mark.parametrize("kind", ("planar", "epipolar", "pnp", "rgbd"))
def test_pair_call_with_cross_check_equals_the_staged_route(own, frames, kind, distance):
    a, b = 2, 3
    n_true = PLANTED[a][0]
    s = Staged(own, frames, a, b, distance, mutual=True, lift=kind == "rgbd")
    try:
        mutual = s.mutual_mask()
        assert int((rule_mask(s.m1, distance, s.n2) & mutual).sum()) == n_true
        if kind == "rgbd":
            staged = s.rigid(True, SEED)
            after = s.m1
        else:
            out = s.m1.copy()
            out["score"][~mutual] = -2.0 if PLANAR[distance]["rule"] == 0 else 1e30  # fails the rule in use
            d = upload(own, out)
            s.bufs.append(d)
            staged = estimate(own, kind, d.ptr, s.n1, s.n2, distance, SEED)
            after = d.to_numpy(SIFT_POINT_DTYPE, (s.n1,))
            after["score"] = s.m1["score"]
        own.set_match_bits(8)
        own.set_cross_check(True)
        fused, g1, g2 = fused_pair(own, kind, frames, a, b, distance, SEED)
        if kind == "rgbd":
            assert same_rgbd(fused, staged) and len(fused[1]) == n_true
        else:
            assert blob(fused) == blob(staged), kind
            assert fused.num_candidates == n_true
        assert g1.tobytes() == after.tobytes()
        assert g2.tobytes() == s.m2.tobytes()  # frame 2's records: match8_mutual's
    finally:
        s.free()


# ---- 3. the pair-list forms equal the pair calls ------------------------------------------------------------------------
def batch_call(ctx, kind, fr, distance, seed):
    pts, cnt = upload(ctx, fr.points), upload(ctx, fr.counters)
    bufs = [pts, cnt]
    try:
        common = dict(distance=distance, loops=LOOPS, seed=seed, **PLANAR[distance])
        if kind == "rgbd":
            dep = upload(ctx, fr.depth)
            bufs.append(dep)
            res = ctx.register_rgbd_batch(pts.ptr, cnt.ptr, 6, MAX_PTS, dep.ptr, W, H, camera(), PAIRS, distance=distance,
                                          loops=LOOPS, thresh2=THRESH2, kind="3d", seed=seed, **SELECT)
        elif kind == "planar":
            res = ctx.register_planar_batch(pts.ptr, cnt.ptr, 6, MAX_PTS, PAIRS, **common, **EST[kind])
        elif kind == "epipolar":
            res = ctx.register_epipolar_batch(pts.ptr, cnt.ptr, 6, MAX_PTS, PAIRS, **common, **EST[kind])
        elif kind == "pose":
            res = ctx.register_pose_batch(pts.ptr, cnt.ptr, 6, MAX_PTS, PAIRS, camera(), **common, **EST[kind])
        else:
            res = ctx.register_pnp_batch(pts.ptr, cnt.ptr, 6, MAX_PTS, PAIRS, camera(), **common, **EST[kind])
        after = pts.to_numpy(SIFT_POINT_DTYPE, (6, MAX_PTS))
        return res, after
    finally:
        for x in bufs:
            x.free()


@pytest.mark.gpu
@pytest.mark.parametrize("cross", (False, True))
@pytest.mark.parametrize("kind", KINDS)
def test_batch_forms_equal_the_pair_calls(own, frames, kind, cross):
    distance = 1
    own.set_match_bits(8)
    own.set_cross_check(cross)
    res, after = batch_call(own, kind, frames, distance, SEED)
    if kind != "rgbd":
        assert after.tobytes() == frames.points.tobytes()  # the records: never written
    busy = 0
    for p, (a, b) in enumerate(PAIRS):
        one, _, _ = fused_pair(own, kind, frames, a, b, distance, SEED + p, want_all=False)
        what = "%s pair %d (%d, %d) cross %d" % (kind, p, a, b, cross)
        if kind == "rgbd":
            rt, sel, flags, n_in = one
            assert res[0][p].tobytes() == rt.tobytes() and res[1][p] == len(sel) and res[2][p] == n_in, what
            assert res[3][p].tobytes() == sel.tobytes() and np.array_equal(res[4][p], flags), what
            busy += len(sel) >= 8
            continue
        n1 = int(frames.n[a])
        for f in (MODEL_FIELD[kind], "ransac", "num_candidates", "num_matches", "num_fit", "best_loop"):
            assert same(getattr(res, f)[p], getattr(one, f)), (what, f)
        assert res.counts[p] == n1 and np.array_equal(res.inliers[p], one.inliers[:n1]), what
        if kind == "pose":
            for f in ("rt", "num_front", "votes", "sigma"):
                assert same(getattr(res, f)[p], getattr(one, f)), (what, f)
        busy += one.num_candidates >= 8
        if a in PLANTED and b == a + 1:
            assert one.num_candidates == (PLANTED[a][0] if cross else sum(PLANTED[a][:2])), what
        if p in (3, 4, 5):  # an empty frame on either side, five records
            assert one.num_candidates < 8, what
    assert busy >= 2  # the two planted pairs run their RANSAC


# ---- 4. on, then off ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bits_32_after_8_is_the_default(own, frames):
    from cusift_amd import capi

    def everything(ctx):
        return ([fused_pair(ctx, k, frames, 0, 1, 1, 5) for k in KINDS], [batch_call(ctx, k, frames, 1, 5) for k in KINDS])

    own.set_match_bits(8)
    with8 = everything(own)
    own.set_match_bits(32)
    again = everything(own)
    fresh = capi.Context(0)
    try:
        want = everything(fresh)
    finally:
        fresh.close()
    for got, ref in zip(again[0] + again[1], want[0] + want[1]):
        assert blob(list(got)) == blob(list(ref))
    assert blob(list(with8[0][0])) != blob(list(again[0][0]))  # and the setting did something while it was 8


# ---- 5. the guided chains, bad values -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_guided_chains_refuse_and_bad_values_are_refused(own, frames):
    from cusift_amd import capi

    f1, f2 = frames.frame(0), frames.frame(1)
    b1, b2 = upload(own, f1), upload(own, f2)
    try:
        for bad in (7, 0, 16):
            with pytest.raises(ValueError):
                own.set_match_bits(bad)
            assert capi.lib().cusift_ctx_set_match_bits(own.handle, bad) == -1
        with pytest.raises(ValueError):
            capi.check_match_bits("8")
        assert own.match_bits == 32
        own.set_match_bits(8)
        assert capi.lib().cusift_ctx_set_match_bits(own.handle, 7) == -1 and own.match_bits == 8  # stays 8
        for chain in (own.register_planar_guided, own.register_epipolar_guided):
            with pytest.raises(capi.CusiftError):
                chain(b1.ptr, len(f1), b2.ptr, len(f2), loops=LOOPS, seed=1)
        own.synchronize()
        assert b1.to_numpy(SIFT_POINT_DTYPE, (len(f1),)).tobytes() == f1.tobytes()
        assert b2.to_numpy(SIFT_POINT_DTYPE, (len(f2),)).tobytes() == f2.tobytes()
        own.set_match_bits(32)
        own.register_planar_guided(b1.ptr, len(f1), b2.ptr, len(f2), loops=LOOPS, seed=1)  # and run again at 32
    finally:
        b1.free()
        b2.free()


# ---- 6. end to end ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_end_to_end_on_a_warped_frame_at_both_settings(oracle, gray1, record_property):
    """gray1 against itself warped by test_planar's homography, BatchExtractor(match_bits=32) and (match_bits=8): each run
    is held to the bound of test_cross_check's end-to-end test -- the corner error against the known homography is at most
    1.5 x that of the all-CPU route (oracle extraction and fp32 matcher, oracle RANSAC on the samples this run drew, numpy
    refit over the CPU candidates) plus r32.  No equality between the two settings is claimed."""
    import torch
    from cusift_amd.batch import BatchExtractor

    Hm = np.array([[0.98, -0.03, 9.0], [0.025, 1.01, -6.0], [1.5e-5, -2.0e-5, 1.0]])
    h, w = gray1.shape
    imgs = np.stack([gray1, warp(gray1, Hm)])
    prm = dict(num_octaves=4, init_blur=0.0, peak_thresh=1.0, max_pts=4096)
    kw = dict(distance=1, rule=1, lo=999.0, hi=0.8, loops=2000, thresh=5.0, refine_loops=5, refine_thresh=3.0, seed=21,
              want_all=True)
    truth = Hm.ravel()[:8] / Hm[2, 2]
    o1, o2 = oracle.extract(imgs[0], **prm).copy(), oracle.extract(imgs[1], **prm).copy()
    oracle.match(o1, o2, 1)
    cand = candidates(o1, 1, 999.0, 0.8, len(o2))
    saved = test_planar.CORNERS
    test_planar.CORNERS = np.array([[0, 0], [w, 0], [0, h], [w, h]], dtype=np.float64)
    try:
        for bits in (32, 8):
            ex = BatchExtractor(2, w, h, match_bits=bits, **prm)
            try:
                ex.extract(ex.images_from_numpy(imgs))
                torch.cuda.synchronize()
                dev1 = ex.to_host()[0].copy()
                res = ex.register_planar(0, 1, **kw)
            finally:
                ex.close()
            used = np.unique(res.drawn)
            key = lambda r: np.c_[r["coords2D"], r["scale"]].astype(np.float64)  # noqa: E731
            dist = np.abs(key(dev1[used])[:, None, :] - key(o1)[None, :, :]).max(axis=2)
            to_oracle = np.zeros(len(dev1), dtype=np.int32)
            to_oracle[used] = dist.argmin(axis=1)
            hom, _, _, _, _ = oracle.find_homography(o1, to_oracle[res.drawn], thresh=5.0)
            cpu = improve(o1, hom, 5, 3.0, cand).astype(np.float32)
            d_dev, d_cpu, r32 = corner_distance(res.homography[:8], truth), corner_distance(cpu, truth), r32_of(cpu)
            print("match_bits %d: %d candidates (%d on the CPU), %d inliers, corner error %.4f px, all-CPU %.4f px, r32 %.3g"
                  % (bits, res.num_candidates, len(cand), res.num_matches, d_dev, d_cpu, r32))
            record_property("inliers_match_bits_%d" % bits, int(res.num_matches))
            assert res.num_matches >= 50
            assert d_dev <= 1.5 * d_cpu + r32, (bits, d_dev, d_cpu, r32)
    finally:
        test_planar.CORNERS = saved
