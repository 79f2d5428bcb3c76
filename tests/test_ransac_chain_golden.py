"""The homography, fundamental-matrix and PnP registrations, byte for byte against recorded results.

The numpy-restatement suites (test_planar.py, test_epipolar.py, test_pnp.py, ...) pin each rule of the device chain --
mark, compact, solve, score, select -- on inputs of their own.  This one pins the chain's BYTES on the smallest input at
which every body the three models share can go wrong: 300 records a frame (two marking blocks, the second partial; four
full 64-point tiles and one of 44; five scoring splits of one tile each), about 200 candidates (the compacted list and
its coordinate rows differ from the records'), 100 hypotheses (two blocks, the second with 28 lanes past the end), five
refit rounds.  Coordinates lie on a planted model -- H, F and [R | t], one scene each -- with a third gross outliers, on a
quarter-pixel grid, so the input is exactly reproducible.  tests/golden/ransac_chain.json holds the SHA-256 of everything
each call returns or writes, recorded on an MI355X from the build BEFORE the score, mark, gather and null-vector bodies
of the three models were put on one template each (sift_ransac_chain.h), and of the input.  No tolerance, no key left
out.  `digests(ctx)` is the whole procedure; a new golden is `json.dump` of it, run against the build that is to be the
reference, never against the code under test.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle_binding import SIFT_POINT_DTYPE

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ransac_chain.json")
N, SLOTS, LOOPS, REFINE_LOOPS, PASS = 300, 320, 100, 5, 200
PAIRS = ((0, 1), (1, 0), (2, 0), (0, 2))  # frame 2 is empty: on either side of a pair
MODELS = ("h", "f", "p")
FEW = {"h": 7, "f": 7, "p": 5}  # one fewer than the model fits
RULES = {0: dict(rule=0, lo=0.85, hi=0.95), 1: dict(rule=1, lo=0.6, hi=0.9)}
CAM = (500.0, 500.0, 320.0, 240.0)
H_TRUE = ((1.02, 0.03, 12.0), (-0.02, 0.98, -7.5), (2e-5, -1e-5, 1.0))
R_TRUE = ((0.96, 0.0, 0.28), (0.0, 1.0, 0.0), (-0.28, 0.0, 0.96))  # X1 = R X2 + t; 0.96^2 + 0.28^2 = 1
T_TRUE = (-0.5, 0.05, 0.1)
GOOD, RIVALS = 170, 50  # descriptor roles of frame 0's records; the other 80 have no look-alike in frame 1
RECORD_FIELDS = ("match_error", "score", "ambiguity", "match", "match_xpos", "match_ypos")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def quarter(a):
    return np.round(a * 4.0) / 4.0


def project(X, Y, Z):
    return quarter(CAM[0] * X / Z + CAM[2]), quarter(CAM[1] * Y / Z + CAM[3])


def unit(d):
    """Rows of unit length, the norm a strictly sequential float64 sum."""
    return d / np.sqrt(np.cumsum(d * d, axis=1)[:, -1:])


def scene(model):
    """(frame 0, frame 1, partner): N records each; record i of frame 0 belongs to record partner[i] of frame 1.  Every
    product is written out element by element (no BLAS), every coordinate rounded to a quarter pixel (3-D: 1 / 64).

    Coordinates: frame 1 holds the model's image of frame 0's point, or -- a third of the records -- a random position.
    Descriptors: GOOD records have a near copy in frame 1 (their partner); RIVALS records of frame 0 are a NEARER copy of
    the partner of one good record each, so that partner's own best is the rival and the good record's match is not
    mutual; the rest and every partner of a record that is not good are unrelated vectors (an ambiguous match)."""
    rng = np.random.default_rng({"h": 20241021, "f": 20241022, "p": 20241023}[model])
    f0, f1 = np.zeros(N, SIFT_POINT_DTYPE), np.zeros(N, SIFT_POINT_DTYPE)
    if model == "h":
        x1 = rng.integers(0, 4 * 640, N) / 4.0
        y1 = rng.integers(0, 4 * 480, N) / 4.0
        (a, b, c), (d, e, f), (g, h, k) = H_TRUE
        w = (g * x1 + h * y1) + k
        x2, y2 = quarter(((a * x1 + b * y1) + c) / w), quarter(((d * x1 + e * y1) + f) / w)
    else:
        X, Y, Z = rng.integers(-128, 129, N) / 64.0, rng.integers(-96, 97, N) / 64.0, rng.integers(128, 385, N) / 64.0
        x1, y1 = project(X, Y, Z)
        dx, dy, dz = X - T_TRUE[0], Y - T_TRUE[1], Z - T_TRUE[2]
        X2, Y2, Z2 = ((R_TRUE[0][j] * dx + R_TRUE[1][j] * dy) + R_TRUE[2][j] * dz for j in range(3))  # R^T (X - t)
        x2, y2 = project(X2, Y2, Z2)
        if model == "p":
            f0["coords3D"] = np.stack([X, Y, Z], axis=1)
            f1["coords3D"] = np.round(np.stack([X2, Y2, Z2], axis=1) * 64.0) / 64.0
    gross = rng.permutation(N)[:N // 3]
    x2[gross] = rng.integers(0, 4 * 640, len(gross)) / 4.0
    y2[gross] = rng.integers(0, 4 * 480, len(gross)) / 4.0
    partner = rng.permutation(N).astype(np.int32)
    f0["coords2D"] = np.stack([x1, y1], axis=1)
    f1["coords2D"][partner] = np.stack([x2, y2], axis=1)
    roles = rng.permutation(N)
    good, rivals = roles[:GOOD], roles[GOOD:GOOD + RIVALS]
    d0 = unit(rng.standard_normal((N, 128)))
    sigma = np.full((N, 1), 0.5)
    sigma[good] = 0.03
    d1 = unit(d0 + sigma * rng.standard_normal((N, 128)))
    d0[rivals] = unit(d1[good[:RIVALS]] + 0.01 * rng.standard_normal((RIVALS, 128)))
    f0["data"] = d0.astype(np.float32)
    f1["data"][partner] = d1.astype(np.float32)
    for f in (f0, f1):
        f["score"], f["ambiguity"], f["match"] = 0.25, 0.5, -5  # what a matcher overwrites
        f["match_xpos"], f["match_ypos"], f["match_error"] = -77.0, -78.0, -79.0
    return f0, f1, partner


SCENES = {}


def scene_of(model):
    if model not in SCENES:
        SCENES[model] = scene(model)
    f0, f1, partner = SCENES[model]
    return f0.copy(), f1.copy(), partner.copy()


def matched(model, rule, passing=PASS):
    """Frame 0 of the scene with the match fields filled in by hand: `passing` records pass `rule`, the others fail it by
    the score or by the ambiguity in turn; four of those pass by the numbers and fail otherwise -- a NaN match_xpos, match
    = -1, match = N (with num_pts2 = N) and an infinite y1 (PnP: Z = 0)."""
    f0, f1, partner = scene_of(model)
    order = np.random.default_rng(77 + rule).permutation(N)
    ok, fail = order[:passing], order[PASS:]  # the same specials whatever `passing` is
    good, bad_score, bad_amb = ((0.9, 0.5), (0.8, 0.5), (0.9, 0.97)) if rule == 0 else ((0.25, 0.5), (0.5, 0.5), (0.25, 0.9))
    f0["match"] = partner
    f0["match_xpos"], f0["match_ypos"] = f1["coords2D"][partner, 0], f1["coords2D"][partner, 1]
    f0["score"], f0["ambiguity"] = bad_score
    f0["score"][order[1::2]], f0["ambiguity"][order[1::2]] = bad_amb
    f0["score"][ok], f0["ambiguity"][ok] = good
    f0["score"][fail[:4]], f0["ambiguity"][fail[:4]] = good
    f0["match_xpos"][fail[0]] = np.nan
    f0["match"][fail[1]] = -1
    f0["match"][fail[2]] = N
    if model == "p":
        f0["coords3D"][fail[3], 2] = 0.0
    else:
        f0["coords2D"][fail[3], 1] = np.inf
    return f0


def batch_of(model):
    """[3][SLOTS] = frame 0, frame 1, nothing; the slots past a count hold NaN descriptors."""
    f0, f1, _ = scene_of(model)
    batch = np.zeros((3, SLOTS), SIFT_POINT_DTYPE)
    batch["data"] = np.float32(np.nan)
    batch["coords2D"] = np.float32(50.0)
    batch[0, :N], batch[1, :N] = f0, f1
    return batch


def nearest(a, b):
    """(index of the nearest row of b, best / second-best squared distance) of every row of a, float64 numpy."""
    a, b = a.astype(np.float64), b.astype(np.float64)
    d2 = ((a * a).sum(axis=1)[:, None] + (b * b).sum(axis=1)[None, :]) - 2.0 * (a @ b.T)
    order = np.argsort(d2, axis=1, kind="stable")
    rows = np.arange(len(a))
    return order[:, 0], d2[rows, order[:, 0]] / d2[rows, order[:, 1]]


def input_digests():
    out = {}
    for m in MODELS:
        f0, f1, partner = scene_of(m)
        out.update({m + "/frame0": sha(f0), m + "/frame1": sha(f1), m + "/partner": sha(partner), m + "/batch": sha(batch_of(m))})
        for rule in RULES:
            out["%s/matched/rule%d" % (m, rule)] = sha(matched(m, rule))
            out["%s/few/rule%d" % (m, rule)] = sha(matched(m, rule, FEW[m]))
    return out


def digests(ctx):
    """{call/.../field: sha256} of everything the registration calls return and write for the inputs above."""
    from cusift_amd import capi
    from cusift_amd.capi import DeviceBuffer

    cam = capi.Camera(CAM[0], CAM[1], CAM[2], CAM[3], 0.0, 0.0, 7)
    kw = dict(loops=LOOPS, refine_loops=REFINE_LOOPS, seed=5)
    out = {}

    def put(key, res):
        for name, v in zip(res._fields, res):
            if isinstance(v, list):
                for p, a in enumerate(v):
                    out["%s.%s.%d" % (key, name, p)] = sha(a)
            else:
                out["%s.%s" % (key, name)] = sha(np.asarray(v))

    def put_records(key, buf):
        after = buf.to_numpy(SIFT_POINT_DTYPE, (N,))
        for f in RECORD_FIELDS:
            out["%s/%s" % (key, f)] = sha(after[f])

    estimate = {"h": lambda b, **o: ctx.estimate_homography(b, N, N, want_all=True, **o),
                "f": lambda b, **o: ctx.estimate_fundamental(b, N, N, want_all=True, **o),
                "p": lambda b, **o: ctx.estimate_pnp(b, N, cam, N, want_all=True, **o)}
    register = {"h": lambda a, b, **o: ctx.register_planar(a, N, b, N, want_all=True, **o),
                "f": lambda a, b, **o: ctx.register_epipolar(a, N, b, N, want_all=True, **o),
                "p": lambda a, b, **o: ctx.register_pnp(a, N, b, N, cam, want_all=True, **o)}
    batch = {"h": lambda p, c, **o: ctx.register_planar_batch(p, c, 3, SLOTS, PAIRS, want_errors=True, **o),
             "f": lambda p, c, **o: ctx.register_epipolar_batch(p, c, 3, SLOTS, PAIRS, want_errors=True, **o),
             "p": lambda p, c, **o: ctx.register_pnp_batch(p, c, 3, SLOTS, PAIRS, cam, want_errors=True, **o)}
    for m in MODELS:
        for rule, rule_args in RULES.items():
            for name, passing in (("estimate", PASS), ("few", FEW[m])):
                key = "%s/%s/rule%d" % (name, m, rule)
                buf = DeviceBuffer.from_numpy(ctx, matched(m, rule, passing))
                try:
                    put(key, estimate[m](buf.ptr, **dict(kw, **rule_args)))
                    put_records(key + "/records", buf)
                finally:
                    buf.free()
        d_pts = DeviceBuffer.from_numpy(ctx, batch_of(m))
        d_cnt = DeviceBuffer.from_numpy(ctx, np.array([N, N, 0], np.uint32))
        try:
            put("batch/" + m, batch[m](d_pts.ptr, d_cnt.ptr, **kw))
        finally:
            d_pts.free()
            d_cnt.free()
        f0, f1, _ = scene_of(m)
        b0, b1 = DeviceBuffer.from_numpy(ctx, f0), DeviceBuffer.from_numpy(ctx, f1)
        try:
            ctx.set_cross_check(True)
            put("cross/" + m, register[m](b0.ptr, b1.ptr, **kw))
            put_records("cross/%s/frame0" % m, b0)
            put_records("cross/%s/frame1" % m, b1)
        finally:
            ctx.set_cross_check(False)
            b0.free()
            b1.free()
    return out


def test_the_input_is_the_recorded_one_and_its_descriptors_make_a_share_of_the_matches_mutual():
    """FIRST: the random stream and the float arithmetic of `scene` give the recorded bytes.  If this fails the generated
    input changed (numpy's generator or its arithmetic), not the registration: the golden below then says nothing.  Then
    the shape of the input, from numpy's nearest neighbours: between a quarter and three quarters of the matches are
    mutual, and about 200 of the 300 pass the ambiguity rule of the fused calls (rule 1, hi = 0.8)."""
    want = json.load(open(GOLDEN))["input"]
    assert input_digests() == want, "the generated INPUT differs from the recorded one: not a registration change"
    for m in MODELS:
        f0, f1, partner = scene_of(m)
        fwd, amb = nearest(f0["data"], f1["data"])
        back, _ = nearest(f1["data"], f0["data"])
        mutual = (back[fwd] == np.arange(N)).mean()
        passing = int((amb < 0.8 * 0.8).sum())
        print("%s: %.3f of the matches mutual, %d pass the ambiguity rule, %d find their partner" %
              (m, mutual, passing, int((fwd == partner).sum())))
        assert 0.25 <= mutual <= 0.75, (m, mutual)
        assert 180 <= passing <= 240, (m, passing)
        for rule in RULES:
            assert sha(matched(m, rule)) != sha(matched(m, rule, FEW[m]))


@pytest.mark.gpu
def test_gpu_everything_the_three_registrations_return_and_write_has_the_recorded_bytes(ctx):
    golden = json.load(open(GOLDEN))
    # the input first, and plainly: a difference here is a change of the generated input, not of the registration
    assert input_digests() == golden["input"], "the generated INPUT differs from the recorded one: not a registration change"
    got, want = digests(ctx), golden["output"]
    assert sorted(got) == sorted(want)
    wrong = sorted(k for k in want if got[k] != want[k])
    assert not wrong, "%d of %d digests differ from the recorded bytes: %s" % (len(wrong), len(want), wrong[:12])
