"""The guided registration chains (capi.Context.register_planar_guided / register_epipolar_guided) on planted scenes with
repeated structure: matches that the ratio test of the first pass must throw away come back in the guided pass.

The scenes.  400 records a side.  250 planted true matches (0.05 px of noise), 30 confidently matched gross outliers, 120
records of frame 1 without a partner.  Every record carries a descriptor 0.75 e_a + 0.5 e_b of its own (b = a + s mod 128,
s in 1..63, so no two descriptors are each other's mirror): dot products are exact in float32, a true match scores 2 - 2
* 0.8125 = 0.375 in L2 and nothing else scores below 0.875, so its ambiguity is at most 0.43.  120 of the true matches --
DUPLICATED -- have their descriptor copied to a decoy record of frame 2, at least 50 px from the true partner and (two
views) from the epipolar line.  The decoy stands 16 records in front of the partner -- the same lane of the matcher's scan,
seen first -- so the strict compare keeps it whatever the column splits are.

On "ambiguity exactly 1": a duplicated row has best == second bit for bit, and the matcher's ambiguity is then best / (best
+ 1e-6) -- the 1e-6 is part of the reference's formula -- which is 0.999997 for a score of 0.375, not 1; it rounds to 1
only for scores above 33, which an L2 score never is.  The condition asserted is therefore the tie itself and an ambiguity
above 0.9999, which no ratio threshold passes.
"""
import functools

import numpy as np
import pytest

from oracle_binding import SIFT_POINT_DTYPE
from test_match_guided import EPIPOLAR, HOMOGRAPHY, guide_mask
from test_matching_exact import ambiguity, auto_candidates, match_model, score_matrix

N, N_TRUE, N_DUP, N_OUT = 400, 250, 120, 30
W, H = 1280, 960
H_TRUE = np.array([1.01, 0.02, -15.0, -0.015, 0.99, 12.0, 1e-5, -8e-6, 1.0])
THRESH = {HOMOGRAPHY: 5.0, EPIPOLAR: 1.0}  # the calls' default thresh, which is the guided pass's radius
OPTS = dict(lo=1.0, loops=2000, seed=5)  # an L2 score below 1: a true match (0.375), not a stranger (2)


def fundamental():
    """F of a second camera 0.8 to the right, turned 0.15 about y: x2^T F x1 = 0; and (R, t, K)."""
    c, s = np.cos(0.15), np.sin(0.15)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    t = -R @ np.array([0.8, 0.0, 0.0])
    K = np.array([[1000.0, 0, W / 2], [0, 1000.0, H / 2], [0, 0, 1.0]])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    return Ki.T @ tx @ R @ Ki, R, t, K


def descriptor(ids):
    ids = np.asarray(ids)
    a, s = ids % 128, 1 + ids // 128
    assert (s <= 63).all()
    d = np.zeros((len(ids), 128), np.float32)
    d[np.arange(len(ids)), a] = 0.75
    d[np.arange(len(ids)), (a + s) % 128] = 0.5
    return d


def true_pairs(model, rng):
    """float64 (p1, p2) [N_TRUE, 2]: planted matches inside both images."""
    if model == HOMOGRAPHY:
        p1 = rng.uniform([40, 40], [W - 40, H - 40], size=(N_TRUE, 2))
        q = np.c_[p1, np.ones(N_TRUE)] @ H_TRUE.reshape(3, 3).T
        return p1, q[:, :2] / q[:, 2:]
    _, R, t, K = fundamental()
    p1, p2 = np.zeros((0, 2)), np.zeros((0, 2))
    while len(p1) < N_TRUE:
        X = rng.uniform([-3, -2, 3], [3, 2, 12], size=(4 * N_TRUE, 3))
        a, b = X @ K.T, (X @ R.T + t) @ K.T
        a, b = a[:, :2] / a[:, 2:], b[:, :2] / b[:, 2:]
        ok = ((a >= 0) & (a < [W, H]) & (b >= 0) & (b < [W, H])).all(axis=1)
        p1, p2 = np.r_[p1, a[ok]], np.r_[p2, b[ok]]
    return p1[:N_TRUE], p2[:N_TRUE]


def line_distance(F, p1, p2):
    l = np.c_[p1, np.ones(len(p1))] @ np.asarray(F).reshape(3, 3).T
    return np.abs((l[:, :2] * p2).sum(axis=1) + l[:, 2]) / np.hypot(l[:, 0], l[:, 1])


@functools.lru_cache(maxsize=None)
def scene(model):
    """(frame 1, frame 2, rows of the duplicated matches, their true partners, their decoys, the true model)."""
    rng = np.random.default_rng(40 + model)
    M = H_TRUE if model == HOMOGRAPHY else fundamental()[0].ravel()
    p1, p2 = true_pairs(model, rng)
    p1, p2 = p1 + rng.normal(0, 0.05, p1.shape), p2 + rng.normal(0, 0.05, p2.shape)
    # frame 2: of every 32 records (the first 12 such groups) ten hold decoys and the records 16 further on their
    # matches' partners; the other 160 slots take the partners of the 130 plain true matches and of the 30 outliers
    k = np.arange(N_DUP)
    decoy_at = 32 * (k // 10) + k % 10
    partner_dup = decoy_at + 16
    rest = np.setdiff1d(np.arange(N), np.r_[decoy_at, partner_dup])
    assert len(rest) == N - 2 * N_DUP == (N_TRUE - N_DUP) + N_OUT
    rest = rng.permutation(rest)
    partner = np.r_[partner_dup, rest[:N_TRUE - N_DUP]]  # of true match k; k < N_DUP are the duplicated ones
    out_partner = rest[N_TRUE - N_DUP:]
    f2 = np.zeros(N, SIFT_POINT_DTYPE)
    xy2 = rng.uniform([0, 0], [W, H], size=(N, 2))  # the outliers' partners keep these
    xy2[partner] = p2
    decoys = np.zeros((0, 2))
    while len(decoys) < N_DUP:  # far from the partner and from where the model allows a partner to be
        i = len(decoys)
        c = rng.uniform([0, 0], [W, H], size=(1, 2))
        far = np.hypot(*(c[0] - p2[i])) >= 50 and (model == HOMOGRAPHY or line_distance(M, p1[i:i + 1], c)[0] >= 50)
        decoys = np.r_[decoys, c] if far else decoys
    xy2[decoy_at] = decoys
    f2["coords2D"] = xy2.astype(np.float32)
    ids2 = np.zeros(N, int)
    ids2[partner], ids2[decoy_at], ids2[out_partner] = np.arange(N_TRUE), k, N_TRUE + np.arange(N_OUT)
    f2["data"] = descriptor(ids2)
    # frame 1: the true matches, the outliers with a partner, the rest without, shuffled
    perm = rng.permutation(N)
    f1 = np.zeros(N, SIFT_POINT_DTYPE)
    xy1 = rng.uniform([0, 0], [W, H], size=(N, 2))
    xy1[:N_TRUE] = p1
    f1["coords2D"] = xy1[perm].astype(np.float32)
    f1["data"] = descriptor(np.arange(N)[perm])  # ids N_TRUE + N_OUT .. N - 1 exist in frame 1 only
    row_of = np.argsort(perm)  # record of frame 1 that carries id u
    for f in (f1, f2):
        f["score"], f["ambiguity"], f["match"] = 0.25, 0.5, -5
        f.setflags(write=False)
    return f1, f2, row_of[:N_DUP], partner_dup, decoy_at, M


@pytest.mark.parametrize("model", (HOMOGRAPHY, EPIPOLAR))
def test_scene_meets_its_conditions(model):
    """What the GPU test relies on, asserted on the inputs alone: the plain matcher ties every duplicated row between its
    partner and the decoy and names the decoy, under every split the host can choose; the other true matches are
    unambiguous; every decoy fails the mask under the true model at the radius the chain uses, every partner passes."""
    f1, f2, dup_rows, partners, decoys, M = scene(model)
    S = score_matrix(f1["data"], f2["data"], 1)
    for cps in [1 << 30] + auto_candidates(N):
        best, second, idx = match_model(S, 1, cps)
        amb = ambiguity(best, second, 1)
        assert best[dup_rows].tobytes() == second[dup_rows].tobytes() and (best[dup_rows] == np.float32(0.375)).all()
        assert (amb[dup_rows] > 0.9999).all()  # see the module's note on "exactly 1"
        assert np.array_equal(idx[dup_rows], decoys)
        confident = (best < 1.0) & (amb < 0.64)  # rule 1 at lo = 1, hi = 0.8
        assert confident.sum() >= (N_TRUE - N_DUP) + N_OUT and not confident[dup_rows].any()
    mask = guide_mask(model, M, f1["coords2D"][dup_rows], f2["coords2D"], THRESH[model])
    assert not mask[np.arange(N_DUP), decoys].any()
    assert mask[np.arange(N_DUP), partners].all()
    far = np.hypot(*(f2["coords2D"][decoys] - f2["coords2D"][partners]).T.astype(np.float64))
    assert far.min() >= 49.9
    if model == EPIPOLAR:
        assert line_distance(M, f1["coords2D"][dup_rows].astype(np.float64), f2["coords2D"][decoys].astype(np.float64)).min() >= 49.9


@pytest.mark.gpu
@pytest.mark.parametrize("model", (HOMOGRAPHY, EPIPOLAR))
def test_guided_pass_recovers_the_duplicated_matches(ctx, model):
    from cusift_amd.capi import DeviceBuffer

    f1, f2, dup_rows, partners, decoys, _ = scene(model)
    chain = ctx.register_planar_guided if model == HOMOGRAPHY else ctx.register_epipolar_guided
    d1, d2 = DeviceBuffer.from_numpy(ctx, f1), DeviceBuffer.from_numpy(ctx, f2)
    try:
        plain, guided = chain(d1.ptr, N, d2.ptr, N, **OPTS)
        after = d1.to_numpy(SIFT_POINT_DTYPE, (N,))
        assert d2.to_numpy(SIFT_POINT_DTYPE, (N,)).tobytes() == f2.tobytes()
    finally:
        d1.free()
        d2.free()
    print("model %d: plain %d candidates, %d inliers, %d fit; guided %d candidates, %d inliers, %d fit" % (
        model, plain.num_candidates, plain.num_matches, plain.num_fit, guided.num_candidates, guided.num_matches,
        guided.num_fit))
    assert plain.num_matches >= 100 and not plain.inliers[dup_rows].any()
    assert guided.inliers[dup_rows].all()
    assert guided.num_fit >= plain.num_fit + N_DUP
    assert np.array_equal(after["match"][dup_rows], partners)
    assert (after["score"][dup_rows] == np.float32(0.375)).all()


@pytest.mark.gpu
def test_guided_chains_refuse_to_run_under_the_cross_check(ctx):
    from cusift_amd import capi
    from cusift_amd.capi import DeviceBuffer

    f1, f2 = scene(HOMOGRAPHY)[:2]
    d1, d2 = DeviceBuffer.from_numpy(ctx, f1), DeviceBuffer.from_numpy(ctx, f2)
    try:
        ctx.set_cross_check(True)
        for chain in (ctx.register_planar_guided, ctx.register_epipolar_guided):
            with pytest.raises(capi.CusiftError, match="cross-check"):
                chain(d1.ptr, N, d2.ptr, N, **OPTS)
        ctx.synchronize()
        assert d1.to_numpy(SIFT_POINT_DTYPE, (N,)).tobytes() == f1.tobytes()  # refused before anything ran
    finally:
        ctx.set_cross_check(False)
        d1.free()
        d2.free()
    assert ctx.cross_check is False
