"""The definitions of include/cusift_amd_extras.h for the 8-bit descriptors, restated in numpy (int64 for every integer):
cusift_quantize_descriptors, cusift_desc8_sums, cusift_match8.  Shared by the test_match8*.py files; no tolerance here."""
import numpy as np

FIELDS = ("score", "ambiguity", "match", "match_xpos", "match_ypos")
SCALE = np.float32(2.0 ** -18)
INIT = {1: np.float32(999.0), 0: np.float32(-1.0)}


def quantize_model(v):
    """uint8 of float32 v, the header's three expressions."""
    v = np.asarray(v, np.float32)
    with np.errstate(all="ignore"):
        t = np.float32(512.0) * v
        u = t + np.float32(0.5)
        assert t.dtype == np.float32 and u.dtype == np.float32
        small = u < np.float32(255.0)
        trunc = np.where(small & (v > 0), u, 0).astype(np.int64)  # (int)u truncates; u >= 0.5 here
        q = np.where(v > 0, np.where(small, trunc, 255), 0)
    return q.astype(np.uint8)


def sums_model(q):
    q = np.asarray(q, np.uint8).astype(np.int64)
    return np.stack([q.sum(-1), (q * q).sum(-1)], -1).astype(np.int32)


def keys_model(q1, q2, distance):
    """int64 [n1, n2]: D for distance 1, -S for distance 0.  The product runs through float64 (BLAS): every term is below
    2^16 and every sum below 2^24, so it is exact there, and it is converted back to int64 at once."""
    a, b = np.asarray(q1, np.uint8).astype(np.int64), np.asarray(q2, np.uint8).astype(np.int64)
    S = (a.astype(np.float64) @ b.T.astype(np.float64)).astype(np.int64)
    if distance == 1:
        return (a * a).sum(1)[:, None] + (b * b).sum(1)[None, :] - 2 * S
    return -S


def ambiguity_model(best, second, distance):
    best, second = best.astype(np.float64), second.astype(np.float64)
    with np.errstate(all="ignore"):
        if distance == 1:
            return (best / (second + 1e-6)).astype(np.float32)
        return ((1 - best) / (1 - second + 1e-6)).astype(np.float32)


def match8_model(q1, q2, distance, xy2):
    """The five fields cusift_match8 writes, as a dict of arrays [n1].  xy2: coords2D of set 2, float32 [n2, 2]."""
    K = keys_model(q1, q2, distance)
    n1, n2 = K.shape
    assert np.abs(K).max() < 2 ** 24
    idx = K.argmin(1)  # the lowest column among equals
    best = K[np.arange(n1), idx]
    sign = 1 if distance == 1 else -1
    score = (sign * best).astype(np.float32) * SCALE
    if n2 > 1:
        second_key = np.partition(K, 1, axis=1)[:, 1]  # second smallest of the multiset
        second = (sign * second_key).astype(np.float32) * SCALE
    else:
        second = np.full(n1, INIT[distance], np.float32)
    xy2 = np.asarray(xy2, np.float32)
    return {"score": score, "ambiguity": ambiguity_model(score, second, distance), "match": idx.astype(np.int32),
            "match_xpos": xy2[idx, 0].copy(), "match_ypos": xy2[idx, 1].copy()}


def assert_fields_equal(got, want, what):
    for f in FIELDS:
        g, w = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero(g.view(np.uint32) != w.view(np.uint32))
            raise AssertionError("%s: field %s differs in %d of %d rows, first row %d: got %r, want %r" %
                                 (what, f, len(bad), len(g), bad[0], g[bad[0]], w[bad[0]]))


# ---- the fp32 matcher, restated for the agreement test (L2 mode): 2 - 2 dot in float32 ------------------------------------
def fp32_l2_model(d1, d2):
    """(best, second, idx) of the float descriptors d1 [n1, 128] against d2 [n2, 128], float64 dots rounded to float32
    (the kernel's fp32 chain agrees to ~1e-7, far below the margins the agreement test works with)."""
    dot = (np.asarray(d1, np.float64) @ np.asarray(d2, np.float64).T).astype(np.float32)
    S = np.where(dot > -1, np.float32(2) - np.float32(2) * dot, np.float32(999)).astype(np.float32)
    idx = S.argmin(1)
    part = np.partition(S, 1, axis=1)
    return part[:, 0], part[:, 1], idx
