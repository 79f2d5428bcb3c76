"""Batched RGB-D sequence registration: cusift_match_batch, cusift_register_rgbd_batch (cusift_amd/csrc/sift_match.hip,
sift_sequence.hip, the pair dimension of sift_rigid.hip), BatchExtractor.register_sequence, capi.chain_poses and
include/rgbd.h: RegisterRGBDSequence.

The yardstick is the pair route that exists already -- cusift_match and cusift_register_rgbd, called pair by pair on
copies of the same records -- and, for the fixture pair, MATLAB's Rt1_2 through the bounds of tests/test_rgbd.py.

Bounds:
  * match rows: score and ambiguity bit-identical on every row.  A (row, column) dot product is the same k-ordered MFMA
    chain however the columns are split, best and second-best are order-free minima, and the ambiguity is one double
    division of the two.  `match` identical except on rows whose best score is shared by two columns exactly: there the
    column splits (sized from max_pts in the batch, from the count in the pair call) decide which of the equals is
    named.  Such a row shows in the pair route's own output as second == best, i.e.
    ambiguity == float32(float64(score) / (float64(score) + 1e-6)) for L2; at most 1 % of a pair's rows may be such.
    One mend of that rule: a best score of exactly 0 (a frame matched against itself or against a cut of itself, pairs
    (0, 2) and (1, 1): 10 of 884 rows of (0, 2)) makes the ambiguity 0 whatever the second-best is, so the equation
    holds without a tie.  Such a row is exempt only if the two routes name different columns AND those two columns
    hold identical descriptors -- a tie that can be seen; otherwise its `match` must be identical like any other row's.
    The exempt rows are a subset of the rule's, and the 1 % bound is applied to them.
  * registration: every output bit-identical to cusift_register_rgbd(seed + p).  A tie row has an ambiguity of about 1
    and is never selected at 0.6, so no exemption applies.
  * chain_poses: 1e-12 against products of the same float64 matrices.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import test_rgbd
from oracle_binding import SIFT_POINT_DTYPE
from test_rgbd import H, LOOPS, SEEDS, THRESH2, W, camera, intrinsics, other_bytes, upload
from test_rgbd import pair  # noqa: F401  (the module-scoped fixture pair of frames)
from test_rigid import planted

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CPP = os.path.join(ROOT, "tests", "cpp_rgbd_batch")
BIN = os.path.join(CPP, "rgbd_batch_dropin")
MAX_PTS = 1024
PAIRS = np.array([(0, 1), (1, 0), (0, 2), (0, 1), (3, 0), (0, 3), (4, 5), (1, 1)], np.int32)
MASK64 = 0xFFFFFFFFFFFFFFFF
SENTINEL = 0xAB


# ------------------------------------------------------------------------------------------------------------------
# without a GPU
# ------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree_on_the_batch_calls():
    from cusift_amd import capi

    text = open(os.path.join(ROOT, "include", "cusift_amd_extras.h")).read()
    handle = C.CDLL(capi.LIB_PATH)
    for name, nargs in (("cusift_match_batch", 9), ("cusift_register_rgbd_batch", 25)):
        assert "int %s(cusift_ctx *ctx" % name in text, name
        assert hasattr(handle, name), name
        res, args = capi.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs, (name, len(args))
    assert "} cusift_match_row;" in text
    assert capi.MatchRow.itemsize == 16 and capi.MatchRow.names == ("score", "ambiguity", "match", "reserved")
    assert [capi.MatchRow.fields[n][1] for n in capi.MatchRow.names] == [0, 4, 8, 12]
    for m in ("match_batch", "register_rgbd_batch"):
        assert callable(getattr(capi.Context, m))
    from cusift_amd.batch import BatchExtractor

    assert callable(BatchExtractor.register_sequence)
    for recipe in ("Makefile", "CMakeLists.txt"):
        assert "rgbd_batch" in open(os.path.join(ROOT, recipe)).read(), recipe
    assert "sift_sequence" in open(os.path.join(ROOT, "Makefile")).read()


def pose_to_matrix(R, t):
    m = np.eye(4, dtype=np.float64)
    m[:3, :3], m[:3, 3] = R, t
    return m


def synthetic_motions(n, seed=5):
    r = np.random.default_rng(seed)
    return [planted(axis=r.normal(size=3), angle=r.uniform(-0.4, 0.4), t=r.uniform(-0.3, 0.3, 3)) for _ in range(n)]


def test_chain_poses_composes_consecutive_pairs():
    from cusift_amd.capi import chain_poses

    motions = synthetic_motions(7)  # 8 frames
    rts = np.stack([np.hstack([R, t[:, None]]) for R, t in motions])
    want = [np.eye(4)]
    for R, t in motions:
        want.append(want[-1] @ pose_to_matrix(R, t))
    for pairs in (None, [(i, i + 1) for i in range(7)]):
        got = chain_poses(rts, pairs)
        assert got.shape == (8, 4, 4) and got.dtype == np.float64
        err = np.abs(got - np.stack(want)).max()
        print("chain_poses against the float64 products: %.3g" % err)
        assert err <= 1e-12
    # frame 7's origin seen from frame 0 goes through every step: x_0 = R_0 (R_1 (...) + t_1) + t_0
    x = np.zeros(3)
    for R, t in reversed(motions):
        x = R @ x + t
    assert np.abs(chain_poses(rts)[7][:3, 3] - x).max() <= 1e-12
    assert chain_poses(np.zeros((0, 3, 4))).shape == (1, 4, 4)


def test_chain_poses_refuses_other_pair_lists():
    from cusift_amd.capi import chain_poses

    rts = np.stack([np.eye(3, 4)] * 3)
    for pairs in ([(0, 1), (0, 2), (2, 3)], [(0, 1), (1, 2)], [(1, 0), (1, 2), (2, 3)], [(1, 2), (2, 3), (3, 4)]):
        with pytest.raises(ValueError):
            chain_poses(rts, pairs)


def build_cpp():
    subprocess.check_call(["make", "-C", CPP, "all"], stdout=subprocess.DEVNULL)
    assert os.path.exists(BIN)


def test_cpp_sequence_program_compiles_and_links_with_plain_gxx():
    if os.path.exists(BIN):
        os.remove(BIN)
    build_cpp()
    text = open(os.path.join(ROOT, "include", "rgbd.h")).read()
    assert "RegisterRGBDSequence(" in text and "cusift_register_rgbd_batch(" in text and "#include <hip" not in text
    recipe = open(os.path.join(CPP, "Makefile")).read()
    assert "hipcc" not in recipe and "/opt/rocm" not in recipe


def test_new_kernels_use_no_scratch_and_only_vector_stores():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs

    found = set()
    for src, wanted in (("sift_sequence.hip", ("sequence_select_kernel",)),
                        ("sift_match.hip", ("match_batch_kernel", "match_batch_merge_kernel", "match_kernel")),
                        ("sift_rigid.hip", ("rigid_solve_kernel", "rigid_score_kernel", "rigid_select_kernel"))):
        asm = kernel_regs.assembly(src)
        assert "gfx950" in asm
        for k in kernel_regs.kernels(asm):
            hit = [w for w in wanted if w in k["name"]]
            if not hit:
                continue
            found.update(hit)
            assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
        # scalar memory writes and scalar atomics, by mnemonic prefix (the prefixes are spelled in pieces on purpose)
        kinds = ("st" "ore", "buffer_" "st" "ore", "scratch_" "st" "ore", "at" "omic", "buffer_" "at" "omic",
                 "dcache_" "wb", "dcache_" "discard")
        prefixes = tuple("s_" + k for k in kinds)
        mnemonics = [line.split()[0] for line in asm.splitlines() if line.startswith("\t") and line.split()]
        assert not [m for m in mnemonics if m.startswith(prefixes)], src
        atomics = [m for m in mnemonics if "atomic" in m]
        if src == "sift_rigid.hip":  # the scoring splits meet in an integer add; nothing in floating point
            assert atomics and all(m.startswith("global_atomic_add") and "_f" not in m for m in atomics), atomics
        else:
            assert not atomics, (src, atomics)
        if src == "sift_match.hip":  # both matchers are built on the exact fp32 MFMA
            assert asm.count("v_mfma_f32_16x16x4_f32") >= 4 * 64
    assert len(found) == 7, sorted(found)


# ------------------------------------------------------------------------------------------------------------------
# the frame batch of the GPU tests
# ------------------------------------------------------------------------------------------------------------------
def encode_depth(mm):
    """The inverse of the SUN3D decoding (r >> 3) | (r << 13), for depths below 8192 mm."""
    mm = np.asarray(mm, np.uint32)
    assert (mm < 8192).all()
    return ((mm << 3) & 0xFFFF).astype(np.uint16)


def unit_descriptors(r, n):
    d = np.abs(r.normal(size=(n, 128))).astype(np.float32)
    return d / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True).astype(np.float32)


def synthetic_frames(template, n_a=MAX_PTS, n_b=900, seed=11, n_c=0):
    """Two frames of unit-norm random descriptors at integer pixels with a depth image each: frame B sees n_b of frame
    A's points after the planted motion x_A = R x_B + t, its descriptors are A's plus 1 % noise.  Pixel and millimetre
    rounding move a lifted point by a few millimetres, far inside the 0.05 m RANSAC threshold.
    n_c > 0: a third frame C, n_c of A's points moved once more (x_A = R2 x_C + t2), drawn after everything of A and B, so
    that those two are the same with and without it; (fc, dc, seen_c, its motion) are appended to the result."""
    r = np.random.default_rng(seed)
    fx, fy, cx, cy = intrinsics()
    flat = r.choice((W - 80) * (H - 80), n_a, replace=False)
    ua, va = 40 + flat % (W - 80), 40 + flat // (W - 80)
    za = r.integers(900, 2800, n_a)
    xa = np.c_[((ua + 1) - cx) * za / 1000.0 / fx, ((va + 1) - cy) * za / 1000.0 / fy, za / 1000.0]

    def view(R, t, n):
        """n of A's points as the moved camera sees them: (their indices in A, pixel u, v, depth in mm)."""
        xb = (xa - t) @ R  # R^T (x_A - t)
        ub = np.rint(xb[:, 0] * fx / xb[:, 2] + cx - 1).astype(np.int64)
        vb = np.rint(xb[:, 1] * fy / xb[:, 2] + cy - 1).astype(np.int64)
        zb = np.rint(xb[:, 2] * 1000).astype(np.int64)
        ok = (ub >= 0) & (ub < W) & (vb >= 0) & (vb < H) & (zb > 0) & (zb < 8192)
        _, first = np.unique(vb * W + ub, return_index=True)  # one point per pixel of the moved frame
        uniq = np.zeros(n_a, bool)
        uniq[first] = True
        seen = r.permutation(np.nonzero(ok & uniq)[0])[:n]
        assert len(seen) == n
        return seen, ub[seen], vb[seen], zb[seen]

    def frame(seen, u, v, z, desc):
        f = np.zeros(len(seen), SIFT_POINT_DTYPE)
        f[:] = template[0]
        f["coords2D"], f["data"] = np.c_[u, v].astype(np.float32), desc
        d = np.zeros((H, W), np.uint16)
        d[v, u] = encode_depth(z)
        return f, d

    def noisy(desc):
        desc = desc + r.normal(0, 0.01 / np.sqrt(128), desc.shape).astype(np.float32)
        return (desc / np.linalg.norm(desc.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)

    R, t = planted(axis=(0.1, 1.0, 0.05), angle=0.08, t=(0.05, -0.02, 0.04))
    seen, ub, vb, zb = view(R, t, n_b)
    desc_a = unit_descriptors(r, n_a)
    fa, da = frame(np.arange(n_a), ua, va, za, desc_a)
    fb, db = frame(seen, ub, vb, zb, noisy(desc_a[seen]))
    out = (fa, fb, da, db, seen, np.hstack([R, t[:, None]]))
    if n_c:
        R2, t2 = planted(axis=(-0.2, 1.0, 0.1), angle=-0.03, t=(-0.02, 0.015, 0.03))
        seen_c, uc, vc, zc = view(R2, t2, n_c)
        out += frame(seen_c, uc, vc, zc, noisy(desc_a[seen_c])) + (seen_c, np.hstack([R2, t2[:, None]]))
    return out


class FrameBatch:
    """Fixture frames 1 and 2, frame 1 cut to 300, an empty frame and the two synthetic frames in max_pts = 1024 slots.
    Frame 4 is full and its counter says 3000.  Records past a count are live-looking copies with valid pixels, so that a
    stage that ignores a count shows."""

    def __init__(self, pair):
        s1, s2, d1, d2, _, _ = pair
        fa, fb, da, db, self.seen, self.motion = synthetic_frames(s1)
        frames = [s1, s2, s1[:300], s1[:0], fa, fb]
        self.points = np.zeros((6, MAX_PTS), SIFT_POINT_DTYPE)
        self.points[:] = np.resize(s2, MAX_PTS)
        self.points["coords2D"] = 17.0
        for k, f in enumerate(frames):
            self.points[k, :len(f)] = f
        self.points["coords3D"] = 7.0
        self.points["score"], self.points["ambiguity"], self.points["match"] = 0.25, 0.5, -5
        self.n = np.array([len(f) for f in frames])
        self.counters = self.n.astype(np.uint32)
        assert self.n[4] == MAX_PTS
        self.counters[4] = 3000
        self.depth = np.stack([d1, d2, d1, np.zeros_like(d1), da, db])

    def upload(self, ctx, counters="own"):
        cnt = None if counters is None else upload(ctx, self.counters if isinstance(counters, str) else counters)
        return upload(ctx, self.points), cnt, upload(ctx, self.depth)


@pytest.fixture(scope="module")
def frames(pair):  # noqa: F811
    return FrameBatch(pair)


def register_batch(ctx, fb, seed, kind="3d", counters="own", pairs=PAIRS, loops=LOOPS):
    pts, cnt, dep = fb.upload(ctx, counters)
    n_images, max_pts = fb.points.shape
    out = ctx.register_rgbd_batch(pts.ptr, cnt.ptr if cnt is not None else None, n_images, max_pts, dep.ptr, W, H,
                                  camera(), pairs, distance=1, score_threshold=999.0, ambiguity_threshold=0.6, loops=loops,
                                  thresh2=THRESH2, kind=kind, seed=seed)
    return out + (pts.to_numpy(SIFT_POINT_DTYPE, (n_images, max_pts)),)


def register_pair(ctx, fb, a, b, seed, kind="3d", loops=LOOPS):
    """cusift_register_rgbd on copies of frames a and b, with the counts the host read."""
    na, nb = int(fb.n[a]), int(fb.n[b])
    b1, b2 = upload(ctx, fb.points[a, :max(na, 1)].copy()), upload(ctx, fb.points[b, :max(nb, 1)].copy())
    e1, e2 = upload(ctx, fb.depth[a]), upload(ctx, fb.depth[b])
    return ctx.register_rgbd(b1.ptr, na, e1.ptr, b2.ptr, nb, e2.ptr, W, H, camera(), distance=1, score_threshold=999.0,
                             ambiguity_threshold=0.6, loops=loops, thresh2=THRESH2, kind=kind, seed=seed & MASK64)


def tie_rows(score, ambiguity, distance):
    """Rows of the pair route whose second-best equals their best."""
    s = score.astype(np.float64)
    tie = s / (s + 1e-6) if distance == 1 else (1 - s) / (1 - s + 1e-6)
    return ambiguity == tie.astype(np.float32)


def compare_rows(ctx, rows, points, counts, pairs, distance, what):
    """rows [P, max_pts] of cusift_match_batch (read back over a SENTINEL fill) against cusift_match per pair on copies
    of points[frame][:count]."""
    from cusift_amd import capi

    untouched = np.full(1, SENTINEL * 0x01010101, np.uint32).view(np.float32)[0]
    raw = rows.view(np.uint8).reshape(rows.shape + (16,))
    for p, (a, b) in enumerate(pairs):
        na, nb = int(counts[a]), int(counts[b])
        if na == 0 or nb == 0:  # nothing to match: no row of the pair is written
            assert (raw[p] == SENTINEL).all(), (what, p)
            continue
        assert (raw[p, na:] == SENTINEL).all(), (what, p)  # rows past the count are untouched
        b1, b2 = upload(ctx, points[a, :na].copy()), upload(ctx, points[b, :nb].copy())
        ctx.match(b1.ptr, na, b2.ptr, nb, distance)
        ctx.synchronize()
        one = b1.to_numpy(capi.SIFT_POINT_DTYPE, (na,))
        got = rows[p, :na]
        assert not np.array_equal(got["score"], np.full(na, untouched)), (what, p)
        assert got["score"].tobytes() == one["score"].tobytes(), (what, p)
        assert got["ambiguity"].tobytes() == one["ambiguity"].tobytes(), (what, p)
        assert (got["reserved"] == 0).all()
        differ = got["match"] != one["match"]
        tie = tie_rows(one["score"], one["ambiguity"], distance)
        blind = tie & (one["ambiguity"] == 0)  # a zero numerator: the equation says nothing about the second-best
        col = np.clip(np.c_[got["match"], one["match"]], 0, nb - 1)
        twins = (points[b, col[:, 0]]["data"] == points[b, col[:, 1]]["data"]).all(axis=1)
        tie &= ~blind | (differ & twins)
        print("%s pair %d (%d, %d): %d rows, %d tie rows, %d indices differ" % (what, p, a, b, na, tie.sum(), differ.sum()))
        assert tie.sum() <= 0.01 * na, (what, p, int(tie.sum()))
        assert not (differ & ~tie).any(), (what, p, np.nonzero(differ & ~tie)[0][:10])
        assert ((got["match"] >= 0) & (got["match"] < nb)).all()


# ------------------------------------------------------------------------------------------------------------------
# on the GPU
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
def test_match_batch_equals_match_per_pair(ctx, frames, distance):
    from cusift_amd import capi

    pts, cnt, _ = frames.upload(ctx)
    rows = upload(ctx, np.full((len(PAIRS), MAX_PTS, 16), SENTINEL, np.uint8))
    ctx.match_batch(pts.ptr, cnt.ptr, 6, MAX_PTS, PAIRS, rows.ptr, distance)
    ctx.synchronize()
    got = rows.to_numpy(capi.MatchRow, (len(PAIRS), MAX_PTS))
    assert pts.to_numpy(SIFT_POINT_DTYPE, (6, MAX_PTS)).tobytes() == frames.points.tobytes()  # the records: untouched
    compare_rows(ctx, got, frames.points, frames.n, PAIRS, distance, "distance %d" % distance)
    # the synthetic pair's matches are the planted correspondences
    assert np.array_equal(got[6, frames.seen]["match"], np.arange(len(frames.seen)))
    # a second run writes the same bytes
    rows2 = upload(ctx, np.full((len(PAIRS), MAX_PTS, 16), SENTINEL, np.uint8))
    ctx.match_batch(pts.ptr, cnt.ptr, 6, MAX_PTS, PAIRS, rows2.ptr, distance)
    ctx.synchronize()
    assert rows2.to_numpy(capi.MatchRow, (len(PAIRS), MAX_PTS)).tobytes() == got.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("3d", "2d"))
@pytest.mark.parametrize("seed", SEEDS + (MASK64 - 2,))
def test_register_batch_equals_register_per_pair_bit_for_bit(ctx, frames, seed, kind):
    """The last seed wraps: seed + p passes 2^64 inside the pair list."""
    rt, n_match, n_in, sel, flags, recs = register_batch(ctx, frames, seed, kind)
    assert rt.shape == (len(PAIRS), 3, 4) and len(sel) == len(PAIRS) and len(flags) == len(PAIRS)
    for p, (a, b) in enumerate(PAIRS):
        prt, ppairs, pflags, pin = register_pair(ctx, frames, a, b, seed + p, kind)
        print("pair %d (%d, %d): %d matches, %d inliers" % (p, a, b, n_match[p], n_in[p]))
        assert rt[p].tobytes() == prt.tobytes(), p
        assert n_match[p] == len(ppairs) and n_in[p] == pin, p
        assert sel[p].tobytes() == ppairs.tobytes() and np.array_equal(flags[p], pflags), p
    assert n_match[0] == 330 and n_match[3] == 330
    # of the records only coords3D is written, and only below the counts
    assert np.array_equal(other_bytes(recs.reshape(-1)), other_bytes(frames.points.reshape(-1)))
    for k in range(6):
        assert (recs["coords3D"][k, frames.n[k]:] == 7.0).all()
        assert (recs["coords3D"][k, :frames.n[k]] != 7.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_fixture_pair_of_the_batch_meets_the_bounds_of_the_pair_call(ctx, frames, pair, seed, monkeypatch):  # noqa: F811
    """Every bound tests/test_rgbd.py applies to cusift_register_rgbd against MATLAB's Rt1_2, applied to pair (0, 1) of
    the batch: that test, run with the batch call in the place of the pair call."""
    rt, n_match, n_in, sel, flags, recs = register_batch(ctx, frames, seed)

    def from_batch(ctx_, pair_, seed_, **kw):
        assert seed_ == seed and not kw
        return rt[0], sel[0], flags[0], int(n_in[0]), recs[0, :frames.n[0]], recs[1, :frames.n[1]]

    monkeypatch.setattr(test_rgbd, "fused", from_batch)
    test_rgbd.test_registration_recovers_the_fixture_motion(ctx, pair, seed)


@pytest.mark.gpu
def test_counts_empty_frames_and_repeatability(ctx, frames):
    ident = np.eye(3, 4, dtype=np.float32)
    base = register_batch(ctx, frames, 9)
    rt, n_match, n_in, sel, flags, recs = base
    for p in (4, 5):  # (3, 0) and (0, 3): frame 3 is empty
        assert np.array_equal(rt[p], ident) and n_match[p] == 0 and n_in[p] == 0 and len(sel[p]) == 0
    # the synthetic pair recovers the planted motion: the lifted points carry pixel and millimetre rounding (below
    # 3 mm at these depths), so a refit over ~900 of them lies within 5 mm / 5e-3 of the motion
    assert n_match[6] >= 0.95 * len(frames.seen) and n_in[6] >= 0.95 * n_match[6]
    assert np.abs(rt[6].astype(np.float64) - frames.motion).max() < 5e-3
    # the same pair twice in one list, with its own seed each: the same matches
    assert np.array_equal(sel[0], sel[3])

    def same(x, y):
        return all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(x[:3], y[:3])) and all(
            u.tobytes() == v.tobytes() for k in (3, 4) for u, v in zip(x[k], y[k])) and x[5].tobytes() == y[5].tobytes()

    assert same(base, register_batch(ctx, frames, 9))  # two runs, the same bytes
    clamped = frames.counters.copy()
    clamped[4] = MAX_PTS
    assert same(base, register_batch(ctx, frames, 9, counters=clamped))  # a counter past max_pts means max_pts
    full = np.full(6, MAX_PTS, np.uint32)
    assert same(register_batch(ctx, frames, 9, counters=None), register_batch(ctx, frames, 9, counters=full))
    # no pairs: nothing to do
    out = register_batch(ctx, frames, 9, pairs=np.zeros((0, 2), np.int32))
    assert out[0].shape == (0, 3, 4) and out[5].tobytes() == frames.points.tobytes()


@pytest.mark.gpu
def test_batch_refusals_leave_everything_untouched(ctx, frames):
    from cusift_amd import capi

    pts, cnt, dep = frames.upload(ctx)
    cam = camera()
    n_pairs = len(PAIRS)
    rt = np.full((n_pairs, 12), 9.0, np.float32)
    nm, ni = np.full(n_pairs, -7, np.int32), np.full(n_pairs, -7, np.int32)
    sel = np.full((n_pairs, MAX_PTS, 2), -7, np.int32)
    fl = np.full((n_pairs, MAX_PTS), 5, np.int8)

    def ptr(a):
        return a.ctypes.data if a is not None else None

    def call(cam=cam, out=rt, pnm=nm, pni=ni, loops=64, th=0.0025, kind=1, dist=1, pitch=W, stride=W * H, d=dep.ptr,
             recs=pts.ptr, pairs=PAIRS, n_pairs=n_pairs, n_images=6, max_pts=MAX_PTS, amb=0.6):
        pairs = None if pairs is None else np.ascontiguousarray(pairs, np.int32)
        return capi.lib().cusift_register_rgbd_batch(ctx.handle, recs, cnt.ptr, n_images, max_pts, d, W, H, pitch,
                                                     stride, C.byref(cam) if cam is not None else None, ptr(pairs),
                                                     n_pairs, dist, 999.0, amb, loops, th, kind, 1, ptr(out), ptr(pnm),
                                                     ptr(pni), ptr(sel), ptr(fl))

    fx0, upm0, enc = camera(), camera(), camera()
    fx0.fx, upm0.units_per_metre, enc.encoding = 0.0, 0.0, 2
    low, high = PAIRS.copy(), PAIRS.copy()
    low[2, 1], high[5, 0] = -1, 6
    cases = (dict(cam=fx0), dict(cam=upm0), dict(cam=enc), dict(cam=None), dict(out=None), dict(pnm=None), dict(pni=None),
             dict(loops=0), dict(th=0.0), dict(th=float("nan")), dict(amb=float("nan")), dict(kind=2), dict(dist=3),
             dict(pitch=W - 1), dict(stride=W * H - W), dict(d=None), dict(recs=None),
             # the batch's own
             dict(pairs=low), dict(pairs=high), dict(n_pairs=-1), dict(n_pairs=65536, pairs=np.zeros((65536, 2))),
             dict(max_pts=-1), dict(max_pts=(1 << 20) + 1), dict(pairs=None), dict(n_images=3))
    for kw in cases:
        assert call(**kw) == -1, kw  # CUSIFT_ERR_INVALID
        assert (rt == 9.0).all() and (nm == -7).all() and (ni == -7).all() and (sel == -7).all() and (fl == 5).all(), kw
    ctx.synchronize()
    assert pts.to_numpy(SIFT_POINT_DTYPE, (6, MAX_PTS)).tobytes() == frames.points.tobytes()  # nothing was enqueued
    rows = upload(ctx, np.full((n_pairs, MAX_PTS, 16), SENTINEL, np.uint8))
    for kw in (dict(pairs=low), dict(pairs=high), dict(distance=2), dict(max_pts=(1 << 20) + 1), dict(n_images=3)):
        args = dict(pairs=PAIRS, distance=1, max_pts=MAX_PTS, n_images=6)
        args.update(kw)
        with pytest.raises(capi.CusiftError):
            ctx.match_batch(pts.ptr, cnt.ptr, args["n_images"], args["max_pts"], args["pairs"], rows.ptr, args["distance"])
    assert capi.lib().cusift_match_batch(ctx.handle, pts.ptr, cnt.ptr, 6, MAX_PTS, None, 2, 1, rows.ptr) == -1
    ctx.synchronize()
    assert (rows.to_numpy(np.uint8, (n_pairs, MAX_PTS, 16)) == SENTINEL).all()
    # n_pairs == 0 is not an error and writes nothing
    assert call(n_pairs=0) == 0 and call(n_pairs=0, pairs=None) == 0
    assert (rt == 9.0).all() and (nm == -7).all()
    # and the same arguments without a fault run
    assert call(loops=LOOPS) == 0 and nm[0] == 330 and 325 <= ni[0] <= 327 and (rt[4] == np.eye(3, 4).ravel()).all()
    assert (sel[0, 330:] == -7).all() and (fl[0, 330:] == 5).all()  # a block's tail is not written


@pytest.mark.gpu
def test_register_sequence_end_to_end():
    """Eight overlapping crops of one synthetic image through BatchExtractor.extract and register_sequence (no count
    read-back), against the pair route over the same device records after reading the counts."""
    import torch

    from cusift_amd import capi, synth
    from cusift_amd.batch import BatchExtractor

    n, step = 8, 24
    wide = synth.tile(4242, w=W + step * (n - 1), h=H, preblur=1.0)
    imgs = np.stack([wide[:, step * i:step * i + W] for i in range(n)])
    ex = BatchExtractor(n, W, H, num_octaves=4, init_blur=1.0, peak_thresh=3.0, max_pts=MAX_PTS)
    try:
        ex.extract(ex.images_from_numpy(imgs))
        # a wall 2 m in front of a camera that slides along it: a rigid scene, in plain millimetres
        depth_np = np.full((n, H, W), 2000, np.uint16)
        depth = torch.from_numpy(depth_np.view(np.int16)).to(ex.device)
        fx, fy, cx, cy = intrinsics()
        cam = capi.Camera(fx, fy, cx, cy, origin=0.0, units_per_metre=1000.0, encoding=0)
        settings = dict(distance=1, score_threshold=999.0, ambiguity_threshold=0.6, loops=LOOPS, thresh2=THRESH2, seed=21)
        rt, n_match, n_in, sel, flags = ex.register_sequence(depth, cam, **settings)
        pairs = np.array([(i, i + 1) for i in range(n - 1)], np.int32)
        assert rt.shape == (n - 1, 3, 4) and len(sel) == n - 1
        rows_t = torch.full((n - 1, MAX_PTS, 16), SENTINEL, dtype=torch.uint8, device=ex.device)
        ex.ctx.match_batch(ex.points.data_ptr(), ex.counts.data_ptr(), n, MAX_PTS, pairs, rows_t.data_ptr(), 1)
        ex.ctx.synchronize()
        # ---- the pair route: now the counts are read ----
        counts = ex.valid_counts().cpu().numpy()
        recs = ex.points.cpu().numpy().view(SIFT_POINT_DTYPE).reshape(n, MAX_PTS)
        print("records per frame:", counts, "raw counters:", ex.counts.cpu().numpy())
        assert (counts > 200).all()
        compare_rows(ex.ctx, rows_t.cpu().numpy().view(capi.MatchRow).reshape(n - 1, MAX_PTS), recs, counts, pairs, 1,
                     "sequence")
        for p, (a, b) in enumerate(pairs):
            na, nb = int(counts[a]), int(counts[b])
            b1, b2 = upload(ex.ctx, recs[a, :na].copy()), upload(ex.ctx, recs[b, :nb].copy())
            e1, e2 = upload(ex.ctx, depth_np[a]), upload(ex.ctx, depth_np[b])
            kw = {k: v for k, v in settings.items() if k != "seed"}
            prt, ppairs, pflags, pin = ex.ctx.register_rgbd(b1.ptr, na, e1.ptr, b2.ptr, nb, e2.ptr, W, H, cam,
                                                            seed=settings["seed"] + p, **kw)
            print("pair %d: %d matches, %d inliers, t = %s" % (p, n_match[p], n_in[p], rt[p][:, 3]))
            assert rt[p].tobytes() == prt.tobytes() and n_in[p] == pin and n_match[p] == len(ppairs), p
            assert sel[p].tobytes() == ppairs.tobytes() and np.array_equal(flags[p], pflags), p
        # Consecutive crops share 616 of their 640 columns, so the frames must chain: most pairs have to register, and
        # where they do the motion is the slide, t = (step * 2 m / fx, 0, 0), to within the lift's pixel rounding
        # (one pixel at 2 m is 2 / fx = 4 mm) -- 0.01 m is asked
        assert (n_in >= 50).sum() >= (n - 1) // 2
        for p in np.nonzero(n_in >= 50)[0]:
            assert np.abs(rt[p][:, 3] - np.array([step * 2.0 / fx, 0, 0])).max() < 0.01, (p, rt[p])
        poses = capi.chain_poses(rt, pairs)
        assert poses.shape == (n, 4, 4) and np.isfinite(poses).all()
        # explicit pairs, a frame first in several of them, through the same door
        out = ex.register_sequence(depth, cam, pairs=[(0, 1), (0, 2), (2, 0), (0, 1)], **settings)
        assert out[0][0].tobytes() == rt[0].tobytes() and np.array_equal(out[3][0], out[3][3])
    finally:
        ex.close()


@pytest.mark.gpu
def test_cpp_sequence_program_passes_on_gpu(tmp_path, pair):  # noqa: F811
    """tests/cpp_rgbd_batch: RegisterRGBDSequence over (0,1) (1,2) (0,2) (1,1) against RegisterRGBD pair by pair."""
    build_cpp()
    _, _, d1, d2, _, _ = pair
    d1.astype("<u2").tofile(str(tmp_path / "depth1.u16"))
    d2.astype("<u2").tofile(str(tmp_path / "depth2.u16"))
    cmd = [BIN, os.path.join(GOLDEN, "vlfeat_sift1.bin"), os.path.join(GOLDEN, "vlfeat_sift2.bin"),
           str(tmp_path / "depth1.u16"), str(tmp_path / "depth2.u16"), os.path.join(GOLDEN, "rgbd_intrinsics.txt")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout
    lines = out.stdout.splitlines()
    i, j = lines.index("pair Rt"), lines.index("sequence Rt")
    assert lines[i + 1:i + 4] == lines[j + 1:j + 4] and len(lines[i + 1].split()) == 4  # the same Rt for the pair (0, 1)
    assert "pair (0, 1): matches 330, inliers " in out.stdout
