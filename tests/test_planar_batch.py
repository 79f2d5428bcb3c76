"""Planar registration of a pair list: cusift_register_planar_batch (cusift_amd/csrc/sift_sequence.hip: the marking
kernel; sift_planar.hip / sift_homography.hip: the per-pair RANSAC and refit; sift_register.hip: the entry point),
capi.Context.register_planar_batch, capi.chain_homographies, BatchExtractor.register_planar_sequence and
RegisterPlanarSequence of include/homography.h.

The defining equality is bit for bit: every output of pair p = (a, b) is what cusift_estimate_homography gives on a copy
of frame a's records into which pair p's row of cusift_match_batch was scattered, with seed + p.  Where the rows equal
what cusift_match writes -- asserted for EVERY pair of the list, on inputs without exactly tied scores -- the outputs are
also those of cusift_register_planar on copies of the two frames.

End to end (gray1 and three frames warped by cumulative mild homographies, 4 octaves, max_pts 4096), measured on an
MI355X: chained corner error of frame k against frame 0, k = 1, 2, 3: see DESIGN.md section 4.8.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import test_planar
from oracle_binding import SIFT_POINT_DTYPE, read_vlfeat_sift
from test_planar import candidates, corner_distance, improve, r32_of, upload, warp
from test_rgbd_batch import MASK64, SENTINEL, tie_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CPP = os.path.join(ROOT, "tests", "cpp_planar_batch")
BIN = os.path.join(CPP, "planar_batch_dropin")
MAX_PTS = 1024
N_FRAMES = 8
LOOPS = 1008
NAME = "cusift_register_planar_batch"
# repeated first members (frame 0 three times, frame 5 twice), reversed pairs, self pairs
PAIRS = np.array([(0, 1), (1, 0), (0, 2), (0, 1), (5, 6), (6, 5), (1, 1), (2, 0), (5, 5)], np.int32)
# (3, 1): frame a is empty; (1, 3): frame b is empty; (4, 0): frame a has 5 records; (7, 1): 12 records, 6 of them with a
# NaN coordinate and so at most 6 candidates; (0, 4) is an ordinary pair onto a frame of 5 records
DEGENERATE = np.array([(0, 1), (3, 1), (1, 3), (4, 0), (5, 6), (7, 1), (0, 4), (6, 5)], np.int32)
DEGENERATE_AT = (1, 2, 3, 5)
RULES = {1: dict(rule=1, lo=999.0, hi=0.8), 0: dict(rule=0, lo=0.0, hi=0.95)}  # by distance, as tests/test_planar.py
IDENT = np.eye(3, dtype=np.float32).ravel()


# ------------------------------------------------------------------------------------------------------------------
# without a GPU
# ------------------------------------------------------------------------------------------------------------------
def test_header_library_binding_and_recipes_agree_on_the_batch_call():
    from cusift_amd import batch, capi

    extras = open(os.path.join(ROOT, "include", "cusift_amd_extras.h")).read()
    front = open(os.path.join(ROOT, "include", "cusift_amd.h")).read()
    assert "int %s(cusift_ctx *ctx, const cusift_point *d_points" % NAME in extras
    assert "int %s(" % NAME not in front
    assert hasattr(C.CDLL(capi.LIB_PATH), NAME)
    res, args = capi.SIGNATURES[NAME]
    assert res is C.c_int and len(args) == 24, len(args)
    assert args[15] is C.c_uint64  # the seed
    assert callable(capi.Context.register_planar_batch) and callable(capi.chain_homographies)
    assert callable(batch.BatchExtractor.register_planar_sequence)
    assert capi.PlanarBatchResult._fields[:6] == capi.PlanarResult._fields[:6]
    make = open(os.path.join(ROOT, "Makefile")).read()
    sources = make.split("SOURCES :=")[1].split("HEADERS")[0]
    assert "sift_sequence" in sources and "sift_planar" in sources and "cpp_planar_batch" in make
    cm = open(os.path.join(ROOT, "CMakeLists.txt")).read()
    assert "csrc/*.hip" in cm and "tests/cpp_planar_batch/planar_batch_dropin.cpp" in cm
    assert "tests/cpp_planar_batch/planar_batch_dropin" in open(os.path.join(ROOT, ".gitignore")).read()
    head = open(os.path.join(ROOT, "include", "homography.h")).read()
    assert "RegisterPlanarSequence(std::vector<SiftData *> &frames" in head and NAME + "(" in head
    planar = open(os.path.join(ROOT, "cusift_amd", "csrc", "sift_planar.hip")).read()
    assert "One pair is launched today" not in planar and NAME in planar


def test_batch_kernels_compile_for_gfx950_without_scratch_and_with_vector_stores_only():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_regs

    found = set()
    for src, wanted in (("sift_sequence.hip", ("sequence_mark_kernel", "sequence_select_kernel")),
                        ("sift_planar.hip", ("planar_mark_kernel", "planar_compact_kernel", "planar_score_kernel",
                                             "planar_select_kernel")),
                        ("sift_homography.hip", ("homography_solve_kernel",))):
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
        if src == "sift_planar.hip":  # the scoring splits meet in an integer add; nothing in floating point
            assert atomics and all(m.startswith("global_atomic_add") and "_f" not in m for m in atomics), atomics
        else:
            assert not atomics, (src, atomics)
        text = open(os.path.join(ROOT, "cusift_amd", "csrc", src)).read().lower()
        assert not [w for w in prefixes if w in text]
    assert len(found) == 7, sorted(found)
    seq = open(os.path.join(ROOT, "cusift_amd", "csrc", "sift_sequence.hip")).read()
    assert not re.search(r"^\s*#\s*(if|ifdef|ifndef|elif)\b", seq, flags=re.M)


def planted_chain(n, seed=4):
    """n mild homographies H_k (frame k onto frame k + 1), float64, of the size the end-to-end test warps with."""
    r = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        a = r.uniform(-0.04, 0.04)
        s = r.uniform(0.97, 1.03)
        out.append(np.array([[s * np.cos(a), -s * np.sin(a), r.uniform(-40, 40)],
                             [s * np.sin(a), s * np.cos(a), r.uniform(-40, 40)],
                             [r.uniform(-3e-5, 3e-5), r.uniform(-3e-5, 3e-5), 1.0]]))
    return out


def apply(G, pts):
    q = np.c_[pts, np.ones(len(pts))] @ G.T
    return q[:, :2] / q[:, 2:3]


def test_chain_homographies_composes_consecutive_pairs():
    """G[k] applied to frame k's corners against the composed truth inv(H_{k-1} ... H_0), which is computed the other way
    round (one product, one inverse).  THE BOUND, from fp64 conditioning and not tuned: inverting H_k and multiplying it
    onto G[k] each carry a relative error of a few eps * cond (Higham, Accuracy and Stability, 14.1 and 3.5: at most
    c n^2 eps cond for an n x n inverse, n eps per product; n = 3), the errors of the K steps add, the truth carries as
    much again, and a relative perturbation d of a homography moves a point of magnitude S by at most about d * cond *
    S pixels.  With kappa = the largest 2-norm condition number among the H_k, the G[k] and the truth, that is
    2 * K * (9 + 3 + 3) * eps * kappa * S <= 32 K eps kappa S -- about 1e-7 px here; anything wrong in the composition
    (an H not inverted, a wrong order, no normalisation) is off by pixels."""
    from cusift_amd.capi import chain_homographies

    K = 6
    hs = planted_chain(K)
    corners = np.array([[0, 0], [1280, 0], [0, 960], [1280, 960]], dtype=np.float64)
    S = 1600.0  # the corner's magnitude
    for pairs in (None, [(i, i + 1) for i in range(K)]):
        got = chain_homographies(np.stack(hs).astype(np.float64).reshape(K, 9), pairs)
        assert got.shape == (K + 1, 3, 3) and got.dtype == np.float64
        assert np.array_equal(got[0], np.eye(3)) and (got[:, 2, 2] == 1.0).all()
        prod = np.eye(3)
        kappa = max(np.linalg.cond(h) for h in hs)
        for k in range(1, K + 1):
            prod = hs[k - 1] @ prod  # frame 0 onto frame k
            truth = np.linalg.inv(prod)
            kappa = max(kappa, np.linalg.cond(got[k]), np.linalg.cond(truth))
            frame_k = apply(prod, corners)  # frame k's image of frame 0's corners comes back onto them
            err = np.abs(apply(got[k], frame_k) - apply(truth, frame_k)).max()
            back = np.abs(apply(got[k], frame_k) - corners).max()
            bound = 32 * K * np.finfo(np.float64).eps * kappa * S
            print("G[%d]: %.3g px from the composed truth, %.3g px from frame 0's corners (bound %.3g, kappa %.3g)" %
                  (k, err, back, bound, kappa))
            assert err <= bound and back <= bound
    assert chain_homographies(np.zeros((0, 9))).shape == (1, 3, 3)
    # float32 results (what the device returns) are composed in float64
    g32 = chain_homographies(np.stack(hs).astype(np.float32).reshape(K, 3, 3))
    assert g32.dtype == np.float64 and np.abs(apply(g32[K], apply(prod, corners)) - corners).max() < 0.05


def test_chain_homographies_refuses_other_pair_lists():
    from cusift_amd.capi import chain_homographies

    hs = np.stack([np.eye(3)] * 3)
    for pairs in ([(0, 1), (0, 2), (2, 3)], [(0, 1), (1, 2)], [(1, 0), (1, 2), (2, 3)], [(1, 2), (2, 3), (3, 4)]):
        with pytest.raises(ValueError):
            chain_homographies(hs, pairs)


def build_cpp():
    subprocess.check_call(["make", "-C", CPP, "all"], stdout=subprocess.DEVNULL)
    assert os.path.exists(BIN)


def test_cpp_sequence_program_compiles_and_links_with_plain_gxx():
    if os.path.exists(BIN):
        os.remove(BIN)
    build_cpp()
    recipe = open(os.path.join(CPP, "Makefile")).read()
    assert "hipcc" not in recipe and "/opt/rocm" not in recipe
    assert "#include <hip" not in open(os.path.join(ROOT, "include", "homography.h")).read()


# ------------------------------------------------------------------------------------------------------------------
# the frame batch of the GPU tests
# ------------------------------------------------------------------------------------------------------------------
def unit_descriptors(r, n):
    d = np.abs(r.normal(size=(n, 128))).astype(np.float32)
    return d / np.linalg.norm(d.astype(np.float64), axis=1, keepdims=True).astype(np.float32)


def planted_frames(template, n_a=MAX_PTS, n_b=900, seed=13, n_planted=700):
    """Two frames of unit-norm random descriptors related by a planted homography: frame B holds n_b of frame A's points
    (n_planted = 700 mapped with 0.3 px of noise, the rest anywhere), in shuffled order, with A's descriptors plus 1 %
    noise.  Random real-valued descriptors: no two scores are exactly equal."""
    r = np.random.default_rng(seed)
    H = np.array([[0.95, -0.08, 30.0], [0.07, 1.03, -18.0], [1.8e-5, -2.6e-5, 1.0]])
    xa = np.c_[r.uniform(0, 1280, n_a), r.uniform(0, 960, n_a)]
    seen = r.permutation(n_a)[:n_b]
    xb = apply(H, xa[seen]) + r.normal(0, 0.3, (n_b, 2))
    xb[n_planted:] = np.c_[r.uniform(0, 1280, n_b - n_planted), r.uniform(0, 960, n_b - n_planted)]
    desc_a = unit_descriptors(r, n_a)
    desc_b = desc_a[seen] + r.normal(0, 0.01 / np.sqrt(128), (n_b, 128)).astype(np.float32)
    desc_b = (desc_b / np.linalg.norm(desc_b.astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    fa, fb = np.zeros(n_a, SIFT_POINT_DTYPE), np.zeros(n_b, SIFT_POINT_DTYPE)
    fa[:], fb[:] = template[0], template[0]
    fa["coords2D"], fa["data"] = xa.astype(np.float32), desc_a
    fb["coords2D"], fb["data"] = xb.astype(np.float32), desc_b
    return fa, fb, seen, H


class FrameBatch:
    """The two VLFeat fixtures (frame 0 without the second copy of its one repeated descriptor, so that no two columns
    tie), a cut of frame 0, an empty frame, a frame of 5 records, the planted pair, and 12 records of which 6 have a NaN
    coordinate -- in max_pts = 1024 slots.  Frame 5 is full and its counter says 3000.  Records past a count are
    live-looking copies with valid pixels, so that a stage that ignores a count shows; the match fields carry values no
    stage produces."""

    def __init__(self):
        s1 = read_vlfeat_sift(os.path.join(GOLDEN, "vlfeat_sift1.bin"))
        s2 = read_vlfeat_sift(os.path.join(GOLDEN, "vlfeat_sift2.bin"))
        _, first = np.unique(s1["data"], axis=0, return_index=True)
        s1 = s1[np.sort(first)]
        assert len(np.unique(s2["data"], axis=0)) == len(s2)
        fa, fb, self.seen, self.H = planted_frames(s1)
        poor = s2[:12].copy()
        poor["coords2D"][::2, 0] = np.nan
        frames = [s1, s2, s1[:300], s1[:0], s2[:5], fa, fb, poor]
        self.points = np.zeros((N_FRAMES, MAX_PTS), SIFT_POINT_DTYPE)
        self.points[:] = np.resize(s2, MAX_PTS)
        self.points["coords2D"] = 17.0
        for k, f in enumerate(frames):
            self.points[k, :len(f)] = f
        self.points["score"], self.points["ambiguity"], self.points["match"] = 0.25, 0.5, -5
        self.points["match_xpos"], self.points["match_ypos"], self.points["match_error"] = -3.0, -4.0, 7.0
        self.n = np.array([len(f) for f in frames])
        self.counters = self.n.astype(np.uint32)
        assert self.n[5] == MAX_PTS
        self.counters[5] = 3000

    def upload(self, ctx, counters="own"):
        cnt = None if counters is None else upload(ctx, self.counters if isinstance(counters, str) else counters)
        return upload(ctx, self.points), cnt


@pytest.fixture(scope="module")
def frames():
    return FrameBatch()


def register_batch(ctx, fb, seed, distance=1, pairs=PAIRS, counters="own", loops=LOOPS, refine_loops=5, **kw):
    """The batch call on a fresh upload; returns (PlanarBatchResult, the records afterwards)."""
    pts, cnt = fb.upload(ctx, counters)
    n_frames, max_pts = fb.points.shape
    args = dict(RULES[distance])
    args.update(kw)
    res = ctx.register_planar_batch(pts.ptr, cnt.ptr if cnt is not None else None, n_frames, max_pts, pairs,
                                    distance=distance, loops=loops, thresh=5.0, refine_loops=refine_loops,
                                    refine_thresh=3.0, seed=seed, want_inliers=True, want_errors=True, **args)
    return res, pts.to_numpy(SIFT_POINT_DTYPE, (n_frames, max_pts))


def match_rows(ctx, fb, pairs, distance, counters="own"):
    from cusift_amd import capi

    pts, cnt = fb.upload(ctx, counters)
    n_frames, max_pts = fb.points.shape
    rows = upload(ctx, np.full((len(pairs), max_pts, 16), SENTINEL, np.uint8))
    ctx.match_batch(pts.ptr, cnt.ptr if cnt is not None else None, n_frames, max_pts, pairs, rows.ptr, distance)
    ctx.synchronize()
    return rows.to_numpy(capi.MatchRow, (len(pairs), max_pts))


def staged(ctx, fb, rows_p, a, b, seed, distance, counts=None, loops=LOOPS, refine_loops=5):
    """The staged route of one pair: its match rows scattered into a copy of frame a's records, then
    cusift_estimate_homography with the counts the host knows.  Returns (PlanarResult, the copy afterwards)."""
    counts = fb.n if counts is None else counts
    na, nb = int(counts[a]), int(counts[b])
    copy = fb.points[a, :max(na, 1)].copy()
    if na > 0 and nb > 0:  # a pair whose frame b is empty has no row
        row = rows_p[:na]
        copy["score"][:na], copy["ambiguity"][:na], copy["match"][:na] = row["score"], row["ambiguity"], row["match"]
        partner = np.where((row["match"] >= 0) & (row["match"] < nb), row["match"], 0)
        copy["match_xpos"][:na] = fb.points[b, partner]["coords2D"][:, 0]
        copy["match_ypos"][:na] = fb.points[b, partner]["coords2D"][:, 1]
    buf = upload(ctx, copy)
    res = ctx.estimate_homography(buf.ptr, na, nb, loops=loops, thresh=5.0, refine_loops=refine_loops, refine_thresh=3.0,
                                  seed=seed & MASK64, **RULES[distance])
    return res, buf.to_numpy(SIFT_POINT_DTYPE, (max(na, 1),))[:na]


def same_pair(res, p, one, after, na, what):
    """Pair p of a PlanarBatchResult against a PlanarResult of the pair routes and the records they left."""
    assert res.homography[p].tobytes() == one.homography.tobytes(), (what, p)
    assert res.ransac[p].tobytes() == one.ransac.tobytes(), (what, p)
    got = (res.num_candidates[p], res.num_matches[p], res.num_fit[p], res.best_loop[p])
    assert got == (one.num_candidates, one.num_matches, one.num_fit, one.best_loop), (what, p, got)
    assert res.counts[p] == na and len(res.inliers[p]) == na and len(res.match_error[p]) == na, (what, p)
    assert np.array_equal(res.inliers[p], one.inliers[:na]), (what, p)
    if one.num_candidates >= 8:
        assert res.match_error[p].tobytes() == after["match_error"][:na].tobytes(), (what, p)
    else:  # no fit: the pair routes leave match_error alone and the batch writes none
        assert np.isnan(res.match_error[p]).all() and (after["match_error"][:na] == 7.0).all(), (what, p)


def same_results(x, y, pairs=None):
    pairs = range(len(x.counts)) if pairs is None else pairs
    for p in pairs:
        for u, v in zip(x[:7], y[:7]):
            if np.asarray(u[p]).tobytes() != np.asarray(v[p]).tobytes():
                return False
        if x.inliers[p].tobytes() != y.inliers[p].tobytes() or x.match_error[p].tobytes() != y.match_error[p].tobytes():
            return False
    return True


# ------------------------------------------------------------------------------------------------------------------
# on the GPU
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
@pytest.mark.parametrize("seed", (1, 0xC0FFEE, MASK64 - 1))
def test_batch_equals_the_staged_route_bit_for_bit(ctx, frames, seed, distance):
    res, recs = register_batch(ctx, frames, seed, distance)
    assert recs.tobytes() == frames.points.tobytes()  # the records: untouched
    rows = match_rows(ctx, frames, PAIRS, distance)
    for p, (a, b) in enumerate(PAIRS):
        one, after = staged(ctx, frames, rows[p], a, b, seed + p, distance)
        print("distance %d seed %#x pair %d (%d, %d): %d candidates, %d inliers, %d fit, loop %d" %
              (distance, seed, p, a, b, one.num_candidates, one.num_matches, one.num_fit, one.best_loop))
        assert one.num_candidates >= 8 and one.num_matches >= 4, p
        same_pair(res, p, one, after, int(frames.n[a]), "staged")
    # the planted pair: at least 90 % of the 700 planted correspondences, and the planted homography within a pixel
    assert res.num_matches[4] >= 630
    assert corner_distance(res.homography[4][:8], frames.H.ravel()[:8]) < 1.0
    # the same pair twice in one list draws from its own seed each
    assert res.best_loop[0] != res.best_loop[3] or res.ransac[0].tobytes() != res.ransac[3].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("distance", (1, 0))
def test_batch_equals_register_planar_bit_for_bit(ctx, frames, distance):
    """First the condition -- the batch rows ARE the pair matcher's fields, for every pair of the list, index included,
    with no tied row among them -- then the equality of every output."""
    seed = 77
    rows = match_rows(ctx, frames, PAIRS, distance)
    res, _ = register_batch(ctx, frames, seed, distance)
    for p, (a, b) in enumerate(PAIRS):
        na, nb = int(frames.n[a]), int(frames.n[b])
        b1, b2 = upload(ctx, frames.points[a, :na].copy()), upload(ctx, frames.points[b, :nb].copy())
        ctx.match(b1.ptr, na, b2.ptr, nb, distance)
        ctx.synchronize()
        m = b1.to_numpy(SIFT_POINT_DTYPE, (na,))
        tie = tie_rows(m["score"], m["ambiguity"], distance)
        # a zero numerator (an exact copy of the record in frame b) makes the ambiguity 0 whatever the second-best is:
        # the equation says nothing there, the index comparison below does
        tie &= m["ambiguity"] != 0
        print("distance %d pair %d (%d, %d): %d rows, %d tied" % (distance, p, a, b, na, int(tie.sum())))
        assert not tie.any(), (p, np.nonzero(tie)[0][:10])
        for f in ("score", "ambiguity", "match"):
            assert rows[p, :na][f].tobytes() == m[f].tobytes(), (p, f)
        d1, d2 = upload(ctx, frames.points[a, :na].copy()), upload(ctx, frames.points[b, :nb].copy())
        one = ctx.register_planar(d1.ptr, na, d2.ptr, nb, distance=distance, loops=LOOPS, thresh=5.0, refine_loops=5,
                                  refine_thresh=3.0, seed=(seed + p) & MASK64, **RULES[distance])
        same_pair(res, p, one, d1.to_numpy(SIFT_POINT_DTYPE, (na,)), na, "register_planar")


@pytest.mark.gpu
def test_counts_on_the_device_and_degenerate_pairs(ctx, frames):
    seed = 9
    res, recs = register_batch(ctx, frames, seed, pairs=DEGENERATE)
    assert recs.tobytes() == frames.points.tobytes()
    rows = match_rows(ctx, frames, DEGENERATE, 1)
    for p, (a, b) in enumerate(DEGENERATE):
        one, after = staged(ctx, frames, rows[p], a, b, seed + p, 1)
        same_pair(res, p, one, after, int(frames.n[a]), "degenerate list")
    for p in DEGENERATE_AT:
        assert np.array_equal(res.homography[p], IDENT) and np.array_equal(res.ransac[p], IDENT), p
        assert res.num_matches[p] == 0 and res.num_fit[p] == 0 and res.best_loop[p] == 0 and not res.inliers[p].any(), p
    print("candidates of the degenerate list:", res.num_candidates.tolist())
    assert res.num_candidates[1] == 0 and res.counts[1] == 0  # frame a is empty
    assert res.num_candidates[2] == 0 and res.counts[2] == frames.n[1]  # frame b is empty: no row, no candidate
    assert res.num_candidates[3] == 0 and res.counts[3] == 5  # fewer than 8 records: nothing is counted
    assert 0 < res.num_candidates[5] <= 6 and res.counts[5] == 12  # fewer than 8 candidates: as counted
    # the other pairs are what a call without the degenerate pairs gives them (ordinary pairs in those places)
    clean = DEGENERATE.copy()
    clean[list(DEGENERATE_AT)] = (0, 1)
    ref, _ = register_batch(ctx, frames, seed, pairs=clean)
    others = [p for p in range(len(DEGENERATE)) if p not in DEGENERATE_AT]
    assert same_results(res, ref, others) and all(ref.num_matches[p] >= 8 for p in DEGENERATE_AT)
    # a counter past max_pts means max_pts; no counters: every frame is full
    base, _ = register_batch(ctx, frames, seed)
    clamped = frames.counters.copy()
    clamped[5] = MAX_PTS
    assert same_results(base, register_batch(ctx, frames, seed, counters=clamped)[0])
    full = np.full(N_FRAMES, MAX_PTS, np.uint32)
    some = PAIRS[[0, 4, 5, 8]]
    no_counters, recs = register_batch(ctx, frames, seed, pairs=some, counters=None)
    assert same_results(no_counters, register_batch(ctx, frames, seed, pairs=some, counters=full)[0])
    assert (no_counters.counts == MAX_PTS).all() and recs.tobytes() == frames.points.tobytes()
    rows = match_rows(ctx, frames, some, 1, counters=None)
    for p, (a, b) in enumerate(some):
        one, after = staged(ctx, frames, rows[p], a, b, seed + p, 1, counts=full)
        same_pair(no_counters, p, one, after, MAX_PTS, "no counters")
    # no pairs: nothing to do
    none, recs = register_batch(ctx, frames, seed, pairs=np.zeros((0, 2), np.int32))
    assert none.homography.shape == (0, 9) and recs.tobytes() == frames.points.tobytes()


@pytest.mark.gpu
def test_same_seed_same_bytes_other_seed_other_samples_and_no_refit(ctx, frames):
    a, _ = register_batch(ctx, frames, 5)
    b, _ = register_batch(ctx, frames, 5)
    assert same_results(a, b)
    c, _ = register_batch(ctx, frames, 6)
    assert not np.array_equal(a.best_loop, c.best_loop) or a.ransac.tobytes() != c.ransac.tobytes()
    # pair p of seed 6 is pair p + 1's seed of seed 5: (0, 1) sits at 0 and at 3, so seed 5 + 3 = seed 8 + 0
    d, _ = register_batch(ctx, frames, 8)
    assert d.ransac[0].tobytes() == a.ransac[3].tobytes() and d.homography[0].tobytes() == a.homography[3].tobytes()
    # refine_loops = 0: the refined estimate is the winner, and the pair call agrees
    e, _ = register_batch(ctx, frames, 5, refine_loops=0)
    assert e.homography.tobytes() == e.ransac.tobytes() == a.ransac.tobytes()
    assert np.array_equal(e.num_matches, a.num_matches)
    rows = match_rows(ctx, frames, PAIRS, 1)
    for p, (u, v) in enumerate(PAIRS):
        one, after = staged(ctx, frames, rows[p], u, v, 5 + p, 1, refine_loops=0)
        same_pair(e, p, one, after, int(frames.n[u]), "no refit")


@pytest.mark.gpu
def test_batch_refusals_leave_everything_untouched(ctx, frames):
    from cusift_amd import capi

    pts, cnt = frames.upload(ctx)
    n_pairs = len(PAIRS)
    hom, ran = np.full((n_pairs, 9), 9.0, np.float32), np.full((n_pairs, 9), 9.0, np.float32)
    ints = [np.full(n_pairs, -7, np.int32) for _ in range(4)]
    fl = np.full((n_pairs, MAX_PTS), 5, np.int8)
    err = np.full((n_pairs, MAX_PTS), -2.0, np.float32)

    def ptr(a):
        return a.ctypes.data if a is not None else None

    def call(recs=pts.ptr, n_images=N_FRAMES, max_pts=MAX_PTS, pairs=PAIRS, n_pairs=n_pairs, dist=1, rule=1, lo=999.0,
             hi=0.8, loops=64, th=5.0, rl=5, rth=3.0, h=hom, r=ran, pc=ints[0], pm=ints[1], pf=ints[2]):
        pairs = None if pairs is None else np.ascontiguousarray(pairs, np.int32)
        return capi.lib().cusift_register_planar_batch(ctx.handle, recs, cnt.ptr, n_images, max_pts, ptr(pairs), n_pairs,
                                                       dist, rule, lo, hi, loops, th, rl, rth, 1, ptr(h), ptr(r), ptr(pc),
                                                       ptr(pm), ptr(pf), ptr(ints[3]), ptr(fl), ptr(err))

    def untouched():
        return ((hom == 9.0).all() and (ran == 9.0).all() and all((v == -7).all() for v in ints) and (fl == 5).all() and
                (err == -2.0).all())

    nan = float("nan")
    low, high = PAIRS.copy(), PAIRS.copy()
    low[2, 1], high[5, 0] = -1, N_FRAMES
    cases = (  # every case of cusift_register_planar
        dict(h=None), dict(r=None), dict(pc=None), dict(pm=None), dict(pf=None), dict(loops=0), dict(loops=-3),
        dict(th=0.0), dict(th=-1.0), dict(th=nan), dict(rth=0.0), dict(rth=nan), dict(lo=nan), dict(hi=nan), dict(rule=2),
        dict(rule=-1), dict(rl=-1), dict(recs=None), dict(dist=2), dict(dist=-1),
        # the batch's own
        dict(pairs=low), dict(pairs=high), dict(n_pairs=-1), dict(n_pairs=65536, pairs=np.zeros((65536, 2))),
        dict(n_images=-1), dict(n_images=65536), dict(max_pts=-1), dict(max_pts=(1 << 20) + 1), dict(pairs=None),
        dict(n_images=3))
    for kw in cases:
        assert call(**kw) == -1, kw  # CUSIFT_ERR_INVALID
        assert untouched(), kw
    ctx.synchronize()
    assert pts.to_numpy(SIFT_POINT_DTYPE, (N_FRAMES, MAX_PTS)).tobytes() == frames.points.tobytes()
    with pytest.raises(capi.CusiftError):
        ctx.register_planar_batch(pts.ptr, cnt.ptr, N_FRAMES, MAX_PTS, high)
    # n_pairs == 0 is not an error and writes nothing
    assert call(n_pairs=0) == 0 and call(n_pairs=0, pairs=None) == 0 and untouched()
    # and the same arguments without a fault run; a block's tail is not written
    assert call(loops=LOOPS) == 0 and not untouched()
    for p, (a, b) in enumerate(PAIRS):
        na = int(frames.n[a])
        assert ints[0][p] >= 8 and ints[1][p] >= 4 and hom[p, 8] == 1.0 and ran[p, 8] == 1.0, p
        assert np.isin(fl[p, :na], (0, 1)).all() and (fl[p, na:] == 5).all(), p
        assert (err[p, :na] != -2.0).all() and (err[p, na:] == -2.0).all(), p
        assert fl[p, :na].sum() == ints[1][p], p
    assert pts.to_numpy(SIFT_POINT_DTYPE, (N_FRAMES, MAX_PTS)).tobytes() == frames.points.tobytes()
    # the optional outputs may be left out
    h2, r2 = np.zeros_like(hom), np.zeros_like(ran)
    c2 = [np.zeros(n_pairs, np.int32) for _ in range(3)]
    assert capi.lib().cusift_register_planar_batch(ctx.handle, pts.ptr, cnt.ptr, N_FRAMES, MAX_PTS, PAIRS.ctypes.data,
                                                   n_pairs, 1, 1, 999.0, 0.8, LOOPS, 5.0, 5, 3.0, 1, ptr(h2), ptr(r2),
                                                   ptr(c2[0]), ptr(c2[1]), ptr(c2[2]), None, None, None) == 0
    assert h2.tobytes() == hom.tobytes() and r2.tobytes() == ran.tobytes() and all(
        np.array_equal(u, v) for u, v in zip(c2, ints))


def optional_outputs_three_ways(call, n_pairs, max_pts, shape, dtype):
    """call(eight output pointers) -> status, made three times: h_inliers and h_match_error both NULL, only h_inliers
    NULL, both given -- the three sizes of the pair-list runner's read-back.  The two models and the four count arrays
    are byte-equal in all three; what is not asked for is not written.  Returns the third call's (models and counts,
    flags, errors)."""
    got = []
    for want_flags, want_err in ((False, False), (False, True), (True, True)):
        models = [np.full((n_pairs,) + shape, 9.0, dtype) for _ in range(2)]
        ints = [np.full(n_pairs, -7, np.int32) for _ in range(4)]
        fl = np.full((n_pairs, max_pts), -1, np.int8)
        err = np.full((n_pairs, max_pts), np.nan, np.float32)
        assert call(*([a.ctypes.data for a in models + ints] + [fl.ctypes.data if want_flags else None,
                                                                err.ctypes.data if want_err else None])) == 0
        assert want_flags or (fl == -1).all()
        assert want_err or np.isnan(err).all()
        got.append((models + ints, fl, err))
    for other in got[:2]:
        for u, v in zip(other[0], got[2][0]):
            assert u.tobytes() == v.tobytes()
    assert got[1][2].tobytes() == got[2][2].tobytes()  # the errors do not depend on the flags being asked for
    return got[2]


@pytest.mark.gpu
def test_optional_outputs_left_out_change_nothing_else(ctx, frames):
    """The read-back branches that capi.Context.register_planar_batch never reaches (it always passes a flags array), on
    the degenerate list: raw calls with neither flags nor errors, with errors only, with both.  Models and counts
    byte-equal; the third call's flags and errors are the wrapper's."""
    from cusift_amd import capi

    seed, n_pairs = 9, len(DEGENERATE)
    pts, cnt = frames.upload(ctx)
    outs, fl, err = optional_outputs_three_ways(
        lambda *out: capi.lib().cusift_register_planar_batch(ctx.handle, pts.ptr, cnt.ptr, N_FRAMES, MAX_PTS,
                                                             DEGENERATE.ctypes.data, n_pairs, 1, 1, 999.0, 0.8, LOOPS,
                                                             5.0, 5, 3.0, seed, *out),
        n_pairs, MAX_PTS, (9,), np.float32)
    res, _ = register_batch(ctx, frames, seed, pairs=DEGENERATE)
    for u, v in zip(outs, res[:6]):
        assert u.tobytes() == np.asarray(v).tobytes()
    for p in range(n_pairs):
        n = int((fl[p] >= 0).sum())
        assert n == res.counts[p] and (fl[p, :n] >= 0).all(), p
        assert np.array_equal(fl[p, :n] == 1, res.inliers[p]), p
        assert err[p, :n].tobytes() == res.match_error[p].tobytes() and np.isnan(err[p, n:]).all(), p
    assert np.isnan(err[list(DEGENERATE_AT)]).all() and not np.isnan(err[0, :frames.n[0]]).all()


@pytest.mark.gpu
def test_register_planar_sequence_end_to_end(ctx, oracle, gray1):
    """gray1.pgm and three frames warped by cumulative mild homographies, extracted by BatchExtractor and registered
    with register_planar_sequence(): every pair has the bits of register_planar on copies of its two frames, and a
    corner error against its true homography no worse than 1.5 x that of the all-CPU route (oracle extraction, oracle
    matcher, oracle RANSAC on the device's samples, numpy refit) plus r32, the rule of
    test_planar.test_end_to_end_on_a_warped_frame; the corners are this frame's own.  The chained corner error to frame
    0 is printed, no bound on it is invented.  Measured: not measured yet."""
    import torch
    from cusift_amd import capi
    from cusift_amd.batch import BatchExtractor

    steps = [np.array([[0.98, -0.03, 9.0], [0.025, 1.01, -6.0], [1.5e-5, -2.0e-5, 1.0]]),
             np.array([[1.01, 0.02, -7.0], [-0.015, 0.99, 8.0], [-1.0e-5, 1.2e-5, 1.0]]),
             np.array([[0.99, -0.02, 6.0], [0.02, 1.005, 5.0], [0.8e-5, 1.0e-5, 1.0]])]
    cumulative = [np.eye(3)]
    for s in steps:
        cumulative.append(s @ cumulative[-1])  # frame 0 onto frame k
    h, w = gray1.shape
    images = np.stack([gray1] + [warp(gray1, c) for c in cumulative[1:]])
    prm = dict(num_octaves=4, init_blur=0.0, peak_thresh=1.0, max_pts=4096)
    ex = BatchExtractor(4, w, h, **prm)
    saved = test_planar.CORNERS
    test_planar.CORNERS = np.array([[0, 0], [w, 0], [0, h], [w, h]], dtype=np.float64)
    try:
        ex.extract(ex.images_from_numpy(images))
        torch.cuda.synchronize()
        before = [r.copy() for r in ex.to_host()]
        kw = dict(distance=1, rule=1, lo=999.0, hi=0.8, loops=2000, thresh=5.0, refine_loops=5, refine_thresh=3.0)
        seed = 21
        res = ex.register_planar_sequence(seed=seed, want_errors=True, **kw)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, ex.to_host()))  # the records: untouched
        assert len(res.counts) == 3 and res.counts.tolist() == [len(r) for r in before[:3]]
        oracle_recs = [oracle.extract(img, **prm).copy() for img in images]
        for p in range(3):
            n1, n2 = len(before[p]), len(before[p + 1])
            c1, c2 = upload(ex.ctx, before[p]), upload(ex.ctx, before[p + 1])
            one = ex.ctx.register_planar(c1.ptr, n1, c2.ptr, n2, seed=seed + p, want_all=True, **kw)
            same_pair(res, p, one, c1.to_numpy(SIFT_POINT_DTYPE, (n1,)), n1, "sequence")
            true = steps[p]
            truth = true.ravel()[:8] / true[2, 2]
            d_dev = corner_distance(res.homography[p][:8], truth)
            # the all-CPU route
            o1, o2 = oracle_recs[p].copy(), oracle_recs[p + 1].copy()
            oracle.match(o1, o2, 1)
            cand = candidates(o1, 1, 999.0, 0.8, len(o2))
            assert len(cand) >= 8
            dev1 = before[p]
            used = np.unique(one.drawn)
            key = lambda r: np.c_[r["coords2D"], r["scale"]].astype(np.float64)
            dist = np.abs(key(dev1[used])[:, None, :] - key(o1)[None, :, :]).max(axis=2)
            to_oracle = np.zeros(len(dev1), dtype=np.int32)
            to_oracle[used] = dist.argmin(axis=1)
            hom, _, _, _, _ = oracle.find_homography(o1, to_oracle[one.drawn], thresh=5.0)
            cpu = improve(o1, hom, 5, 3.0, cand).astype(np.float32)
            d_cpu = corner_distance(cpu, truth)
            r32 = r32_of(cpu)
            print("pair %d: corner error against the known homography: device %.4f px, all-CPU %.4f px (r32 %.3g); "
                  "%d candidates, %d inliers, %d fit" % (p, d_dev, d_cpu, r32, res.num_candidates[p], res.num_matches[p],
                                                         res.num_fit[p]))
            assert res.num_matches[p] >= 50
            assert d_dev <= 1.5 * d_cpu + r32, (p, d_dev, d_cpu, r32)
        chain = capi.chain_homographies(res.homography, [(i, i + 1) for i in range(3)])
        for k in range(1, 4):
            frame_k = apply(cumulative[k], test_planar.CORNERS)  # where frame 0's corners lie in frame k
            err = np.sqrt(((apply(chain[k], frame_k) - test_planar.CORNERS) ** 2).sum(axis=1)).max()
            print("chained corner error of frame %d against frame 0: %.4f px" % (k, err))
    finally:
        test_planar.CORNERS = saved
        ex.close()


@pytest.mark.gpu
def test_cpp_sequence_program_passes_on_gpu():
    """tests/cpp_planar_batch/planar_batch_dropin.cpp: RegisterPlanarSequence against RegisterPlanar per pair."""
    build_cpp()
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    print(out.stdout[-3000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout and "pair 4 (2, 2):" in out.stdout
