"""Detection and keypoint stages on tied, symmetric and non-finite images (tests/degenerate_images.py).

On noise, gray1, synth.tile / synth.blobs and a Gaussian blob no two DoG values are equal, no orientation histogram has
two equal peaks and no arithmetic leaves the normal float range -- the places where the kernels (min3f / max3f trees, DPP
column exchange, wave-row pre-test, IEEE division sequences) and the oracle (fminf / fmaxf loops, two strict compares)
are written differently.  Here:

  * the PREMISE tests (CPU, the oracle alone) assert that each family still is what it is used for: zero strict extrema
    among hundreds of tied centres, orientation peaks that are exactly equal, NaN DoG values, refinement products that
    leave the normal range.  They print the counts.
  * the GPU tests compare every stage with the oracle on the same input, every size, init_blur 0.0 and 1.0, every
    keypoint: LaplaceMulti, FindPointsMulti (aligned and odd pitch), the fused detection with and without the next
    octave on batches of two images of DIFFERENT families, and cusift_extract_batch on the six launch routes, fused
    or two-stage, tex_frac_bits 8 and 0.

Record sets are compared as multisets of bit keys with NaNs normalised (parity_utils.same_records); images under the
same rule (same_values).  No fraction of records or pixels is exempt.
"""
import functools

import numpy as np
import pytest

import degenerate_images as dg
from cusift_amd import capi
from cusift_amd.capi import SIFT_POINT_DTYPE, DeviceBuffer
from oracle_binding import pitched
from parity_utils import HEAD_FIELDS, same_records
from test_detect_refine_sites_gpu import ROUTES

THRESH = 0.1
EDGE = 10.0
BLURS = (0.0, 1.0)
SEED_A, SEED_B = 21, 22
DETECTED = ("coords2D", "scale", "sharpness", "edgeness", "subsampling")
MAX_PTS = 16384


# ---- the oracle's DoG, and a numpy restatement of its extremum and edge tests ------------------------------------------
def dog_of(oracle, img, blur):
    h, w = img.shape
    return oracle.laplace_multi(pitched(img), w, h, blur)[:, :, :w]


def centres(dog, thr):
    """([5, h, w] strict, [5, h, w] tied): centres of DoG planes 1..5 beyond the threshold that are strictly beyond all
    26 neighbours / that EQUAL their extreme neighbour.  np.fmin / np.fmax drop NaNs as fminf / fmaxf do.  Border pixels
    are neither (clamped addressing compares them with themselves: never strict, trivially tied)."""
    _, h, w = dog.shape
    thr = np.float32(thr)
    strict = np.zeros((5, h, w), dtype=bool)
    tied = np.zeros((5, h, w), dtype=bool)
    for s in range(1, 6):
        c = dog[s, 1:-1, 1:-1]
        mx = np.full_like(c, -np.inf)
        mn = np.full_like(c, np.inf)
        for p in (s - 1, s, s + 1):
            for dy in range(3):
                for dx in range(3):
                    if (p, dy, dx) != (s, 1, 1):
                        n = dog[p, dy:h - 2 + dy, dx:w - 2 + dx]
                        mx, mn = np.fmax(mx, n), np.fmin(mn, n)
        strict[s - 1, 1:-1, 1:-1] = ((c > thr) & (c > mx)) | ((c < -thr) & (c < mn))
        tied[s - 1, 1:-1, 1:-1] = ((c > thr) & (c == mx)) | ((c < -thr) & (c == mn))
    return strict, tied


def keypoint_sites(dog, thr, edge=EDGE):
    """[n, 3] (y, x, s) of the sites the oracle turns into keypoints, in its emission order (y, x, s): the strict extrema
    that pass `tra * tra < edge * det`, restated operation by operation in float32 (the oracle is built without
    implicit fusion)."""
    strict, _ = centres(dog, thr)
    f = np.float32
    with np.errstate(all="ignore"):
        out = []
        for s in range(1, 6):
            c = dog[s]
            ys, xs = np.nonzero(strict[s - 1])
            val = c[ys, xs]
            dxx = f(2.0) * val - c[ys, xs - 1] - c[ys, xs + 1]
            dyy = f(2.0) * val - c[ys - 1, xs] - c[ys + 1, xs]
            dxy = f(0.25) * (c[ys + 1, xs + 1] + c[ys - 1, xs - 1] - c[ys - 1, xs + 1] - c[ys + 1, xs - 1])
            tra = dxx + dyy
            det = dxx * dyy - dxy * dxy
            ok = tra * tra < f(edge) * det
            out.append(np.stack([ys[ok], xs[ok], np.full(int(ok.sum()), s - 1)], axis=1))
    sites = np.concatenate(out)
    return sites[np.lexsort((sites[:, 2], sites[:, 1], sites[:, 0]))]


def oracle_points(oracle, dog, thr, sub=1.0):
    _, h, w = dog.shape
    src = np.ascontiguousarray(dog)
    want, n = oracle.find_points_multi(src, w, h, thr, EDGE, sub, 1 << 16)
    assert n < (1 << 16)
    return want[:n]


# ---- the cases: two images of different families per case, one threshold scale -----------------------------------------
def build_cases(w, h):
    """{name: (image a, image b, e)}: the two images of a batch come from different families (per-image lists; a wave-row
    skipped for one image must not be skipped for the other); thresholds are THRESH * 2^e."""
    clean = dg.noise(SEED_A, w, h)
    cases = {
        "rows+checker": (dg.rows(SEED_A, w, h), dg.checker(w, h), 0),
        "cols+dots8": (dg.cols(SEED_B, w, h), dg.dots(w, h, 8), 0),
        "dots16+" + ("mirror" if w % 2 == 0 else "noise"): (
            dg.dots(w, h, 16), dg.mirror(SEED_B, w, h) if w % 2 == 0 else dg.noise(SEED_B, w, h), 0),
    }
    for kind, value in (("nan_pixel", np.nan), ("inf_pixel", np.inf)):
        for pos, y, x in dg.pixel_positions(w, h):
            cases["%s@%s+noise" % (kind, pos)] = (dg.poisoned(SEED_A, w, h, value, y, x), clean, 0)
    for e in dg.SCALED_EXPONENTS:
        cases["scaled(%+d)" % e] = (dg.scaled(SEED_A, w, h, e), dg.scaled(SEED_B, w, h, e), e)
    return cases


CASE_NAMES = list(build_cases(256, 40))  # the same names at every size except the partner of dots16
EXTRACT_CASES = [c for c in CASE_NAMES if not c.startswith("scaled") or c in ("scaled(-48)", "scaled(+36)")]


@functools.lru_cache(maxsize=None)
def cases_of(w, h):
    return build_cases(w, h)


def case(w, h, name):
    if name.startswith("dots16+"):
        name = "dots16+" + ("mirror" if w % 2 == 0 else "noise")
    a, b, e = cases_of(w, h)[name]
    return (a, b), float(np.float32(THRESH) * np.float32(2.0 ** e))


# =========================================================================================================================
# Premise tests (CPU): the oracle alone
# =========================================================================================================================
def tally(oracle, img, blur, thr=THRESH):
    dog = dog_of(oracle, img, blur)
    strict, tied = centres(dog, thr)
    return int(strict.sum()), int(tied.sum()), len(oracle_points(oracle, dog, thr))


@pytest.mark.parametrize("w,h", dg.SIZES)
@pytest.mark.parametrize("blur", BLURS)
def test_premise_stripes_have_tied_centres_and_no_strict_one(oracle, w, h, blur):
    for name, img in (("rows", dg.rows(SEED_A, w, h)), ("cols", dg.cols(SEED_B, w, h))):
        strict, tied, kp = tally(oracle, img, blur)
        print("%s %dx%d init_blur %.1f: %d strict extrema, %d keypoints, %d tied centres" % (name, w, h, blur, strict, kp, tied))
        assert strict == 0 and kp == 0 and tied > 200, (name, strict, kp, tied)


@pytest.mark.parametrize("w,h", dg.SIZES)
def test_premise_checker_has_strict_extrema_among_tied_centres(oracle, w, h):
    strict, tied, kp = tally(oracle, dg.checker(w, h), 1.0)
    print("checker %dx%d init_blur 1.0: %d strict extrema, %d keypoints, %d tied centres" % (w, h, strict, kp, tied))
    assert kp > 400 and tied > kp, (kp, tied)


def exact_orientation_ties(oracle, img, frac_bits, **kw):
    pts, peaks = oracle.extract_with_orientation_peaks(img, num_octaves=3, init_blur=1.0, peak_thresh=THRESH,
                                                       edge_thresh=EDGE, max_pts=MAX_PTS, tex_frac_bits=frac_bits, **kw)
    return len(pts), int((peaks[:, 0] == 1.0).sum()), int((peaks[:, 0] > 0.999).sum())


@pytest.mark.parametrize("w,h", dg.SIZES[:2])
@pytest.mark.parametrize("frac_bits", [8, 0])
def test_premise_dots_have_exactly_tied_orientation_peaks(oracle, w, h, frac_bits):
    for period, bar in ((8, 100), (16, 20)):
        n, exact, near = exact_orientation_ties(oracle, dg.dots(w, h, period), frac_bits)
        print("dots%d %dx%d tex_frac_bits %d, 3 octaves: %d keypoints, %d with second peak == first, %d above 0.999"
              % (period, w, h, frac_bits, n, exact, near))
        assert exact >= bar, (period, n, exact)


def test_premise_mirror_has_tied_and_strict_centres(oracle):
    w, h = 256, 40
    for blur in BLURS:
        strict, tied, kp = tally(oracle, dg.mirror(SEED_B, w, h), blur)
        print("mirror %dx%d init_blur %.1f: %d strict extrema, %d keypoints, %d tied centres" % (w, h, blur, strict, kp, tied))
        assert tied >= 1 and strict >= 50, (strict, tied)


@pytest.mark.parametrize("w,h", dg.SIZES)
@pytest.mark.parametrize("kind,value", [("nan_pixel", np.nan), ("inf_pixel", np.inf)])
def test_premise_one_bad_pixel_spoils_its_neighbourhood_only(oracle, w, h, kind, value):
    """NaN DoG values exist, and the keypoints whose 3 x 3 x 3 neighbourhood holds none of them are the clean image's."""
    clean = dg.noise(SEED_A, w, h)
    for blur in BLURS:
        dog0 = dog_of(oracle, clean, blur)
        sites0 = keypoint_sites(dog0, THRESH)
        pts0 = oracle_points(oracle, dog0, THRESH)
        assert len(sites0) == len(pts0)  # the restatement finds the oracle's sites
        for pos, y, x in dg.pixel_positions(w, h):
            dog = dog_of(oracle, dg.poisoned(SEED_A, w, h, value, y, x), blur)
            bad = np.isnan(dog)
            assert bad.sum() >= 1 and np.array_equal(dog[~bad], dog0[~bad])
            sites, pts = keypoint_sites(dog, THRESH), oracle_points(oracle, dog, THRESH)
            assert len(sites) == len(pts)

            def far(st):
                return np.array([not bad[s:s + 3, yy - 1:yy + 2, xx - 1:xx + 2].any() for yy, xx, s in st], dtype=bool)

            f0, f1 = far(sites0), far(sites)
            print("%s@%s %dx%d init_blur %.1f: %d NaN DoG values, %d keypoints, %d of them away from every NaN (clean: %d "
                  "of %d)" % (kind, pos, w, h, blur, int(bad.sum()), len(pts), int(f1.sum()), int(f0.sum()), len(pts0)))
            assert np.array_equal(sites0[f0], sites[f1])
            assert pts[f1].tobytes() == pts0[f0].tobytes()
            assert f1.sum() > 0


@pytest.mark.parametrize("w,h", dg.SIZES[:2])
def test_premise_inf_pixel_gives_nan_orientations(oracle, w, h):
    img = dg.poisoned(SEED_A, w, h, np.inf, h // 2, w // 2)
    seen = 0
    for blur in BLURS:
        pts = oracle.extract(img, num_octaves=3, init_blur=blur, peak_thresh=THRESH, edge_thresh=EDGE, max_pts=MAX_PTS)
        n_ori = int(np.isnan(pts["orientation"]).sum())
        seen = max(seen, n_ori)
        n_desc = int((~np.isfinite(pts["data"]).all(axis=1)).sum())
        print("inf_pixel@centre %dx%d init_blur %.1f, 3 octaves: %d keypoints, %d NaN orientations, %d non-finite "
              "descriptors" % (w, h, blur, len(pts), n_ori, n_desc))
    assert seen >= 1  # the dense list (init_blur 1.0) holds them; the sparse one need not


def scaled_kinds(oracle, w, h, blur, e):
    """(count unscaled, count scaled, identical, finite but different, non-finite): octave-0 keypoints of noise * 2^e
    under thresholds * 2^e against the unscaled ones scaled back (the DoG scales exactly: asserted)."""
    two_e = np.float32(2.0 ** e)
    dog0 = dog_of(oracle, dg.noise(SEED_A, w, h), blur)
    dog = dog_of(oracle, dg.scaled(SEED_A, w, h, e), blur)
    assert np.array_equal(dog, dog0 * two_e) and np.isfinite(dog).all()
    p0 = oracle_points(oracle, dog0, THRESH)
    p = oracle_points(oracle, dog, float(np.float32(THRESH) * two_e))
    fields = np.column_stack([p["coords2D"], p["scale"], p["sharpness"], p["edgeness"]])
    nonfinite = ~np.isfinite(fields).all(axis=1)
    if len(p) != len(p0):
        return len(p0), len(p), 0, 0, int(nonfinite.sum())
    same = (p["coords2D"] == p0["coords2D"]).all(axis=1)  # both strict extrema of the same sites, in the same order
    return len(p0), len(p), int((same & ~nonfinite).sum()), int((~same & ~nonfinite).sum()), int(nonfinite.sum())


def test_premise_scaled_noise_leaves_the_normal_range(oracle):
    w, h = 256, 40
    got = {}
    for e in dg.SCALED_EXPONENTS:
        for blur in BLURS:
            got[e, blur] = k = scaled_kinds(oracle, w, h, blur, e)
            print("scaled(%+d) %dx%d init_blur %.1f, octave 0: %d keypoints unscaled, %d scaled: %d identical, %d finite "
                  "but different, %d non-finite" % ((e, w, h, blur) + k))
    for e in (-46, -48, -50):  # subnormal triple products: finite, but not the unscaled result
        assert max(got[e, b][3] for b in BLURS) >= 1, (e, got[e, 0.0], got[e, 1.0])
    assert got[-52, 0.0][4] >= 1
    assert min(got[36, 1.0][2:5]) >= 1, got[36, 1.0]
    assert any(got[60, b][0] != got[60, b][1] for b in BLURS)


# =========================================================================================================================
# GPU tests: every stage against the oracle on the same input
# =========================================================================================================================
def same_values(want, got, label):
    """Two float32 arrays: NaN at the same positions, everything else bit for bit (so +-Inf by value, signed zeros
    exactly).  NaN sign and payload are not compared: `inf - inf` gives the computing machine's default NaN."""
    want, got = np.ascontiguousarray(want, dtype=np.float32), np.ascontiguousarray(got, dtype=np.float32)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg="%s: NaN positions" % label)
    np.testing.assert_array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan], err_msg="%s: values" % label)


PAD = np.frombuffer(b"\x5a" * 4, dtype=np.uint32)[0]
GRID = [pytest.param(w, h, blur, id="%dx%d-blur%.0f" % (w, h, blur)) for w, h in dg.SIZES for blur in BLURS]


@functools.lru_cache(maxsize=None)
def oracle_stage(oracle, w, h, name, blur):
    """Per image of the case: (oracle DoG on the aligned pitch, its keypoints with subsampling 2.0)."""
    imgs, thr = case(w, h, name)
    out = []
    for img in imgs:
        dog = oracle.laplace_multi(pitched(img), w, h, blur)
        pts, n = oracle.find_points_multi(dog, w, h, thr, EDGE, 2.0, MAX_PTS)
        assert n < MAX_PTS
        out.append((dog, pts[:n]))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("w,h,blur", GRID)
def test_laplace_multi_equals_the_oracle(ctx, oracle, w, h, blur, name):
    imgs, _ = case(w, h, name)
    for i, img in enumerate(imgs):
        src = pitched(img)
        p = src.shape[1]
        want = oracle_stage(oracle, w, h, name, blur)[i][0]
        d_src = DeviceBuffer.from_numpy(ctx, src)
        d_dog = DeviceBuffer(ctx, 7 * h * p * 4)
        ctx.memset(d_dog.ptr, 0x5A, 7 * h * p * 4)
        ctx.laplace_multi(d_src.ptr, w, h, p, blur, d_dog.ptr)
        got = d_dog.to_numpy(np.float32, (7, h, p)).copy()
        d_src.free()
        d_dog.free()
        same_values(want[:, :, :w], got[:, :, :w], "%s[%d]" % (name, i))
        assert (got[:, :, w:].view(np.uint32) == PAD).all(), "pad columns written"


def find_points(ctx, dog, w, h, thr, sub):
    p = dog.shape[2]
    d_dog = DeviceBuffer.from_numpy(ctx, dog)
    d_pts = DeviceBuffer(ctx, MAX_PTS * 588)
    d_pts.zero()
    d_cnt = DeviceBuffer(ctx, 4)
    d_cnt.zero()
    ctx.find_points_multi(d_dog.ptr, w, h, p, thr, EDGE, sub, d_pts.ptr, MAX_PTS, d_cnt.ptr)
    n = int(d_cnt.to_numpy(np.uint32, (1,))[0])
    pts = d_pts.to_numpy(SIFT_POINT_DTYPE, (MAX_PTS,)).copy()
    for b in (d_dog, d_pts, d_cnt):
        b.free()
    return n, pts


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("w,h,blur", GRID)
def test_find_points_multi_on_the_oracles_dog(ctx, oracle, w, h, blur, name):
    """The fast kernel (aligned pitch) and the generic one (rows not 16-byte aligned) on the oracle's DoG."""
    _, thr = case(w, h, name)
    odd = w + 1 if (w + 1) % 4 else w + 3
    for i, (dog, want) in enumerate(oracle_stage(oracle, w, h, name, blur)):
        for p in (dog.shape[2], odd):
            src = np.zeros((7, h, p), dtype=np.float32)
            src[:, :, :w] = dog[:, :, :w]
            n, got = find_points(ctx, src, w, h, thr, 2.0)
            label = "%s[%d] pitch %d" % (name, i, p)
            assert n == len(want), (label, n, len(want))
            same_records(want, got[:n], DETECTED, label)


def heads_as_records(heads):
    rec = np.zeros(len(heads), dtype=SIFT_POINT_DTYPE)
    rec["coords2D"] = heads[:, 0:2]
    for f, col in (("scale", 2), ("sharpness", 3), ("edgeness", 4), ("subsampling", 12)):
        rec[f] = heads[:, col]
    return rec


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("w,h,blur", GRID)
def test_fused_detection_of_two_families_per_call(ctx, oracle, w, h, blur, name):
    """cusift_detect_multi and cusift_detect_multi_down, n_images = 2: per-image lists equal the oracle's, the heads of
    the second equal the records of the first, the emitted next octave equals the oracle's ScaleDown."""
    imgs, thr = case(w, h, name)
    stack = np.stack([pitched(i) for i in imgs])
    p = stack.shape[2]
    ow, oh = w // 2, h // 2
    op = capi.ialign_up(ow, 128)
    d_img = DeviceBuffer.from_numpy(ctx, stack)
    d_pts = DeviceBuffer(ctx, 2 * MAX_PTS * 588)
    d_heads = DeviceBuffer(ctx, 2 * MAX_PTS * 64)
    d_cnt = DeviceBuffer(ctx, 8)
    d_cnt2 = DeviceBuffer(ctx, 8)
    d_next = DeviceBuffer(ctx, 2 * oh * op * 4)
    for b in (d_pts, d_heads, d_cnt, d_cnt2):
        b.zero()
    ctx.memset(d_next.ptr, 0x5A, 2 * oh * op * 4)
    ctx.detect_multi(d_img.ptr, w, h, p, blur, thr, EDGE, 2.0, d_pts.ptr, MAX_PTS, d_cnt.ptr, n_images=2)
    ctx.detect_multi_down(d_img.ptr, w, h, p, blur, thr, EDGE, 2.0, d_heads.ptr, MAX_PTS, d_cnt2.ptr, d_next.ptr, op,
                          n_images=2)
    cnt = d_cnt.to_numpy(np.uint32, (2,)).copy()
    cnt2 = d_cnt2.to_numpy(np.uint32, (2,)).copy()
    pts = d_pts.to_numpy(SIFT_POINT_DTYPE, (2, MAX_PTS)).copy()
    heads = d_heads.to_numpy(np.float32, (2, MAX_PTS, 16)).copy()
    nxt = d_next.to_numpy(np.float32, (2, oh, op)).copy()
    for b in (d_img, d_pts, d_heads, d_cnt, d_cnt2, d_next):
        b.free()
    for i, (_, want) in enumerate(oracle_stage(oracle, w, h, name, blur)):
        label = "%s[%d]" % (name, i)
        assert cnt[i] == cnt2[i] == len(want), (label, int(cnt[i]), int(cnt2[i]), len(want))
        same_records(want, pts[i, :cnt[i]], DETECTED, label + " records")
        same_records(pts[i, :cnt[i]], heads_as_records(heads[i, :cnt2[i]]), DETECTED, label + " heads")
        same_values(oracle.scale_down(stack[i], w, h)[:oh, :ow], nxt[i, :, :ow], label + " next octave")
        assert (nxt[i, :, ow:].view(np.uint32) == PAD).all(), label + ": pad columns written"


# ---- the whole extraction: six launch routes, fused or two-stage, tex_frac_bits 8 and 0 --------------------------------
@pytest.fixture(scope="module")
def routes():
    ctxs = {}
    for name, (side, lists, per_octave, pyramid) in ROUTES.items():
        c = capi.Context(0)
        c.set_policy(capi.POLICY_SIDE_STREAM, side)
        c.set_policy(capi.POLICY_OCTAVE_LISTS, lists)
        if per_octave:
            c.set_policy(capi.POLICY_LAUNCH_PER_OCTAVE, 1)
        c.set_policy(capi.POLICY_PYRAMID_IN_DETECT, pyramid)
        ctxs[name] = c
    yield ctxs
    for c in ctxs.values():
        c.close()


def extract_batch(ctx, stack, w, h, prm):
    n, _, p = stack.shape
    d_imgs = DeviceBuffer.from_numpy(ctx, stack)
    d_pts = DeviceBuffer(ctx, n * prm.max_pts * 588)
    d_pts.zero()
    d_cnt = DeviceBuffer(ctx, 4 * n)
    ctx.extract_batch(d_imgs.ptr, n, w, h, p, h * p, prm, d_pts.ptr, d_cnt.ptr)
    ctx.synchronize()
    cnt = d_cnt.to_numpy(np.uint32, (n,)).copy()
    pts = d_pts.to_numpy(SIFT_POINT_DTYPE, (n, prm.max_pts)).copy()
    for b in (d_imgs, d_pts, d_cnt):
        b.free()
    return cnt, pts


@pytest.mark.gpu
@pytest.mark.parametrize("name", EXTRACT_CASES)
@pytest.mark.parametrize("w,h,blur", GRID)
def test_extract_batch_on_every_route(routes, oracle, record_property, w, h, blur, name):
    """Head fields identical, NaN-descriptor rows in the same places, every finite descriptor within 1e-4 L2.  On dots8 /
    dots16 most orientation arg-maxes are exactly tied: this pins which of two equal peaks wins."""
    imgs, thr = case(w, h, name)
    stack = np.stack([pitched(i) for i in imgs])
    compared, ties, worst = 0, 0, 0.0
    for frac_bits in (8, 0):
        kw = dict(num_octaves=3, init_blur=blur, peak_thresh=thr, edge_thresh=EDGE, max_pts=MAX_PTS,
                  tex_frac_bits=frac_bits)
        want = []
        for img in imgs:  # once, shared by the routes
            pts, peaks = oracle.extract_with_orientation_peaks(img, **kw)
            assert len(pts) < MAX_PTS
            want.append(pts)
            ties += int((peaks[:, 0] == 1.0).sum())
        for route, c in routes.items():
            for fused in (0, 1):
                cnt, pts = extract_batch(c, stack, w, h, capi.default_params(fused_detect=fused, **kw))
                for i in range(2):
                    label = "%s[%d], %s, fused_detect %d, tex_frac_bits %d" % (name, i, route, fused, frac_bits)
                    assert cnt[i] == len(want[i]), (label, int(cnt[i]), len(want[i]))
                    worst = max(worst, same_records(want[i], pts[i, :cnt[i]], HEAD_FIELDS, label, desc_tol=1e-4))
                    compared += len(want[i])
    record_property("keypoints_compared", compared)
    record_property("exactly_tied_orientation_peaks", ties)
    record_property("max_descriptor_l2", worst)
    print("%s %dx%d init_blur %.1f: %d keypoints compared, %d exactly tied orientation peaks in the oracle's lists, "
          "largest descriptor L2 %.3e" % (name, w, h, blur, compared, ties, worst))
