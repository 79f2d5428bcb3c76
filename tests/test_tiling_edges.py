"""Strip tiling where it can go wrong: odd strip borders with keypoints on both sides of every one, both routes of
cusift_tiled_process (one launch for all bands / octave by octave), the options that reach the band kernels, a smaller
halo, overflow beyond max_pts, an extractor that is used again, and the distributed form on the per-octave route.

The image (`pyramid_noise`) has structure in every octave and is dense at the borders; the cases put the borders of
every tiled octave at rows that come from an odd b_k (197 >> 1 = 98, 197 >> 2 = 49, 395 >> 1 = 197 ...), so the shift of
the ownership rule [b_k >> o, b_{k+1} >> o) rounds.  The CPU tests hold the premise from the oracle alone: every border
of every tiled octave has a keypoint in its last owned row above and its first owned row below, and every footprint
stays inside the halo by the kernels' own flag condition restated -- so "nothing is found twice, nothing is lost" and
check() == 0 are claims about the kernels.

No tolerance of this file's own: tiled against the whole image is bit for bit on every field extraction writes; the
whole image against the CPU oracle uses same_set's bars (head fields and orientation bit for bit, descriptors below
1e-4 L2).
"""
import collections
import contextlib

import numpy as np
import pytest
import torch

from cusift_amd import capi
from cusift_amd.capi import SIFT_POINT_DTYPE
from cusift_amd.tiling import HALO, StripExtractor, StripPlan, run_distributed, run_virtual
from test_detect_refine_sites_gpu import same_set
from test_keypoint_routes import reach_of
from test_tiling_gpu import canonical_order, whole_image

gpu = pytest.mark.gpu

MAX_PTS = 65536
FIELDS = ("coords2D", "scale", "sharpness", "edgeness", "orientation", "subsampling", "data")  # what extraction writes
ROUTES = ("bands", "per-octave")
SENTINEL = 0x5A


def pyramid_noise(seed, w, h, levels=5):
    r = np.random.RandomState(seed)
    img = np.zeros((h, w))
    for k in range(levels):
        s = 1 << k
        c = r.rand(-(-h // s) + 1, -(-w // s) + 1) * 255.0
        oy, ox = r.randint(0, s), r.randint(0, s)
        img += np.kron(c, np.ones((s, s)))[oy:oy + h, ox:ox + w]
    return (img / levels).astype(np.float32)


Case = collections.namedtuple("Case", "W H P n_oct blur thresh seed bounds collapse")
# The seeds: 7 for `two` as measured in the issue; for `three` and `narrow` seed 7 leaves one side of an octave-2 border
# empty -- 1 and 2 are the first seeds (searched upwards from 1 on the CPU oracle) at which the premise test below holds.
CASES = {
    # borders at 197, 98 and 49, all from an odd b_1; ragged width crossing a 240-column strip; octaves 3 and 4 collapse
    "two": Case(481, 394, 2, 5, 1.0, 0.5, 7, [0, 197, 394], 3),
    # uneven strips of 197/198/198 rows, two borders per octave, identity taps
    "three": Case(256, 593, 3, 5, 0.0, 0.5, 1, [0, 197, 395, 593], 3),
    # one detection strip, w % 4 == 0 but w/2 = 122 and w/4 = 61 ragged, general taps
    "narrow": Case(244, 394, 2, 4, 0.5, 1.0, 2, [0, 197, 394], 3),
}
THREE_B = 2           # the other image of the reuse test (the premise holds on it as well)
SMALL_HALO = 24       # the smallest multiple of 8 the footprint test admits (16 < reach + margin = 19.7 <= 24)
SMALL_HALO_COLLAPSE = 4  # `two` at halo 24: octave 3 (24 and 25 owned rows) is tiled as well, octave 4 (12 rows) collapses
HALOS = {"two": (HALO, SMALL_HALO), "three": (HALO,), "narrow": (HALO,)}  # every halo the GPU tests use
# the option sets of test_options_reach_the_band_kernels (case `two`)
OPTIONS = {
    "root_sift": dict(root_sift=1),
    "tex_frac_bits 0": dict(tex_frac_bits=0),
    "lowest_scale 2": dict(lowest_scale=2.0),   # octave 0 is skipped: the first band is octave 1
    "lowest_scale 8": dict(lowest_scale=8.0),   # no tiled octave is searched: only the root's collapsed octaves
    "subsampling 0.5": dict(subsampling=0.5),
}
# every (case, seed, options) whose whole-image result a tiled run below is compared to
ANCHORS = [("two", None, "default")] + [("two", None, o) for o in OPTIONS] + \
          [("three", None, "default"), ("three", THREE_B, "default"), ("narrow", None, "default")]

_images = {}


def image(name, seed=None):
    c = CASES[name]
    key = (name, c.seed if seed is None else seed)
    if key not in _images:
        img = pyramid_noise(key[1], c.W, c.H)
        img.setflags(write=False)
        _images[key] = img
    return _images[key]


def extract_kw(name, options="default", max_pts=MAX_PTS):
    c = CASES[name]
    kw = dict(num_octaves=c.n_oct, init_blur=c.blur, peak_thresh=c.thresh, max_pts=max_pts)
    kw.update(OPTIONS.get(options, {}))
    return kw


_oracle_records = {}


def oracle_records(oracle, name, seed=None, options="default"):
    """The CPU oracle's records, once per (case, seed, option set), read-only."""
    key = (name, CASES[name].seed if seed is None else seed, options)
    if key not in _oracle_records:
        kw = extract_kw(name, options)
        rooted = kw.pop("root_sift", 0)
        pts = oracle.extract(image(name, seed), **kw).copy()
        if rooted:
            oracle.rootsift(pts, len(pts))
        pts.setflags(write=False)
        _oracle_records[key] = pts
    return _oracle_records[key]


def octave_of(pts, sub0=1.0):
    return np.round(np.log2(pts["subsampling"] / sub0)).astype(int)


# ------------------------------------------------------------------------------------------------------------------
# without a GPU: the plans and the premise, from the oracle alone
# ------------------------------------------------------------------------------------------------------------------
def test_the_plans_are_the_ones_the_cases_are_built_for():
    for name, c in CASES.items():
        pl = StripPlan(c.W, c.H, c.P, c.n_oct)
        assert pl.bounds == c.bounds and pl.collapse == c.collapse and pl.n_oct == c.n_oct, name
        assert any(b & 1 for b in pl.bounds[1:-1]), name  # an odd border: b_k >> o rounds
    pl = StripPlan(*CASES["two"][:4], halo=SMALL_HALO)
    assert pl.bounds == [0, 197, 394] and pl.collapse == SMALL_HALO_COLLAPSE
    assert [pl.own(0, o)[1] for o in range(4)] == [197, 98, 49, 24] and pl.own(1, 3) == (24, 49)
    assert pl.band(0, 0) == (0, 197 + 24) and pl.band(1, 3) == (0, 49)
    # `three`: uneven strips, both borders of octave 1 and 2 come from odd base rows
    pl = StripPlan(*CASES["three"][:4])
    assert [pl.own(k, 0)[1] - pl.own(k, 0)[0] for k in range(3)] == [197, 198, 198]
    assert [pl.own(1, o) for o in range(3)] == [(197, 395), (98, 197), (49, 98)]


def border_table(pts, pl):
    """Per tiled octave and interior border: keypoints with y / subsampling in [border - 1.5, border) and in
    [border, border + 1.5); per tiled octave and rank the keypoints inside the owned rows; per collapsed octave the count."""
    octv = octave_of(pts)
    rows, owned, collapsed = [], [], []
    for o in range(pl.n_oct):
        y = pts["coords2D"][octv == o, 1] / np.float32(2.0 ** o)
        if o >= pl.collapse:
            collapsed.append((o, len(y)))
            continue
        for k in range(1, pl.world):
            b = pl.bounds[k] >> o
            rows.append((o, b, int(((y >= b - 1.5) & (y < b)).sum()), int(((y >= b) & (y < b + 1.5)).sum())))
        for k in range(pl.world):
            a, b = pl.own(k, o)
            owned.append((o, k, int(((y >= a) & (y < b)).sum())))
    return rows, owned, collapsed


@pytest.mark.parametrize("name,seed,halo", [("two", None, HALO), ("two", None, SMALL_HALO), ("three", None, HALO),
                                            ("three", THREE_B, HALO), ("narrow", None, HALO)])
def test_every_border_of_every_tiled_octave_has_keypoints_on_both_sides(oracle, name, seed, halo):
    """A condition on the inputs, not on the code: if it fails, the seed is wrong."""
    c = CASES[name]
    pts = oracle_records(oracle, name, seed)
    pl = StripPlan(c.W, c.H, c.P, c.n_oct, halo)
    rows, owned, collapsed = border_table(pts, pl)
    per_octave = np.bincount(octave_of(pts), minlength=pl.n_oct)
    print("\n%s seed %s halo %d: %d keypoints, per octave %s" % (name, c.seed if seed is None else seed, halo, len(pts),
                                                               " / ".join(str(n) for n in per_octave)))
    for o, b, above, below in rows:
        print("  octave %d, row %d: %d above, %d below" % (o, b, above, below))
    for o, k, n in owned:
        print("  octave %d, rank %d owns %d" % (o, k, n))
    print("  collapsed: %s" % ", ".join("octave %d: %d" % x for x in collapsed))
    assert len(rows) == (c.P - 1) * pl.collapse and pl.collapse >= 3
    assert all(above >= 1 and below >= 1 for _, _, above, below in rows), rows
    assert all(n > 0 for _, _, n in owned), owned
    assert collapsed and all(n >= 1 for _, n in collapsed), collapsed
    assert len(pts) < MAX_PTS
    if name == "two" and halo == HALO:  # as measured when the case was chosen
        assert len(pts) == 44609 and list(per_octave) == [43788, 538, 220, 54, 9]
        assert rows == [(0, 197, 161, 155), (1, 98, 5, 2), (2, 49, 5, 3)]


@pytest.mark.parametrize("name,seed", [("two", None), ("three", None), ("three", THREE_B), ("narrow", None)])
def test_footprints_stay_inside_the_halo_by_the_restated_reach(oracle, name, seed):
    """The flag condition of descriptors_kernel and describe_bands_kernel, band_footprint_cut() of sift_keypoints.hip:

        r = fmaxf(7.5f * (12.0f / 16.0f * kscale) * (|sin| + |cos|), 6.0f) + 2.5f
        cut = (row0 > 0 && !(py - r >= row0)) || (row0 + h < hg && !(py + r <= row0 + h - 1))

    with row0 = own_begin - halo and row0 + h = own_end + halo.  reach_of(kscale) is the same grid term at |sin| + |cos|
    = sqrt 2 plus 1.01, so r <= max(reach_of, 6) + 2.5.  A keypoint of an owned row iy in [own_begin, own_end) has
    py = iy + pdy with |pdy| <= 0.5 (the refinement's accepted range), so nothing is flagged while
    max(reach_of, 6) + 2.5 (the margin of the flag) + 1 (the band's last row is row0 + h - 1) + 0.5 (pdy) <= halo.
    This over-covers by reach_of's own 1.01; a keypoint placed by the refinement's fallback (pdy = dy / dyy, unbounded)
    has (halo - bound) rows to spare, printed below."""
    pts = oracle_records(oracle, name, seed)
    kscale = (pts["scale"] / pts["subsampling"]).astype(np.float32)
    reach = max(float(np.float32(reach_of(kscale.max()))), 6.0)
    bound = reach + 2.5 + 1.0 + 0.5
    print("\n%s: largest scale / subsampling %.4f, reach %.3f, reach + margin %.3f" % (name, kscale.max(), reach, bound))
    for halo in HALOS[name]:
        print("  halo %d: %.3f rows to spare" % (halo, halo - bound))
        assert bound <= halo, (name, halo, bound)
    if name == "two":
        assert SMALL_HALO == min(HALOS[name]) and SMALL_HALO % 8 == 0 and bound > SMALL_HALO - 8  # the smallest such


# ------------------------------------------------------------------------------------------------------------------
# on the GPU
# ------------------------------------------------------------------------------------------------------------------
DEV = torch.device("cuda", 0)
_whole = {}


@pytest.fixture(scope="module")
def whole(ctx):
    """whole(name, seed, options) -> the whole-image extraction's records, once per module, read-only."""
    def get(name, seed=None, options="default"):
        key = (name, CASES[name].seed if seed is None else seed, options)
        if key not in _whole:
            pts = whole_image(ctx, image(name, seed), capi.default_params(**extract_kw(name, options))).copy()
            pts.setflags(write=False)
            _whole[key] = pts
        return _whole[key]

    yield get
    _whole.clear()
    _runs.clear()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_bits(got, want, label):
    """Every field extraction writes, bit for bit (NaN in the same places), as sets."""
    assert len(got) == len(want), (label, len(got), len(want))
    a, b = canonical_order(got), canonical_order(want)
    for f in FIELDS:
        np.testing.assert_array_equal(bits(a[f]), bits(b[f]), err_msg="%s: %s" % (label, f))


def record_keys(pts):
    return [b"".join(np.ascontiguousarray(r[f]).tobytes() for f in FIELDS) for r in pts]


@contextlib.contextmanager
def extractors(name, route, prm, halo=HALO, strict=True):
    """The P virtual ranks of a case.  bands: the constructor's own contexts (default policy); per-octave: a context of
    the caller's per rank, CUSIFT_POLICY_TILED_PER_OCTAVE set before capi.Tiled reads it."""
    c = CASES[name]
    ctxs, exts = [], []
    try:
        with torch.cuda.device(DEV):
            for k in range(c.P):
                if route == "per-octave":
                    own = capi.Context(DEV.index, stream=torch.cuda.current_stream().cuda_stream)
                    ctxs.append(own)
                    own.set_policy(capi.POLICY_TILED_PER_OCTAVE, 1)
                    e = StripExtractor(k, c.P, c.W, c.H, prm, device=DEV, halo=halo, strict=strict, ctx=own)
                    assert e.ctx is own and not e.owns_ctx
                else:
                    e = StripExtractor(k, c.P, c.W, c.H, prm, device=DEV, halo=halo, strict=strict)
                    assert e.owns_ctx
                exts.append(e)
                assert e.ctx.get_policy(capi.POLICY_TILED_PER_OCTAVE) == (1 if route == "per-octave" else 0)
        yield exts
    finally:
        for e in exts:
            e.close()
        for own in ctxs:  # close() left the caller's context alone
            assert own.get_policy(capi.POLICY_TILED_PER_OCTAVE) == 1
            own.close()


def strips_of(exts, img):
    full = torch.from_numpy(np.array(img)).to(DEV)  # (a copy: the cached image is read-only)
    b = exts[0].plan.bounds
    return [full[b[k]:b[k + 1]] for k in range(len(exts))]


def run_once(exts, img):
    """run_virtual, then per rank (records, raw counter, flagged)."""
    parts = run_virtual(exts, strips_of(exts, img))
    return [p.copy() for p in parts], [int(e.counts.item()) for e in exts], [e.check() for e in exts]


Run = collections.namedtuple("Run", "parts counters flagged")
_runs = {}


def tiled_run(name, route, options="default", halo=HALO, collapse=None):
    """One tiled run per (case, route, option set, halo), shared by the tests that compare against it."""
    key = (name, route, options, halo)
    if key not in _runs:
        prm = capi.default_params(**extract_kw(name, options))
        with extractors(name, route, prm, halo) as exts:
            for e in exts:
                assert e.tiled.collapse == e.plan.collapse == (CASES[name].collapse if collapse is None else collapse)
            _runs[key] = Run(*run_once(exts, image(name)))
    return _runs[key]


def assert_ownership_and_order(parts, pl, sub0=1.0):
    """The ownership and ordering assertions of test_strips_equal_whole_image."""
    for k, pts in enumerate(parts):
        tiled = pts[pts["subsampling"] < sub0 * 2 ** pl.collapse]
        if len(tiled):
            yb, slack = tiled["coords2D"][:, 1] / sub0, 0.51 * tiled["subsampling"].max() / sub0
            assert yb.min() >= pl.bounds[k] - slack - tiled["subsampling"].max() / sub0, k
            assert yb.max() < pl.bounds[k + 1] + slack, k
        if k != pl.root:
            assert len(tiled) == len(pts), k
        assert np.all(np.diff(pts["subsampling"]) <= 0), k  # coarsest octave first inside each rank's list


def assert_tiled_equals_whole(name, run, want, label, halo=HALO, sub0=1.0):
    c = CASES[name]
    pl = StripPlan(c.W, c.H, c.P, c.n_oct, halo)
    assert run.flagged == [0] * c.P, (label, run.flagged)
    assert run.counters == [len(p) for p in run.parts], label
    assert_ownership_and_order(run.parts, pl, sub0)
    assert_same_bits(np.concatenate(run.parts), want, label)


@gpu
@pytest.mark.parametrize("name,seed,options", ANCHORS)
def test_whole_image_equals_the_oracle_on_these_images(oracle, whole, name, seed, options):
    """What the tiled results are compared to, anchored: same_set's bars, every keypoint."""
    want = oracle_records(oracle, name, seed, options)
    assert 0 < len(want) < MAX_PTS
    same_set(want, whole(name, seed, options), "%s, %s" % (name, options))


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_both_routes_equal_the_whole_image(whole, name):
    want = whole(name)
    runs = {route: tiled_run(name, route) for route in ROUTES}
    for route, run in runs.items():
        assert_tiled_equals_whole(name, run, want, "%s, %s" % (name, route))
        assert all(len(p) > 0 for p in run.parts)
    # the two routes give every rank the same set, field for field
    for k in range(CASES[name].P):
        assert runs["bands"].counters[k] == runs["per-octave"].counters[k]
        assert_same_bits(runs["per-octave"].parts[k], runs["bands"].parts[k], "%s, rank %d, route against route" % (name, k))


@gpu
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("options", sorted(OPTIONS))
def test_options_reach_the_band_kernels(whole, options, route):
    """Each option set against the whole image under the same parameters."""
    want = whole("two", None, options)
    sub0 = OPTIONS[options].get("subsampling", 1.0)
    run = tiled_run("two", route, options)
    label = "two, %s, %s" % (options, route)
    assert_tiled_equals_whole("two", run, want, label, sub0=sub0)
    got = np.concatenate(run.parts)
    plain = whole("two")
    if options == "root_sift":
        a, b = canonical_order(got), canonical_order(plain)
        assert len(a) == len(b)
        np.testing.assert_array_equal(bits(a["coords2D"]), bits(b["coords2D"]))
        fin = np.isfinite(b["data"]).all(axis=1)
        assert fin.mean() > 0.99 and not np.any(np.all(a["data"][fin] == b["data"][fin], axis=1))  # every descriptor differs
        # as test_rootsift_matches_oracle: sqrt(v / L1) has unit length
        np.testing.assert_allclose((a["data"][fin].astype(np.float64) ** 2).sum(axis=1), 1.0, atol=1e-5)
    elif options == "tex_frac_bits 0":
        assert len(got) == len(plain) and not np.array_equal(canonical_order(got)["data"], canonical_order(plain)["data"])
    elif options == "lowest_scale 2":
        assert len(got) == int((plain["subsampling"] >= 2.0).sum()) > 500
        assert not np.any(got["subsampling"] == 1.0) and got["subsampling"].min() == 2.0
        assert all(np.any(p["subsampling"] == 2.0) for p in run.parts)  # the first band is octave 1, on every rank
    elif options == "lowest_scale 8":
        assert run.counters[1:] == [0] * (CASES["two"].P - 1) and all(len(p) == 0 for p in run.parts[1:])
        assert_same_bits(run.parts[0], want, label + ", the root")
        assert len(want) == int((plain["subsampling"] >= 8.0).sum()) == 63 and want["subsampling"].min() == 8.0
    elif options == "subsampling 0.5":
        assert got["subsampling"].min() == 0.5 and got["subsampling"].max() == 8.0
        a, b = canonical_order(got), canonical_order(plain)
        assert len(a) == len(b)
        np.testing.assert_array_equal(a["coords2D"], b["coords2D"] * np.float32(0.5))  # coordinates and scales halve
        np.testing.assert_array_equal(a["scale"], b["scale"] * np.float32(0.5))


@gpu
@pytest.mark.parametrize("route", ROUTES)
def test_a_smaller_halo_changes_the_bands_not_the_result(whole, route):
    """`two` at the smallest halo test_footprints_stay_inside_the_halo_by_the_restated_reach admits: octave 3 is tiled
    as well (a border at row 24), only octave 4 collapses -- the records are the whole image's all the same."""
    run = tiled_run("two", route, halo=SMALL_HALO, collapse=SMALL_HALO_COLLAPSE)
    assert_tiled_equals_whole("two", run, whole("two"), "two, halo %d, %s" % (SMALL_HALO, route), halo=SMALL_HALO)
    # octave 3 moved from the root's whole-image run to the bands: rank 1 now reports its share of it
    wide = tiled_run("two", route)
    assert not np.any(wide.parts[1]["subsampling"] == 8.0) and np.any(run.parts[1]["subsampling"] == 8.0)
    assert run.parts[0]["subsampling"].max() == 16.0 and run.parts[1]["subsampling"].max() == 8.0


def drive(exts, strips, bufs, cnts):
    """run_virtual's sequence on ext.tiled, the records going to buffers of the caller's."""
    pl = exts[0].plan
    tiles = [e.tiled for e in exts]
    for e, s in zip(exts, strips):
        e.load_strip(s)
    for o in range(min(pl.collapse + 1, pl.n_oct)):
        if o > 0:
            for e in exts:
                e.tiled.build_octave(o)
        capi.tiled_exchange_virtual(tiles, o)
    for e, b, c in zip(exts, bufs, cnts):
        e.tiled.process(b.data_ptr(), c.data_ptr())


@gpu
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("max_pts", [16, 300, 1000])  # below the root's 63 collapsed / inside a coarse band / inside octave 0
def test_overflow_keeps_the_coarse_octaves_and_counts_on(oracle, max_pts, route):
    """join_counts_kernel's header: the running sums are clamped at max_pts, so the coarser segments survive whole, and
    the counter is the sum of what every detection counted (it keeps counting beyond max_pts).  The per-octave route
    appends in place; its first / counter pair keeps counting past max_pts as well."""
    c = CASES["two"]
    unclipped = tiled_run("two", route)
    prm = capi.default_params(**extract_kw("two", max_pts=max_pts))
    room = max_pts + 64
    with extractors("two", route, prm, strict=False) as exts:
        bufs, cnts = [], []
        for e in exts:
            with torch.cuda.stream(e.stream):
                bufs.append(torch.full((room * capi.SIFT_POINT_BYTES,), SENTINEL, dtype=torch.uint8, device=DEV))
                cnts.append(torch.zeros((1,), dtype=torch.int32, device=DEV))
        drive(exts, strips_of(exts, image("two")), bufs, cnts)
        torch.cuda.synchronize(DEV)
        raw = [int(x.item()) for x in cnts]
        recs = [b.cpu().numpy().view(SIFT_POINT_DTYPE).reshape(-1) for b in bufs]
    assert raw == unclipped.counters and sum(raw) == len(oracle_records(oracle, "two"))
    cut_octaves = []
    for k in range(c.P):
        full = unclipped.parts[k]
        assert raw[k] > max_pts  # every rank overflows at these sizes
        n = min(max_pts, raw[k])
        kept, rest = recs[k][:n], recs[k][n:]
        assert np.all(np.diff(kept["subsampling"]) <= 0), k
        # every kept record is a record of the rank's unclipped set, none twice
        keys, pool = record_keys(kept), set(record_keys(full))
        assert len(pool) == len(full) and len(set(keys)) == n and set(keys) <= pool, (k, len(set(keys)), n)
        # octaves coarser than the one the cut falls in are whole, the cut octave fills the list, nothing finer appears
        have = np.bincount(octave_of(full), minlength=c.n_oct)
        got = np.bincount(octave_of(kept), minlength=c.n_oct)
        before, cut = 0, None
        for o in range(c.n_oct - 1, -1, -1):
            if cut is not None:
                assert got[o] == 0, (k, o, got)
            elif before + have[o] > max_pts:
                cut = o
                assert got[o] == max_pts - before, (k, o, got, have)
            else:
                assert got[o] == have[o], (k, o, got, have)
            before += have[o]
        cut_octaves.append(cut)
        # nothing beyond the kept records is written: up to max_pts, and the 64 records behind
        assert len(rest) == room - n >= 64 and np.all(rest.view(np.uint8) == SENTINEL), k
    assert cut_octaves == {16: [3, 2], 300: [1, 1], 1000: [0, 0]}[max_pts], cut_octaves


@gpu
@pytest.mark.parametrize("route", ROUTES)
def test_an_extractor_is_reused_for_another_image(whole, route):
    """The bands' halo rows, d_small (flag and fstPts) and the arena layout survive from one image to the next."""
    want_a, want_b = whole("three"), whole("three", THREE_B)
    prm = capi.default_params(**extract_kw("three"))
    with extractors("three", route, prm) as exts:
        first = Run(*run_once(exts, image("three")))
        other = Run(*run_once(exts, image("three", THREE_B)))
        again = Run(*run_once(exts, image("three")))
    assert_tiled_equals_whole("three", first, want_a, "three, %s, image A" % route)
    assert_tiled_equals_whole("three", other, want_b, "three, %s, image B after A" % route)
    assert_tiled_equals_whole("three", again, want_a, "three, %s, image A after B" % route)
    assert again.counters == first.counters and other.counters != first.counters
    for k in range(CASES["three"].P):
        assert_same_bits(again.parts[k], first.parts[k], "three, %s, rank %d, A again" % (route, k))


@gpu
@pytest.mark.parametrize("route", ROUTES)
def test_distributed_form_with_odd_borders_and_the_per_octave_route(whole, route):
    """cusift_tiled_extract over a communicator (fake transport, one thread per rank) on `three`: each rank equals its
    virtual twin, the merged all-gatherv is the whole image's SiftData.  The policy is set on the context before the
    communicator is made; a communicator and ctx= together are refused."""
    from cusift_amd.dist import SiftGatherer
    from test_multirank_gpu import run_ranks

    c = CASES["three"]
    want = whole("three")
    virt = tiled_run("three", route)
    prm = capi.default_params(**extract_kw("three"))
    full = torch.from_numpy(np.array(image("three"))).to(DEV)
    torch.cuda.synchronize(DEV)
    region_cap = 8192
    per_octave = 1 if route == "per-octave" else 0

    def rank_fn(rank, make_comm):
        with torch.cuda.device(DEV):
            own = capi.Context(0)  # a context with a stream of its own
            if per_octave:
                own.set_policy(capi.POLICY_TILED_PER_OCTAVE, 1)
            comm = make_comm(own)
            with pytest.raises(ValueError, match="not both"):
                StripExtractor(rank, c.P, c.W, c.H, prm, device=DEV, comm=comm, ctx=own)
            ext = StripExtractor(rank, c.P, c.W, c.H, prm, device=DEV, comm=comm)
            assert ext.ctx.get_policy(capi.POLICY_TILED_PER_OCTAVE) == per_octave and ext.tiled.collapse == c.collapse
            pts, cnt = run_distributed(ext, full[c.bounds[rank]:c.bounds[rank + 1]])
            flagged = ext.check()
            mine = ext.result().copy()
            g = SiftGatherer(comm, 1, prm.max_pts, region_cap=region_cap, device=DEV)
            counts, gathered, totals = g.gather(pts, cnt)
            own.synchronize()
            merged = np.concatenate([x.cpu().numpy() for x in SiftGatherer.regions(gathered, totals)])
            ext.close()
            comm.close()
            own.close()
            return mine, merged.view(SIFT_POINT_DTYPE).reshape(-1), counts, flagged

    res = run_ranks(c.P, rank_fn)
    for k in range(c.P):
        assert res[k][3] == 0
        assert_same_bits(res[k][0], virt.parts[k], "three, %s: rank %d against its virtual twin" % (route, k))
    for k in range(c.P):
        assert_same_bits(res[k][1], want, "three, %s: rank %d's merged SiftData" % (route, k))
        np.testing.assert_array_equal(res[k][2][:, 0], [len(v) for v in virt.parts])
