"""The staging routes of the orientation and descriptor stages (cusift_amd/csrc/sift_keypoints.hip), pinned on
hand-placed keypoints.

Detection never emits a keypoint outside the image or at a chosen distance from one of the switches below, so the
stage entry points are the only way to put one there:

  stage_patch       interior route (six patch rows per instruction, no clamp) / border route (a row per instruction,
                    clamped per column and row);
  patch_for_reach   LDS patch / global sampler (reach >= 20, pw or ph > 40, |p| >= 1e5);
  orientations_kernel  its own 16-float-stride patch, always the border route, global at |k| >= 1e5.

`route()` restates those expressions in float32, operation for operation; `case_table()` places keypoints on both
sides of every switch; the CPU tests assert the table's coverage from the restatement alone and that the oracle is
finite wherever a footprint is not flat.  The GPU tests hold the kernels to the project's own bars on the table:
orientations bit for bit, descriptors within 1e-4 L2 with NaN in the same places.
"""
import numpy as np
import pytest

from cusift_amd import capi
from cusift_amd.capi import SIFT_POINT_DTYPE, DeviceBuffer

F = np.float32
K_DESC_PATCH = 40
SENTINEL = 0x5A
INPUT_FIELDS = ("coords2D", "scale", "orientation")
DESC_WRITES = ("coords2D", "scale", "data")
OTHER_FIELDS = tuple(f for f in SIFT_POINT_DTYPE.names if f not in ("coords2D", "scale", "orientation", "data"))


# ------------------------------------------------------------------------------------------------
# The kernels' expressions, restated (float32 scalars: every operation rounds as the device's does)
# ------------------------------------------------------------------------------------------------
def reach_of(scale):
    """descriptors_kernel: 7.5f * (12.0f / 16.0f * kscale) * 1.41422f + 1.0f + 0.01f"""
    return F(7.5) * (F(12.0) / F(16.0) * F(scale)) * F(1.41422) + F(1.0) + F(0.01)


def patch_for_reach(px, py, reach):
    """-> (fits, x0, y0, pw, ph), as the device function of that name"""
    px, py, reach = F(px), F(py), F(reach)
    x0 = int(np.floor(px - reach - F(0.5))) - 1
    y0 = int(np.floor(py - reach - F(0.5))) - 1
    pw = int(np.floor(px + reach - F(0.5))) + 2 - x0 + 1
    ph = int(np.floor(py + reach - F(0.5))) + 2 - y0 + 1
    fits = bool(reach < F(0.5) * F(K_DESC_PATCH) and abs(px) < F(1e5) and abs(py) < F(1e5) and pw <= K_DESC_PATCH
                and ph <= K_DESC_PATCH)
    return fits, x0, y0, pw, ph


def crossed_sides(x0, y0, pw, ph, w, hg):
    """Which borders of the (whole) image a patch [x0, x0 + pw) x [y0, y0 + ph) crosses."""
    s = set()
    if x0 < 0:
        s.add("left")
    if x0 + pw > w:
        s.add("right")
    if y0 < 0:
        s.add("top")
    if y0 + ph > hg:
        s.add("bottom")
    return frozenset(s)


def route(px, py, scale, w, h, row0=0, hg=None, reach_shift=0.0):
    """The descriptor stage's route of a keypoint on a w x h image (rows [row0, row0 + h) of an image of hg rows):
    ('interior' | 'border' | 'global-scale' | 'global-far', sides, geometry).  `sides` names the image borders the
    patch crosses (plus 'pad' where only the interior route's columns rounded up to four leave the image, and 'band'
    where only the band's own first or last row is crossed); `reach_shift` moves reach, for the stability check."""
    hg = h if hg is None else hg
    reach = F(reach_of(scale) + F(reach_shift))
    fits, x0, y0, pw, ph = patch_for_reach(px, py, reach)
    geom = dict(x0=x0, y0=y0, pw=pw, ph=ph, gx=(pw + 3) & ~3, reach=float(reach))
    if not (abs(F(px)) < F(1e5) and abs(F(py)) < F(1e5)):
        return "global-far", frozenset(), geom
    if not fits:
        return "global-scale", frozenset(), geom
    gx = geom["gx"]
    lo_row = max(row0, 0)
    hi_row = min(row0 + h, hg) - 1
    interior = x0 >= 0 and x0 + gx <= w and y0 >= lo_row and y0 + ph - 1 <= hi_row  # (g.stride == kDescPatch: always)
    if interior:
        return "interior", frozenset(), geom
    sides = set(crossed_sides(x0, y0, pw, ph, w, hg))
    if not sides and x0 + gx > w:
        sides.add("pad")
    if not sides:
        sides.add("band")
    return "border", frozenset(sides), geom


def ori_route(kx, ky, w, h):
    """The orientation stage: PatchGeom{floor(kx - 6.5) - 1, floor(ky - 6.5) - 1, 16}, 16 x 16, never the interior
    route (its stride is not kDescPatch); the global sampler at |k| >= 1e5."""
    kx, ky = F(kx), F(ky)
    if not (abs(kx) < F(1e5) and abs(ky) < F(1e5)):
        return "global-far", frozenset(), None
    x0 = int(np.floor(kx - F(6.5))) - 1
    y0 = int(np.floor(ky - F(6.5))) - 1
    return "border", crossed_sides(x0, y0, 16, 16, w, h), dict(x0=x0, y0=y0, pw=16, ph=16)


def stable(px, py, scale, w, h):
    """The classification holds when reach moves by +-1e-3 (the geometry's integers too)."""
    r = [route(px, py, scale, w, h, reach_shift=d) for d in (-1e-3, 0.0, 1e-3)]
    key = [(a, s, g["x0"], g["y0"], g["pw"], g["ph"]) for a, s, g in r]
    far = r[1][0] == "global-far"
    return far or (key[0] == key[1] == key[2] and (r[0][2]["reach"] < 20.0) == (r[2][2]["reach"] < 20.0))


def scale_for_reach(reach):
    return (reach - 1.01) / (7.5 * 0.75 * 1.41422)


# ------------------------------------------------------------------------------------------------
# Images and the case table
# ------------------------------------------------------------------------------------------------
def random_field(w, h, seed):
    """Fixed-seed random field, lightly smoothed (1 2 1 both ways), kept on multiples of 1/16 in [0, 256): any footprint
    that touches two distinct pixels is non-flat, and a footprint of ONE pixel is exactly flat -- the bilinear weights
    are multiples of 2^-8 that sum to one and their products with a 12-bit pixel are exact."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.0, 255.0, (h + 2, w + 2))
    a = (a[:-2] + 2 * a[1:-1] + a[2:]) / 4
    a = (a[:, :-2] + 2 * a[:, 1:-1] + a[:, 2:]) / 4
    return (np.round(a * 16) / 16).astype(np.float32)


def saw_tooth(w, h):
    """test_descriptor_quirk_paths' image: identical rows of falling and rising ramps.  At orientation 0 dy == +0 exactly
    and dx < 0 on the falling ramps: atan2f == +pi, the angle index 8 that spills into the next cell's bin 0."""
    x = np.arange(w, dtype=np.float32)
    row = np.where((x // 16) % 2 == 0, 200 - 8 * (x % 16), 72 + 8 * (x % 16))
    return np.tile(row, (h, 1)).astype(np.float32)


def with_pitch(img, pitch, pad_seed=99):
    """(h, pitch) copy; the columns beyond the width hold large finite numbers no tap may read."""
    h, w = img.shape
    out = np.random.default_rng(pad_seed).uniform(1e6, 2e6, (h, pitch)).astype(np.float32)
    out[:, :w] = img
    return out


IMAGES = {  # name: (w, h, pitch, content)
    "A": (96, 80, 128, "field"), "B": (96, 80, 99, "field"), "C": (40, 40, 128, "field40"),
    "D": (13, 7, 128, "field13"), "E": (1, 1, 128, "one"), "S": (96, 80, 128, "saw"),
}
_image_cache = {}


def image(name):
    if name not in _image_cache:
        w, h, pitch, content = IMAGES[name]
        if content == "saw":
            img = saw_tooth(w, h)
        elif content == "one":
            img = np.full((1, 1), 77.0, dtype=np.float32)
        else:
            img = random_field(w, h, {"field": 11, "field40": 12, "field13": 13}[content])
        _image_cache[name] = with_pitch(img, pitch)
    return _image_cache[name]


_table_cache = []


def case_table():
    """Every hand-placed keypoint: dicts of image, group, px, py, scale, hand (the hand-set orientation), flat."""
    if _table_cache:
        return _table_cache[0]
    rng = np.random.default_rng(2024)
    cases = []

    def add(img, group, px, py, scale, hand=None, flat=False, settle=True):
        w, h = IMAGES[img][:2]
        px, py, scale = float(F(px)), float(F(py)), float(F(scale))
        for _ in range(40):  # nudge the scale until reach +- 1e-3 decides nothing
            if not settle or stable(px, py, scale, w, h):
                break
            scale = float(F(scale + 0.0037))
        assert stable(px, py, scale, w, h), (img, group, px, py, scale)
        if hand is None:
            hand = 0.0 if len(cases) % 3 == 0 else float(F(rng.uniform(0.0, 360.0)))
        cases.append(dict(img=img, group=group, px=px, py=py, scale=scale, hand=float(hand), flat=flat))

    def placed(img, group, x0, y0, pw, ph=None, **kw):
        """A keypoint whose patch is exactly [x0, x0 + pw) x [y0, y0 + ph): reach = (pw - 4) / 2 puts both ends of the
        patch in the middle of an integer cell (half a pixel from the next value, against the 1e-3 asked for);
        ph = pw + 1 moves the reach, px and py by fractions that keep 0.2 px on every side."""
        ph = pw if ph is None else ph
        assert ph in (pw, pw + 1)
        reach = (pw - 4) / 2.0 + (0.2 if ph == pw + 1 else 0.0)
        scale = scale_for_reach(reach)
        reach = float(reach_of(scale))
        px = x0 + 2.0 + reach - (0.2 if ph == pw + 1 else 0.0)
        py = y0 + 2.0 + reach + (0.3 if ph == pw + 1 else 0.0)
        add(img, group, px, py, scale, settle=False, **kw)
        w, h = IMAGES[img][:2]
        g = route(cases[-1]["px"], cases[-1]["py"], cases[-1]["scale"], w, h)[2]
        assert (g["x0"], g["y0"], g["pw"], g["ph"]) == (x0, y0, pw, ph), (g, x0, y0, pw, ph)

    for img in ("A",):
        w, h = IMAGES[img][:2]
        # the interior predicate with zero margin and one column / row past it, on all four sides
        for pw in (33, 34, 35, 36, 37, 38, 39, 40):  # pw % 4 takes all four values, gx = 36 and 40
            gx = (pw + 3) & ~3
            for x0 in (0, -1):
                placed(img, "switch-left", x0, 20, pw)
            for x0 in (w - gx, w - gx + 1):
                placed(img, "switch-right", x0, 20, pw)
            for y0 in (0, -1):
                placed(img, "switch-top", 28, y0, pw)
            for y0 in (h - pw, h - pw + 1):
                placed(img, "switch-bottom", 28, y0, pw)
        # ph over the six-row groups of the interior route: a last group of one row, of two rows, full, with ph != pw too
        for pw, ph in ((35, 36), (36, 36), (36, 37), (37, 37), (37, 38), (38, 38), (30, 30), (30, 31), (25, 25)):
            placed(img, "rows-of-six", 11, 9, pw, ph)
            placed(img, "rows-of-six", w - 40, h - ph, pw, ph)
        # corners and edges: on the border pixel, half a pixel outside, 3 px outside
        xs = {"l": (0.0, -0.5, -3.0), "m": (47.3, 47.3, 47.3), "r": (w - 1.0, w - 0.5, w + 2.0)}
        ys = {"t": (0.0, -0.5, -3.0), "m": (40.6, 40.6, 40.6), "b": (h - 1.0, h - 0.5, h + 2.0)}
        for cx in "lmr":
            for cy in "tmb":
                if cx == cy == "m":
                    continue
                for k in range(3):
                    for scale in (0.8, 1.7):
                        add(img, "edge-%s%s" % (cx, cy), xs[cx][k], ys[cy][k], scale)
        # far outside one edge: every tap clamps to a column (row) that varies along the edge
        for px, py in ((-45.0, 40.3), (w + 45.0, 40.3), (47.7, -45.0), (47.7, h + 45.0)):
            for scale in (0.9, 1.6):
                add(img, "far-edge", px, py, scale)
        # far outside a corner: every tap clamps to ONE pixel.  Positions and scales on multiples of 1/4 and hand-set
        # orientation 0, so that the exact (tex_frac_bits 0) weights sum to one as well: exactly flat either way.
        for px, py in ((-45.25, -45.5), (w + 45.25, -45.5), (-45.25, h + 45.5), (w + 45.25, h + 45.5)):
            for scale in (1.0, 2.0):
                add(img, "flat", px, py, scale, hand=0.0, flat=True)
        # the patch-fit switch: pw and ph cross 40 while reach < 20, at four fractional positions; then reach crosses 20
        for fx, fy in ((0.0, 0.0), (0.27, 0.71), (0.5, 0.5), (0.93, 0.12)):
            for scale in np.arange(1.9, 2.4001, 0.025):
                add(img, "patch-fit", 48.0 + fx, 40.0 + fy, scale)
        for scale in np.arange(2.35, 2.4501, 0.005):
            add(img, "reach-20", 48.4, 40.2, scale)
        # |p| = 2e5: the global sampler, in x, in y; in both every tap clamps to one pixel (flat)
        for px, py in ((2e5, 40.25), (-2e5, 40.25), (47.75, 2e5), (47.75, -2e5)):
            for scale in (1.0, 3.0):
                add(img, "far-2e5", px, py, scale)
        for px, py in ((2e5, 2e5), (-2e5, -2e5), (2e5, -2e5)):
            for scale in (1.0, 2.0):
                add(img, "flat", px, py, scale, hand=0.0, flat=True)
        # scales from 0.8 to 9 at random positions in and around the image
        for scale in np.linspace(0.8, 9.0, 24):
            add(img, "scales", rng.uniform(-2.0, w + 2.0), rng.uniform(-2.0, h + 2.0), scale)
    cases += [dict(c, img="B") for c in cases]  # the odd pitch: the same keypoints on the same pixels
    # 40 x 40: pw == ph == 40 at x0 == y0 == 0 is the only interior position; its four neighbours
    for x0, y0 in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1)):
        placed("C", "one-position", x0, y0, 40)
    for x0, y0 in ((0, 0), (2, 3), (3, 2), (-1, 0), (0, -1), (4, 0), (0, 4)):  # gx == 36 leaves x0 = 0 .. 4 interior
        placed("C", "one-position", x0, y0, 36)
    # small images: every keypoint a border case
    for px, py in ((6.3, 3.4), (0.0, 0.0), (12.0, 6.0), (-0.5, 3.0), (6.0, -3.0), (15.0, 9.0), (12.5, 3.2), (3.1, 6.5)):
        for scale in (0.8, 1.5):
            add("D", "small-13x7", px, py, scale)
    for scale in (2.5, 5.0):
        add("D", "small-13x7", 6.4, 3.3, scale)
    for px, py in ((0.0, 0.0), (0.25, 0.5), (-0.5, 0.0), (3.0, -2.0), (-6.25, 7.5), (1.0, 1.0), (0.5, -30.0)):
        for scale in (1.0, 2.0):
            add("E", "flat", px, py, scale, hand=0.0, flat=True)
    add("E", "flat", 0.0, 0.0, 4.0, hand=0.0, flat=True)  # the global sampler on one pixel
    # the saw-tooth: orientation 0 on identical rows (the atan2f == +pi spill), scales into the global sampler
    w, h = IMAGES["S"][:2]
    for i in range(40):
        scale = rng.uniform(0.8, 2.2) if i < 28 else rng.uniform(2.6, 9.0)
        add("S", "saw", rng.uniform(-2.0, w + 2.0), rng.uniform(-2.0, h + 2.0), scale, hand=0.0)
    add("S", "saw", 0.0, 0.0, 1.2, hand=0.0)
    add("S", "saw", w - 1.0, h - 1.0, 1.2, hand=0.0)
    _table_cache.append(cases)
    return cases


def cases_of(img):
    return [c for c in case_table() if c["img"] == img]


def records_of(cases, orientation="hand", pad=0):
    """SiftPoint records of the cases (+ `pad` canaries), every byte the sentinel but the stage's inputs."""
    raw = np.full((len(cases) + pad) * 588, SENTINEL, dtype=np.uint8)
    pts = raw.view(SIFT_POINT_DTYPE)
    n = len(cases)
    pts["coords2D"][:n, 0] = [c["px"] for c in cases]
    pts["coords2D"][:n, 1] = [c["py"] for c in cases]
    pts["scale"][:n] = [c["scale"] for c in cases]
    if isinstance(orientation, str):
        assert orientation == "hand"
        pts["orientation"][:n] = [c["hand"] for c in cases]
    elif orientation is not None:
        pts["orientation"][:n] = orientation
    return pts


def classify(c):
    w, h = IMAGES[c["img"]][:2]
    return route(c["px"], c["py"], c["scale"], w, h)


def route_label(c):
    r, sides, _ = classify(c)
    return r if r != "border" else "border:" + "+".join(sorted(sides))


_oracle_cache = {}


def oracle_results(oracle, img, frac_bits):
    """(orientations, descriptors at those, descriptors at the hand-set ones) of an image's cases -- computed once."""
    key = (img, frac_bits)
    if key not in _oracle_cache:
        cases = cases_of(img)
        w, h = IMAGES[img][:2]
        src = image(img)
        n = len(cases)
        ori = records_of(cases, None)
        oracle.compute_orientations(src, w, h, ori, 0, n, frac_bits)
        d_ori = records_of(cases, ori["orientation"][:n])
        oracle.extract_descriptors(src, w, h, d_ori, 0, n, 1.0, frac_bits)
        d_hand = records_of(cases, "hand")
        oracle.extract_descriptors(src, w, h, d_hand, 0, n, 1.0, frac_bits)
        _oracle_cache[key] = (ori["orientation"][:n].copy(), d_ori["data"][:n].copy(), d_hand["data"][:n].copy())
    return _oracle_cache[key]


# ------------------------------------------------------------------------------------------------
# CPU: the table's coverage, from the restatement alone; the oracle's finiteness on it
# ------------------------------------------------------------------------------------------------
CORNERS = [frozenset(p) for p in (("left", "top"), ("right", "top"), ("left", "bottom"), ("right", "bottom"))]
SIDES = [frozenset((s,)) for s in ("left", "right", "top", "bottom")]


def test_route_restatement_on_known_geometry():
    """The restatement itself, on numbers worked out by hand."""
    assert float(reach_of(1.0)) == pytest.approx(7.5 * 0.75 * 1.41422 + 1.01, abs=1e-5)
    # px = 30, reach = 10: the patch starts at floor(19.5) - 1 = 18 and holds floor(39.5) + 3 - 18 = 24 columns
    assert patch_for_reach(30.0, 50.0, 10.0) == (True, 18, 38, 24, 24)
    assert patch_for_reach(30.0, 50.0, 20.0)[0] is False and patch_for_reach(1e5, 50.0, 10.0)[0] is False
    assert route(30.0, 50.0, scale_for_reach(10.0), 96, 80)[:2] == ("interior", frozenset())
    assert route(30.0, 50.0, scale_for_reach(10.0), 96, 60)[:2] == ("border", frozenset(("bottom",)))
    assert route(30.0, 26.0, scale_for_reach(10.0), 96, 32, row0=16, hg=80)[:2] == ("border", frozenset(("band",)))
    assert route(30.0, 34.0, scale_for_reach(10.0), 96, 32, row0=16, hg=80)[0] == "interior"
    assert route(30.0, 50.0, 9.0, 96, 80)[0] == "global-scale" and route(-2e5, 50.0, 1.0, 96, 80)[0] == "global-far"
    assert ori_route(10.25, 3.0, 96, 80) == ("border", frozenset(("top",)), dict(x0=2, y0=-5, pw=16, ph=16))
    assert ori_route(2e5, 3.0, 96, 80)[0] == "global-far"


def test_case_table_covers_every_route_and_switch():
    table = case_table()
    assert 300 <= len(table) <= 1200
    on_a = [classify(c) for c in cases_of("A")]
    # every route, and for `border` every side and every corner, at least four times on the aligned-pitch image
    for r in ("interior", "global-scale", "global-far"):
        assert sum(1 for x in on_a if x[0] == r) >= 4, r
    for s in SIDES + CORNERS:
        assert sum(1 for x in on_a if x[0] == "border" and x[1] == s) >= 4, sorted(s)
    ori_a = [ori_route(c["px"], c["py"], 96, 80) for c in cases_of("A")]
    assert sum(1 for x in ori_a if x[0] == "global-far") >= 4
    for s in [frozenset()] + SIDES + CORNERS:
        assert sum(1 for x in ori_a if x[0] == "border" and x[1] == s) >= 4, sorted(s)
    # the odd-pitch image carries the same cases
    assert [(c["px"], c["py"], c["scale"]) for c in cases_of("A")] == [(c["px"], c["py"], c["scale"]) for c in cases_of("B")]
    # both sides of every integer switch of the interior predicate, with every pw % 4
    g = [x[2] for x in on_a if x[0] in ("interior", "border")]
    w, h = 96, 80
    for m in range(4):
        gm = [q for q in g if q["pw"] % 4 == m]
        for want in (0, -1):
            assert any(q["x0"] == want for q in gm), (m, want)
        for want in (w, w + 1):
            assert any(q["x0"] + q["gx"] == want for q in gm), (m, want)
    assert any(q["gx"] != q["pw"] and q["x0"] + q["gx"] == w + 1 and q["x0"] + q["pw"] <= w for q in g)  # 'pad' alone
    for want in (0, -1):
        assert any(q["y0"] == want for q in g), want
    for want in (h - 1, h):
        assert any(q["y0"] + q["ph"] - 1 == want for q in g), want
    # ... each with the route the predicate gives it: zero margin is interior, one past it is not
    for c in cases_of("A"):
        if c["group"].startswith("switch-"):
            r, _, q = classify(c)
            zero = {"switch-left": q["x0"] == 0, "switch-right": q["x0"] + q["gx"] == w, "switch-top": q["y0"] == 0,
                    "switch-bottom": q["y0"] + q["ph"] == h}[c["group"]]
            assert r == ("interior" if zero else "border"), (c, q)
    # a last row group of one row, of two rows, and a full one, on the interior route
    ph_interior = {x[2]["ph"] for x in on_a if x[0] == "interior"}
    assert {36, 37, 38} <= ph_interior and any(x[2]["ph"] != x[2]["pw"] for x in on_a if x[0] == "interior")
    # the patch-fit switch: pw crosses 40 below reach 20, and reach crosses 20
    fit = [classify(c) for c in cases_of("A") if c["group"] == "patch-fit"]
    assert sum(1 for x in fit if x[0] == "interior" and x[2]["pw"] == 40) >= 2
    assert sum(1 for x in fit if x[0] == "global-scale" and x[2]["reach"] < 20 and max(x[2]["pw"], x[2]["ph"]) == 41) >= 2
    r20 = [classify(c)[2]["reach"] for c in cases_of("A") if c["group"] == "reach-20"]
    assert min(r20) < 20 - 1e-3 and max(r20) > 20 + 1e-3 and len(r20) >= 12
    # 40 x 40: the one interior position and its four neighbours
    one = {(q["x0"], q["y0"]): r for r, _, q in (classify(c) for c in cases_of("C")) if q["pw"] == 40}
    assert one == {(0, 0): "interior", (-1, 0): "border", (1, 0): "border", (0, -1): "border", (0, 1): "border"}
    # small images: every keypoint a border case (or the global sampler), six positions or more
    for img in ("D", "E"):
        cs = cases_of(img)
        assert len({(c["px"], c["py"]) for c in cs}) >= 6
        assert all(classify(c)[0] in ("border", "global-scale") for c in cs)
    # |p| = 2e5 in x, in y, in both; scales from 0.8 to 9
    far = [(abs(c["px"]) >= 1e5, abs(c["py"]) >= 1e5) for c in cases_of("A") if classify(c)[0] == "global-far"]
    assert {(True, False), (False, True), (True, True)} <= set(far)
    sc = [c["scale"] for c in cases_of("A")]
    assert min(sc) <= 0.8001 and max(sc) >= 8.999
    assert all(c["hand"] == 0.0 for c in cases_of("S"))


def test_oracle_is_nan_on_flat_footprints_and_finite_elsewhere(oracle):
    """What keeps a NaN from hiding a failure: only the `flat` group (every tap clamps to one pixel) may be NaN."""
    for img in IMAGES:
        flat = np.array([c["flat"] for c in cases_of(img)])
        for frac_bits in (8, 0):
            ori, d_ori, d_hand = oracle_results(oracle, img, frac_bits)
            assert np.isnan(ori[flat]).all() and np.isfinite(ori[~flat]).all(), (img, frac_bits)
            for d in (d_ori, d_hand):
                assert np.isnan(d[flat]).all() and np.isfinite(d[~flat]).all(), (img, frac_bits)
                norm = np.linalg.norm(d[~flat].astype(np.float64), axis=1)
                assert np.allclose(norm, 1.0, atol=1e-5)


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
def upload_image(ctx, img):
    return DeviceBuffer.from_numpy(ctx, image(img))


def counter(ctx, *values):
    return DeviceBuffer.from_numpy(ctx, np.array(values, dtype=np.uint32))


def assert_fields_bytes(got, want, fields, msg=""):
    for f in fields:
        a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        assert a.tobytes() == b.tobytes(), "%s field %s differs at rows %s" % (
            msg, f, np.flatnonzero((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1))[:8])


@pytest.mark.gpu
@pytest.mark.parametrize("frac_bits", [8, 0])
def test_orientations_on_the_table(ctx, oracle, frac_bits):
    """cusift_compute_orientations: bit for bit the oracle's, NaN included; every other byte of every record untouched."""
    for img, (w, h, pitch, _) in IMAGES.items():
        cases = cases_of(img)
        n = len(cases)
        want_ori = oracle_results(oracle, img, frac_bits)[0]
        pts = records_of(cases, None, pad=3)
        d_img, d_pts, d_cnt = upload_image(ctx, img), DeviceBuffer.from_numpy(ctx, pts), counter(ctx, n)
        ctx.compute_orientations(d_img.ptr, w, h, pitch, d_pts.ptr, len(pts), None, d_cnt.ptr, frac_bits)
        ctx.synchronize()
        got = d_pts.to_numpy(SIFT_POINT_DTYPE, (len(pts),))
        bad = np.flatnonzero(got["orientation"][:n].view(np.uint32) != want_ori.view(np.uint32))
        # (a NaN's payload is not pinned: NaN where the oracle has NaN)
        bad = [i for i in bad if not (np.isnan(want_ori[i]) and np.isnan(got["orientation"][i]))]
        assert not bad, (img, [(cases[i]["group"], route_label(cases[i]), cases[i]["px"], cases[i]["py"], cases[i]["scale"],
                                float(got["orientation"][i]), float(want_ori[i])) for i in bad[:6]])
        want = pts.copy()
        want["orientation"][:n] = got["orientation"][:n]
        assert got.tobytes() == want.tobytes(), img
        for b in (d_img, d_pts, d_cnt):
            b.free()


@pytest.mark.gpu
@pytest.mark.parametrize("sub", [0.5, 1.0, 4.0])
@pytest.mark.parametrize("frac_bits", [8, 0])
def test_descriptors_on_the_table(ctx, oracle, frac_bits, sub, record_property):
    """cusift_extract_descriptors at the oracle's orientations and at the hand-set ones: the oracle's finite mask, every
    finite descriptor within 1e-4 L2 (compare_sets' bar), coords2D and scale the oracle's products bit for bit."""
    worst = {}
    for img, (w, h, pitch, _) in IMAGES.items():
        cases = cases_of(img)
        n = len(cases)
        ori, want_ori, want_hand = oracle_results(oracle, img, frac_bits)
        d_img, d_cnt = upload_image(ctx, img), counter(ctx, n)
        for source, orientation, want_data in (("oracle", ori, want_ori), ("hand", "hand", want_hand)):
            pts = records_of(cases, orientation, pad=3)
            d_pts = DeviceBuffer.from_numpy(ctx, pts)
            ctx.extract_descriptors(d_img.ptr, w, h, pitch, d_pts.ptr, len(pts), None, d_cnt.ptr, sub, frac_bits)
            ctx.synchronize()
            got = d_pts.to_numpy(SIFT_POINT_DTYPE, (len(pts),))
            d_pts.free()
            want = pts.copy()
            want["coords2D"][:n] = pts["coords2D"][:n] * F(sub)  # float32 products, as the oracle's
            want["scale"][:n] = pts["scale"][:n] * F(sub)
            want["data"] = got["data"]
            assert got.tobytes() == want.tobytes(), (img, source)  # nothing but data was written beside them
            assert (got["data"][n:].view(np.uint8) == SENTINEL).all()
            fin = np.isfinite(want_data).all(axis=1)
            got_fin = np.isfinite(got["data"][:n]).all(axis=1)
            assert np.array_equal(got_fin, fin), (img, source, [(cases[i]["group"], route_label(cases[i])) for i in
                                                                np.flatnonzero(got_fin != fin)[:6]])
            assert np.isnan(got["data"][:n][~fin]).all()
            l2 = np.linalg.norm(want_data[fin].astype(np.float64) - got["data"][:n][fin].astype(np.float64), axis=1)
            for i, d in zip(np.flatnonzero(fin), l2):
                r = classify(cases[i])[0]
                worst[r] = max(worst.get(r, 0.0), float(d))
            over = np.flatnonzero(l2 >= 1e-4)
            assert len(over) == 0, (img, source, [(cases[np.flatnonzero(fin)[i]]["group"],
                                                   route_label(cases[np.flatnonzero(fin)[i]]), float(l2[i])) for i in over[:6]])
        for b in (d_img, d_cnt):
            b.free()
    for r, d in sorted(worst.items()):
        record_property("max_l2_" + r, d)
        print("max descriptor L2, tex_frac_bits %d, subsampling %g, %s: %.3e" % (frac_bits, sub, r, d))
    assert set(worst) == {"interior", "border", "global-scale", "global-far"}


def batch_cases(k):
    """24 cases of image A's table that take every route (every k-th of each route's, so the sets differ by image)."""
    by_route = {}
    for c in cases_of("A"):
        if not c["flat"]:
            by_route.setdefault(classify(c)[0], []).append(c)
    out = []
    for r in ("interior", "border", "global-scale", "global-far"):
        out += by_route[r][k::max(1, len(by_route[r]) // 6)][:6]
    assert len(out) == 24
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("ranges", [((3, 40), (5, 5), (0, 0)), ((0, 0), (2, 20), (7, 30)), ((24, 24), (0, 24), (23, 25))])
def test_batched_stages_equal_the_single_image_calls(ctx, ranges):
    """n_images = 3 with a stride beyond h * pitch and (first, count) per image -- first == count, count == 0,
    count > max_pts among them: records [first, min(count, max_pts)) are the single-image call's bit for bit, every
    other record and the canaries behind the block keep their bytes."""
    w, h, pitch = 96, 80, 128
    max_pts, n_img, canaries = 24, 3, 4
    stride = h * pitch + 256 + 3
    content = [image("A"), with_pitch(random_field(w, h, 21), pitch), with_pitch(random_field(w, h, 22), pitch)]
    stack = np.random.default_rng(5).uniform(1e6, 2e6, n_img * stride).astype(np.float32)
    for i in range(n_img):
        stack[i * stride: i * stride + h * pitch] = content[i].ravel()
    cases = [batch_cases(i) for i in range(n_img)]
    start = np.concatenate([records_of(cases[i], None) for i in range(n_img)] + [records_of([], None, pad=canaries)])
    # the single-image calls: orientation, then descriptor, of every record
    single_ori, single_desc = [], []
    for i in range(n_img):
        d_img = DeviceBuffer.from_numpy(ctx, content[i])
        d_pts = DeviceBuffer.from_numpy(ctx, start[i * max_pts:(i + 1) * max_pts])
        d_cnt = counter(ctx, max_pts)
        ctx.compute_orientations(d_img.ptr, w, h, pitch, d_pts.ptr, max_pts, None, d_cnt.ptr, 8)
        ctx.synchronize()
        single_ori.append(d_pts.to_numpy(SIFT_POINT_DTYPE, (max_pts,)).copy())
        ctx.extract_descriptors(d_img.ptr, w, h, pitch, d_pts.ptr, max_pts, None, d_cnt.ptr, 2.0, 8)
        ctx.synchronize()
        single_desc.append(d_pts.to_numpy(SIFT_POINT_DTYPE, (max_pts,)).copy())
        assert np.isfinite(single_desc[-1]["data"]).all() and np.isfinite(single_ori[-1]["orientation"]).all()
        for b in (d_img, d_pts, d_cnt):
            b.free()
    d_imgs = DeviceBuffer.from_numpy(ctx, stack)
    d_pts = DeviceBuffer.from_numpy(ctx, start)
    d_fst = counter(ctx, *[r[0] for r in ranges])
    d_cnt = counter(ctx, *[r[1] for r in ranges])
    want = start.copy()
    ctx.compute_orientations(d_imgs.ptr, w, h, pitch, d_pts.ptr, max_pts, d_fst.ptr, d_cnt.ptr, 8, n_images=n_img,
                             img_stride=stride)
    ctx.synchronize()
    for i, (first, count) in enumerate(ranges):
        last = min(count, max_pts)
        want[i * max_pts + first: i * max_pts + max(last, first)] = single_ori[i][first:max(last, first)]
    got = d_pts.to_numpy(SIFT_POINT_DTYPE, (len(start),))
    assert_fields_bytes(got, want, SIFT_POINT_DTYPE.names, "orientations:")
    ctx.extract_descriptors(d_imgs.ptr, w, h, pitch, d_pts.ptr, max_pts, d_fst.ptr, d_cnt.ptr, 2.0, 8, n_images=n_img,
                            img_stride=stride)
    ctx.synchronize()
    for i, (first, count) in enumerate(ranges):
        last = min(count, max_pts)
        want[i * max_pts + first: i * max_pts + max(last, first)] = single_desc[i][first:max(last, first)]
    got = d_pts.to_numpy(SIFT_POINT_DTYPE, (len(start),))
    assert_fields_bytes(got, want, SIFT_POINT_DTYPE.names, "descriptors:")
    assert (got[n_img * max_pts:].view(np.uint8) == SENTINEL).all()
    for b in (d_imgs, d_pts, d_fst, d_cnt):
        b.free()


# ---- cusift_describe_band ----
BANDS = ((0, 32), (24, 56), (48, 80))


def band_radius(oracle, scale, ori):
    """band_footprint_cut()'s radius (sift_keypoints.hip), restated: fmaxf(7.5 (12/16 scale) (|sin| + |cos|), 6) + 2.5 at
    theta = 2 * 3.1415 / 360 * orientation, with the kernels' own sincosf (sift_math.h, which the oracle compiles too)."""
    theta = (F(2.0) * F(3.1415) / F(360.0) * np.asarray(ori, dtype=np.float32)).astype(np.float32)
    sn, cs = oracle.math_eval("sincos", theta)
    s = (F(12.0) / F(16.0) * np.asarray(scale, dtype=np.float32)).astype(np.float32)
    r = (F(7.5) * s).astype(np.float32) * (np.abs(sn) + np.abs(cs)).astype(np.float32)
    return (np.maximum(r.astype(np.float32), F(6.0)) + F(2.5)).astype(np.float32)


def band_slack(py, r, row0, row1, h_global):
    """How far (px) a footprint of radius r at py stays inside the band [row0, row1) where the band does not end at the
    image border: negative = it leaves the band (the kernel counts it), zero = it ends exactly on the first / last row."""
    py = np.asarray(py, dtype=np.float64)
    top = (py - r) - row0 if row0 > 0 else np.full(len(py), 99.0)
    bot = (row1 - 1) - (py + r) if row1 < h_global else np.full(len(py), 99.0)
    return np.minimum(top, bot)


_band_cache = []


def band_keypoints(oracle):
    """Keypoints across the borders of the three bands of image A: a grid in y at a few x (outside the left and right
    borders too) and scales, and -- at scale 0.7, where the radius is 8.5 whatever the orientation -- keypoints whose
    footprint ends EXACTLY on a band's first or last row (inside: the kernel's tests are >= and <=).  Kept are the
    keypoints that are, in every band, 0.05 px or more on either side of the limit or exactly on it; the orientation that
    decides it is the oracle's, which the whole-image kernel equals bit for bit (asserted by the test)."""
    if _band_cache:
        return _band_cache[0]
    rng = np.random.default_rng(77)
    pts = []
    for py in np.arange(-2.0, 82.0, 0.93):
        pts.append((float(rng.choice([-1.5, 8.25, 47.6, 90.3, 97.0])), float(py), float(rng.choice([0.7, 0.9, 1.3, 1.6]))))
    for row in (24, 48):
        pts.append((30.5, row + 8.5, 0.7))   # py - r == row0
        pts.append((31.5, row + 8.75, 0.7))
    for row_last in (31, 55):
        pts.append((60.5, row_last - 8.5, 0.7))  # py + r == row0 + h - 1
        pts.append((61.5, row_last - 8.75, 0.7))
    cases = [dict(img="A", group="band", px=p[0], py=p[1], scale=p[2], hand=0.0, flat=False) for p in pts]
    w, h_global = IMAGES["A"][:2]
    out = {}
    for frac_bits in (8, 0):
        rec = records_of(cases, None)
        oracle.compute_orientations(image("A"), w, h_global, rec, 0, len(cases), frac_bits)
        r = band_radius(oracle, rec["scale"], rec["orientation"])
        ok = np.isfinite(rec["orientation"])
        for row0, row1 in BANDS:
            slack = band_slack(rec["coords2D"][:, 1], r, row0, row1, h_global)
            ok &= (slack <= -0.05) | (slack == 0.0) | (slack >= 0.05)
        out[frac_bits] = ok
    keep = out[8] & out[0]
    _band_cache.append([c for c, k in zip(cases, keep) if k])
    return _band_cache[0]


@pytest.mark.gpu
@pytest.mark.parametrize("frac_bits", [8, 0])
def test_describe_band_equals_the_whole_image_where_the_footprint_fits(ctx, oracle, frac_bits):
    """cusift_describe_band on three overlapping bands of image A.  A keypoint whose footprint -- the kernel's own formula,
    restated from the whole-image orientation -- stays inside the band wherever the band does not end at the image border
    gets the record of cusift_compute_orientations + cusift_extract_descriptors on the whole image, byte for byte;
    d_flags counts the others; root_sift = 1 is cusift_rootsift of the root_sift = 0 result, bit for bit."""
    w, h_global, pitch, _ = IMAGES["A"]
    cases = band_keypoints(oracle)
    n = len(cases)
    assert n >= 60
    src = image("A")
    d_img = DeviceBuffer.from_numpy(ctx, src)
    d_cnt = counter(ctx, n)
    start = records_of(cases, None, pad=2)
    d_pts = DeviceBuffer.from_numpy(ctx, start)
    ctx.compute_orientations(d_img.ptr, w, h_global, pitch, d_pts.ptr, len(start), None, d_cnt.ptr, frac_bits)
    ctx.extract_descriptors(d_img.ptr, w, h_global, pitch, d_pts.ptr, len(start), None, d_cnt.ptr, 2.0, frac_bits)
    ctx.synchronize()
    whole = d_pts.to_numpy(SIFT_POINT_DTYPE, (len(start),)).copy()
    d_pts.free()
    want_ori = records_of(cases, None)
    oracle.compute_orientations(src, w, h_global, want_ori, 0, n, frac_bits)
    assert whole["orientation"][:n].tobytes() == want_ori["orientation"].tobytes()
    assert np.isfinite(whole["data"][:n]).all()
    py = start["coords2D"][:n, 1]
    r = band_radius(oracle, start["scale"][:n], whole["orientation"][:n])
    exact = 0
    for row0, row1 in BANDS:
        hb = row1 - row0
        # the kernel's test, in its own float32 operations
        cut = ((row0 > 0) & ~((py - r).astype(np.float32) >= F(row0))) | \
              ((row1 < h_global) & ~((py + r).astype(np.float32) <= F(row0 + hb - 1)))
        slack = band_slack(py, r, row0, row1, h_global)
        assert ((slack <= -0.05) | (slack == 0.0) | (slack >= 0.05)).all() and np.array_equal(cut, slack < 0)
        exact += int((slack == 0.0).sum())
        assert 8 <= cut.sum() <= n - 8
        d_band = DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(src[row0:row1]))
        rooted = None
        for root in (0, 1):
            d_pts = DeviceBuffer.from_numpy(ctx, start)
            d_flags = counter(ctx, 0)
            ctx.describe_band(d_band.ptr, w, hb, pitch, row0, h_global, d_pts.ptr, len(start), None, d_cnt.ptr, 2.0,
                              frac_bits, d_flags.ptr, root)
            ctx.synchronize()
            got = d_pts.to_numpy(SIFT_POINT_DTYPE, (len(start),)).copy()
            flags = int(d_flags.to_numpy(np.uint32, (1,))[0])
            assert flags == int(cut.sum()), ((row0, row1), root, flags, int(cut.sum()))
            label = "band [%d,%d) root_sift %d:" % (row0, row1, root)
            keep = np.concatenate([~cut, np.ones(2, dtype=bool)])  # the canaries too
            if root == 0:
                assert_fields_bytes(got[keep], whole[keep], SIFT_POINT_DTYPE.names, label)
                ctx.rootsift(d_pts.ptr, n)
                ctx.synchronize()
                rooted = d_pts.to_numpy(SIFT_POINT_DTYPE, (len(start),)).copy()
                assert not np.array_equal(rooted["data"][:n], got["data"][:n])
            else:
                assert_fields_bytes(got[keep], rooted[keep], SIFT_POINT_DTYPE.names, label)
                for f in SIFT_POINT_DTYPE.names:  # the keypoints that are cut as well (a NaN's payload aside)
                    assert np.array_equal(got[f], rooted[f], equal_nan=(f in ("orientation", "data", "coords2D", "scale"))), (label, f)
            for f in OTHER_FIELDS:  # a keypoint that is cut still leaves every other field alone
                assert (np.ascontiguousarray(got[f]).view(np.uint8) == SENTINEL).all(), f
            d_pts.free()
            d_flags.free()
        d_band.free()
    assert exact >= 4  # both limits were hit exactly, in a band that has them
    for b in (d_img, d_cnt):
        b.free()
