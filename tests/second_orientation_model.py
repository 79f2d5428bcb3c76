"""Second-peak orientations restated from the CPU oracle (include/cusift_amd_extras.h pins the stage expression by
expression): which records get a duplicate, where it goes and what it holds.  The oracle's diagnostic tap gives, per
record, maxval2 / maxval1 and the orientation of the second peak; the duplicate's descriptor comes from the oracle's
descriptor stage at that orientation.  Shared by test_second_orientation_model.py (no GPU) and
test_second_orientation.py."""
import numpy as np

import describe_model as dm

# The inputs of the GPU tests: gray1.pgm whole and two crops of it, and the oracle's figures for them at ratio 0.8
# (test_second_orientation_model.py asserts them).  name: (rows, columns, oracle keywords, keypoints, parents at 0.8)
CASES = {
    "full-3.0": ((0, 480), (0, 640), dict(num_octaves=5, peak_thresh=3.0, max_pts=32768), 106, 20),
    "full-0.1": ((0, 480), (0, 640), dict(num_octaves=5, peak_thresh=0.1, max_pts=32768), 9501, 2687),
    "crop-200x150": ((50, 200), (300, 500), dict(num_octaves=4, peak_thresh=1.0, max_pts=32768), 234, 32),
    "crop-128x96": ((100, 196), (200, 328), dict(num_octaves=3, peak_thresh=1.0, max_pts=32768), 7, 2),
}
RATIO = 0.8      # the reference's constant
RATIO_LOW = 0.5  # the second tested ratio (its band is empty on every case: asserted)
BAND = 1e-5      # no record's oracle ratio lies this close to a tested ratio


def case_image(gray1, name):
    (y0, y1), (x0, x1) = CASES[name][:2]
    return np.ascontiguousarray(gray1[y0:y1, x0:x1])


def parents_of(tap, ratio):
    """The records that get a duplicate: the oracle's maxval2 / maxval1 above `ratio` in float32 (a NaN -- no first
    peak -- is not), and a second orientation that is a number."""
    tap = np.asarray(tap, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (tap[:, 0] > np.float32(ratio)) & ~np.isnan(tap[:, 1])


def band_count(tap, ratio, band=BAND):
    """Records whose oracle ratio lies within `band` of `ratio`: the oracle divides where the device multiplies, so
    only these could be decided differently."""
    r = np.asarray(tap, dtype=np.float32)[:, 0].astype(np.float64)
    return int((np.abs(r - float(np.float32(ratio))) <= band).sum())


def oracle_tap(oracle, levels, sub, recs, flags=0, tex_frac_bits=8):
    """The tap of the oracle's orientation stage run on `recs` (image units) per octave, as cusift_describe_batch
    assigns the octaves: [n, 2] float32 (ratio, second orientation), NaN rows for records that are skipped."""
    ok = dm.valid(recs["coords2D"][:, 0], recs["coords2D"][:, 1], recs["scale"])
    octv = dm.octave_of(recs["scale"], recs["subsampling"], sub, flags)
    tap = np.full((len(recs), 2), np.nan, dtype=np.float32)
    for o, (lvl, lw, lh) in enumerate(levels):
        idx = np.flatnonzero(ok & (octv == o))
        if not len(idx):
            continue
        work = recs[idx].copy()
        px, py, ks = dm.octave_units(work, np.full(len(idx), sub[o], dtype=np.float32))
        work["coords2D"][:, 0], work["coords2D"][:, 1], work["scale"] = px, py, ks
        diag = np.full((len(idx), 2), np.nan, dtype=np.float32)
        oracle.lib.oracle_set_orientation_diag(diag.ctypes.data, len(idx))
        try:
            oracle.compute_orientations(lvl, lw, lh, work, 0, len(work), tex_frac_bits)
        finally:
            oracle.lib.oracle_set_orientation_diag(None, 0)
        tap[idx] = diag
    return tap


def expected_records(oracle, recs, tap, ratio, max_pts, levels, sub, flags=0, tex_frac_bits=8, root_sift=0):
    """What the stage must leave for one image: `recs` (the image's records, image units, len(recs) <= max_pts), then
    the duplicates of the parents in ascending index, cut where max_pts ends.  A duplicate is its parent's record with
    orientation = the tap's second orientation, data = the oracle's descriptor stage on the parent's octave image at
    that orientation (+ rootsift) and subsampling = the octave's.  Returns (records, parent index per duplicate)."""
    n = len(recs)
    assert n <= max_pts and len(tap) == n
    par = np.flatnonzero(parents_of(tap, ratio))[: max_pts - n]
    dup = recs[par].copy()
    dup["orientation"] = tap[par, 1]
    octv = dm.octave_of(recs["scale"], recs["subsampling"], sub, flags)[par]
    for o, (lvl, lw, lh) in enumerate(levels):
        idx = np.flatnonzero(octv == o)
        if not len(idx):
            continue
        work = dup[idx].copy()
        px, py, ks = dm.octave_units(work, np.full(len(idx), sub[o], dtype=np.float32))
        work["coords2D"][:, 0], work["coords2D"][:, 1], work["scale"] = px, py, ks
        oracle.extract_descriptors(lvl, lw, lh, work, 0, len(work), float(sub[o]), tex_frac_bits)
        if root_sift:
            oracle.rootsift(work, len(work))
        dup["data"][idx] = work["data"]
        dup["subsampling"][idx] = sub[o]
    return np.concatenate([recs, dup]), par


# The settings the 200 x 150 crop is extracted with, and the second crop of the batch test
VARIANTS = {"alone": {}, "root_sift": dict(root_sift=1), "frac0": dict(tex_frac_bits=0), "sub2": dict(subsampling=2.0),
            "upsample": dict(upsample=1)}
CROP = "crop-200x150"
OTHER_CROP = ((250, 400), (100, 300))


def other_crop(gray1):
    (y0, y1), (x0, x1) = OTHER_CROP
    return np.ascontiguousarray(gray1[y0:y1, x0:x1])


def oracle_input(oracle, img, **kw):
    """The oracle's extraction of `img` with the tap, and what the model needs beside it: (records, tap, octave images,
    octave subsamplings).  kw: the oracle's keywords plus upsample (the extraction of the enlarged image with half the
    subsampling and twice the init_blur, as the drivers define octave -1) and root_sift (ignored here: the detection
    does not depend on it)."""
    kw = dict(kw)
    up = kw.pop("upsample", 0)
    kw.pop("root_sift", 0)
    okw = dict(kw)
    if up:
        okw["subsampling"] = float(np.float32(kw.get("subsampling", 1.0)) * np.float32(0.5))
        okw["init_blur"] = 2.0 * kw.get("init_blur", 0.0)
    recs, tap = oracle.extract_with_orientation_peaks(dm.up2(img) if up else img, **okw)
    h, w = img.shape
    levels = dm.oracle_pyramid(oracle, img, kw.get("num_octaves", 5), up)
    sub = dm.octave_subsamplings(kw.get("num_octaves", 5), kw.get("subsampling", 1.0), up, w, h)
    assert len(levels) == len(sub)
    return recs, tap.copy(), levels, sub


def grid_records(dtype, w=200, h=150):
    """Caller-supplied keypoints on the 200 x 150 crop: an 8-pixel grid at two scales (octaves 0 and 2), with one record
    whose coordinate is a NaN and one outside the image among them; everything but coords2D and scale a marker."""
    gx, gy = np.meshgrid(np.arange(4, w, 8, dtype=np.float32), np.arange(4, h, 8, dtype=np.float32))
    kp = np.concatenate([np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, s, np.float32)], 1) for s in (1.5, 4.5)])
    kp = np.insert(kp, 7, (np.nan, 20.0, 2.0), axis=0)
    kp = np.insert(kp, 501, (w + 9.5, -6.25, 3.0), axis=0)
    recs = np.zeros(len(kp), dtype=dtype)
    recs.view(np.uint8)[...] = 0x5A
    recs["coords2D"], recs["scale"] = kp[:, :2], kp[:, 2]
    recs["subsampling"] = 0
    return recs
