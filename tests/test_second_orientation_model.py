"""The inputs of tests/test_second_orientation.py, pinned on the CPU.  The oracle's tap DIVIDES (maxval2 / maxval1 >
ratio) where the device MULTIPLIES (maxval2 > ratio * maxval1), so the two can decide a record differently only when its
ratio lies within rounding (about 2e-7) of the tested ratio.  On every input of the GPU tests no record lies within
1e-5 of either tested ratio -- asserted here, so that the GPU comparison has no tolerated record -- and the counts are
the ones the issue measured."""
import numpy as np
import pytest

import describe_model as dm
import second_orientation_model as som
from oracle_binding import SIFT_POINT_DTYPE


def figures(tap):
    return (len(tap), int(som.parents_of(tap, som.RATIO).sum()), int(som.parents_of(tap, som.RATIO_LOW).sum()),
            som.band_count(tap, som.RATIO), som.band_count(tap, som.RATIO_LOW))


@pytest.mark.parametrize("name", sorted(som.CASES))
def test_fixture_counts_and_empty_bands(oracle, gray1, name):
    kw, n_want, parents_want = som.CASES[name][2:]
    recs, tap, levels, sub = som.oracle_input(oracle, som.case_image(gray1, name), **kw)
    n, parents, parents_low, band, band_low = figures(tap)
    print("%s: %d keypoints, %d parents at %.1f (%d within 1e-5, %d within 1e-4), %d at %.1f (%d within 1e-5)"
          % (name, n, parents, som.RATIO, band, som.band_count(tap, som.RATIO, 1e-4), parents_low, som.RATIO_LOW, band_low))
    assert (n, parents) == (n_want, parents_want)
    assert band == 0 and band_low == 0
    assert parents_low > parents  # the second ratio gives another set
    assert not som.parents_of(tap, 1.0).any()  # ratio 1: maxval2 <= maxval1 always


# the oracle's figures for the other inputs of the GPU tests: (keypoints, parents at 0.8, parents at 0.5)
VARIANT_FIGURES = {"alone": (234, 32, 100), "root_sift": (234, 32, 100), "frac0": None, "sub2": (234, 32, 100), "upsample": None}


@pytest.mark.parametrize("variant", sorted(som.VARIANTS))
def test_crop_variants_have_empty_bands(oracle, gray1, variant):
    kw = dict(som.CASES[som.CROP][2], **som.VARIANTS[variant])
    recs, tap, levels, sub = som.oracle_input(oracle, som.case_image(gray1, som.CROP), **kw)
    n, parents, parents_low, band, band_low = figures(tap)
    print("%s: %d keypoints, %d / %d parents, bands %d / %d" % (variant, n, parents, parents_low, band, band_low))
    assert band == 0 and band_low == 0 and 0 < parents < parents_low < n
    if VARIANT_FIGURES[variant]:
        assert (n, parents, parents_low) == VARIANT_FIGURES[variant]
    if variant == "upsample":  # the enlarged octave is one more octave of the table, and it holds parents
        assert sub[0] == 0.5 and (recs["subsampling"][som.parents_of(tap, som.RATIO)] == 0.5).any()
    if variant == "sub2":
        assert sub[0] == 2.0


def test_batch_crop_and_constant_image(oracle, gray1):
    recs, tap, _, _ = som.oracle_input(oracle, som.other_crop(gray1), **som.CASES[som.CROP][2])
    n, parents, parents_low, band, band_low = figures(tap)
    print("other crop: %d keypoints, %d / %d parents" % (n, parents, parents_low))
    assert band == 0 and band_low == 0 and 0 < parents < n
    assert not np.array_equal(som.other_crop(gray1), som.case_image(gray1, som.CROP))
    flat = np.full((150, 200), 93.0, dtype=np.float32)
    assert len(oracle.extract(flat, **som.CASES[som.CROP][2])) == 0


def test_grid_keypoints_have_empty_bands(oracle, gray1):
    img = som.case_image(gray1, som.CROP)
    recs = som.grid_records(SIFT_POINT_DTYPE)
    levels = dm.oracle_pyramid(oracle, img, 4)
    sub = dm.octave_subsamplings(4, 1.0, 0, 200, 150)
    tap = som.oracle_tap(oracle, levels, sub, recs)
    ok = dm.valid(recs["coords2D"][:, 0], recs["coords2D"][:, 1], recs["scale"])
    octv = dm.octave_of(recs["scale"], recs["subsampling"], sub)
    assert (~ok).sum() == 1 and np.isnan(tap[~ok]).all()
    assert set(octv[ok].tolist()) == {0, 1, 2}, np.bincount(octv[ok])
    n, parents, parents_low, band, band_low = figures(tap)
    print("grid: %d records, %d / %d parents, bands %d / %d" % (n, parents, parents_low, band, band_low))
    assert band == 0 and band_low == 0 and 0 < parents < parents_low


def test_model_places_and_clamps(oracle, gray1):
    """Order and clamp of expected_records on the smallest case: duplicates in ascending parent index behind the
    records, cut at max_pts; a duplicate differs from its parent in orientation and data only."""
    kw = som.CASES["crop-128x96"][2]
    recs, tap, levels, sub = som.oracle_input(oracle, som.case_image(gray1, "crop-128x96"), **kw)
    full, par = som.expected_records(oracle, recs, tap, som.RATIO, 32768, levels, sub)
    assert len(full) == 9 and list(par) == sorted(par) and len(par) == 2
    assert full[:7].tobytes() == recs.tobytes()
    for k, p in enumerate(par):
        d, r = full[7 + k].copy(), recs[p].copy()
        assert d["orientation"] == tap[p, 1] and d["orientation"] != r["orientation"]
        assert 0.5 < np.linalg.norm(d["data"]) < 1.5 and not np.array_equal(d["data"], r["data"])
        d["orientation"], d["data"] = r["orientation"], r["data"]
        assert d.tobytes() == r.tobytes()
    cut, par_cut = som.expected_records(oracle, recs, tap, som.RATIO, 8, levels, sub)
    assert len(cut) == 8 and list(par_cut) == list(par[:1]) and cut.tobytes() == full[:8].tobytes()
    none, par_none = som.expected_records(oracle, recs, tap, 1.0, 32768, levels, sub)
    assert len(par_none) == 0 and none.tobytes() == recs.tobytes()
