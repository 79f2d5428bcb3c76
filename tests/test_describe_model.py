"""The octave rule of cusift_describe_batch (include/cusift_amd_extras.h) on the CPU: applied to the scales of an
extraction it names the octave the detector recorded, for every record; the unit conversion round-trips; the
handcrafted edges."""
import numpy as np

import describe_model as dm

KW = dict(num_octaves=5, peak_thresh=1.0)


def test_rule_reproduces_the_recorded_octave_of_every_record(oracle, gray1):
    pts = oracle.extract(gray1, **KW)
    sub = dm.octave_subsamplings(5, 1.0, 0, 640, 480)
    np.testing.assert_array_equal(sub, [1, 2, 4, 8, 16])
    recorded = np.log2(pts["subsampling"]).astype(np.int64)
    assert len(pts) == 1222
    np.testing.assert_array_equal(np.bincount(recorded, minlength=5), [983, 149, 57, 24, 9])
    # from the scale alone -- the flag set, and the record's subsampling wiped
    np.testing.assert_array_equal(dm.octave_of(pts["scale"], pts["subsampling"], sub, dm.OCTAVE_FROM_SCALE), recorded)
    np.testing.assert_array_equal(dm.octave_of(pts["scale"], np.zeros(len(pts), np.float32), sub), recorded)
    # the recorded octave wins while it is there: a scale that belongs to another octave does not move the record
    np.testing.assert_array_equal(dm.octave_of(pts["scale"][::-1].copy(), pts["subsampling"], sub), recorded)
    ratio = pts["scale"] / pts["subsampling"]
    print("smallest scale / subsampling %.5f against the bound %.5f" % (float(ratio.min()), float(dm.K_LOW)))
    assert ratio.min() >= dm.K_LOW and abs(float(ratio.min()) - 0.93341) < 5e-6
    assert (dm.valid(pts["coords2D"][:, 0], pts["coords2D"][:, 1], pts["scale"])).all()
    # octave units and back: the same bits for every coordinate and scale (the subsamplings are powers of two)
    px, py, ks = dm.octave_units(pts, pts["subsampling"])
    for got, want in ((px, pts["coords2D"][:, 0]), (py, pts["coords2D"][:, 1]), (ks, pts["scale"])):
        back = (got * pts["subsampling"]).astype(np.float32)
        np.testing.assert_array_equal(back.view(np.uint32), want.view(np.uint32))


def test_bound_constant_is_the_detectors_lowest_scale():
    # scales[0] * 2^(-0.5 / NUM_SCALES) with scales[0] = 2^(-0.5 / 5) ... the refinement's lowest: 2^-0.1
    assert dm.K_LOW == np.float32(2.0 ** -0.1)
    assert dm.K_LOW.view(np.uint32) == np.float32(0.93303299).view(np.uint32)


def test_handcrafted_scales():
    sub = dm.octave_subsamplings(4, 1.0)
    zero = np.zeros(1, np.float32)

    def from_scale(s):
        return int(dm.octave_of(np.array([s], np.float32), zero, sub)[0])

    for o in range(1, 4):
        edge = np.float32(dm.K_LOW * sub[o])  # exactly on kLow * sub[o]: belongs to octave o
        assert from_scale(edge) == o
        assert from_scale(np.nextafter(edge, np.float32(0))) == o - 1
    assert from_scale(1e-6) == 0 and from_scale(0.5) == 0  # below every octave
    assert from_scale(1e30) == 3  # far beyond the coarsest
    # the octave rule answers 0 for what the validity test rejects anyway
    for bad in (np.nan, np.inf, -np.inf, 0.0, -2.0):
        s = np.array([bad], np.float32)
        assert not dm.valid(np.ones(1), np.ones(1), s)[0]
    assert not dm.valid(np.array([np.nan]), np.ones(1), np.ones(1))[0]
    assert not dm.valid(np.ones(1), np.array([-np.inf]), np.ones(1))[0]
    assert dm.valid(np.array([-1e6]), np.array([1e6]), np.array([1e-20]))[0]  # everything finite is legal
    # a stale subsampling (3.0 is no octave's), NaN and 0: from the scale; an exact one: that octave, unless the flag says no
    s = np.array([5.0], np.float32)
    for stale in (3.0, np.nan, 0.0, -2.0, 32.0):
        assert int(dm.octave_of(s, np.array([stale], np.float32), sub)[0]) == 2
    assert int(dm.octave_of(s, np.array([8.0], np.float32), sub)[0]) == 3
    assert int(dm.octave_of(s, np.array([8.0], np.float32), sub, dm.OCTAVE_FROM_SCALE)[0]) == 2


def test_subsamplings_of_the_pyramid():
    np.testing.assert_array_equal(dm.octave_subsamplings(3, 2.0, 1), [1, 2, 4])
    np.testing.assert_array_equal(dm.octave_subsamplings(6, 1.0, 1, 64, 48), [0.5, 1, 2, 4, 8, 16])
    np.testing.assert_array_equal(dm.octave_subsamplings(16, 1.0, 0, 64, 48), [1, 2, 4, 8, 16, 32])  # 1 x 0 ends it
    np.testing.assert_array_equal(dm.octave_subsamplings(0, 1.0), [1])
