"""cusift_bundle_adjust's factorisation (bundle_solve_kernel, cusift_amd/csrc/sift_bundle.hip) at the sizes where its
second row turn starts to work, against tests/bundle_model.py through test_bundle.py's compare() at the project's bar of
1e-9 * max(1, |value|).  The kernel is one workgroup of 1024 threads for up to 1536 unknowns: every loop over a thread's
rows has a second turn for row J + tx + 1024, live only above 1024 unknowns, and the right-hand side (row M) is a
second-turn row while M - J >= 1024.  Scene B (planted_scene(n_tracks, n_cams, max_views, 0, 3, 0.01, 0.02)) at

  170 frames, 1020 unknowns: the largest size with the first turn alone; the right-hand side sits at tx == 1020;
  171 frames, 1026 unknowns: the smallest with the second turn (rows 1024, 1025 and the right-hand side at J == 0,
                             first-turn rows from J >= 6); 1026 is no multiple of the 8 the inner loops step by;
  256 frames, 1536 unknowns: the cap, M == kBundleMaxDim; the right-hand side is a second-turn row until J == 516.

At 171 frames the second turn works in the pass J == 0 alone, on frame 0's six columns.  With frame 0 held (h_fixed
NULL) those columns are the identity and the right-hand side there is zero, so rows 1024, 1025 and y[0 .. 5] are zeros
whether the second turn computes them or not: a build with the accumulation's second turn skipped passed that case.
Hence the fourth case, 171_frame_0_free: the same scene with frame 85 held in frame 0's place.  Track 190 joins frames
0 and 170, so S[1020 .. 1025][0 .. 5] and the right-hand side's first six entries hold data (asserted on the model's
system), and the second turn at J == 0 decides the result.

Two iterations at 170 and 171 (the second starts from the flipped buffers), one at 256.  The conditions a scene must
meet -- every frame but the held one free, a step accepted, the accepted steps above 1e-6 relative so that their flags
are compared -- are asserted on the model here and, without a GPU, in tests/test_bundle_model.py.

The numpy model on the CPU: 4.6 s for the two iterations at 170 frames, 4.4 s at 171, 7.2 s for the one at 256; each
is computed once (functools.lru_cache).

Measured on an MI355X, largest deviation from the model (bar 1e-9):
  170: 6.24e-13    171: 3.9e-13    171_frame_0_free: 1.26e-13    256: 6.15e-14 (its poses bit-identical)
The bar held with three orders to spare, so the model's reduced system was not solved again in long double.

A build with the second row turn of the accumulation skipped (`r < 1` in that loop, acc zero-initialised: every address
unchanged), run once: 170 passes (6.24e-13), 171 passes (3.9e-13, the zeros described above), 171_frame_0_free fails
(poses 0.172 off, a trial cost 5.2e5 times the model's), 256 fails (an infinite deviation)."""
import functools

import numpy as np
import pytest

import bundle_model as bm
from test_bundle import compare, fixed_mask

pytestmark = pytest.mark.gpu

# name -> (n_cams, n_tracks, max_views, iterations, the held frame; 0: h_fixed NULL)
SIZES = {"170": (170, 200, 12, 2, 0), "171": (171, 200, 12, 2, 0), "171_frame_0_free": (171, 200, 12, 2, 85),
         "256": (256, 260, 16, 1, 0)}
JOINING_TRACK = 190  # of the 171-frame scene: seen by frames 0 and 170 (and by neither 85 nor any frame twice)


def size_kw(name):
    n_cams, _, _, iterations, held = SIZES[name]
    return dict(iterations=iterations, **(dict(fixed=fixed_mask(n_cams, (held,))) if held else {}))


@functools.lru_cache(maxsize=None)
def size_case(name):
    """(scene, model) of Scene B for SIZES[name].  Shared: treat both as read-only."""
    n_cams, n_tracks, max_views, _, held = SIZES[name]
    sc = bm.planted_scene(n_tracks, n_cams, max_views, 0, 3, 0.01, 0.02)
    return sc, bm.run_model(sc, keep_system=bool(held), **size_kw(name))


def check_size_conditions(name):
    """On the model alone: the factorisation runs at 6 * n_cams unknowns with data in every row, and its result decides."""
    n_cams, _, _, iterations, held = SIZES[name]
    sc, model = size_case(name)
    h = model["history"]
    assert sc["n"] == n_cams and model["summary"][6] == n_cams - 1  # every frame but the held one is free
    assert model["held"].tolist() == [f == held for f in range(n_cams)]
    assert model["summary"][2] >= 1 and model["summary"][3] == iterations
    accepted = h[h[:, 3] == 1]
    assert len(accepted) == model["summary"][2]
    assert ((accepted[:, 0] - accepted[:, 1]) / accepted[:, 0] > 1e-6).all()  # compare() compares these flags
    assert not any(c["sfail"] or c["vfail"] or c["behind"] for c in model["causes"])
    if held:  # the second turn's rows of the pass J == 0 hold data: in S through the joining track, and in the right-hand side
        s = slice(sc["offsets"][JOINING_TRACK], sc["offsets"][JOINING_TRACK + 1])
        frames = (sc["obs"][s] // sc["max_pts"]).tolist()
        assert 0 in frames and n_cams - 1 in frames and held not in frames and model["used_obs"][s].all()
        for S, rhs, step in model["systems"]:
            assert (S[1024:1026, 0:6] != 0.0).all() and (rhs[0:6] != 0.0).all() and (step[0:6] != 0.0).all()
    return sc, model


@pytest.mark.parametrize("name", list(SIZES))
def test_factorisation_at_the_row_turn_sizes(ctx, name):
    n_cams, n_tracks, _, iterations, _ = SIZES[name]
    sc, model = check_size_conditions(name)
    dev = bm.DeviceBundle(ctx, sc)
    try:
        out = dev.run(**size_kw(name))
        # (printed before anything is asserted)
        print("bundle_adjust %s: %d frames (%d unknowns) x %d tracks, %d iteration(s): poses %.3g, points %.3g, history "
              "%.3g of the model" % (name, n_cams, 6 * n_cams, n_tracks, iterations,
                                     np.abs(out["poses"] - model["poses"]).max(),
                                     np.abs(out["points3d"][:len(model["points3d"])] - model["points3d"]).max(),
                                     np.abs(out["history"][:iterations, :2] / model["history"][:, :2] - 1.0).max()))
        worst, decided = compare(out, model, sc, iterations)
        print("bundle_adjust %s: largest deviation %.3g (bar 1e-9), %d of %d flags decided" %
              (name, worst, decided, iterations))
        assert decided == iterations
        assert dev.records_back().tobytes() == dev.recs.tobytes()
        if name == "256":
            again = dev.run(**size_kw(name))
            for k in ("points3d", "poses", "history", "summary"):
                assert again[k].tobytes() == out[k].tobytes(), k  # the same bytes on every run
    finally:
        dev.close()
