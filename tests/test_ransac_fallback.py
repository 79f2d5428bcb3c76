"""The sampler's fallback on the device.  ransac_sample of cusift_amd/csrc/sift_ransac.h serves the three RANSAC solve
kernels (3, 4 and 8 slots); a slot that was redrawn 64 times takes the lowest index not taken yet.  With three or four
slots no input reaches that branch in practice ((2/3)^64 and (3/8)^64 per loop at the fewest points allowed), with eight
slots over eight candidates about one loop in 5000 does: tests/test_epipolar.py::test_sampler_fallback_after_64_redraws
shows without a GPU that some of the first 40 000 loops of seed 0 take it.  The same loops on the device, every index."""
import numpy as np
import pytest

from test_epipolar import eight_of, run, sample_loop8, scene
from test_planar import RULE_ARGS, draw

LOOPS = 40000


@pytest.mark.gpu
def test_eight_candidates_seed_0_40000_loops_draw_the_restatement_fallback_included(ctx):
    good = np.array([3, 41, 77, 120, 166, 201, 250, 299])
    pts = eight_of(scene(200, 100)[0], good)
    drawn = [sample_loop8(0, l, 8) for l in range(LOOPS)]
    want = np.array([p for p, _ in drawn], dtype=np.int32).T  # [8, loops], positions in the candidate list
    # slot 8 was redrawn 64 times and every redraw was refused (the condition of the test without a GPU)
    fallback = [l for l, (p, redraws) in enumerate(drawn) if redraws[6] == 64 and
                all(draw(0, l, 8 + sum(redraws[:6]) + t, 8) in p[:7] for t in range(64))]
    assert fallback, "no loop of 40 000 reached the fallback"
    res, _ = run(ctx, pts, loops=LOOPS, seed=0, refine_loops=0, **RULE_ARGS[0])
    assert res.num_candidates == 8
    assert np.array_equal(res.drawn, good[want].astype(np.int32))
