#!/usr/bin/env python3
"""Wall time of the absolute pose (PnP) of a 64-frame sequence on one MI355X, both routes in one process, alternating:

    batch   cusift_register_pnp_batch over the 63 consecutive pairs: one call, one synchronisation, no count read back
    loop    cusift_register_pnp(i, i + 1) for the same pairs with seed + i: one synchronisation per pair

    python tools/bench_pnp_batch.py [--out profiles/pnp_batch.json] [--reps 10] [--warmup 2] [--sizes 4096 8192]
    python tools/bench_pnp_batch.py --kernel-trace TRACE.csv [--out ...]       # adds `kernels` to the record at --out

The sequence, the settings, the timed region and the record are those of tools/bench_pose_batch.py (which this tool
shares its code with); the 60 % planted records of every frame carry their planted point, in the frame's own camera
coordinates, in coords3D, the rest carry none: 60 % of the records are candidates.  Scoring threshold 3 px, refit at 2 px.
A record, not an assertion.  The C ABI only, no torch.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_pose_batch import LOOPS, N_FRAMES, SEED, run  # noqa: E402


def pnp_routes(ctx, capi, buf, n, pairs):
    cam = capi.Camera(1000.0, 1000.0, 640.0, 480.0, 0.0, 1000.0, 0)
    kw = dict(distance=0, rule=0, lo=0.85, hi=0.95, loops=LOOPS, thresh=3.0, refine_loops=5, refine_thresh=2.0)
    stride = n * capi.SIFT_POINT_BYTES

    def batch():
        res = ctx.register_pnp_batch(buf.ptr, None, N_FRAMES, n, pairs, cam, seed=SEED, want_inliers=False, **kw)
        return res.rt, res.num_fit

    def loop():
        out = [ctx.register_pnp(buf.ptr + int(a) * stride, n, buf.ptr + int(b) * stride, n, cam, seed=SEED + p, **kw)
               for p, (a, b) in enumerate(pairs)]
        return np.stack([r.rt for r in out]), np.array([r.num_fit for r in out])

    return {"batch": batch, "loop": loop}


if __name__ == "__main__":
    run("tools/bench_pnp_batch.py", "pnp_batch.json",
        "loop is cusift_register_pnp per pair, the call that existed before the pair-list form and the yardstick; the "
        "routes alternate repetition by repetition in one process", pnp_routes, True)
