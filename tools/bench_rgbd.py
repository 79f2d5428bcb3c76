#!/usr/bin/env python3
"""Timing record of the RGB-D pair registration on one MI355X: the fused device-resident call against the staged
host-filter route, on the same inputs (the reference's frame pair under tests/golden/: 1093 + 1058 VLFeat keypoints,
two 640 x 480 depth images; 1024 hypotheses, 0.05 m).

    python tools/bench_rgbd.py --route fused  [--out profiles/rgbd_fused.json]  [--iters 30] [--warmup 5]
    python tools/bench_rgbd.py --route staged [--out profiles/rgbd_staged.json]

One route per process, so that each runs under a time limit of its own.
  fused   cusift_register_rgbd: lift x 2, match, select, RANSAC + refit; one synchronisation, at the read-back
  staged  what include/rgbd.h's LiftSiftData + include/matching.h + include/rigidTransform.h do: lift and read coords3D
          back (twice), cusift_match and read its five fields back, filter on the host, gather h_coord,
          cusift_estimate_rigid (upload, three launches, read-back) -- four synchronisations; the host filter is numpy
Both start from records and depth images already on the device.  `wall_us` is the median over `iters` calls after
`warmup` calls of the whole route as the caller sees it.  A record, not an assertion; both routes print the same Rt for
the same seed.  The C ABI only, no torch.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
W, H, LOOPS, SEED = 640, 480, 1024, 7


def read_vlfeat(capi, path):
    raw = open(path, "rb").read()
    n = int(np.frombuffer(raw[:4], "<u4")[0])
    out = np.zeros(n, dtype=capi.SIFT_POINT_DTYPE)
    frames = np.frombuffer(raw[4:4 + 16 * n], "<f4").reshape(n, 4)
    out["coords2D"], out["scale"], out["orientation"] = frames[:, :2], frames[:, 2], frames[:, 3]
    out["data"] = np.frombuffer(raw[4 + 16 * n:], "<f4").reshape(n, 128)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=("fused", "staged"), required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert a.iters >= 20 and a.warmup >= 5
    from cusift_amd import capi

    s1 = read_vlfeat(capi, os.path.join(GOLDEN, "vlfeat_sift1.bin"))
    s2 = read_vlfeat(capi, os.path.join(GOLDEN, "vlfeat_sift2.bin"))
    z = np.load(os.path.join(GOLDEN, "rgbd_depth.npz"))
    K = np.array(open(os.path.join(GOLDEN, "rgbd_intrinsics.txt")).read().split(), np.float64).reshape(3, 3)
    cam = capi.Camera(K[0, 0], K[1, 1], K[0, 2], K[1, 2], origin=1.0, units_per_metre=1000.0, encoding=1)
    n1, n2 = len(s1), len(s2)
    thresh2 = float(np.float32(0.05) * np.float32(0.05))
    with capi.Context(0) as ctx:
        lib = capi.lib()
        b1, b2 = capi.DeviceBuffer.from_numpy(ctx, s1), capi.DeviceBuffer.from_numpy(ctx, s2)
        e1 = capi.DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(z["depth1"]))
        e2 = capi.DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(z["depth2"]))
        h1, h2 = s1.copy(), s2.copy()
        off3d = capi.SIFT_POINT_DTYPE.fields["coords3D"][1]
        off_score = capi.SIFT_POINT_DTYPE.fields["score"][1]

        def fields_back(host, dev, n, off, nbytes):
            capi.check(lib.cusift_memcpy2d_d2h(ctx.handle, host.ctypes.data + off, 588, dev.ptr + off, 588, nbytes, n))

        def fused():
            rt, pairs, flags, n_in = ctx.register_rgbd(b1.ptr, n1, e1.ptr, b2.ptr, n2, e2.ptr, W, H, cam, distance=1,
                                                       score_threshold=1000.0, ambiguity_threshold=0.6, loops=LOOPS,
                                                       thresh2=thresh2, kind="3d", seed=SEED)
            return rt, len(pairs), n_in

        def staged():
            ctx.lift_depth(b1.ptr, n1, e1.ptr, W, H, cam)
            fields_back(h1, b1, n1, off3d, 12)
            ctx.lift_depth(b2.ptr, n2, e2.ptr, W, H, cam)
            fields_back(h2, b2, n2, off3d, 12)
            ctx.match(b1.ptr, n1, b2.ptr, n2, 1)
            fields_back(h1, b1, n1, off_score, 20)
            keep = capi.match_filter(h1, 1000.0, 0.6)
            m = h1["match"][keep]
            ok = (m >= 0) & (m < n2)
            keep, m = keep[ok], m[ok]
            ok = (h1["coords3D"][keep, 2] != 0) & (h2["coords3D"][m, 2] != 0)
            coord = np.ascontiguousarray(np.hstack([h1["coords3D"][keep[ok]], h2["coords3D"][m[ok]]]))
            rt, n_in, _, _ = ctx.estimate_rigid(coord, None, loops=LOOPS, thresh2=thresh2, kind="3d", seed=SEED)
            return rt, len(coord), n_in

        fn = fused if a.route == "fused" else staged
        wall = []
        for i in range(a.warmup + a.iters):
            ctx.synchronize()
            t0 = time.perf_counter()
            rt, n_match, n_in = fn()
            t1 = time.perf_counter()
            if i >= a.warmup:
                wall.append((t1 - t0) * 1e6)
    rec = {"tool": "tools/bench_rgbd.py", "route": a.route, "iters": a.iters, "warmup": a.warmup,
           "unit": "microseconds per registration", "num_pts": [n1, n2], "num_loops": LOOPS, "seed": SEED,
           "wall_us": round(float(np.median(wall)), 1), "wall_us_min": round(float(np.min(wall)), 1),
           "wall_us_p90": round(float(np.percentile(wall, 90)), 1), "num_matches": int(n_match),
           "num_inliers": int(n_in), "rt": [round(float(v), 6) for v in rt.reshape(-1)]}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
