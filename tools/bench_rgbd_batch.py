"""Wall time of registering a 64-frame RGB-D sequence, one route per process:

    python tools/bench_rgbd_batch.py --route batch     cusift_register_rgbd_batch: one call, one synchronisation
    python tools/bench_rgbd_batch.py --route loop      one read-back of the 64 counters, then 63 x cusift_register_rgbd

The sequence: the two fixture frames (tests/golden/vlfeat_sift1/2.bin, 884 and 856 records, with their depth images)
alternating, in the layout cusift_extract_batch produces (d_points[64][1024] + d_counters[64]); the 63 consecutive
pairs; 1024 hypotheses per pair; ratio test 0.6, 0.05 m.  The timed region is the whole route, from device-resident
records and depth images to the 63 [R | t] on the host.  The median over --reps repetitions (after --warmup) goes to
profiles/rgbd_batch_<route>.json.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden")
N_FRAMES, MAX_PTS, W, H, LOOPS = 64, 1024, 640, 480, 1024


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--route", choices=("batch", "loop"), required=True)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from cusift_amd import capi
    from oracle_binding import read_vlfeat_sift

    frames = [read_vlfeat_sift(os.path.join(GOLDEN, "vlfeat_sift%d.bin" % k)) for k in (1, 2)]
    z = np.load(os.path.join(GOLDEN, "rgbd_depth.npz"))
    depths = [np.ascontiguousarray(z["depth1"]), np.ascontiguousarray(z["depth2"])]
    K = np.array(open(os.path.join(GOLDEN, "rgbd_intrinsics.txt")).read().split(), np.float64).reshape(3, 3)
    cam = capi.Camera(K[0, 0], K[1, 1], K[0, 2], K[1, 2], origin=1.0, units_per_metre=1000.0, encoding=1)
    points = np.zeros((N_FRAMES, MAX_PTS), capi.SIFT_POINT_DTYPE)
    counters = np.zeros(N_FRAMES, np.uint32)
    depth = np.zeros((N_FRAMES, H, W), np.uint16)
    for i in range(N_FRAMES):
        f = frames[i % 2]
        points[i, :len(f)], counters[i], depth[i] = f, len(f), depths[i % 2]
    pairs = np.array([(i, i + 1) for i in range(N_FRAMES - 1)], np.int32)

    ctx = capi.Context(0)
    d_points, d_counters = capi.DeviceBuffer.from_numpy(ctx, points), capi.DeviceBuffer.from_numpy(ctx, counters)
    d_depth = capi.DeviceBuffer.from_numpy(ctx, depth)
    settings = dict(distance=1, score_threshold=999.0, ambiguity_threshold=0.6, loops=LOOPS,
                    thresh2=float(np.float32(0.05) * np.float32(0.05)))
    rec, img = capi.SIFT_POINT_BYTES * MAX_PTS, 2 * W * H

    def batch():
        rt, _, n_in, _, _ = ctx.register_rgbd_batch(d_points.ptr, d_counters.ptr, N_FRAMES, MAX_PTS, d_depth.ptr, W, H,
                                                    cam, pairs, seed=1, **settings)
        return rt, n_in

    def loop():
        counts = np.zeros(N_FRAMES, np.uint32)
        ctx.d2h(counts, d_counters.ptr)  # the one read-back the pair calls need
        counts = np.minimum(counts, MAX_PTS)
        rts, n_ins = [], []
        for p, (a, b) in enumerate(pairs):
            rt, _, _, n_in = ctx.register_rgbd(d_points.ptr + int(a) * rec, int(counts[a]), d_depth.ptr + int(a) * img,
                                               d_points.ptr + int(b) * rec, int(counts[b]), d_depth.ptr + int(b) * img,
                                               W, H, cam, seed=1 + p, **settings)
            rts.append(rt)
            n_ins.append(n_in)
        return np.stack(rts), np.array(n_ins)

    route = batch if args.route == "batch" else loop
    for _ in range(args.warmup):
        rt, n_in = route()
    times = []
    for _ in range(args.reps):
        ctx.synchronize()
        t0 = time.perf_counter()
        rt, n_in = route()
        times.append((time.perf_counter() - t0) * 1e3)
    result = {"route": args.route, "frames": N_FRAMES, "pairs": len(pairs), "max_pts": MAX_PTS, "hypotheses": LOOPS,
              "reps": args.reps, "warmup": args.warmup, "median_ms": float(np.median(times)), "min_ms": float(min(times)),
              "max_ms": float(max(times)), "inliers_min": int(n_in.min()), "inliers_max": int(n_in.max()),
              "rt_checksum": float(np.abs(rt.astype(np.float64)).sum())}
    out = args.out or os.path.join(ROOT, "profiles", "rgbd_batch_%s.json" % args.route)
    with open(out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
