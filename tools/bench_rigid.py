#!/usr/bin/env python3
"""Timing record of cusift_estimate_rigid (RANSAC rigid transform) on one MI355X, beside its sibling
cusift_find_homography at the same sizes in the same process.

    python tools/bench_rigid.py [--out profiles/rigid_ransac.json] [--iters 30] [--warmup 5]

Cases (num_pts, num_loops) = (120, 4096), (4096, 4096), (4096, 65536).  Every figure is the median over `iters` calls
after `warmup` calls: `wall_us` is the whole blocking call as the caller sees it (upload, three launches, one read-back),
`device_us` the span between two events recorded on the context's stream around the call.  The rigid call is timed with
caller-given samples (3-D and 2-D) and with samples drawn on the device; the homography with caller-given samples, its
only mode.  A record, not an assertion.  The C ABI only, no torch.
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

CASES = ((120, 4096), (4096, 4096), (4096, 65536))


def rigid_scene(n, seed):
    """70 % inliers of a planted motion (0.35 rad about a skew axis) with 4 mm noise in a 1.8 x 1.2 x 2.7 m volume."""
    r = np.random.default_rng(seed)
    ax = np.array([0.2, 0.9, 0.1]) / np.linalg.norm([0.2, 0.9, 0.1])
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    R = np.eye(3) + np.sin(0.35) * K + (1 - np.cos(0.35)) * K @ K
    y = np.c_[r.uniform(-0.9, 0.9, n), r.uniform(-0.6, 0.6, n), r.uniform(0.8, 3.5, n)]
    x = y @ R.T + [0.12, -0.03, 0.2] + r.normal(0, 0.004, (n, 3))
    out = r.random(n) > 0.7
    x[out] = np.c_[r.uniform(-0.9, 0.9, out.sum()), r.uniform(-0.6, 0.6, out.sum()), r.uniform(0.8, 3.5, out.sum())]
    return np.ascontiguousarray(np.hstack([x, y]).astype(np.float32))


def homography_scene(capi, n, seed):
    r = np.random.default_rng(seed)
    H = np.array([[1.02, 0.03, 12.0], [-0.02, 0.98, -7.0], [2e-5, -1e-5, 1.0]])
    pts = np.zeros(n, dtype=capi.SIFT_POINT_DTYPE)
    xy = np.c_[r.uniform(0, 1280, n), r.uniform(0, 960, n)]
    p = np.c_[xy, np.ones(n)] @ H.T
    m = p[:, :2] / p[:, 2:] + r.normal(0, 0.5, (n, 2))
    out = r.random(n) > 0.7
    m[out] = np.c_[r.uniform(0, 1280, out.sum()), r.uniform(0, 960, out.sum())]
    pts["coords2D"] = xy
    pts["match_xpos"], pts["match_ypos"] = m[:, 0], m[:, 1]
    return pts


def distinct(n, loops, k, seed):
    r = np.random.default_rng(seed)
    s = r.integers(0, n, (loops, k))
    for _ in range(64):  # redraw rows with a repeated index
        bad = np.array([len(set(row)) < k for row in s])
        if not bad.any():
            break
        s[bad] = r.integers(0, n, (int(bad.sum()), k))
    return np.ascontiguousarray(s.astype(np.int32))


def timed(capi, ctx, fn, iters, warmup):
    lib = capi.lib()
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        capi.check(lib.cusift_event_create(ctx.handle, C.byref(e)))
    wall, dev = [], []
    for i in range(warmup + iters):
        capi.check(lib.cusift_event_record(ev[0], ctx.handle))
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        capi.check(lib.cusift_event_record(ev[1], ctx.handle))
        ctx.synchronize()
        ms = C.c_float(0)
        capi.check(lib.cusift_event_elapsed_ms(ev[0], ev[1], C.byref(ms)))
        if i >= warmup:
            wall.append((t1 - t0) * 1e6)
            dev.append(ms.value * 1e3)
    for e in ev:
        lib.cusift_event_destroy(e)
    return {"wall_us": round(float(np.median(wall)), 1), "device_us": round(float(np.median(dev)), 1),
            "wall_us_min": round(float(np.min(wall)), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert a.iters >= 20 and a.warmup >= 5
    from cusift_amd import capi

    rows = []
    with capi.Context(0) as ctx:
        for n, loops in CASES:
            coord = rigid_scene(n, 1)
            idx = distinct(n, loops, 3, 2)
            pts = homography_scene(capi, n, 3)
            d_pts = capi.DeviceBuffer.from_numpy(ctx, pts)
            rand_pts = np.ascontiguousarray(distinct(n, loops, 4, 4).T)
            row = {"num_pts": n, "num_loops": loops}
            row["rigid_3d_given"] = timed(capi, ctx, lambda: ctx.estimate_rigid(coord, idx, kind="3d"), a.iters, a.warmup)
            row["rigid_3d_drawn"] = timed(capi, ctx, lambda: ctx.estimate_rigid(coord, None, loops=loops, kind="3d", seed=7),
                                          a.iters, a.warmup)
            row["rigid_2d_given"] = timed(capi, ctx, lambda: ctx.estimate_rigid(coord, idx, kind="2d"), a.iters, a.warmup)
            row["find_homography"] = timed(capi, ctx, lambda: ctx.find_homography(d_pts.ptr, n, rand_pts, thresh=5.0),
                                           a.iters, a.warmup)
            row["rigid_3d_inliers"] = int(ctx.estimate_rigid(coord, idx, kind="3d")[1])
            row["homography_inliers"] = int(ctx.find_homography(d_pts.ptr, n, rand_pts, thresh=5.0)[1])
            d_pts.free()
            rows.append(row)
            print(json.dumps(row), flush=True)
    rec = {"tool": "tools/bench_rigid.py", "iters": a.iters, "warmup": a.warmup, "unit": "microseconds, median",
           "cases": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
