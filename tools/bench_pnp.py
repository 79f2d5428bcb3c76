#!/usr/bin/env python3
"""Timing record of the absolute pose (PnP) on one MI355X, beside the two-view pose a caller would otherwise run on a
third frame: cusift_register_pnp and cusift_register_pose on tools/bench_epipolar.py's two frames (a planted non-planar
scene, 40 % gross outliers, f = 1000 at (640, 480)) of 4,096 and 32,768 records with 10,000 hypotheses and five refit
rounds.  For the PnP call the 60 % planted records of frame 1 carry their planted point in coords3D, the rest carry none.

    python tools/bench_pnp.py --out profiles/pnp.json [--iters 20] [--warmup 5]
    python tools/bench_pnp.py --kernel-trace TRACE.csv --out profiles/pnp.json     # adds `kernels` to the record

The two calls alternate, call by call, in the same process, each on record buffers of its own (register_pose writes
coords3D).  Per call the record holds the median wall time over `iters` calls after `warmup` calls of the whole call as
the caller sees it, the matcher included, and the spread: minimum, 10th and 90th percentile, maximum.  A record, not an
assertion.  The C ABI only, no torch.
--kernel-trace: the *_kernel_trace.csv of a run of this tool under `rocprofv3 --kernel-trace --output-format csv`, a run
of its own; the average duration per size of every kernel of the two calls (the sizes run one after the other, so a
kernel's calls split into equal runs in time order) is added to the record at --out as `kernels`, with
pnp_select_kernel over epipolar_select_kernel.
"""
import argparse
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_epipolar import LOOPS, SEED, SIZES, frames  # noqa: E402  (the same frames)

KERNELS = (r"(pnp_mark_kernel|pnp_solve_kernel|pnp_score_kernel|pnp_select_kernel|planar_mark_kernel|planar_compact_kernel|"
           r"epipolar_solve_kernel|epipolar_score_kernel|epipolar_select_kernel|pose_vote_kernel|pose_write_kernel|"
           r"match_kernel|match_merge_kernel)")


def planted_points(n, seed=3):
    """The 3-D points behind frames(capi, n): its generator once more, keeping what it drops.  [n, 3] in the coordinates of
    camera 1, zeros for the records that are not planted."""
    rng = np.random.default_rng(seed)
    n_in = int(round(0.6 * n))
    c, s = np.cos(0.15), np.sin(0.15)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    t = -R @ np.array([0.8, 0.0, 0.0])
    p1, world = np.zeros((0, 2)), np.zeros((0, 3))
    while len(p1) < n_in:
        X = rng.uniform([-3, -2, 3], [3, 2, 12], size=(4 * n_in, 3))
        X2 = X @ R.T + t
        a = 1000.0 * X[:, :2] / X[:, 2:] + [640, 480]
        b = 1000.0 * X2[:, :2] / X2[:, 2:] + [640, 480]
        ok = ((a >= 0) & (a < [1280, 960]) & (b >= 0) & (b < [1280, 960])).all(axis=1)
        p1, world = np.r_[p1, a[ok]], np.r_[world, X[ok]]
    first = (p1[:n_in] + rng.normal(0, 0.3, (n_in, 2))).astype(np.float32)
    return np.r_[world[:n_in], np.zeros((n - n_in, 3))].astype(np.float32), first, R, t


def spread(wall):
    w = np.sort(np.asarray(wall))
    return {"median_us": round(float(np.median(w)), 1), "min_us": round(float(w[0]), 1),
            "p10_us": round(float(np.percentile(w, 10)), 1), "p90_us": round(float(np.percentile(w, 90)), 1),
            "max_us": round(float(w[-1]), 1)}


def alternating(ctx, fns, iters, warmup):
    """Times the calls of `fns` in turn, call by call; returns ([wall times] per call, the last result per call)."""
    wall, out = [[] for _ in fns], [None] * len(fns)
    for i in range(warmup + iters):
        for j, fn in enumerate(fns):
            ctx.synchronize()
            t0 = time.perf_counter()
            out[j] = fn()
            t1 = time.perf_counter()
            if i >= warmup:
                wall[j].append((t1 - t0) * 1e6)
    return wall, out


def kernel_times(path):
    import csv

    calls = {}
    for r in sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"])):
        m = re.search(KERNELS, r["Kernel_Name"])
        if m:
            calls.setdefault(m.group(1), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {}
    for name, t in calls.items():
        per = len(t) // len(SIZES)
        for i, n in enumerate(SIZES):
            out.setdefault("%d records, %d loops" % (n, LOOPS), {})[name + "_avg_us"] = round(
                float(np.mean(t[i * per:(i + 1) * per])), 1)
    for case in out.values():
        if "pnp_select_kernel_avg_us" in case and "epipolar_select_kernel_avg_us" in case:
            case["pnp_select_over_epipolar_select"] = round(case["pnp_select_kernel_avg_us"] /
                                                            case["epipolar_select_kernel_avg_us"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-trace", default=None)
    a = ap.parse_args()
    if a.kernel_trace:
        rec = json.load(open(a.out))
        rec["kernels"] = kernel_times(a.kernel_trace)
        rec["kernels_note"] = ("average kernel durations under a kernel trace, a run of its own (warm-up calls included; the "
                               "matcher runs in both calls, planar_compact_kernel too)")
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
        print(json.dumps(rec["kernels"], indent=1))
        return
    from cusift_amd import capi

    cam = capi.Camera(1000.0, 1000.0, 640.0, 480.0, 0.0, 1000.0, 0)
    cases = {}
    with capi.Context(0) as ctx:
        for n in SIZES:
            f1, f2 = frames(capi, n)
            world, first, R21, t21 = planted_points(n)
            assert np.array_equal(first, f1["coords2D"][:len(first)])  # the replay is the generator
            g1 = f1.copy()
            g1["coords3D"] = world
            b1, b2 = capi.DeviceBuffer.from_numpy(ctx, g1), capi.DeviceBuffer.from_numpy(ctx, f2)
            p1 = capi.DeviceBuffer.from_numpy(ctx, f1)
            common = dict(distance=0, rule=0, lo=0.85, hi=0.95, loops=LOOPS, refine_loops=5, seed=SEED)
            (wall_n, wall_p), (pnp, pose) = alternating(ctx, [
                lambda: ctx.register_pnp(b1.ptr, n, b2.ptr, n, cam, thresh=3.0, refine_thresh=2.0, **common),
                lambda: ctx.register_pose(p1.ptr, n, b2.ptr, n, cam, thresh=1.0, refine_thresh=1.0, **common)],
                a.iters, a.warmup)
            truth_t = -R21.T @ t21
            cases["%d records, %d loops" % (n, LOOPS)] = {
                "register_pnp_wall": spread(wall_n),
                "register_pose_wall": spread(wall_p),
                "register_pnp_over_register_pose": round(float(np.median(wall_n) / np.median(wall_p)), 4),
                "pnp": {"num_candidates": pnp.num_candidates, "num_matches": pnp.num_matches, "num_fit": pnp.num_fit,
                        "translation_error_over_length": round(float(np.linalg.norm(pnp.rt[:, 3] - truth_t) /
                                                                     np.linalg.norm(truth_t)), 6),
                        "rotation_max_abs_difference": round(float(np.abs(pnp.rt[:, :3] - R21.T).max()), 8)},
                "pose": {"num_candidates": pose.num_candidates, "num_fit": pose.num_fit, "num_front": pose.num_front}}
            for b in (b1, b2, p1):
                b.free()
    rec = {"tool": "tools/bench_pnp.py", "unit": "microseconds per call (wall time, the matcher included)",
           "iters": a.iters, "warmup": a.warmup, "seed": SEED, "cases": cases,
           "note": "register_pose is the call a user without PnP would make on the same frames and the yardstick of cost; "
                   "the two calls alternate call by call in one process.  register_pnp has 60 % of the records as "
                   "candidates (those that carry a point), register_pose all of them"}
    text = json.dumps(rec, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
