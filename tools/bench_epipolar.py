#!/usr/bin/env python3
"""Timing record of the epipolar registration on one MI355X, beside the planar registration that existed before it:
cusift_register_epipolar and cusift_register_planar on the same two frames -- a planted non-planar scene (two 1280 x 960
views, 0.3 px noise, 40 % gross outliers; every record of frame 1 carries its partner's descriptor) of 4,096 and 32,768
records with 10,000 hypotheses, five refit rounds each.

    python tools/bench_epipolar.py --out profiles/epipolar.json [--iters 20] [--warmup 5] [--test-log LOG]
    python tools/bench_epipolar.py --kernel-trace TRACE.csv --out profiles/epipolar.json     # adds `kernels` to the record

`wall_us` is the median over `iters` calls after `warmup` calls of the whole call as the caller sees it, the matcher
included (it is the same launch in both).  --test-log: the output of `pytest -s -m gpu tests/test_epipolar.py`, from which
the largest hypothesis difference per scene and the real pair's medians are copied into the record.  A record, not an
assertion.  The C ABI only, no torch.
--kernel-trace: the *_kernel_trace.csv of a run of this tool under `rocprofv3 --kernel-trace --output-format csv`; the
average duration of every registration kernel per size (the sizes run one after the other, so a kernel's calls split
into equal runs in time order) is added to the record at --out as `kernels`.
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
SIZES = (4096, 32768)
LOOPS = 10000
SEED = 7


def frames(capi, n, seed=3):
    """Two frames of n records: 60 % see the same 3-D points from two cameras, the rest lie anywhere; record i of frame 1
    and record perm[i] of frame 2 share a unit descriptor."""
    rng = np.random.default_rng(seed)
    n_in = int(round(0.6 * n))
    c, s = np.cos(0.15), np.sin(0.15)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    t = -R @ np.array([0.8, 0.0, 0.0])
    p1, p2 = np.zeros((0, 2)), np.zeros((0, 2))
    while len(p1) < n_in:
        X = rng.uniform([-3, -2, 3], [3, 2, 12], size=(4 * n_in, 3))
        X2 = X @ R.T + t
        a = 1000.0 * X[:, :2] / X[:, 2:] + [640, 480]
        b = 1000.0 * X2[:, :2] / X2[:, 2:] + [640, 480]
        ok = ((a >= 0) & (a < [1280, 960]) & (b >= 0) & (b < [1280, 960])).all(axis=1)
        p1, p2 = np.r_[p1, a[ok]], np.r_[p2, b[ok]]
    p1 = np.r_[p1[:n_in] + rng.normal(0, 0.3, (n_in, 2)), rng.uniform([0, 0], [1280, 960], (n - n_in, 2))]
    p2 = np.r_[p2[:n_in] + rng.normal(0, 0.3, (n_in, 2)), rng.uniform([0, 0], [1280, 960], (n - n_in, 2))]
    desc = rng.random((n, 128)).astype(np.float32)
    desc /= np.linalg.norm(desc, axis=1, keepdims=True)
    perm = rng.permutation(n)
    f1, f2 = np.zeros(n, dtype=capi.SIFT_POINT_DTYPE), np.zeros(n, dtype=capi.SIFT_POINT_DTYPE)
    f1["coords2D"], f1["data"] = p1.astype(np.float32), desc
    f2["coords2D"][perm], f2["data"][perm] = p2.astype(np.float32), desc
    return f1, f2


def timed(ctx, fn, iters, warmup):
    wall = []
    for i in range(warmup + iters):
        ctx.synchronize()
        t0 = time.perf_counter()
        out = fn()
        t1 = time.perf_counter()
        if i >= warmup:
            wall.append((t1 - t0) * 1e6)
    return wall, out


def figures(path):
    out = {}
    text = open(path).read()
    for m in re.finditer(r"scene \((\d+), (\d+)\): largest difference over the seeds ([0-9.e+-]+)", text):
        out["hypothesis_max_abs_difference_%s_%s" % m.group(1, 2)] = float(m.group(3))
    m = re.search(r"median Sampson distance over MATLAB's matches: ground truth ([0-9.]+) px, device ([0-9.]+) px", text)
    if m:
        out["real_pair_median_sampson_ground_truth_px"] = float(m.group(1))
        out["real_pair_median_sampson_device_px"] = float(m.group(2))
    # the figures are read from what the tests print: a reworded print must not drop them from the record unnoticed
    if len(out) != 5:
        raise SystemExit("%s: found %d of the 5 figures the tests print (%s)" % (path, len(out), sorted(out)))
    return out


def kernel_times(path):
    import csv

    calls = {}
    for r in sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"])):
        m = re.search(r"(epipolar_\w+|planar_\w+|homography_solve_kernel)", r["Kernel_Name"])
        if m:
            calls.setdefault(m.group(1), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {}
    for name, t in calls.items():
        per = len(t) // len(SIZES)
        for i, n in enumerate(SIZES):
            out.setdefault("%d records, %d loops" % (n, LOOPS), {})[name + "_avg_us"] = round(
                float(np.mean(t[i * per:(i + 1) * per])), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--test-log", default=None)
    ap.add_argument("--kernel-trace", default=None)
    a = ap.parse_args()
    if a.kernel_trace:
        rec = json.load(open(a.out))
        rec["kernels"] = kernel_times(a.kernel_trace)
        rec["kernels_note"] = ("average kernel durations under a kernel trace (warm-up calls included; planar_mark and "
                               "planar_compact serve both registrations)")
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
        print(json.dumps(rec["kernels"], indent=1))
        return
    from cusift_amd import capi

    cases = {}
    with capi.Context(0) as ctx:
        for n in SIZES:
            f1, f2 = frames(capi, n)
            b1, b2 = capi.DeviceBuffer.from_numpy(ctx, f1), capi.DeviceBuffer.from_numpy(ctx, f2)
            common = dict(distance=0, rule=0, lo=0.85, hi=0.95, loops=LOOPS, refine_loops=5, seed=SEED)
            wall_e, e = timed(ctx, lambda: ctx.register_epipolar(b1.ptr, n, b2.ptr, n, thresh=1.0, refine_thresh=1.0,
                                                                 **common), a.iters, a.warmup)
            wall_p, p = timed(ctx, lambda: ctx.register_planar(b1.ptr, n, b2.ptr, n, thresh=5.0, refine_thresh=3.0,
                                                               **common), a.iters, a.warmup)
            wall_m, _ = timed(ctx, lambda: (ctx.match(b1.ptr, n, b2.ptr, n, 0), ctx.synchronize()), a.iters, a.warmup)
            cases["%d records, %d loops" % (n, LOOPS)] = {
                "register_epipolar_wall_us": round(float(np.median(wall_e)), 1),
                "register_planar_wall_us": round(float(np.median(wall_p)), 1),
                "match_enqueue_and_wait_wall_us": round(float(np.median(wall_m)), 1),
                "epipolar": {"num_candidates": e.num_candidates, "num_matches": e.num_matches, "num_fit": e.num_fit},
                "planar": {"num_candidates": p.num_candidates, "num_matches": p.num_matches, "num_fit": p.num_fit}}
            b1.free()
            b2.free()
    rec = {"tool": "tools/bench_epipolar.py", "unit": "microseconds per call (median wall time, the matcher included)",
           "iters": a.iters, "warmup": a.warmup, "seed": SEED, "cases": cases,
           "note": "the scene is not planar, so register_planar's counts say nothing about its fit; it is there as the "
                   "yardstick of cost: the same matcher, marking and compaction, fp32 4-point hypotheses scored over all "
                   "records against fp64 8-point hypotheses scored over the candidates"}
    if a.test_log:
        rec["tests"] = figures(a.test_log)
    text = json.dumps(rec, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
