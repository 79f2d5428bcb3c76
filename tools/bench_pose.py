#!/usr/bin/env python3
"""Timing record of the calibrated pose on one MI355X, beside the epipolar registration it extends: cusift_register_pose
and cusift_register_epipolar on tools/bench_epipolar.py's two frames (a planted non-planar scene, 40 % gross outliers, f =
1000 at (640, 480)) of 4,096 and 32,768 records with 10,000 hypotheses and five refit rounds, and the staged
cusift_estimate_pose alone on records that carry the match fields.

    python tools/bench_pose.py --out profiles/pose.json [--iters 20] [--warmup 5]
    python tools/bench_pose.py --kernel-trace TRACE.csv --out profiles/pose.json     # adds `kernels` to the record

`wall_us` is the median over `iters` calls after `warmup` calls of the whole call as the caller sees it, the matcher
included.  The difference of the two fused calls is what the pose stage adds: a memset, two launches and a 256-byte copy
in front of the same synchronisation.  A record, not an assertion.  The C ABI only, no torch.
--kernel-trace: the *_kernel_trace.csv of a run of this tool under `rocprofv3 --kernel-trace --output-format csv`, a run
of its own; the average duration of the two pose kernels and of epipolar_select_kernel per size (the sizes run one after
the other, so a kernel's calls split into equal runs in time order), their sum and its ratio to the select kernel's time
are added to the record at --out as `kernels`.
"""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_epipolar import LOOPS, SEED, SIZES, frames, timed  # noqa: E402  (the same frames, the same clock)


def kernel_times(path):
    import csv

    calls = {}
    for r in sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"])):
        m = re.search(r"(pose_vote_kernel|pose_write_kernel|epipolar_select_kernel)", r["Kernel_Name"])
        if m:
            calls.setdefault(m.group(1), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {}
    for name, t in calls.items():
        per = len(t) // len(SIZES)
        for i, n in enumerate(SIZES):
            out.setdefault("%d records, %d loops" % (n, LOOPS), {})[name + "_avg_us"] = round(
                float(np.mean(t[i * per:(i + 1) * per])), 1)
    for case in out.values():
        case["pose_kernels_sum_us"] = round(case["pose_vote_kernel_avg_us"] + case["pose_write_kernel_avg_us"], 1)
        case["pose_kernels_over_select"] = round(case["pose_kernels_sum_us"] / case["epipolar_select_kernel_avg_us"], 4)
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
        rec["kernels_note"] = ("average kernel durations under a kernel trace, a run of its own (warm-up calls included; "
                               "the pose kernels run in both the fused and the staged call, the select kernel in both "
                               "fused calls)")
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
            b1, b2 = capi.DeviceBuffer.from_numpy(ctx, f1), capi.DeviceBuffer.from_numpy(ctx, f2)
            common = dict(distance=0, rule=0, lo=0.85, hi=0.95, loops=LOOPS, refine_loops=5, seed=SEED, thresh=1.0,
                          refine_thresh=1.0)
            wall_e, e = timed(ctx, lambda: ctx.register_epipolar(b1.ptr, n, b2.ptr, n, **common), a.iters, a.warmup)
            wall_p, p = timed(ctx, lambda: ctx.register_pose(b1.ptr, n, b2.ptr, n, cam, **common), a.iters, a.warmup)
            wall_s, s = timed(ctx, lambda: ctx.estimate_pose(b1.ptr, n, p.fundamental, cam, num_pts2=n, rule=0, lo=0.85,
                                                             hi=0.95, thresh=1.0), a.iters, a.warmup)
            assert s.rt.tobytes() == p.rt.tobytes() and s.num_front == p.num_front
            we, wp = float(np.median(wall_e)), float(np.median(wall_p))
            cases["%d records, %d loops" % (n, LOOPS)] = {
                "register_epipolar_wall_us": round(we, 1),
                "register_pose_wall_us": round(wp, 1),
                "added_wall_us": round(wp - we, 1),
                "added_over_register_epipolar": round((wp - we) / we, 4),
                "estimate_pose_alone_wall_us": round(float(np.median(wall_s)), 1),
                "pose": {"num_candidates": p.num_candidates, "num_fit": p.num_fit, "num_front": p.num_front,
                         "votes": p.votes.tolist(), "sigma2_over_sigma1": round(float(p.sigma[1] / p.sigma[0]), 6)}}
            b1.free()
            b2.free()
    rec = {"tool": "tools/bench_pose.py", "unit": "microseconds per call (median wall time, the matcher included)",
           "iters": a.iters, "warmup": a.warmup, "seed": SEED, "cases": cases,
           "note": "register_epipolar is the parent's call and the yardstick; added_wall_us is the difference of two "
                   "medians of calls that take milliseconds, so it carries their run-to-run spread"}
    text = json.dumps(rec, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
