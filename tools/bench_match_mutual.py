#!/usr/bin/env python3
"""Timing record of mutual matching on one MI355X: both directions from one pass against the matcher called twice.

    python tools/bench_match_mutual.py --out profiles/match_mutual.json [--reps 30] [--warmup 5]
    python tools/bench_match_mutual.py --regs-into profiles/match_mutual.json      # needs hipcc, no GPU

Two routes, in the same process, interleaved repetition by repetition (A, B, A, B, ...), after `warmup` rounds of both:
  A  cusift_match(s1, s2) followed by cusift_match(s2, s1): what a caller had to do for a cross-check before
     cusift_match_mutual existed (match_kernel is unchanged, so A is also the previous revision's figure)
  B  one cusift_match_mutual(s1, s2)
on n x n synthetic unit descriptors (bench_legs/match.py's construction, two independent sets), L2 distance, n = 4096
and 16384.  One repetition is `inner` back-to-back calls of the route between two stream synchronisations, timed with
the host clock and divided by `inner`, so that the figure is the device's time per call and not the launch latency.
Per route: median, min, 10th and 90th percentile; `spread_us` is p90 - p10 of that route's repetitions.  The claim to
confirm is B < A by more than A's spread; `b_faster_by_more_than_spread` says whether it held.  After the timing the
results of both routes are compared (the row side byte for byte; the column side's score and ambiguity against the reverse
call).  --regs-into adds VGPRs, LDS bytes and waves per SIMD of match_kernel and match_mutual_kernel to a record, from
tools/kernel_regs.py (a compile, no run).
A record, not an assertion.  The C ABI only, no torch.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = ((4096, 10), (16384, 4))  # (n, inner calls per repetition)
FIELDS = ("score", "ambiguity", "match", "match_xpos", "match_ypos")


def unit_descriptors(capi, n, seed):
    rng = np.random.default_rng(seed)
    p = np.zeros(n, dtype=capi.SIFT_POINT_DTYPE)
    d = np.abs(rng.normal(size=(n, 128))).astype(np.float32)
    p["data"] = d / np.linalg.norm(d, axis=1, keepdims=True)
    p["coords2D"] = rng.uniform(0, 1000, (n, 2)).astype(np.float32)
    return p


def stats(us):
    us = np.asarray(us)
    return {"median_us": round(float(np.median(us)), 1), "min_us": round(float(us.min()), 1),
            "p10_us": round(float(np.percentile(us, 10)), 1), "p90_us": round(float(np.percentile(us, 90)), 1),
            "spread_us": round(float(np.percentile(us, 90) - np.percentile(us, 10)), 1)}


def kernel_resources():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), "sift_match.hip", "match_kernel",
                          "match_mutual_kernel"], capture_output=True, text=True, timeout=600)
    rows = {}
    lines = out.stdout.splitlines()
    head = lines[0].split() if lines else []
    for line in lines[1:]:
        cells = line.split()
        if len(cells) == len(head):
            rows[cells[0]] = {k: int(v) for k, v in zip(head[1:], cells[1:])}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--regs-into", default=None, help="add the kernels' VGPRs and LDS to this record (needs hipcc)")
    a = ap.parse_args()
    if a.regs_into:
        rec = json.load(open(a.regs_into)) if os.path.exists(a.regs_into) else {
            "tool": "tools/bench_match_mutual.py", "cases": "not measured yet: no timed run of this tool is recorded"}
        rec["kernel_resources"] = kernel_resources()
        with open(a.regs_into, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
        print(json.dumps(rec["kernel_resources"], indent=1))
        return
    assert a.reps >= 20 and a.warmup >= 3
    from cusift_amd import capi

    cases = {}
    with capi.Context(0) as ctx:
        for n, inner in SIZES:
            s1, s2 = unit_descriptors(capi, n, 5), unit_descriptors(capi, n, 6)
            a1, a2 = capi.DeviceBuffer.from_numpy(ctx, s1), capi.DeviceBuffer.from_numpy(ctx, s2)
            b1, b2 = capi.DeviceBuffer.from_numpy(ctx, s1), capi.DeviceBuffer.from_numpy(ctx, s2)

            def route_a():
                ctx.match(a1.ptr, n, a2.ptr, n, 1)
                ctx.match(a2.ptr, n, a1.ptr, n, 1)

            def route_b():
                ctx.match_mutual(b1.ptr, n, b2.ptr, n, 1)

            def once(fn):
                ctx.synchronize()
                t0 = time.perf_counter()
                for _ in range(inner):
                    fn()
                ctx.synchronize()
                return (time.perf_counter() - t0) * 1e6 / inner

            ta, tb = [], []
            for i in range(a.warmup + a.reps):
                x, y = once(route_a), once(route_b)
                if i >= a.warmup:
                    ta.append(x)
                    tb.append(y)
            ra1, ra2 = a1.to_numpy(capi.SIFT_POINT_DTYPE, n), a2.to_numpy(capi.SIFT_POINT_DTYPE, n)
            rb1, rb2 = b1.to_numpy(capi.SIFT_POINT_DTYPE, n), b2.to_numpy(capi.SIFT_POINT_DTYPE, n)
            sa, sb = stats(ta), stats(tb)
            flop = 2.0 * n * n * 128
            cases["%d x %d" % (n, n)] = {
                "inner_calls_per_repetition": inner,
                "A_match_twice": dict(sa, tflops=round(2 * flop / sa["median_us"] / 1e6, 1)),
                "B_match_mutual": dict(sb, tflops_of_one_pass=round(flop / sb["median_us"] / 1e6, 1)),
                "B_over_A": round(sb["median_us"] / sa["median_us"], 3),
                "b_faster_by_more_than_spread": bool(sa["median_us"] - sb["median_us"] > sa["spread_us"]),
                "row_side_bytes_equal": all(ra1[f].tobytes() == rb1[f].tobytes() for f in FIELDS),
                "column_side_score_and_ambiguity_equal_the_reverse_call":
                    all(ra2[f].tobytes() == rb2[f].tobytes() for f in ("score", "ambiguity")),
                "column_side_match_differs_on": int((ra2["match"] != rb2["match"]).sum()),
            }
            for b in (a1, a2, b1, b2):
                b.free()
    rec = {"tool": "tools/bench_match_mutual.py", "unit": "microseconds per call of the route (host clock around `inner` "
           "calls between two stream synchronisations, divided by `inner`)", "reps": a.reps, "warmup": a.warmup,
           "distance": "L2", "cases": cases}
    text = json.dumps(rec, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
