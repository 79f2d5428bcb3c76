#!/usr/bin/env python3
"""Timing record of guided matching on one MI355X: cusift_match_guided against cusift_match on the same record sets.

    python tools/bench_match_guided.py --out profiles/match_guided.json [--reps 30] [--warmup 5]
    python tools/bench_match_guided.py --regs-into profiles/match_guided.json      # needs hipcc, no GPU

Three routes, in the same process, interleaved repetition by repetition (A, H, F, A, H, F, ...), after `warmup` rounds
of all three:
  A  cusift_match(s1, s2)                      match_kernel, which this feature does not change
  H  cusift_match_guided under a homography    radius 56.4 px: about 1 % of the pairs pass
  F  cusift_match_guided under an F            radius 5 px from the epipolar line: about 1 % of the pairs pass
on n x n synthetic unit descriptors with coordinates uniform in a 1000 x 1000 image (two independent sets), L2 distance,
n = 4096 and 32768.  One repetition is `inner` back-to-back calls of the route between two stream synchronisations, timed
with the host clock and divided by `inner`, so that the figure is the device's time per call and not the launch latency.
Per route: median, min, 10th and 90th percentile; `spread_us` is p90 - p10 of that route's repetitions.  `H_over_A` and
`F_over_A` are ratios of medians; `share_passing` is counted on 512 rows with the definition restated in float64.  After
the timing each guided route is run once more at radius 1e6 and compared byte for byte with route A's records.
--regs-into adds VGPRs, LDS bytes and waves per SIMD of match_kernel and match_guided_kernel to a record, from
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
SIZES = ((4096, 10), (32768, 4))  # (n, inner calls per repetition)
FIELDS = ("score", "ambiguity", "match", "match_xpos", "match_ypos")
H_MODEL = np.array([1.01, 0.02, -15.0, -0.015, 0.99, 12.0, 1e-5, -8e-6, 1.0])
F_MODEL = np.array([0.0, 1e-6, -5e-4, -1e-6, 0.0, -1e-2, 5e-4, 1e-2, 0.05])  # near-horizontal lines through the image
ROUTES = {"H": ("homography", H_MODEL, 56.4), "F": ("epipolar", F_MODEL, 5.0)}


def unit_descriptors(capi, n, seed):
    rng = np.random.default_rng(seed)
    p = np.zeros(n, dtype=capi.SIFT_POINT_DTYPE)
    d = np.abs(rng.normal(size=(n, 128))).astype(np.float32)
    p["data"] = d / np.linalg.norm(d, axis=1, keepdims=True)
    p["coords2D"] = rng.uniform(0, 1000, (n, 2)).astype(np.float32)
    return p


def share_passing(kind, M, s1, s2, radius, rows=512):
    """The share of (row, column) pairs that pass, on the first `rows` rows, in float64 (a count, not the pinned test)."""
    x1 = np.c_[s1["coords2D"][:rows].astype(np.float64), np.ones(min(rows, len(s1)))] @ M.reshape(3, 3).T
    x2 = s2["coords2D"].astype(np.float64)
    if kind == "homography":
        p = x1[:, :2] / x1[:, 2:]
        d2 = (x2[None, :, 0] - p[:, None, 0]) ** 2 + (x2[None, :, 1] - p[:, None, 1]) ** 2
    else:
        l = x1 / np.hypot(x1[:, 0], x1[:, 1])[:, None]
        d2 = (l[:, None, 0] * x2[None, :, 0] + l[:, None, 1] * x2[None, :, 1] + l[:, None, 2]) ** 2
    return float((d2 < radius * radius).mean())


def stats(us):
    us = np.asarray(us)
    return {"median_us": round(float(np.median(us)), 1), "min_us": round(float(us.min()), 1),
            "p10_us": round(float(np.percentile(us, 10)), 1), "p90_us": round(float(np.percentile(us, 90)), 1),
            "spread_us": round(float(np.percentile(us, 90) - np.percentile(us, 10)), 1)}


def kernel_resources():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), "sift_match.hip", "match_kernel",
                          "match_guided_kernel"], capture_output=True, text=True, timeout=600)
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
            "tool": "tools/bench_match_guided.py", "cases": "not measured yet: no timed run of this tool is recorded"}
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
            d2 = capi.DeviceBuffer.from_numpy(ctx, s2)
            d1 = {r: capi.DeviceBuffer.from_numpy(ctx, s1) for r in ("A", "H", "F")}

            def route(r, radius=None):
                if r == "A":
                    ctx.match(d1[r].ptr, n, d2.ptr, n, 1)
                else:
                    kind, M, rad = ROUTES[r]
                    ctx.match_guided(d1[r].ptr, n, d2.ptr, n, kind, M, rad if radius is None else radius, 1)

            def once(r):
                ctx.synchronize()
                t0 = time.perf_counter()
                for _ in range(inner):
                    route(r)
                ctx.synchronize()
                return (time.perf_counter() - t0) * 1e6 / inner

            times = {r: [] for r in d1}
            for i in range(a.warmup + a.reps):
                for r in ("A", "H", "F"):
                    t = once(r)
                    if i >= a.warmup:
                        times[r].append(t)
            plain = d1["A"].to_numpy(capi.SIFT_POINT_DTYPE, n)
            st = {r: stats(times[r]) for r in times}
            flop = 2.0 * n * n * 128
            case = {"inner_calls_per_repetition": inner,
                    "A_match": dict(st["A"], tflops=round(flop / st["A"]["median_us"] / 1e6, 1))}
            for r in ("H", "F"):
                kind, M, rad = ROUTES[r]
                guided = d1[r].to_numpy(capi.SIFT_POINT_DTYPE, n)
                route(r, 1e6)
                ctx.synchronize()
                wide = d1[r].to_numpy(capi.SIFT_POINT_DTYPE, n)
                case["%s_match_guided_%s" % (r, kind)] = dict(
                    st[r], tflops=round(flop / st[r]["median_us"] / 1e6, 1), radius=rad,
                    share_passing=round(share_passing(kind, M, s1, s2, rad), 4),
                    rows_matched=int((guided["match"] >= 0).sum()),
                    rows_that_kept_the_unguided_match=int((guided["match"] == plain["match"]).sum()),
                    radius_1e6_bytes_equal_route_A=all(wide[f].tobytes() == plain[f].tobytes() for f in FIELDS))
                case["%s_over_A" % r] = round(st[r]["median_us"] / st["A"]["median_us"], 3)
            cases["%d x %d" % (n, n)] = case
            for b in list(d1.values()) + [d2]:
                b.free()
    rec = {"tool": "tools/bench_match_guided.py", "unit": "microseconds per call of the route (host clock around `inner` "
           "calls between two stream synchronisations, divided by `inner`)", "reps": a.reps, "warmup": a.warmup,
           "distance": "L2", "cases": cases}
    text = json.dumps(rec, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
