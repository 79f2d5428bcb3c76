#!/usr/bin/env python3
"""Timing record of 8-bit guided matching on one MI355X: cusift_match8_guided / cusift_match8_projected against cusift_match8
(what the predicate costs) and against the fp32 calls cusift_match_guided / cusift_match_projected (what a caller would
otherwise run), on the same record sets.

    python tools/bench_match8_guided.py --out profiles/match8_guided.json [--reps 30] [--warmup 5]
    python tools/bench_match8_guided.py --regs-into profiles/match8_guided.json          # needs hipcc, no GPU
    python tools/bench_match8_guided.py --trace-into profiles/match8_guided.json --trace-csv kernel_stats.csv

Seven routes, in the same process, interleaved repetition by repetition, after `warmup` rounds of all seven:
  M8   cusift_match8(s1, s2)                     the parent's unguided call
  H8   cusift_match8_guided under a homography   radius 56.4 px: about 1 % of the pairs pass
  F8   cusift_match8_guided under an F           radius 5 px from the epipolar line: about 1 % of the pairs pass
  P8   cusift_match8_projected under a pose      radius 56.4 px around the projection of coords3D: about 1 %
  H32, F32, P32   cusift_match_guided / cusift_match_projected, the same models and radii on the float descriptors
on tools/bench_match_guided.py's records -- n x n synthetic unit descriptors, coordinates uniform in a 1000 x 1000 image,
two independent sets, coords3D the records' own pixels at depths of 2 to 6 -- quantised once with
cusift_quantize_descriptors, L2 distance, n = 4096 and 32768.  One repetition is `inner` back-to-back calls of the route
between two stream synchronisations, timed with the host clock and divided by `inner`.  Per route: median, min, 10th and
90th percentile; `spread_us` is p90 - p10 of that route's repetitions.  The ratios are ratios of medians;
`below_fp32_by_more_than_both_spreads` says whether the 8-bit route's median lies below the fp32 route's by more than the
sum of the two routes' p90 - p10.  After the timing each guided 8-bit route is run once more at radius 1e6 and compared
byte for byte with route M8's records.
--regs-into adds registers, LDS bytes and waves per SIMD of the guided kernels (sift_match8_guided.hip), from
tools/kernel_regs.py (a compile, no run); --trace-into adds per-kernel times from the kernel_stats CSV of a
`rocprofv3 --kernel-trace --stats` run of this tool, a run of its own.
A record, not an assertion.  The C ABI only, no torch.
"""
import argparse
import csv
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_match_guided import F_MODEL, FIELDS, H_MODEL, share_passing, stats, unit_descriptors  # noqa: E402

SIZES = ((4096, 10), (32768, 4))  # (n, inner calls per repetition)
CAM = (1000.0, 1000.0, 500.0, 500.0, 0.0)
POSE = np.array([1.0, 0.0, 0.0, 0.02, 0.0, 1.0, 0.0, -0.01, 0.0, 0.0, 1.0, 0.03])  # [I | t]: a small translation
RADII = {"H": 56.4, "F": 5.0, "P": 56.4}
ORDER = ("M8", "H8", "F8", "P8", "H32", "F32", "P32")


def lifted(p, seed):
    """coords3D: every record's own pixel back-projected at a depth of 2 to 6."""
    z = np.random.default_rng(seed).uniform(2.0, 6.0, len(p))
    xy = p["coords2D"].astype(np.float64)
    p["coords3D"] = np.c_[(xy[:, 0] - CAM[2]) / CAM[0] * z, (xy[:, 1] - CAM[3]) / CAM[1] * z, z].astype(np.float32)
    return p


def share_projected(s1, s2, radius, rows=512):
    X = s1["coords3D"][:rows].astype(np.float64) - POSE.reshape(3, 4)[:, 3]
    Y = X @ POSE.reshape(3, 4)[:, :3]  # R^T (X - t), row-wise
    q = np.c_[CAM[0] * Y[:, 0] / Y[:, 2] + CAM[2], CAM[1] * Y[:, 1] / Y[:, 2] + CAM[3]]
    x2 = s2["coords2D"].astype(np.float64)
    d2 = (x2[None, :, 0] - q[:, None, 0]) ** 2 + (x2[None, :, 1] - q[:, None, 1]) ** 2
    return float((d2 < radius * radius).mean())


def kernel_resources():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), "sift_match8_guided.hip",
                          "match8_guided_kernel", "match8_batch_guided_kernel"], capture_output=True, text=True, timeout=600)
    rows = {}
    lines = out.stdout.splitlines()
    head = lines[0].split() if lines else []
    for line in lines[1:]:
        cells = line.split()
        if len(cells) == len(head):
            rows[cells[0]] = {k: int(v) for k, v in zip(head[1:], cells[1:])}
    return rows


def kernel_trace(path):
    """{kernel: calls, shortest, longest and total microseconds} of the matchers' kernels in a rocprofv3 kernel_stats CSV.
    A kernel's calls cover both sizes: the shortest is a call at 4,096 records a side, the longest one at 32,768."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            if "match" in name:
                out[name.split("(")[0]] = {"calls": int(row["Calls"]),
                                           "min_us": round(float(row["MinNs"]) / 1e3, 1),
                                           "max_us": round(float(row["MaxNs"]) / 1e3, 1),
                                           "total_us": round(float(row["TotalDurationNs"]) / 1e3, 1)}
    return out


def merge_into(path, key, value):
    rec = json.load(open(path)) if os.path.exists(path) else {
        "tool": "tools/bench_match8_guided.py", "cases": "not measured yet: no timed run of this tool is recorded"}
    rec[key] = value
    with open(path, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(value, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--regs-into", default=None, help="add the kernels' registers and LDS to this record (needs hipcc)")
    ap.add_argument("--trace-into", default=None, help="add per-kernel times from --trace-csv to this record")
    ap.add_argument("--trace-csv", default=None, help="the kernel_stats CSV of a rocprofv3 --kernel-trace --stats run")
    a = ap.parse_args()
    if a.regs_into:
        return merge_into(a.regs_into, "kernel_resources", kernel_resources())
    if a.trace_into:
        return merge_into(a.trace_into, "kernel_trace", kernel_trace(a.trace_csv))
    assert a.reps >= 3 and a.warmup >= 1
    from cusift_amd import capi

    cam = capi.Camera(*CAM)
    cases = {}
    with capi.Context(0) as ctx:
        for n, inner in SIZES:
            s1, s2 = lifted(unit_descriptors(capi, n, 5), 7), lifted(unit_descriptors(capi, n, 6), 8)
            d2 = capi.DeviceBuffer.from_numpy(ctx, s2)
            d1 = {r: capi.DeviceBuffer.from_numpy(ctx, s1) for r in ORDER}
            tab = [capi.DeviceBuffer(ctx, n * k) for _ in range(2) for k in (128, 8)]
            ctx.quantize_descriptors(d1["M8"].ptr, n, tab[0].ptr, tab[1].ptr)
            ctx.quantize_descriptors(d2.ptr, n, tab[2].ptr, tab[3].ptr)

            def route(r, radius=None):
                rad = RADII.get(r[0]) if radius is None else radius
                if r == "M8":
                    ctx.match8(d1[r].ptr, n, tab[0].ptr, tab[1].ptr, d2.ptr, n, tab[2].ptr, tab[3].ptr, 1)
                elif r == "P8":
                    ctx.match8_projected(d1[r].ptr, n, tab[0].ptr, tab[1].ptr, d2.ptr, n, tab[2].ptr, tab[3].ptr, POSE, cam,
                                         rad, 1)
                elif r == "P32":
                    ctx.match_projected(d1[r].ptr, n, d2.ptr, n, POSE, cam, rad, 1)
                else:
                    kind, M = ("homography", H_MODEL) if r[0] == "H" else ("epipolar", F_MODEL)
                    if r.endswith("8"):
                        ctx.match8_guided(d1[r].ptr, n, tab[0].ptr, tab[1].ptr, d2.ptr, n, tab[2].ptr, tab[3].ptr, kind, M,
                                          rad, 1)
                    else:
                        ctx.match_guided(d1[r].ptr, n, d2.ptr, n, kind, M, rad, 1)

            def once(r):
                ctx.synchronize()
                t0 = time.perf_counter()
                for _ in range(inner):
                    route(r)
                ctx.synchronize()
                return (time.perf_counter() - t0) * 1e6 / inner

            times = {r: [] for r in ORDER}
            for i in range(a.warmup + a.reps):
                for r in ORDER:
                    t = once(r)
                    if i >= a.warmup:
                        times[r].append(t)
            st = {r: stats(times[r]) for r in ORDER}
            plain = d1["M8"].to_numpy(capi.SIFT_POINT_DTYPE, n)
            shares = {"H": share_passing("homography", H_MODEL, s1, s2, RADII["H"]),
                      "F": share_passing("epipolar", F_MODEL, s1, s2, RADII["F"]), "P": share_projected(s1, s2, RADII["P"])}
            case = {"inner_calls_per_repetition": inner, "M8_match8": st["M8"]}
            for g in ("H", "F", "P"):
                r8, r32 = g + "8", g + "32"
                guided = d1[r8].to_numpy(capi.SIFT_POINT_DTYPE, n)
                route(r8, 1e6)
                ctx.synchronize()
                wide = d1[r8].to_numpy(capi.SIFT_POINT_DTYPE, n)
                case[r8] = dict(st[r8], radius=RADII[g], share_passing=round(shares[g], 4),
                                rows_matched=int((guided["match"] >= 0).sum()),
                                radius_1e6_bytes_equal_route_M8=all(wide[f].tobytes() == plain[f].tobytes() for f in FIELDS))
                case[r32] = st[r32]
                case["%s_over_M8" % r8] = round(st[r8]["median_us"] / st["M8"]["median_us"], 3)
                case["%s_over_%s" % (r8, r32)] = round(st[r8]["median_us"] / st[r32]["median_us"], 3)
                case["%s_below_fp32_by_more_than_both_spreads" % r8] = bool(
                    st[r32]["median_us"] - st[r8]["median_us"] > st[r8]["spread_us"] + st[r32]["spread_us"])
            cases["%d x %d" % (n, n)] = case
            for b in list(d1.values()) + [d2] + tab:
                b.free()
    rec = {"tool": "tools/bench_match8_guided.py", "unit": "microseconds per call of the route (host clock around `inner` "
           "calls between two stream synchronisations, divided by `inner`)", "reps": a.reps, "warmup": a.warmup,
           "distance": "L2", "cases": cases}
    text = json.dumps(rec, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
