#!/usr/bin/env python3
"""Timing record of matching by projection on one MI355X: cusift_match_projected against cusift_match and against
cusift_match_guided under a homography, on the same record sets.

    python tools/bench_match_projected.py --out profiles/match_projected.json [--reps 30] [--warmup 5]
    python tools/bench_match_projected.py --regs-into profiles/match_projected.json      # needs hipcc, no GPU

Three routes, in the same process, interleaved repetition by repetition (A, H, P, A, H, P, ...), after `warmup` rounds
of all three:
  A  cusift_match(s1, s2)                      match_kernel
  H  cusift_match_guided under a homography    radius 56.4 px: about 1 % of the pairs pass
  P  cusift_match_projected under a pose       radius 56.4 px around the projection of coords3D: about 1 % of the pairs pass
on n x n synthetic unit descriptors with coordinates uniform in a 1000 x 1000 image (two independent sets; tools/
bench_match_guided.py's), set 1's coords3D its own pixel back-projected at a depth of 2 to 6, L2 distance, n = 4096 and
32768.  One repetition is `inner` back-to-back calls of the route between two stream synchronisations, timed with the host
clock and divided by `inner`.  Per route: median, min, 10th and 90th percentile; `spread_us` is p90 - p10 of that route's
repetitions.  `H_over_A`, `P_over_A` and `P_over_H` are ratios of medians; `P_above_H_by_more_than_the_spreads` says whether
P's median stands above H's by more than the two routes' p90 - p10 together.  `share_passing` is counted on 512 rows in
float64.  After the timing route P is run once more at radius 1e6 and compared byte for byte with route A's records.
The expectation to read the record against is the H guide's ratio to cusift_match in profiles/match_guided.json (1.05 at
4,096, 1.03 at 32,768): the per-pair work is identical, only the per-row prologue differs.
--regs-into adds VGPRs, LDS bytes and waves per SIMD of the projected kernels to a record, from tools/kernel_regs.py (a
compile, no run).
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_match_guided import FIELDS, H_MODEL, SIZES, share_passing, stats, unit_descriptors  # noqa: E402

RADIUS = 56.4
CAM = (800.0, 800.0, 500.0, 500.0, 0.0)  # fx, fy, cx, cy, origin
POSE = np.array([0.9995, -0.015, -0.03, 0.05, 0.0152, 0.9998, 0.02, -0.03, 0.0297, -0.0204, 0.9993, 0.04])


def lift(s1, seed):
    """coords3D of every record: its own pixel back-projected at a depth of 2 to 6."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(2.0, 6.0, len(s1))
    xy = s1["coords2D"].astype(np.float64)
    s1["coords3D"] = np.stack([(xy[:, 0] - CAM[2]) / CAM[0] * z, (xy[:, 1] - CAM[3]) / CAM[1] * z, z], axis=1)
    return s1


def share_projected(s1, s2, radius, rows=512):
    """The share of (row, column) pairs that pass, on the first `rows` rows, in float64 (a count, not the pinned test)."""
    R, t = POSE.reshape(3, 4)[:, :3], POSE.reshape(3, 4)[:, 3]
    X2 = (s1["coords3D"][:rows].astype(np.float64) - t) @ R
    p = np.stack([CAM[0] * X2[:, 0] / X2[:, 2] + CAM[2], CAM[1] * X2[:, 1] / X2[:, 2] + CAM[3]], axis=1)
    x2 = s2["coords2D"].astype(np.float64)
    d2 = (x2[None, :, 0] - p[:, None, 0]) ** 2 + (x2[None, :, 1] - p[:, None, 1]) ** 2
    return float(((d2 < radius * radius) & (X2[:, 2:] > 0)).mean())


def kernel_resources():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), "sift_match_project.hip"],
                         capture_output=True, text=True, timeout=600)
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
            "tool": "tools/bench_match_projected.py", "cases": "not measured yet: no timed run of this tool is recorded"}
        rec["kernel_resources"] = kernel_resources()
        with open(a.regs_into, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
        print(json.dumps(rec["kernel_resources"], indent=1))
        return
    assert a.reps >= 20 and a.warmup >= 3
    from cusift_amd import capi

    cam = capi.Camera(*CAM)
    cases = {}
    with capi.Context(0) as ctx:
        for n, inner in SIZES:
            s1, s2 = lift(unit_descriptors(capi, n, 5), 7), unit_descriptors(capi, n, 6)
            d2 = capi.DeviceBuffer.from_numpy(ctx, s2)
            d1 = {r: capi.DeviceBuffer.from_numpy(ctx, s1) for r in ("A", "H", "P")}

            def route(r, radius=RADIUS):
                if r == "A":
                    ctx.match(d1[r].ptr, n, d2.ptr, n, 1)
                elif r == "H":
                    ctx.match_guided(d1[r].ptr, n, d2.ptr, n, "homography", H_MODEL, radius, 1)
                else:
                    ctx.match_projected(d1[r].ptr, n, d2.ptr, n, POSE, cam, radius, 1)

            def once(r):
                ctx.synchronize()
                t0 = time.perf_counter()
                for _ in range(inner):
                    route(r)
                ctx.synchronize()
                return (time.perf_counter() - t0) * 1e6 / inner

            times = {r: [] for r in d1}
            for i in range(a.warmup + a.reps):
                for r in ("A", "H", "P"):
                    t = once(r)
                    if i >= a.warmup:
                        times[r].append(t)
            plain = d1["A"].to_numpy(capi.SIFT_POINT_DTYPE, n)
            projected = d1["P"].to_numpy(capi.SIFT_POINT_DTYPE, n)
            route("P", 1e6)
            ctx.synchronize()
            wide = d1["P"].to_numpy(capi.SIFT_POINT_DTYPE, n)
            st = {r: stats(times[r]) for r in times}
            flop = 2.0 * n * n * 128
            case = {"inner_calls_per_repetition": inner,
                    "A_match": dict(st["A"], tflops=round(flop / st["A"]["median_us"] / 1e6, 1)),
                    "H_match_guided_homography": dict(
                        st["H"], tflops=round(flop / st["H"]["median_us"] / 1e6, 1), radius=RADIUS,
                        share_passing=round(share_passing("homography", H_MODEL, s1, s2, RADIUS), 4)),
                    "P_match_projected": dict(
                        st["P"], tflops=round(flop / st["P"]["median_us"] / 1e6, 1), radius=RADIUS,
                        share_passing=round(share_projected(s1, s2, RADIUS), 4),
                        rows_matched=int((projected["match"] >= 0).sum()),
                        rows_that_kept_the_unguided_match=int((projected["match"] == plain["match"]).sum()),
                        radius_1e6_bytes_equal_route_A=all(wide[f].tobytes() == plain[f].tobytes() for f in FIELDS)),
                    "H_over_A": round(st["H"]["median_us"] / st["A"]["median_us"], 3),
                    "P_over_A": round(st["P"]["median_us"] / st["A"]["median_us"], 3),
                    "P_over_H": round(st["P"]["median_us"] / st["H"]["median_us"], 3),
                    "P_above_H_by_more_than_the_spreads":
                        bool(st["P"]["median_us"] - st["H"]["median_us"] > st["P"]["spread_us"] + st["H"]["spread_us"])}
            cases["%d x %d" % (n, n)] = case
            for b in list(d1.values()) + [d2]:
                b.free()
    rec = {"tool": "tools/bench_match_projected.py", "unit": "microseconds per call of the route (host clock around "
           "`inner` calls between two stream synchronisations, divided by `inner`)", "reps": a.reps, "warmup": a.warmup,
           "distance": "L2", "cases": cases}
    text = json.dumps(rec, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
