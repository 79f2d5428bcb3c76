#!/usr/bin/env python3
"""Timing record of the planar registration on one MI355X: the fused device-resident call against the route the
previous revision offered through the same C ABI, on planted sets (tests/test_homography.py's construction: a known
homography, 0.3 px noise, 40 % gross outliers) of 650, 8,000 and 32,768 records with 1,008 and 10,000 hypotheses.

    python tools/bench_planar.py --route fused  --out fused.json   [--iters 30] [--warmup 5]
    python tools/bench_planar.py --route parent --out parent.json
    python tools/bench_planar.py --route kernels --pts 8000 --loops 10000      # under a kernel trace, see below
    python tools/bench_planar.py --merge fused.json parent.json [--kernel-stats DIR] --out profiles/planar_registration.json

One route per process, so that each runs under a time limit of its own.
  fused   cusift_estimate_homography: candidates, samples drawn on the device, hypotheses, counts, selection, five
          rounds of refit, match_error; one synchronisation, at the read-back
  parent  what include/homography.h's FindHomography + ImproveHomography do: two strided device-to-host copies (score,
          ambiguity), the host filter, four distinct samples per hypothesis drawn on the host, cusift_find_homography
          (upload, three launches, read-back), a device-to-host copy of all records, five rounds of the weighted normal
          equations on the host.  The host arithmetic here is vectorised numpy, NOT the header's scalar C++ loop: the
          record says so and the two must not be confused
  kernels both routes a few times for ONE size, meant to run under `rocprofv3 --kernel-trace --stats -d DIR -o NAME
          --output-format csv -- python tools/bench_planar.py --route kernels ...`: the trace then holds the average
          duration of planar_score_kernel (the fused call's scoring) and of homography_test_kernel (the previous
          revision's, still behind cusift_find_homography) over the same points and hypotheses; --merge reads the
          *kernel_stats.csv files under --kernel-stats
Both routes start from records already on the device.  `wall_us` is the median over `iters` calls after `warmup` calls of
the whole route as the caller sees it.  A record, not an assertion.  The C ABI only, no torch.
"""
import argparse
import csv
import glob
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = ((390, 260), (4800, 3200), (19661, 13107))  # 650, 8,000 and 32,768 records, 60 % planted
LOOPS = (1008, 10000)
SEED = 7


def planted(capi, n_in, n_out, seed=3, noise=0.3):
    rng = np.random.default_rng(seed)
    H = np.array([[0.92, -0.11, 37.0], [0.08, 1.05, -21.0], [2.1e-5, -3.4e-5, 1.0]])
    n = n_in + n_out
    pts = np.zeros(n, dtype=capi.SIFT_POINT_DTYPE)
    xy = rng.uniform([0, 0], [1280, 960], size=(n, 2))
    proj = np.c_[xy, np.ones(n)] @ H.T
    proj = proj[:, :2] / proj[:, 2:]
    proj[:n_in] += rng.normal(0, noise, size=(n_in, 2))
    proj[n_in:] = rng.uniform([0, 0], [1280, 960], size=(n_out, 2))
    perm = rng.permutation(n)
    pts["coords2D"] = xy[perm].astype(np.float32)
    pts["match_xpos"] = proj[perm, 0].astype(np.float32)
    pts["match_ypos"] = proj[perm, 1].astype(np.float32)
    pts["score"], pts["ambiguity"] = 0.9, 0.5
    return pts


def host_samples(rng, n_valid, loops):
    s = rng.integers(0, n_valid, size=(4, loops))
    for slot in (1, 2, 3):
        while True:
            clash = (s[slot][None, :] == s[:slot]).any(axis=0)
            if not clash.any():
                break
            s[slot, clash] = rng.integers(0, n_valid, size=int(clash.sum()))
    return s


def host_improve(pts, hom, loops, lo, hi, thresh):
    limit = np.float32(thresh) * np.float32(thresh)
    sub = pts[~((pts["score"] < lo) | (pts["ambiguity"] > hi))]
    px, py, mx, my = sub["coords2D"][:, 0], sub["coords2D"][:, 1], sub["match_xpos"], sub["match_ypos"]
    Yx = np.zeros((len(sub), 8))
    Yy = np.zeros((len(sub), 8))
    Yx[:, 0], Yx[:, 1], Yx[:, 2], Yx[:, 6], Yx[:, 7] = px, py, 1.0, -(px * mx), -(py * mx)
    Yy[:, 3], Yy[:, 4], Yy[:, 5], Yy[:, 6], Yy[:, 7] = px, py, 1.0, -(px * my), -(py * my)
    A = hom[:8].astype(np.float64)

    def err_of(p, A):
        den = (A[6] * p["coords2D"][:, 0] + A[7] * p["coords2D"][:, 1] + 1.0).astype(np.float32)
        dx = ((A[0] * p["coords2D"][:, 0] + A[1] * p["coords2D"][:, 1] + A[2]) / den - p["match_xpos"]).astype(np.float32)
        dy = ((A[3] * p["coords2D"][:, 0] + A[4] * p["coords2D"][:, 1] + A[5]) / den - p["match_ypos"]).astype(np.float32)
        return dx * dx + dy * dy

    for _ in range(loops):
        wei = (limit / (err_of(sub, A) + limit)).astype(np.float64)
        M = (Yx * wei[:, None]).T @ Yx + (Yy * wei[:, None]).T @ Yy
        X = (Yx * wei[:, None]).T @ mx.astype(np.float64) + (Yy * wei[:, None]).T @ my.astype(np.float64)
        try:
            L = np.linalg.cholesky(M)
            A = np.linalg.solve(L.T, np.linalg.solve(L, X))
        except np.linalg.LinAlgError:
            pass
    err = err_of(pts, A)
    pts["match_error"] = np.sqrt(err)
    return np.r_[A, 1.0].astype(np.float32), int((err < limit).sum())


def make_routes(capi, ctx, pts, loops):
    lib = capi.lib()
    n = len(pts)
    buf = capi.DeviceBuffer.from_numpy(ctx, pts)
    host = pts.copy()
    score, amb = np.zeros(n, np.float32), np.zeros(n, np.float32)
    off_s, off_a = capi.SIFT_POINT_DTYPE.fields["score"][1], capi.SIFT_POINT_DTYPE.fields["ambiguity"][1]
    rng = np.random.default_rng(SEED)

    def fused():
        r = ctx.estimate_homography(buf.ptr, n, -1, rule=0, lo=0.0, hi=0.8, loops=loops, thresh=5.0, refine_loops=5,
                                    refine_thresh=3.0, seed=SEED)
        return r.homography, r.num_matches, r.num_fit

    def parent():
        capi.check(lib.cusift_memcpy2d_d2h(ctx.handle, score.ctypes.data, 4, buf.ptr + off_s, 588, 4, n))
        capi.check(lib.cusift_memcpy2d_d2h(ctx.handle, amb.ctypes.data, 4, buf.ptr + off_a, 588, 4, n))
        valid = np.flatnonzero((score > 0.0) & (amb < 0.8)).astype(np.int32)
        rand_pts = valid[host_samples(rng, len(valid), loops)]
        hom, n_match = ctx.find_homography(buf.ptr, n, rand_pts, thresh=5.0)
        capi.check(lib.cusift_memcpy_d2h(ctx.handle, host.ctypes.data, buf.ptr, 588 * n))
        hom, n_fit = host_improve(host, hom, 5, np.float32(0.0), np.float32(0.8), 3.0)
        return hom, n_match, n_fit

    return fused, parent, buf


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


def kernel_stats(directory):
    """{kernel name fragment: average ns} per (pts, loops) from the *kernel_stats.csv files of the traced runs, whose
    names carry _<pts>_<loops>."""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)):
        m = re.search(r"_(\d+)_(\d+)_kernel_stats\.csv$", os.path.basename(path))
        if not m:
            continue
        row = {}
        for r in csv.DictReader(open(path)):
            for needle in ("planar_score_kernel", "homography_test_kernel", "planar_select_kernel",
                           "homography_solve_kernel"):
                if needle in r.get("Name", ""):
                    row[needle + "_avg_us"] = round(float(r["AverageNs"]) / 1e3, 2)
                    row[needle + "_calls"] = int(r["Calls"])
        out["%s records, %s loops" % (m.group(1), m.group(2))] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=("fused", "parent", "kernels"))
    ap.add_argument("--merge", nargs="+")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pts", type=int, default=8000)
    ap.add_argument("--loops", type=int, default=10000)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.merge:
        rec = {"tool": "tools/bench_planar.py", "unit": "microseconds per registration (median wall time of the call)",
               "routes": {}}
        for path in a.merge:
            piece = json.load(open(path))
            rec["routes"][piece["route"]] = piece
        if a.kernel_stats:
            rec["scoring_kernels"] = kernel_stats(a.kernel_stats)
        f, p = rec["routes"].get("fused"), rec["routes"].get("parent")
        if f and p:
            rec["speedup_parent_over_fused"] = {k: round(p["cases"][k]["wall_us"] / f["cases"][k]["wall_us"], 2)
                                                for k in f["cases"] if k in p["cases"]}
        text = json.dumps(rec, indent=1)
    else:
        assert a.route and a.iters >= 20 and a.warmup >= 5
        from cusift_amd import capi

        with capi.Context(0) as ctx:
            if a.route == "kernels":
                n_in = int(round(a.pts * 0.6))
                pts = planted(capi, n_in, a.pts - n_in)
                fused, parent, buf = make_routes(capi, ctx, pts, a.loops)
                for _ in range(12):
                    fused()
                    parent()
                ctx.synchronize()
                print(json.dumps({"route": "kernels", "pts": a.pts, "loops": a.loops}))
                return
            cases = {}
            for n_in, n_out in SIZES:
                pts = planted(capi, n_in, n_out)
                for loops in LOOPS:
                    fused, parent, buf = make_routes(capi, ctx, pts, loops)
                    wall, (hom, n_match, n_fit) = timed(ctx, fused if a.route == "fused" else parent, a.iters, a.warmup)
                    cases["%d records, %d loops" % (len(pts), loops)] = {
                        "wall_us": round(float(np.median(wall)), 1), "wall_us_min": round(float(np.min(wall)), 1),
                        "wall_us_p90": round(float(np.percentile(wall, 90)), 1), "num_matches": int(n_match),
                        "num_fit": int(n_fit), "homography": [round(float(v), 6) for v in hom]}
        rec = {"tool": "tools/bench_planar.py", "route": a.route, "iters": a.iters, "warmup": a.warmup, "seed": SEED,
               "host_arithmetic": "vectorised numpy (filter, sampling, refit), not the C++ header's scalar loops"
               if a.route == "parent" else "none", "cases": cases}
        text = json.dumps(rec, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
