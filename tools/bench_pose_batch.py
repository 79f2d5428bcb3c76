#!/usr/bin/env python3
"""Wall time of the calibrated pose of a 64-frame sequence on one MI355X, both routes in one process, alternating:

    batch   cusift_register_pose_batch over the 63 consecutive pairs: one call, one synchronisation, no count read back
    loop    cusift_register_pose(i, i + 1) for the same pairs with seed + i: one synchronisation per pair

    python tools/bench_pose_batch.py [--out profiles/pose_batch.json] [--reps 10] [--warmup 2] [--sizes 4096 8192]
    python tools/bench_pose_batch.py --kernel-trace TRACE.csv [--out ...]      # adds `kernels` to the record at --out

The sequence is tools/bench_epipolar.py's planted scene (two 1280 x 960 views of a non-planar scene, 0.3 px of noise, 40 %
gross outliers, f = 1000 at (640, 480)) as 64 frames: the even frames are its first view, the odd frames its second, so
every consecutive pair sees the planted geometry, in alternating directions.  4,096 and 8,192 records per frame, 10,000
hypotheses and five refit rounds per pair, dot-product distance, rule 0.  The timed region of a route is the whole route as
the caller sees it, the matcher included, from device-resident records to the 63 poses on the host.  The routes alternate
repetition by repetition after --warmup repetitions of each; the record holds the median, the 10th and the 90th percentile
of each route and the ratio of the medians.  The routes compute the same thing: the record counts the pairs whose [R | t]
has the same bits in both (the matcher's one licence to differ is an exactly tied score).  A record, not an assertion.  The
C ABI only, no torch.
--kernel-trace: the *_kernel_trace.csv of a run of this tool under `rocprofv3 --kernel-trace --stats --output-format csv`,
a run of its own: the average duration of the registration kernels, the launches with one grid layer per pair (the batch)
apart from those with one layer (the loop), is added to the record as `kernels`.
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
from bench_epipolar import LOOPS, SEED, frames  # noqa: E402  (the same scene)

N_FRAMES = 64
SIZES = (4096, 8192)
KERNELS = (r"(sequence_mark_kernel|sequence_pnp_mark_kernel|pnp_mark_kernel|planar_mark_kernel|planar_compact_kernel|"
           r"epipolar_solve_kernel|epipolar_score_kernel|epipolar_select_kernel|pose_vote_kernel|pose_write_kernel|"
           r"pnp_solve_kernel|pnp_score_kernel|pnp_select_kernel|match_batch_kernel|match_batch_merge_kernel|"
           r"match_kernel|match_merge_kernel)")


def sequence(capi, n, lift=False):
    """[64][n] records: tools/bench_epipolar.py's two views in turn.  lift: coords3D of the planted records = the planted
    point in the frame's own camera coordinates (tools/bench_pnp.py's replay), zeros elsewhere."""
    f1, f2 = frames(capi, n)
    if lift:
        from bench_pnp import planted_points

        world, first, R21, t21 = planted_points(n)
        assert np.array_equal(first, f1["coords2D"][:len(first)])  # the replay is the generator
        f1, f2 = f1.copy(), f2.copy()
        f1["coords3D"] = world
        # record i of frame 1 and the record of frame 2 with the same descriptor are partners
        order = {d.tobytes(): j for j, d in enumerate(f2["data"])}
        partner = np.array([order[d.tobytes()] for d in f1["data"]])
        planted = world[:, 2] != 0
        second = np.zeros((n, 3), np.float32)
        second[partner[planted]] = (world[planted].astype(np.float64) @ R21.T + t21).astype(np.float32)
        f2["coords3D"] = second
    out = np.zeros((N_FRAMES, n), dtype=capi.SIFT_POINT_DTYPE)
    out[0::2], out[1::2] = f1, f2
    return out


def spread(wall):
    w = np.asarray(wall)
    return {"median_ms": round(float(np.median(w)), 3), "p10_ms": round(float(np.percentile(w, 10)), 3),
            "p90_ms": round(float(np.percentile(w, 90)), 3)}


def alternate(ctx, routes, reps, warmup):
    """Times the routes in turn, repetition by repetition; returns ({name: [ms]}, {name: the last result})."""
    wall, last = {name: [] for name in routes}, {}
    for i in range(warmup + reps):
        for name, route in routes.items():
            ctx.synchronize()
            t0 = time.perf_counter()
            last[name] = route()
            t1 = time.perf_counter()
            if i >= warmup:
                wall[name].append((t1 - t0) * 1e3)
    return wall, last


def case_record(wall, last, extra):
    same = int(sum(a.tobytes() == b.tobytes() for a, b in zip(last["batch"][0], last["loop"][0])))
    rec = {"batch_wall": spread(wall["batch"]), "loop_wall": spread(wall["loop"]),
           "loop_over_batch": round(float(np.median(wall["loop"]) / np.median(wall["batch"])), 4),
           "pairs_with_the_same_bits": same, "fit_min": int(last["batch"][1].min()), "fit_max": int(last["batch"][1].max())}
    rec.update(extra)
    return rec


def kernel_times(path):
    import csv

    calls = {}
    for r in csv.DictReader(open(path)):
        m = re.search(KERNELS, r["Kernel_Name"])
        if m:
            layered = int(r.get("Grid_Size_Z", r.get("Grid_Size_z", "1")) or 1) > 1
            key = m.group(1) + (" (one layer per pair)" if layered else "")
            calls.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"calls": len(t), "avg_us": round(float(np.mean(t)), 1), "max_us": round(float(np.max(t)), 1)}
            for k, t in sorted(calls.items())}


def write(rec, out):
    text = json.dumps(rec, indent=1)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text + "\n")
    print(text)


def run(tool, default_out, note, routes_of, lift):
    """The command line that tools/bench_pose_batch.py and tools/bench_pnp_batch.py share; routes_of(ctx, capi, buffer,
    n, pairs) returns {"batch": fn, "loop": fn}, each fn returning ([P] poses, [P] num_fit)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", default_out))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", type=int, nargs="+", default=list(SIZES))
    ap.add_argument("--kernel-trace", default=None)
    a = ap.parse_args()
    if a.kernel_trace:
        rec = json.load(open(a.out))
        rec["kernels"] = kernel_times(a.kernel_trace)
        rec["kernels_note"] = ("average kernel durations under a kernel trace, a run of its own, over all its sizes and "
                               "repetitions, warm-up included")
        write(rec, a.out)
        return
    from cusift_amd import capi

    pairs = np.array([(i, i + 1) for i in range(N_FRAMES - 1)], np.int32)
    cases = {}
    with capi.Context(0) as ctx:
        for n in a.sizes:
            buf = capi.DeviceBuffer.from_numpy(ctx, sequence(capi, n, lift))
            wall, last = alternate(ctx, routes_of(ctx, capi, buf, n, pairs), a.reps, a.warmup)
            cases["%d records, %d loops" % (n, LOOPS)] = case_record(wall, last, {})
            buf.free()
    write({"tool": tool, "unit": "milliseconds per route (wall time, the matcher included)", "frames": N_FRAMES,
           "pairs": len(pairs), "reps": a.reps, "warmup": a.warmup, "seed": SEED, "cases": cases, "note": note}, a.out)


def pose_routes(ctx, capi, buf, n, pairs):
    cam = capi.Camera(1000.0, 1000.0, 640.0, 480.0, 0.0, 1000.0, 0)
    kw = dict(distance=0, rule=0, lo=0.85, hi=0.95, loops=LOOPS, thresh=1.0, refine_loops=5, refine_thresh=1.0)
    stride = n * capi.SIFT_POINT_BYTES

    def batch():
        res = ctx.register_pose_batch(buf.ptr, None, N_FRAMES, n, pairs, cam, None, seed=SEED, want_inliers=False, **kw)
        return res.rt, res.num_fit

    def loop():
        out = [ctx.register_pose(buf.ptr + int(a) * stride, n, buf.ptr + int(b) * stride, n, cam, None, seed=SEED + p, **kw)
               for p, (a, b) in enumerate(pairs)]
        return np.stack([r.rt for r in out]), np.array([r.num_fit for r in out])

    return {"batch": batch, "loop": loop}


if __name__ == "__main__":
    run("tools/bench_pose_batch.py", "pose_batch.json",
        "loop is cusift_register_pose per pair, the call that existed before the pair-list form and the yardstick; the "
        "routes alternate repetition by repetition in one process", pose_routes, False)
