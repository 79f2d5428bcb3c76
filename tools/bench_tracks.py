#!/usr/bin/env python3
"""Timing record of cusift_build_tracks on one MI355X beside the route a caller had before it, on the same match rows:
read d_rows and d_rows_back back and run the union-find in host code (tests/tracks_model.py, the definition in numpy and
Python; and, as the stronger yardstick, the same definition vectorised over scipy's connected_components).

The scene is tools/bench_epipolar.py's as a sequence: 64 frames of 4,096 records, 60 % of them views of the same 3-D points
from a camera that moves on, each under one unit descriptor, the rest anywhere with descriptors of their own; every frame
in an order of its own.  Matched once by cusift_match_batch_mutual (dot product), then measured twice: with the 63
consecutive pairs and with all 420 pairs inside a window of 8.

    python tools/bench_tracks.py --out profiles/tracks.json [--iters 30] [--warmup 3]
    python tools/bench_tracks.py --kernel-trace TRACE.csv --out profiles/tracks.json     # adds `kernels` to the record

The routes alternate in one process; each figure is the median of `iters` with p10 and p90, in microseconds of wall time
from the call to the synchronised result: the device route ends with T on the host (one 32-byte read-back), the host
routes start from rows on the device.  cusift_triangulate_tracks is timed on the device route's tracks.  A record, not an
assertion.  --kernel-trace: the *_kernel_trace.csv of a run of this tool under `rocprofv3 --kernel-trace --output-format
csv` in a run of its own; the average duration of every tracks_* kernel per pair list is added as `kernels`.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
N_FRAMES, MAX_PTS, WINDOW = 64, 4096, 8
RULE = dict(rule=0, lo=0.85, hi=0.95)
LISTS = ("63 consecutive pairs", "420 pairs inside a window of 8")


def sequence(capi, seed=3):
    """records [N_FRAMES, MAX_PTS], poses [N_FRAMES, 3, 4] camera to world, the camera."""
    rng = np.random.default_rng(seed)
    n_in = int(round(0.6 * MAX_PTS))
    X = rng.uniform([-3, -2, 5], [9, 2, 12], size=(n_in, 3))
    desc = rng.random((n_in, 128)).astype(np.float32)
    desc /= np.linalg.norm(desc, axis=1, keepdims=True)
    recs = np.zeros((N_FRAMES, MAX_PTS), dtype=capi.SIFT_POINT_DTYPE)
    poses = np.zeros((N_FRAMES, 3, 4))
    for f in range(N_FRAMES):
        ang = 0.15 * f / (N_FRAMES - 1)
        c, s = np.cos(ang), np.sin(ang)
        R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])  # camera to world
        centre = np.array([6.0 * f / (N_FRAMES - 1), 0.0, 0.0])
        poses[f, :, :3], poses[f, :, 3] = R, centre
        Xc = (X - centre) @ R
        px = 1000.0 * Xc[:, :2] / Xc[:, 2:] + [640, 480] + rng.normal(0, 0.3, (n_in, 2))
        noise = rng.random((MAX_PTS - n_in, 128)).astype(np.float32)
        noise /= np.linalg.norm(noise, axis=1, keepdims=True)
        perm = rng.permutation(MAX_PTS)
        recs["coords2D"][f, perm] = np.r_[px, rng.uniform([0, 0], [1280, 960], (MAX_PTS - n_in, 2))].astype(np.float32)
        recs["data"][f, perm] = np.r_[desc, noise]
    return recs, poses, capi.Camera(1000.0, 1000.0, 640.0, 480.0)


def scipy_tracks(pairs, rows, back, min_views=2):
    """The definition vectorised: the edge filter in numpy, scipy's connected components, a sort for the listing."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    n = N_FRAMES * MAX_PTS
    i = np.broadcast_to(np.arange(MAX_PTS), rows.shape)
    m = rows["match"]
    ok = (m >= 0) & (m < MAX_PTS) & (rows["score"] > np.float32(RULE["lo"])) & (rows["ambiguity"] < np.float32(RULE["hi"]))
    ok &= (pairs[:, :1] != pairs[:, 1:])
    mm = np.where(ok, m, 0)
    ok &= np.take_along_axis(back["match"], mm, axis=1) == i
    u = (pairs[:, :1] * MAX_PTS + i)[ok]
    v = (pairs[:, 1:] * MAX_PTS + mm)[ok]
    _, label = connected_components(coo_matrix((np.ones(len(u), np.int8), (u, v)), shape=(n, n)), directed=False)
    order = np.lexsort((np.arange(n), label))
    lab = label[order]
    start = np.flatnonzero(np.r_[True, lab[1:] != lab[:-1]])
    size = np.diff(np.r_[start, n])
    frames = order // MAX_PTS
    dup = np.r_[False, (lab[1:] == lab[:-1]) & (frames[1:] == frames[:-1])]
    shared = np.add.reduceat(dup, start) > 0
    kept = (size >= min_views) & ~shared
    first = order[start]  # the smallest node of every component: tracks in ascending order of it
    rank = np.argsort(first[kept], kind="stable")
    return int(kept.sum()), start[kept][rank], size[kept][rank], order


def kernel_times(path):
    import csv

    calls = {}
    for r in sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"])):
        m = re.search(r"(tracks_\w+_kernel|match_batch\w*_kernel)", r["Kernel_Name"])
        if m:
            calls.setdefault(m.group(1), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    out = {}
    for name, t in calls.items():
        if name.startswith("match_batch"):  # run once per pair list, of different sizes
            out.setdefault("all", {})[name + "_avg_us"] = round(float(np.mean(t)), 1)
            continue
        per = len(t) // len(LISTS)
        for k, label in enumerate(LISTS):
            out.setdefault(label, {})[name + "_avg_us"] = round(float(np.mean(t[k * per:(k + 1) * per])), 1)
    return out


def spread(t):
    return {"median_us": round(float(np.median(t)), 1), "p10_us": round(float(np.percentile(t, 10)), 1),
            "p90_us": round(float(np.percentile(t, 90)), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-trace", default=None)
    a = ap.parse_args()
    if a.kernel_trace:
        rec = json.load(open(a.out))
        rec["kernels"] = kernel_times(a.kernel_trace)
        rec["kernels_note"] = "average kernel durations under a kernel trace, in a run of its own (warm-up calls included)"
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
        print(json.dumps(rec["kernels"], indent=1))
        return
    from cusift_amd import capi
    from tracks_model import ROW, build_tracks_model

    recs, poses, camera = sequence(capi)
    lists = (np.array([(i, i + 1) for i in range(N_FRAMES - 1)], np.int32),
             np.array([(i, j) for i in range(N_FRAMES) for j in range(i + 1, min(i + WINDOW, N_FRAMES))], np.int32))
    n_nodes = N_FRAMES * MAX_PTS
    cases = {}
    with capi.Context(0) as ctx:
        d_recs = capi.DeviceBuffer.from_numpy(ctx, recs)
        d_track, d_offsets, d_obs = (capi.DeviceBuffer(ctx, 4 * n) for n in (n_nodes, n_nodes // 2 + 1, n_nodes))
        d_stats, d_pts, d_front = capi.DeviceBuffer(ctx, 32), capi.DeviceBuffer(ctx, 32 * (n_nodes // 2)), \
            capi.DeviceBuffer(ctx, 4 * (n_nodes // 2))
        for label, pairs in zip(LISTS, lists):
            assert len(pairs) == int(label.split()[0])
            row_bytes = 16 * len(pairs) * MAX_PTS
            d_rows, d_back = capi.DeviceBuffer(ctx, row_bytes), capi.DeviceBuffer(ctx, row_bytes)
            ctx.match_batch_mutual(d_recs.ptr, None, N_FRAMES, MAX_PTS, pairs, d_rows.ptr, d_back.ptr, distance=0)
            ctx.synchronize()
            stats = np.zeros(8, np.uint32)

            def device():
                ctx.build_tracks(None, N_FRAMES, MAX_PTS, pairs, d_rows.ptr, d_track.ptr, d_offsets.ptr, d_obs.ptr,
                                 d_stats.ptr, d_rows_back=d_back.ptr, min_views=2, **RULE)
                ctx.d2h(stats, d_stats.ptr)
                return stats.copy()

            def read_back():
                return (d_rows.to_numpy(ROW, (len(pairs), MAX_PTS)), d_back.to_numpy(ROW, (len(pairs), MAX_PTS)))

            def host_model():
                rows, back = read_back()
                return build_tracks_model([MAX_PTS] * N_FRAMES, MAX_PTS, pairs, rows, back, None, min_views=2, **RULE)

            def host_scipy():
                rows, back = read_back()
                return scipy_tracks(pairs, rows, back)

            def triangulate():
                ctx.triangulate_tracks(d_recs.ptr, N_FRAMES, MAX_PTS, d_offsets.ptr, d_obs.ptr, d_stats.ptr,
                                       n_nodes // 2, poses, camera, d_pts.ptr, d_front.ptr)
                ctx.synchronize()

            routes = {"device": device, "host_model": host_model, "host_scipy": host_scipy, "read_back_only": read_back,
                      "triangulate": triangulate}
            wall = {k: [] for k in routes}
            result = {}
            for it in range(a.warmup + a.iters):
                for name, fn in routes.items():  # the routes alternate
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    result[name] = fn()
                    t1 = time.perf_counter()
                    if it >= a.warmup:
                        wall[name].append((t1 - t0) * 1e6)
            dev_stats, model = result["device"], result["host_model"]
            assert dev_stats.tolist() == model[3].tolist(), (dev_stats, model[3])
            assert result["host_scipy"][0] == int(dev_stats[0])
            n_tracks = int(dev_stats[0])
            pts = d_pts.to_numpy(np.float64, (n_tracks, 4))
            good = (pts != 0).any(axis=1)
            long3 = good & (np.diff(model[1]) >= 3)  # two-view tracks of chance matches triangulate to anything
            cases[label] = {
                "pairs": len(pairs), "rows_read_back_MB": round(2 * row_bytes / 1e6, 1),
                "tracks": n_tracks, "observations": int(dev_stats[1]), "accepted_rows": int(dev_stats[2]),
                "dropped_shared_frame": int(dev_stats[3]), "longest_track": int(np.diff(model[1]).max()),
                "build_tracks_device": spread(wall["device"]),
                "read_back_and_python_union_find": spread(wall["host_model"]),
                "read_back_and_scipy_connected_components": spread(wall["host_scipy"]),
                "read_back_alone": spread(wall["read_back_only"]),
                "triangulate_tracks_device": spread(wall["triangulate"]),
                "triangulated": int(good.sum()), "median_reprojection_error_px": round(float(np.median(pts[good, 3])), 3),
                "tracks_of_3_or_more_views": int(long3.sum()),
                "median_reprojection_error_px_3_or_more_views": round(float(np.median(pts[long3, 3])), 3)}
            d_rows.free()
            d_back.free()
    rec = {"tool": "tools/bench_tracks.py", "unit": "microseconds of wall time per call, synchronised",
           "frames": N_FRAMES, "records_per_frame": MAX_PTS, "iters": a.iters, "warmup": a.warmup, "cases": cases,
           "note": "the device route ends with d_stats on the host; the host routes start from the rows on the device and "
                   "end with the tracks in host memory, so they also skip the upload a device consumer would need"}
    text = json.dumps(rec, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
