#!/usr/bin/env python3
"""Timing record of cusift_bundle_adjust on one MI355X beside the routes a caller had before it: read the tracks, the
records and the points back and minimise in host code -- tests/bundle_model.py (the definition in numpy) and, where scipy
is importable, scipy.optimize.least_squares (trf) with a sparse finite-difference Jacobian on the same residuals.

The scene is tools/bench_tracks.py's: 64 frames of 4,096 records, matched once by cusift_match_batch_mutual, tracks built
and triangulated on the device, once from the 63 consecutive pairs and once from the 420 pairs inside a window of 8.  The
poses the adjuster starts from are the scene's with every frame but the first a little off (0.002 rad, 0.01 units: the
drift of a chain), the points are cusift_triangulate_tracks' under those poses, max_error = 20 px keeps the chance tracks
of two views out and huber = 2 px holds the rest.

    python tools/bench_bundle.py --out profiles/bundle.json [--iters 20] [--warmup 3] [--host-reps 2] [--no-scipy]
    python tools/bench_bundle.py --kernel-trace TRACE.csv --out profiles/bundle.json     # adds `kernels` to the record

The routes alternate in one process; each figure is the median with p10 and p90, in microseconds of wall time from the
call to the synchronised result (the device route ends with d_summary on the host; the host routes start from host
arrays, so they skip both the read-back and the upload a device consumer would need).  The device call is timed with
ITERATIONS and with 1 iteration enqueued; per iteration = the difference over the iterations that ran.  A record, not an
assertion.  --kernel-trace: the *_kernel_trace.csv of a run of this tool under `rocprofv3 --kernel-trace --output-format
csv` in a run of its own; the average duration of every bundle_* kernel is added as `kernels`."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
ITERATIONS, HOST_ITERATIONS = 10, 2
OPTS = dict(huber=2.0, max_error=20.0)


def scipy_route(xy, max_pts, offsets, obs, poses, cam, points, used_obs, held, max_nfev=15):
    """least_squares on the used observations' residuals from the same start, stopped at max_nfev evaluations.  Its
    Huber loss acts on each residual component, not on an observation's norm, so its cost is a neighbour of the
    device's, not the same number.  Returns (2 * cost, nfev)."""
    from scipy.optimize import least_squares
    from scipy.sparse import coo_matrix
    from bundle_model import rodrigues

    nodes = np.asarray(obs, np.int64)[used_obs]
    tracks = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets))[used_obs]
    frames = nodes // max_pts
    fx, fy, cx, cy = cam
    pix = np.asarray(xy, np.float32).reshape(-1, 2)[nodes].astype(np.float64)
    free = np.flatnonzero(~held)
    col_of = np.full(len(poses), -1)
    col_of[free] = 6 * np.arange(len(free))
    used_t, point_col = np.unique(tracks, return_inverse=True)
    n_cam = 6 * len(free)
    start = np.asarray(poses, np.float64)

    def residuals(p):
        cur = start.copy()
        for k, f in enumerate(free):
            cur[f, :, :3] = start[f, :, :3] @ rodrigues(p[6 * k:6 * k + 3])
            cur[f, :, 3] = start[f, :, 3] + p[6 * k + 3:6 * k + 6]
        X = p[n_cam:].reshape(-1, 3)[point_col]
        P = cur[frames]
        c = np.einsum("nji,nj->ni", P[:, :, :3], X - P[:, :, 3])
        return np.stack([fx * c[:, 0] / c[:, 2] + cx - pix[:, 0], fy * c[:, 1] / c[:, 2] + cy - pix[:, 1]], axis=1).ravel()

    k = np.arange(len(nodes))
    rows, cols = [], []
    for r in (0, 1):
        for j in range(3):
            rows.append(2 * k + r)
            cols.append(n_cam + 3 * point_col + j)
        moving = col_of[frames] >= 0
        for j in range(6):
            rows.append(2 * k[moving] + r)
            cols.append(col_of[frames[moving]] + j)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    pattern = coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(2 * len(nodes), n_cam + 3 * len(used_t)))
    p0 = np.concatenate([np.zeros(n_cam), np.asarray(points)[used_t, :3].ravel()])
    sol = least_squares(residuals, p0, jac="2-point", jac_sparsity=pattern.tocsr(), method="trf", loss="huber",
                        f_scale=OPTS["huber"], max_nfev=max_nfev)
    return 2.0 * float(sol.cost), int(sol.nfev)


def kernel_times(path):
    import csv

    calls = {}
    for r in csv.DictReader(open(path)):
        m = re.search(r"(bundle_\w+_kernel)", r["Kernel_Name"])
        if m:
            calls.setdefault(m.group(1), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {name: {"calls": len(t), "avg_us": round(float(np.mean(t)), 1), "max_us": round(float(np.max(t)), 1)}
            for name, t in sorted(calls.items())}


def spread(t):
    return {"median_us": round(float(np.median(t)), 1), "p10_us": round(float(np.percentile(t, 10)), 1),
            "p90_us": round(float(np.percentile(t, 90)), 1), "n": len(t)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--kernel-trace", default=None)
    a = ap.parse_args()
    if a.kernel_trace:
        rec = json.load(open(a.out))
        rec["kernels"] = kernel_times(a.kernel_trace)
        rec["kernels_note"] = "kernel durations under a kernel trace, in a run of its own (every call of that run)"
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
        print(json.dumps(rec["kernels"], indent=1))
        return
    from bench_tracks import LISTS, MAX_PTS, N_FRAMES, RULE, WINDOW, sequence
    from bundle_model import bundle_model, perturbed
    from cusift_amd import capi

    try:
        import scipy  # noqa: F401
        have_scipy = not a.no_scipy
    except ImportError:
        have_scipy = False
    recs, true_poses, camera = sequence(capi)
    cam = (camera.fx, camera.fy, camera.cx, camera.cy)
    start = perturbed(true_poses, 0.002, 0.01, range(1, N_FRAMES))
    lists = (np.array([(i, i + 1) for i in range(N_FRAMES - 1)], np.int32),
             np.array([(i, j) for i in range(N_FRAMES) for j in range(i + 1, min(i + WINDOW, N_FRAMES))], np.int32))
    n_nodes = N_FRAMES * MAX_PTS
    cap = n_nodes // 2
    cases = {}
    with capi.Context(0) as ctx:
        d_recs = capi.DeviceBuffer.from_numpy(ctx, recs)
        d_track, d_offsets, d_obs = (capi.DeviceBuffer(ctx, 4 * n) for n in (n_nodes, n_nodes // 2 + 1, n_nodes))
        d_stats, d_pts, d_front = capi.DeviceBuffer(ctx, 32), capi.DeviceBuffer(ctx, 32 * cap), capi.DeviceBuffer(ctx, 4 * cap)
        d_x, d_poses = capi.DeviceBuffer(ctx, 32 * cap), capi.DeviceBuffer(ctx, 96 * N_FRAMES)
        d_hist, d_sum = capi.DeviceBuffer(ctx, 32 * ITERATIONS), capi.DeviceBuffer(ctx, 64)
        for label, pairs in zip(LISTS, lists):
            row_bytes = 16 * len(pairs) * MAX_PTS
            d_rows, d_back = capi.DeviceBuffer(ctx, row_bytes), capi.DeviceBuffer(ctx, row_bytes)
            ctx.match_batch_mutual(d_recs.ptr, None, N_FRAMES, MAX_PTS, pairs, d_rows.ptr, d_back.ptr, distance=0)
            ctx.build_tracks(None, N_FRAMES, MAX_PTS, pairs, d_rows.ptr, d_track.ptr, d_offsets.ptr, d_obs.ptr,
                             d_stats.ptr, d_rows_back=d_back.ptr, min_views=2, **RULE)
            ctx.triangulate_tracks(d_recs.ptr, N_FRAMES, MAX_PTS, d_offsets.ptr, d_obs.ptr, d_stats.ptr, cap, start,
                                   camera, d_pts.ptr, d_front.ptr)
            ctx.synchronize()
            d_rows.free()
            d_back.free()
            n_tracks = int(d_stats.to_numpy(np.uint32, (8,))[0])
            offsets = d_offsets.to_numpy(np.int32, (n_tracks + 1,))
            obs = d_obs.to_numpy(np.int32, (int(offsets[-1]),))
            points = d_pts.to_numpy(np.float64, (n_tracks, 4))
            summary = np.zeros(8)

            def device(iterations):
                check = capi.lib().cusift_memcpy_d2d(ctx.handle, d_x.ptr, d_pts.ptr, 32 * n_tracks)
                assert check == 0
                ctx.bundle_adjust(d_recs.ptr, N_FRAMES, MAX_PTS, d_offsets.ptr, d_obs.ptr, d_stats.ptr, cap, start, camera,
                                  d_x.ptr, d_poses.ptr, d_hist.ptr, d_sum.ptr, iterations=iterations, **OPTS)
                ctx.d2h(summary, d_sum.ptr)
                return summary.copy()

            wall = {"device": [], "device_1": [], "model": [], "scipy": []}
            model = sci = None
            for it in range(a.warmup + a.iters):
                for name, k in (("device", ITERATIONS), ("device_1", 1)):
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    result = device(k)
                    t1 = time.perf_counter()
                    if it >= a.warmup:
                        wall[name].append((t1 - t0) * 1e6)
                    if name == "device":
                        dev = result
                if it < a.host_reps:  # the host routes alternate with the device's
                    t0 = time.perf_counter()
                    model = bundle_model(recs["coords2D"], MAX_PTS, offsets, obs, start, *cam, points,
                                         iterations=HOST_ITERATIONS, **OPTS)
                    wall["model"].append((time.perf_counter() - t0) * 1e6)
                    if have_scipy and it == 0:  # once: it is stopped at 15 evaluations and still takes the longest
                        t0 = time.perf_counter()
                        sci = scipy_route(recs["coords2D"], MAX_PTS, offsets, obs, start, cam, points, model["used_obs"],
                                          model["held"])
                        wall["scipy"].append((time.perf_counter() - t0) * 1e6)
            history = d_hist.to_numpy(np.float64, (ITERATIONS, 4))
            pts_out = d_x.to_numpy(np.float64, (n_tracks, 4))
            used = model["used"]
            ran = int(dev[3])
            per_iter = (np.median(wall["device"]) - np.median(wall["device_1"])) / max(ran - 1, 1)
            assert (dev[4:7] == model["summary"][4:7]).all(), (dev, model["summary"])
            assert abs(history[0, 0] / model["history"][0, 0] - 1) < 1e-9 and abs(history[1, 1] / model["history"][1, 1] - 1) < 1e-6
            cases[label] = {
                "pairs": len(pairs), "tracks": n_tracks, "used_tracks": int(dev[4]), "used_observations": int(dev[5]),
                "free_frames": int(dev[6]), "reduced_system": 6 * N_FRAMES,
                "iterations_enqueued": ITERATIONS, "iterations_run": ran, "accepted": int(dev[2]),
                "entry_cost": float(dev[0]), "final_cost": float(dev[1]),
                "median_error_px_before": round(float(np.median(points[used, 3])), 3),
                "median_error_px_after": round(float(np.median(pts_out[used, 3])), 3),
                "bundle_adjust_device": spread(wall["device"]), "bundle_adjust_device_1_iteration": spread(wall["device_1"]),
                "device_us_per_iteration": round(float(per_iter), 1),
                "numpy_model_%d_iterations" % HOST_ITERATIONS: spread(wall["model"]),
                "numpy_model_us_per_iteration": round(float(np.median(wall["model"])) / HOST_ITERATIONS, 1),
                "scipy_least_squares": spread(wall["scipy"]) if have_scipy else "scipy is not importable",
                "scipy_final_cost_and_nfev": sci}
    rec = {"tool": "tools/bench_bundle.py", "unit": "microseconds of wall time per call, synchronised",
           "frames": N_FRAMES, "records_per_frame": MAX_PTS, "iters": a.iters, "warmup": a.warmup, "options": OPTS,
           "cases": cases,
           "note": "the device route copies the triangulated points, adjusts and ends with d_summary on the host; the host "
                   "routes start from host arrays and skip the read-back of records, tracks and points"}
    text = json.dumps(rec, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
