#!/usr/bin/env python3
"""Timing record of the cross-checked registrations on one MI355X: the same call with cusift_ctx_set_cross_check off and on.

    python tools/bench_cross_check.py --out profiles/cross_check.json [--reps 10] [--warmup 2]
    python tools/bench_cross_check.py --regs-into profiles/cross_check.json      # needs hipcc, no GPU

The workload: 64 seeded 1920 x 1080 frames (cusift_amd.synth.batch: shifted mirror tilings of the fixture image, the
repeated structure the cross-check is for), extracted once by BatchExtractor with --max-pts records per frame; the 63
consecutive pairs; register_planar_sequence (L2 distance, ratio test 0.8, --loops hypotheses, 5 px, 5 rounds of refit at
3 px) and register_sequence (a flat depth image of 2 m per frame, 1024 hypotheses, 5 cm).  Two extractors over the same
records, one with cross_check=False and one with cross_check=True, on one device in one process; the four routes
alternate repetition by repetition (planar off, planar on, RGB-D off, RGB-D on, ...), after --warmup rounds of all.  A
repetition is the whole call, from device-resident records to the results on the host, ending in its own
synchronisation, on the host clock.

The baseline of each "on" figure is the same call with the setting off, in the same run.  What the setting adds on the
device: the column fold inside the matcher's tile loop (match_batch_mutual_kernel in place of match_batch_kernel) and one
more launch, match_batch_mutual_merge_kernel; what it takes away: RANSAC work on candidates that drop out.  Read
on_over_off against that.  Per step: median, min, max; candidates (selected matches for RGB-D) and RANSAC inliers per
pair as min / median / max over the pairs.  --regs-into adds VGPRs, SGPRs and LDS bytes of the three touched kernels
(planar_mark_kernel, sequence_mark_kernel, sequence_select_kernel) from tools/kernel_regs.py: a compile, no run.
A record, not an assertion.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
N_FRAMES, W, H = 64, 1920, 1080
TOUCHED = (("sift_planar.hip", ("planar_mark_kernel",)),
           ("sift_sequence.hip", ("sequence_mark_kernel", "sequence_select_kernel")))


def kernel_resources():
    import kernel_regs

    rows = {}
    for src, wanted in TOUCHED:
        for k in kernel_regs.kernels(kernel_regs.assembly(src)):
            for w in wanted:
                if w in k["name"]:
                    rows[w] = {f: k[f] for f in ("vgpr_count", "sgpr_count", "group_segment_fixed_size",
                                                 "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")}
    return rows


def spread(v):
    v = np.asarray(v)
    return {"min": int(v.min()), "median": float(np.median(v)), "max": int(v.max())}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--loops", type=int, default=10000, help="hypotheses per pair of the planar registration")
    ap.add_argument("--max-pts", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=N_FRAMES)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cross_check.json"))
    ap.add_argument("--regs-into", default=None, help="add the touched kernels' resources to this record (needs hipcc)")
    a = ap.parse_args()
    if a.regs_into:
        rec = json.load(open(a.regs_into)) if os.path.exists(a.regs_into) else {
            "tool": "tools/bench_cross_check.py", "steps": "not measured yet: no timed run of this tool is recorded"}
        rec["kernel_resources"] = kernel_resources()
        with open(a.regs_into, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
        print(json.dumps(rec["kernel_resources"], indent=1))
        return

    import torch
    from cusift_amd import capi, synth
    from cusift_amd.batch import BatchExtractor

    n = a.frames
    imgs = synth.batch(n, W, H)
    exs = {on: BatchExtractor(n, W, H, max_pts=a.max_pts, cross_check=on) for on in (False, True)}
    for ex in exs.values():
        ex.extract(ex.images_from_numpy(imgs))
    torch.cuda.synchronize()
    counts = exs[False].valid_counts().cpu().numpy()
    depth = torch.full((n, H, W), (2000 << 3) & 0xFFFF, dtype=torch.int16, device=exs[False].device)  # 2 m, SUN3D coding
    cam = capi.Camera(1000.0, 1000.0, W / 2.0, H / 2.0, origin=1.0, units_per_metre=1000.0, encoding=1)
    planar_kw = dict(distance=1, rule=1, lo=999.0, hi=0.8, loops=a.loops, thresh=5.0, refine_loops=5, refine_thresh=3.0,
                     seed=1, want_inliers=False)
    rgbd_kw = dict(distance=1, score_threshold=999.0, ambiguity_threshold=0.8, loops=1024, thresh2=0.0025, kind="3d", seed=1)

    def planar(on):
        res = exs[on].register_planar_sequence(**planar_kw)
        return res.num_candidates, res.num_matches

    def rgbd(on):
        out = exs[on].register_sequence(depth, cam, **rgbd_kw)
        return out[1], out[2]

    routes = {"planar_off": lambda: planar(False), "planar_on": lambda: planar(True),
              "rgbd_off": lambda: rgbd(False), "rgbd_on": lambda: rgbd(True)}
    last = {}
    for _ in range(a.warmup):
        for name, route in routes.items():
            last[name] = route()
    times = {name: [] for name in routes}
    for _ in range(a.reps):
        for name, route in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = route()
            times[name].append((time.perf_counter() - t0) * 1e3)
    steps = {}
    for name in routes:
        t = times[name]
        steps[name] = {"median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t)),
                       "candidates_per_pair": spread(last[name][0]), "ransac_inliers_per_pair": spread(last[name][1])}
    rec = {"tool": "tools/bench_cross_check.py", "frames": n, "width": W, "height": H, "pairs": n - 1,
           "max_pts": a.max_pts, "planar_hypotheses": a.loops, "rgbd_hypotheses": 1024, "records_min": int(counts.min()),
           "records_max": int(counts.max()), "reps": a.reps, "warmup": a.warmup,
           "unit": "milliseconds per call, host clock, from device-resident records to the results on the host",
           "expected_extra": "the column fold inside the matcher's tile loop plus one merge launch "
                             "(match_batch_mutual_merge_kernel); fewer candidates for RANSAC",
           "steps": steps,
           "planar_on_over_off": steps["planar_on"]["median_ms"] / steps["planar_off"]["median_ms"],
           "rgbd_on_over_off": steps["rgbd_on"]["median_ms"] / steps["rgbd_off"]["median_ms"]}
    if os.path.exists(a.out):
        old = json.load(open(a.out))
        if "kernel_resources" in old:
            rec["kernel_resources"] = old["kernel_resources"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))
    for ex in exs.values():
        ex.close()


if __name__ == "__main__":
    main()
