"""What keeping the K strongest keypoints costs and saves: the extraction step with K in {0, 2048, 8192} on the two
contents of bench.py, and the selection kernels' own time.

    python tools/bench_keep_strongest.py [--frames 64] [--reps 15] [--warmup 3] [--out profiles/keep_strongest.json]
    python tools/bench_keep_strongest.py --trace        # + the kernel times of a rocprofv3 --kernel-trace --stats run

step     cusift_extract_batch of `frames` x 1920 x 1080 (5 octaves, init_blur 1.0 declared, peak threshold 3.0, max_pts
         32768: bench.py's parameters) on one stream, back to back, for `raw` tiles (synth.tile without pre-blur: every
         image saturates max_pts) and `preblurred` tiles (the headline content), K = 0 (off), 2048, 8192.  The windows of
         the three settings alternate within a repetition; the figure is the median over --reps windows of --inner steps,
         timed with device events.  Per setting also the keypoints per image the step leaves.
trace    --trace starts THIS tool again under `rocprofv3 --kernel-trace --stats` as a fresh child process with --child
         (raw tiles, K = 2048 and 8192, a few steps) and sums the select_* kernels' time per step from its kernel
         statistics, beside describe_all_kernel's.
The parent commit's saturated step, for the comparison the record asks for, is this tool's K = 0 row on raw tiles (the
setting off runs the parent's launch sequence).
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1920, 1080
KS = (0, 2048, 8192)


def make_images(synth, frames, blur):
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(max_workers=8) as pool:
        return np.stack(list(pool.map(lambda s: synth.tile(s, W, H, blur), [1000 + i for i in range(frames)])))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=4, help="steps per timed window")
    ap.add_argument("--max-pts", type=int, default=32768)
    ap.add_argument("--trace", action="store_true", help="also run the kernel trace (needs rocprofv3)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keep_strongest.json"))
    args = ap.parse_args()

    import torch

    from cusift_amd import capi, synth
    from cusift_amd.batch import BatchExtractor

    if not torch.cuda.is_available():
        raise SystemExit("bench_keep_strongest needs a GPU")
    prm = dict(num_octaves=5, init_blur=1.0, peak_thresh=3.0, max_pts=args.max_pts)
    contents = {"raw": 0.0} if args.child else {"raw": 0.0, "preblurred": 1.0}
    ks = KS[1:] if args.child else KS
    record = {"frames": args.frames, "width": W, "height": H, "params": prm, "reps": args.reps, "inner": args.inner,
              "device": torch.cuda.get_device_name(0), "contents": {}}
    for name, blur in contents.items():
        imgs = make_images(synth, args.frames, blur)
        exs = {k: BatchExtractor(args.frames, W, H, keep_strongest=k, **prm) for k in ks}
        d_imgs = exs[ks[0]].images_from_numpy(imgs)
        rows = {k: {"ms": []} for k in ks}
        for k, ex in exs.items():
            for _ in range(max(1, args.warmup)):
                ex.extract(d_imgs)
            torch.cuda.synchronize()
            cnt = ex.valid_counts().cpu().numpy()
            rows[k]["keypoints_per_image_mean"] = float(cnt.mean())
            rows[k]["keypoints_per_image_min_max"] = [int(cnt.min()), int(cnt.max())]
            rows[k]["images_at_max_pts"] = int((ex.counts.cpu().numpy() >= args.max_pts).sum())
        for _ in range(1 if args.child else args.reps):
            for k, ex in exs.items():  # alternate the settings inside a repetition
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.inner):
                    ex.extract(d_imgs)
                b.record()
                b.synchronize()
                rows[k]["ms"].append(a.elapsed_time(b) / args.inner)
        out = {}
        for k in ks:
            ms = np.array(rows[k].pop("ms"))
            rows[k].update(ms_per_step_median=round(float(np.median(ms)), 4), ms_per_step_min=round(float(ms.min()), 4),
                           ms_per_step_max=round(float(ms.max()), 4),
                           Mpix_per_s=round(args.frames * W * H / (float(np.median(ms)) * 1e-3) / 1e6, 1))
            out["K=%d" % k] = rows[k]
        record["contents"][name] = out
        for ex in exs.values():
            ex.close()
        del d_imgs
    if args.child:
        return
    if args.trace:
        record["kernel_trace"] = kernel_trace(args)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(json.dumps(record["contents"], indent=1))
    if args.trace:
        print(json.dumps(record["kernel_trace"], indent=1))


def kernel_trace(args):
    """Per kernel name: calls and total ns of a child run (raw tiles; warm-up + one window for K = 2048 and for K = 8192)."""
    steps = 2 * (max(1, args.warmup) + args.inner)
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--child", "--frames", str(args.frames), "--warmup", str(args.warmup),
               "--inner", str(args.inner), "--max-pts", str(args.max_pts)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=600)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"error": "no kernel_stats.csv in the trace"}
        kernels = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                for key in ("select_gather", "select_cut", "select_partition", "describe_all", "join_counts", "detect_"):
                    if key in name:
                        d = kernels.setdefault(key, {"calls": 0, "total_ns": 0})
                        d["calls"] += int(row["Calls"])
                        d["total_ns"] += int(float(row["TotalDurationNs"]))
    sel = sum(v["total_ns"] for k, v in kernels.items() if k.startswith("select_"))
    return {"steps_traced": steps, "ks": list(KS[1:]), "kernels": kernels,
            "select_ms_per_step": round(sel / steps * 1e-6, 4),
            "describe_all_ms_per_step": round(kernels.get("describe_all", {}).get("total_ns", 0) / steps * 1e-6, 4)}


if __name__ == "__main__":
    main()
