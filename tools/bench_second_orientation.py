"""What second-peak orientations cost: the extraction step with the setting 0 (off) and 0.8 on bench.py's content, the
keypoints before and after, and the time of each of the stage's three launches.

    python tools/bench_second_orientation.py [--frames 64] [--reps 30] [--warmup 3] [--out profiles/second_orientation.json]
    python tools/bench_second_orientation.py --trace   # + the kernel times of a rocprofv3 --kernel-trace --stats run

step     cusift_extract_batch of `frames` x 1920 x 1080 pre-blurred tiles (5 octaves, init_blur 1.0 declared, peak
         threshold 3.0, max_pts 32768: bench.py's content and parameters) on one stream, back to back.  The windows of
         the two settings alternate within a repetition; the figures are the median, p10 and p90 over --reps windows of
         --inner steps, timed with device events.  Per setting also the records per image the step leaves.
trace    --trace starts THIS tool again under `rocprofv3 --kernel-trace --stats` as a fresh child process with --child
         (the setting at 0.8, warm-up + one window) and reports the time per step of second_peak_kernel,
         second_scan_kernel and second_describe_kernel from its kernel statistics, beside describe_all_kernel's.  The
         step times above come from the run without the profiler.
The peak kernel repeats the orientation stage of every record: that is the price of leaving describe_all_kernel alone,
and the number that says whether emitting the mark from inside that kernel would be worth a change of its own.
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
RATIOS = (0.0, 0.8)
KERNELS = ("second_peak", "second_scan", "second_describe", "describe_all", "join_counts", "detect_")


def make_images(synth, frames, blur):
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(max_workers=8) as pool:
        return np.stack(list(pool.map(lambda s: synth.tile(s, W, H, blur), [1000 + i for i in range(frames)])))


def commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=4, help="steps per timed window")
    ap.add_argument("--max-pts", type=int, default=32768)
    ap.add_argument("--trace", action="store_true", help="also run the kernel trace (needs rocprofv3)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--parent-commit", default=None, help="the commit this tree sits on, when it is no git checkout")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "second_orientation.json"))
    args = ap.parse_args()

    import torch

    from cusift_amd import synth
    from cusift_amd.batch import BatchExtractor

    if not torch.cuda.is_available():
        raise SystemExit("bench_second_orientation needs a GPU")
    prm = dict(num_octaves=5, init_blur=1.0, peak_thresh=3.0, max_pts=args.max_pts)
    ratios = RATIOS[1:] if args.child else RATIOS
    record = {"what": "cusift_extract_batch with cusift_ctx_set_second_orientation 0 and 0.8, alternating in one process",
              "measured_on_top_of_commit": args.parent_commit or commit(), "frames": args.frames, "width": W, "height": H,
              "content": "synth.tile pre-blurred with sigma 1.0 (bench.py's timed workload)", "params": prm,
              "reps": args.reps, "inner": args.inner, "device": torch.cuda.get_device_name(0), "settings": {}}
    imgs = make_images(synth, args.frames, 1.0)
    exs = {r: BatchExtractor(args.frames, W, H, second_orientation=r, **prm) for r in ratios}
    d_imgs = exs[ratios[0]].images_from_numpy(imgs)
    rows = {r: {"ms": []} for r in ratios}
    for r, ex in exs.items():
        for _ in range(max(1, args.warmup)):
            ex.extract(d_imgs)
        torch.cuda.synchronize()
        cnt = ex.valid_counts().cpu().numpy()
        rows[r]["records_per_step"] = int(cnt.sum())
        rows[r]["records_per_image_mean"] = float(cnt.mean())
        rows[r]["records_per_image_min_max"] = [int(cnt.min()), int(cnt.max())]
        rows[r]["images_at_max_pts"] = int((ex.counts.cpu().numpy() >= args.max_pts).sum())
    for _ in range(1 if args.child else args.reps):
        for r, ex in exs.items():  # alternate the settings inside a repetition
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.inner):
                ex.extract(d_imgs)
            b.record()
            b.synchronize()
            rows[r]["ms"].append(a.elapsed_time(b) / args.inner)
    for r in ratios:
        ms = np.array(rows[r].pop("ms"))
        rows[r].update(ms_per_step_median=round(float(np.median(ms)), 4),
                       ms_per_step_p10=round(float(np.percentile(ms, 10)), 4),
                       ms_per_step_p90=round(float(np.percentile(ms, 90)), 4),
                       Mpix_per_s=round(args.frames * W * H / (float(np.median(ms)) * 1e-3) / 1e6, 1))
        record["settings"]["ratio=%g" % r] = rows[r]
    for ex in exs.values():
        ex.close()
    if args.child:
        return
    off, on = record["settings"]["ratio=0"], record["settings"]["ratio=0.8"]
    record["duplicates_per_step"] = on["records_per_step"] - off["records_per_step"]
    record["duplicates_share_of_keypoints"] = round(record["duplicates_per_step"] / max(1, off["records_per_step"]), 4)
    record["ms_per_step_added_median"] = round(on["ms_per_step_median"] - off["ms_per_step_median"], 4)
    if args.trace:
        record["kernel_trace"] = kernel_trace(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(json.dumps(record, indent=1))


def kernel_trace(args):
    """Per kernel name: calls and total ns of a child run (the setting at 0.8; warm-up + one window), per step."""
    steps = max(1, args.warmup) + args.inner
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
                for key in KERNELS:
                    if key in name:
                        d = kernels.setdefault(key, {"calls": 0, "total_ns": 0})
                        d["calls"] += int(row["Calls"])
                        d["total_ns"] += int(float(row["TotalDurationNs"]))
    out = {"steps_traced": steps, "ratio": RATIOS[1], "kernels": kernels}
    for key in KERNELS[:4]:
        out["%s_ms_per_step" % key] = round(kernels.get(key, {}).get("total_ns", 0) / steps * 1e-6, 4)
    out["stage_ms_per_step"] = round(sum(out["%s_ms_per_step" % k] for k in KERNELS[:3]), 4)
    return out


if __name__ == "__main__":
    main()
