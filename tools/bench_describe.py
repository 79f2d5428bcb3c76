"""What describing caller-supplied keypoints costs: cusift_describe_batch over the records of an extraction, beside the
extraction's own description of the very same records, and over a dense grid.

    python tools/bench_describe.py [--frames 64] [--reps 30] [--warmup 3] [--out profiles/describe.json]

records  bench.py's workload -- `frames` x 1920 x 1080 pre-blurred tiles, 5 octaves, init_blur 1.0 declared, peak
         threshold 3.0, max_pts 32768 -- extracted once; the describe call then re-describes those records in place (they
         come back byte for byte, so every repetition does the same work).  Two passes, each alternating the extraction
         and the describe call inside a repetition, medians with p10 / p90 over --reps:
           wall    device events around one call each, stage timers off;
           stages  stage timers on: CUSIFT_STAGE_SCALEDOWN and CUSIFT_STAGE_DESCRIBE_ALL of both calls from
                   cusift_ctx_timing_read -- the extraction's two are the unchanged describe_all_kernel and pyramid on the
                   same records.  (With the timers on the extraction takes its launch-per-octave sequence.)
dense    one 1080p frame, a keypoint every 4 px at scale 2.0 (129,600 records, d_counters = NULL): wall time and the two
         stage times of the describe call.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1920, 1080


def make_images(synth, frames, blur):
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(max_workers=8) as pool:
        return np.stack(list(pool.map(lambda s: synth.tile(s, W, H, blur), [1000 + i for i in range(frames)])))


def stats(ms):
    ms = np.asarray(ms, dtype=np.float64)
    return {"median_ms": round(float(np.median(ms)), 4), "p10_ms": round(float(np.percentile(ms, 10)), 4),
            "p90_ms": round(float(np.percentile(ms, 90)), 4)}


def measure(torch, ex, calls, reps, warmup):
    """calls: {name: function that enqueues one call}.  Returns {name: {"wall": ..., "scale_down": ..., "describe_all": ...}}."""
    for fn in calls.values():
        for _ in range(max(1, warmup)):
            fn()
    torch.cuda.synchronize()
    wall = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():  # alternate the calls inside a repetition
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            wall[k].append(a.elapsed_time(b))
    stage = {k: {"scale_down": [], "describe_all": []} for k in calls}
    ex.ctx.timing_enable(True)
    try:
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        for _ in range(reps):
            for k, fn in calls.items():
                ex.ctx.timing_reset()
                fn()
                torch.cuda.synchronize()
                t = ex.ctx.timing_read()
                for s in stage[k]:
                    stage[k][s].append(t[s][0])
    finally:
        ex.ctx.timing_enable(False)
    return {k: {"wall": stats(wall[k]), "stage_scale_down": stats(stage[k]["scale_down"]),
                "stage_describe_all": stats(stage[k]["describe_all"])} for k in calls}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-pts", type=int, default=32768)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "describe.json"))
    args = ap.parse_args()

    import torch

    from cusift_amd import capi, synth
    from cusift_amd.batch import BatchExtractor

    if not torch.cuda.is_available():
        raise SystemExit("bench_describe needs a GPU")
    prm = dict(num_octaves=5, init_blur=1.0, peak_thresh=3.0, max_pts=args.max_pts)
    record = {"frames": args.frames, "width": W, "height": H, "params": prm, "reps": args.reps,
              "device": torch.cuda.get_device_name(0)}

    imgs = make_images(synth, args.frames, 1.0)
    ex = BatchExtractor(args.frames, W, H, **prm)
    d_imgs = ex.images_from_numpy(imgs)
    points, counts = ex.extract(d_imgs)
    torch.cuda.synchronize()
    n = ex.valid_counts().cpu().numpy()
    rows = measure(torch, ex, {"extract": lambda: ex.extract(d_imgs), "describe": lambda: ex.describe(d_imgs)},
                   args.reps, args.warmup)
    # (the append order inside an octave differs from extraction to extraction: compare with the LAST one's records)
    ex.extract(d_imgs)
    torch.cuda.synchronize()
    want = points.clone()
    ex.describe(d_imgs)
    torch.cuda.synchronize()
    differing = sum(int((points[i, :int(n[i])] != want[i, :int(n[i])]).any(dim=1).sum()) for i in range(args.frames))
    same = differing == 0
    total = int(n.sum())
    d, e = rows["describe"], rows["extract"]
    record["records"] = {
        "keypoints": total, "keypoints_per_image_mean": round(float(n.mean()), 1),
        "records_come_back_byte_for_byte": bool(same), "records_differing": differing, "extract": e, "describe": d,
        "describe_launch_over_extractions_describe_all": round(d["stage_describe_all"]["median_ms"] /
                                                               e["stage_describe_all"]["median_ms"], 3),
        "describe_pyramid_over_extractions_scale_down": round(d["stage_scale_down"]["median_ms"] /
                                                              max(e["stage_scale_down"]["median_ms"], 1e-9), 3),
        "describe_wall_over_extract_wall": round(d["wall"]["median_ms"] / e["wall"]["median_ms"], 3),
        "ns_per_keypoint_describe_launch": round(d["stage_describe_all"]["median_ms"] * 1e6 / max(total, 1), 1),
        "ns_per_keypoint_extractions_describe_all": round(e["stage_describe_all"]["median_ms"] * 1e6 / max(total, 1), 1),
    }
    ex.close()
    del d_imgs, points, want

    # dense SIFT: one frame, a keypoint every 4 px at one scale
    gx, gy = np.meshgrid(np.arange(2, W, 4, dtype=np.float32), np.arange(2, H, 4, dtype=np.float32))
    recs = np.zeros(gx.size, dtype=capi.SIFT_POINT_DTYPE)
    recs["coords2D"][:, 0], recs["coords2D"][:, 1], recs["scale"] = gx.ravel(), gy.ravel(), 2.0
    dense = BatchExtractor(1, W, H, **dict(prm, max_pts=len(recs)))
    d_img = dense.images_from_numpy(imgs[:1])
    d_recs = torch.from_numpy(recs.view(np.uint8).reshape(1, len(recs), capi.SIFT_POINT_BYTES)).to(dense.device)
    row = measure(torch, dense, {"describe": lambda: dense.describe(d_img, points=d_recs)}, args.reps, args.warmup)["describe"]
    back = d_recs.cpu().numpy().view(capi.SIFT_POINT_DTYPE).reshape(-1)
    record["dense"] = dict(row, keypoints=len(recs), step_px=4, scale=2.0,
                           described=int((back["subsampling"] > 0).sum()),
                           ns_per_keypoint_describe_launch=round(row["stage_describe_all"]["median_ms"] * 1e6 / len(recs), 1))
    dense.close()

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(json.dumps(record, indent=1))


if __name__ == "__main__":
    main()
