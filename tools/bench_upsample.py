"""What octave -1 costs: the enlargement kernel against a device-to-device copy, and the driver option against the same
extraction of an image that is enlarged already.

    python tools/bench_upsample.py [--frames 64] [--reps 15] [--warmup 3] [--out profiles/upsample.json]

kernel   cusift_scale_up on `frames` x 1920 x 1080 (pitch 1920 -> 3840 x 2160 at pitch 3840).  Algorithmic bytes: 4 read +
         16 written per source pixel = 20 w h n.  Beside it a device-to-device copy of the output-sized buffer (16 w h n
         bytes read and as many written) in the same process: the practical ceiling of a streaming kernel on this chip.
         Both are timed with device events around `--inner` back-to-back launches; repetitions alternate between the two.
driver   cusift_extract_batch with upsample = 1 against the staged route -- the enlarged images already in HBM, extracted
         with upsample = 0, subsampling 0.5 and init_blur doubled, which resolves to the same plan and gives the same
         records -- for `frames` x 1080p and for one frame.  The difference is the enlargement launch.
Frames: one seeded `tile` image pre-blurred to sigma 0.5, rolled by a different offset per frame; init_blur 0.5, peak
threshold 3.0, edge threshold 10, 6 octaves (-1 .. 4).  Medians over --reps repetitions after --warmup.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 1920, 1080


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10, help="launches per timed window")
    ap.add_argument("--max-pts", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upsample.json"))
    args = ap.parse_args()

    import torch

    from cusift_amd import capi, synth

    if not torch.cuda.is_available():
        raise capi.CusiftError("bench_upsample needs a GPU (no CPU fallback)")
    dev = torch.device("cuda", 0)
    n = args.frames
    base = synth.tile(1000, W, H, preblur=0.5)
    frames = np.stack([np.roll(base, (37 * i, 53 * i), axis=(0, 1)) for i in range(n)])
    p, up_p = capi.ialign_up(W, 128), capi.ialign_up(2 * W, 128)
    d_src = torch.zeros((n, H, p), dtype=torch.float32, device=dev)
    d_src[:, :, :W] = torch.from_numpy(frames).to(dev)
    d_up = torch.zeros((n, 2 * H, up_p), dtype=torch.float32, device=dev)
    d_copy = torch.empty_like(d_up)
    stream = torch.cuda.current_stream()
    ctx = capi.Context(0, stream=stream.cuda_stream)

    def window(fn, inner):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(inner):
            fn()
        b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) / inner

    def alternate(fns, inner):
        """{name: median ms per call}, the routes taken in turn inside every repetition"""
        for _ in range(args.warmup):
            for f in fns.values():
                window(f, 1)
        times = {k: [] for k in fns}
        for _ in range(args.reps):
            for k, f in fns.items():
                times[k].append(window(f, inner))
        return {k: float(np.median(v)) for k, v in times.items()}, {k: [float(min(v)), float(max(v))] for k, v in times.items()}

    # ---- the kernel ----
    def scale_up():
        ctx.scale_up(d_up.data_ptr(), up_p, d_src.data_ptr(), W, H, p, n_images=n)

    def copy():
        d_copy.copy_(d_up)

    med, spread = alternate({"scale_up": scale_up, "copy": copy}, args.inner)
    px = W * H * n
    up_rate = 20.0 * px / (med["scale_up"] * 1e-3) / 1e9
    copy_rate = 32.0 * px / (med["copy"] * 1e-3) / 1e9
    kernel = {
        "frames": n, "w": W, "h": H, "scale_up_ms": med["scale_up"], "scale_up_ms_min_max": spread["scale_up"],
        "copy_ms": med["copy"], "copy_ms_min_max": spread["copy"],
        "scale_up_algorithmic_bytes": 20 * px, "copy_bytes_read_plus_written": 32 * px,
        "scale_up_GBps": round(up_rate, 1), "copy_GBps": round(copy_rate, 1), "ratio_scale_up_to_copy": round(up_rate / copy_rate, 3),
    }
    del d_copy

    # ---- the driver ----
    kw = dict(num_octaves=6, init_blur=0.5, peak_thresh=3.0, edge_thresh=10.0, max_pts=args.max_pts)
    on = capi.default_params(upsample=1, **kw)
    staged = capi.default_params(**dict(kw, upsample=0, subsampling=0.5, init_blur=1.0))
    driver = {}
    for m in sorted({n, 1}, reverse=True):
        pts = [torch.zeros((m, args.max_pts, capi.SIFT_POINT_BYTES), dtype=torch.uint8, device=dev) for _ in range(2)]
        cnt = [torch.zeros((m,), dtype=torch.int32, device=dev) for _ in range(2)]
        ctx.reserve(m, W, H, on)
        ctx.scale_up(d_up.data_ptr(), up_p, d_src.data_ptr(), W, H, p, n_images=m)  # the staged route's input

        def route_on():
            ctx.extract_batch(d_src.data_ptr(), m, W, H, p, H * p, on, pts[0].data_ptr(), cnt[0].data_ptr())

        def route_staged():
            ctx.extract_batch(d_up.data_ptr(), m, 2 * W, 2 * H, up_p, 2 * H * up_p, staged, pts[1].data_ptr(), cnt[1].data_ptr())

        med, spread = alternate({"upsample": route_on, "staged": route_staged}, args.inner if m == 1 else max(1, args.inner // 5))
        stream.synchronize()
        c0, c1 = cnt[0].cpu().numpy(), cnt[1].cpu().numpy()
        if not np.array_equal(c0, c1) or c0.max() >= args.max_pts:
            raise RuntimeError("the routes disagree or saturate: %s vs %s" % (c0[:4], c1[:4]))
        driver["%d_frames" % m] = {
            "upsample_ms": med["upsample"], "upsample_ms_min_max": spread["upsample"], "staged_ms": med["staged"],
            "staged_ms_min_max": spread["staged"], "difference_ms": med["upsample"] - med["staged"],
            "keypoints_per_frame_mean": float(c0.mean()),
        }
        del pts, cnt
    result = {"_source": "python tools/bench_upsample.py --frames %d --reps %d --warmup %d --inner %d" %
                         (n, args.reps, args.warmup, args.inner),
              "device": torch.cuda.get_device_name(0), "params": kw, "kernel": kernel, "driver": driver}
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
