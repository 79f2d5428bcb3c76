"""Wall time of the planar registration of a 64-frame 1080p sequence, both routes in one process, alternating:

    batch   BatchExtractor.register_planar_sequence(): cusift_register_planar_batch, one call, one synchronisation, no count
            read back
    loop    BatchExtractor.register_planar(i, i + 1) for the 63 consecutive pairs: two counts read back and one
            synchronisation per pair (cusift_register_planar)

The sequence: 64 seeded 1920 x 1080 frames (cusift_amd.synth.batch: shifted mirror tilings of the fixture image, so
consecutive frames overlap), extracted once by BatchExtractor with --max-pts records per frame; the 63 consecutive
pairs; --loops hypotheses per pair; L2 distance, ratio test 0.8, 5 px, 5 rounds of refit at 3 px.  The timed region of a
route is the whole route, from device-resident records to the 63 homographies on the host; it ends in the route's own
last synchronisation.  The routes alternate repetition by repetition (other work shares the host), after --warmup
repetitions of each; the medians over --reps and their ratio go to profiles/planar_batch.json.  The routes compute the
same thing: the tool checks that pair 0's homography has the same bits in both (the matcher's one licence to differ,
exactly tied scores, is counted over all pairs and reported, not hidden).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_FRAMES, W, H = 64, 1920, 1080


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--loops", type=int, default=10000, help="hypotheses per pair (the default of register_planar)")
    ap.add_argument("--max-pts", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=N_FRAMES)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planar_batch.json"))
    args = ap.parse_args()

    import torch
    from cusift_amd import synth
    from cusift_amd.batch import BatchExtractor

    n = args.frames
    ex = BatchExtractor(n, W, H, max_pts=args.max_pts)
    ex.extract(ex.images_from_numpy(synth.batch(n, W, H)))
    torch.cuda.synchronize()
    counts = ex.valid_counts().cpu().numpy()
    kw = dict(distance=1, rule=1, lo=999.0, hi=0.8, loops=args.loops, thresh=5.0, refine_loops=5, refine_thresh=3.0)

    def batch():
        res = ex.register_planar_sequence(seed=1, want_inliers=False, **kw)
        return res.homography, res.num_matches

    def loop():
        hs, ms = [], []
        for i in range(n - 1):
            res = ex.register_planar(i, i + 1, seed=1 + i, **kw)
            hs.append(res.homography)
            ms.append(res.num_matches)
        return np.stack(hs), np.array(ms)

    routes = {"batch": batch, "loop": loop}
    last = {}
    for _ in range(args.warmup):
        for name, route in routes.items():
            last[name] = route()
    times = {name: [] for name in routes}
    for _ in range(args.reps):
        for name, route in routes.items():
            ex.ctx.synchronize()
            t0 = time.perf_counter()
            last[name] = route()
            times[name].append((time.perf_counter() - t0) * 1e3)
    same = int((last["batch"][0] == last["loop"][0]).all(axis=1).sum())
    if last["batch"][0][0].tobytes() != last["loop"][0][0].tobytes():
        raise SystemExit("pair 0: the routes disagree")
    med = {name: float(np.median(t)) for name, t in times.items()}
    result = {"frames": n, "width": W, "height": H, "pairs": n - 1, "max_pts": args.max_pts, "hypotheses": args.loops,
              "records_min": int(counts.min()), "records_max": int(counts.max()), "reps": args.reps,
              "warmup": args.warmup, "batch_median_ms": med["batch"], "batch_min_ms": float(min(times["batch"])),
              "batch_max_ms": float(max(times["batch"])), "loop_median_ms": med["loop"],
              "loop_min_ms": float(min(times["loop"])), "loop_max_ms": float(max(times["loop"])),
              "loop_over_batch": med["loop"] / med["batch"], "pairs_with_the_same_bits": same,
              "inliers_min": int(last["batch"][1].min()), "inliers_max": int(last["batch"][1].max())}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    ex.close()


if __name__ == "__main__":
    main()
