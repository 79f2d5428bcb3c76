#!/usr/bin/env python3
"""Timing record of cusift_ctx_set_match_bits on one MI355X: the registrations with their matcher front on the 8-bit path
against the same calls on the fp32 path.

    python tools/bench_match_bits.py --out profiles/match_bits.json [--reps 30] [--warmup 5]

register_planar, register_epipolar and register_pnp on the scene of tools/bench_epipolar.py (60 % of the records see the
same 3-D points from two cameras) at 4,096 and 32,768 records a side, L2 distance, 10,000 hypotheses, with the cross-check
off and on; per call and setting, bits 32 and bits 8 alternate repetition by repetition in one process, each on a context
of its own, after `warmup` rounds of both.  One repetition is one blocking call (its one synchronisation included), timed
with the host clock.  Then register_pose_batch over 64 frames of 4,096 records (63 consecutive pairs), cross-check off.
register_pnp reads coords3D of a plane at one depth, not the scene's points: its figures time the call, its pose means
nothing.  Per route: median, min, 10th and 90th percentile, `spread_us` = p90 - p10; `bits8_over_bits32` is the ratio of medians.
A record, not an assertion.  The C ABI only, no torch.
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
from bench_epipolar import LOOPS, SEED, SIZES, frames  # noqa: E402
from bench_match8 import stats  # noqa: E402

SEQUENCE = (64, 4096)  # frames, records per frame


def with_xyz(f, depth=5.0):
    f["coords3D"] = np.c_[(f["coords2D"][:, 0] - 640) / 1000 * depth, (f["coords2D"][:, 1] - 480) / 1000 * depth,
                          np.full(len(f), depth)].astype(np.float32)
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert a.reps >= 20 and a.warmup >= 3
    from cusift_amd import capi

    cam = capi.Camera(1000.0, 1000.0, 640.0, 480.0)
    ctxs = {32: capi.Context(0), 8: capi.Context(0)}
    ctxs[8].set_match_bits(8)
    cases = {}
    try:
        for n in SIZES:
            f1, f2 = frames(capi, n)
            f1 = with_xyz(f1)
            bufs = {b: (capi.DeviceBuffer.from_numpy(c, f1), capi.DeviceBuffer.from_numpy(c, f2)) for b, c in ctxs.items()}
            calls = {
                "register_planar": lambda c, d1, d2: c.register_planar(d1.ptr, n, d2.ptr, n, distance=1, loops=LOOPS, seed=SEED),
                "register_epipolar": lambda c, d1, d2: c.register_epipolar(d1.ptr, n, d2.ptr, n, distance=1, loops=LOOPS,
                                                                          seed=SEED),
                "register_pnp": lambda c, d1, d2: c.register_pnp(d1.ptr, n, d2.ptr, n, cam, distance=1, loops=LOOPS, seed=SEED)}
            for cross in (False, True):
                for c in ctxs.values():
                    c.set_cross_check(cross)
                for name, call in calls.items():
                    times, last = {32: [], 8: []}, {}
                    for i in range(a.warmup + a.reps):
                        for bits, c in ctxs.items():
                            c.synchronize()
                            t0 = time.perf_counter()
                            last[bits] = call(c, *bufs[bits])
                            t = (time.perf_counter() - t0) * 1e6
                            if i >= a.warmup:
                                times[bits].append(t)
                    st = {b: stats(times[b]) for b in times}
                    cases["%s, %d x %d, cross-check %s" % (name, n, n, "on" if cross else "off")] = {
                        "bits_32": dict(st[32], candidates=int(last[32].num_candidates), inliers=int(last[32].num_matches)),
                        "bits_8": dict(st[8], candidates=int(last[8].num_candidates), inliers=int(last[8].num_matches)),
                        "bits8_over_bits32": round(st[8]["median_us"] / st[32]["median_us"], 3)}
            for pair in bufs.values():
                for b in pair:
                    b.free()
        # the 64-frame pose sequence: every frame is the scene's frame 1 or frame 2 in turn
        n_frames, per = SEQUENCE
        f1, f2 = frames(capi, per)
        pts = np.stack([f1 if k % 2 == 0 else f2 for k in range(n_frames)])
        pairs = np.array([(k, k + 1) for k in range(n_frames - 1)], np.int32)
        times = {32: [], 8: []}
        dev = {b: capi.DeviceBuffer.from_numpy(c, pts) for b, c in ctxs.items()}
        for c in ctxs.values():
            c.set_cross_check(False)
        for i in range(a.warmup + a.reps):
            for bits, c in ctxs.items():
                c.synchronize()
                t0 = time.perf_counter()
                c.register_pose_batch(dev[bits].ptr, None, n_frames, per, pairs, cam, distance=1, loops=LOOPS, seed=SEED,
                                      want_inliers=False)
                t = (time.perf_counter() - t0) * 1e6
                if i >= a.warmup:
                    times[bits].append(t)
        st = {b: stats(times[b]) for b in times}
        cases["register_pose_batch, %d frames x %d, %d pairs, cross-check off" % (n_frames, per, len(pairs))] = {
            "bits_32": st[32], "bits_8": st[8], "bits8_over_bits32": round(st[8]["median_us"] / st[32]["median_us"], 3)}
        for b in dev.values():
            b.free()
    finally:
        for c in ctxs.values():
            c.close()
    rec = {"tool": "tools/bench_match_bits.py", "unit": "microseconds per blocking call (host clock)", "reps": a.reps,
           "warmup": a.warmup, "distance": "L2", "loops": LOOPS, "cases": cases}
    text = json.dumps(rec, indent=1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
