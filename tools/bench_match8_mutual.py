#!/usr/bin/env python3
"""Timing record of the mutual 8-bit matcher on one MI355X.  The method of tools/bench_match8.py.

    python tools/bench_match8_mutual.py --out profiles/match8_mutual.json [--reps 30] [--warmup 5]

Three routes that leave both record sets with their five match fields, in the same process, interleaved repetition by
repetition (M, F, A, M, F, A, ...), after `warmup` rounds of all three:
  M  cusift_match8_mutual(1, 2)                        match8_mutual_kernel (+ the column merge): one pass over the scores
  F  cusift_match8(1, 2), then cusift_match8(2, 1)     the row-side kernel twice; by the symmetry of the integer keys the
                                                       same bytes as M (checked after the timing, an assertion)
  A  cusift_match_mutual(1, 2)                         the fp32 mutual matcher
on n x n synthetic unit descriptors (two independent sets), L2 distance, n = 4096 and 32768.  One repetition is `inner`
back-to-back calls of the route between two stream synchronisations, timed with the host clock and divided by `inner`.  Per
route: median, min, 10th and 90th percentile; `spread_us` is p90 - p10.  `one_pass_wins` is the decision rule of the
one-pass kernel: M's median below F's by more than the two routes' spreads together.  A record, not an assertion (except
the equality of bytes).  The C ABI only, no torch.
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
from bench_match8 import stats, unit_descriptors  # noqa: E402

SIZES = ((4096, 10), (32768, 4))  # (n, inner calls per repetition)
FIELDS = ("score", "ambiguity", "match", "match_xpos", "match_ypos")


class Pair:
    """Two record sets per route and the byte tables on the device."""

    def __init__(self, capi, ctx, n):
        self.capi, self.ctx, self.n = capi, ctx, n
        s1, s2 = unit_descriptors(capi, n, 5), unit_descriptors(capi, n, 6)
        B = capi.DeviceBuffer
        self.d = {r: (B.from_numpy(ctx, s1), B.from_numpy(ctx, s2)) for r in "MFA"}
        self.q = [B(ctx, n * 128), B(ctx, n * 128)]
        self.s = [B(ctx, n * 8), B(ctx, n * 8)]
        ctx.quantize_descriptors(self.d["M"][0].ptr, n, self.q[0].ptr, self.s[0].ptr)
        ctx.quantize_descriptors(self.d["M"][1].ptr, n, self.q[1].ptr, self.s[1].ptr)
        ctx.synchronize()

    def route(self, r):
        n, (d1, d2) = self.n, self.d[r]
        t1, t2 = (self.q[0].ptr, self.s[0].ptr), (self.q[1].ptr, self.s[1].ptr)
        if r == "M":
            self.ctx.match8_mutual(d1.ptr, n, *t1, d2.ptr, n, *t2, 1)
        elif r == "F":
            self.ctx.match8(d1.ptr, n, *t1, d2.ptr, n, *t2, 1)
            self.ctx.match8(d2.ptr, n, *t2, d1.ptr, n, *t1, 1)
        else:
            self.ctx.match_mutual(d1.ptr, n, d2.ptr, n, 1)

    def fields(self, r):
        return [b.to_numpy(self.capi.SIFT_POINT_DTYPE, self.n) for b in self.d[r]]

    def free(self):
        for b in [x for pair in self.d.values() for x in pair] + self.q + self.s:
            b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    assert a.reps >= 20 and a.warmup >= 3
    from cusift_amd import capi

    cases = {}
    with capi.Context(0) as ctx:
        for n, inner in SIZES:
            pair = Pair(capi, ctx, n)

            def once(r):
                ctx.synchronize()
                t0 = time.perf_counter()
                for _ in range(inner):
                    pair.route(r)
                ctx.synchronize()
                return (time.perf_counter() - t0) * 1e6 / inner

            times = {r: [] for r in "MFA"}
            for i in range(a.warmup + a.reps):
                for r in "MFA":
                    t = once(r)
                    if i >= a.warmup:
                        times[r].append(t)
            m, f, fp = pair.fields("M"), pair.fields("F"), pair.fields("A")
            for side in range(2):
                for name in FIELDS:
                    assert np.ascontiguousarray(m[side][name]).tobytes() == np.ascontiguousarray(f[side][name]).tobytes(), \
                        (n, side, name)
            st = {r: stats(times[r]) for r in times}
            spreads = st["M"]["spread_us"] + st["F"]["spread_us"]
            cases["%d x %d" % (n, n)] = {
                "inner_calls_per_repetition": inner,
                "M_match8_mutual": st["M"], "F_match8_forward_then_swapped": st["F"], "A_match_mutual_fp32": st["A"],
                "M_over_F": round(st["M"]["median_us"] / st["F"]["median_us"], 3),
                "M_over_A": round(st["M"]["median_us"] / st["A"]["median_us"], 3),
                "F_minus_M_us": round(st["F"]["median_us"] - st["M"]["median_us"], 1),
                "sum_of_spreads_M_F_us": round(spreads, 1),
                "one_pass_wins": bool(st["F"]["median_us"] - st["M"]["median_us"] > spreads),
                "M_bytes_equal_F_bytes": True,
                "share_of_columns_with_the_fp32_match": round(float((m[1]["match"] == fp[1]["match"]).mean()), 4)}
            pair.free()
    rec = {"tool": "tools/bench_match8_mutual.py", "unit": "microseconds per call of the route (host clock around `inner` "
           "calls between two stream synchronisations, divided by `inner`)", "reps": a.reps, "warmup": a.warmup,
           "distance": "L2", "cases": cases}
    text = json.dumps(rec, indent=1)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
