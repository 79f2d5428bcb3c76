#!/usr/bin/env python3
"""Timing record of the 8-bit matcher on one MI355X: cusift_match8 against cusift_match on the same record sets, and the
quantiser's throughput.  The method of tools/bench_match_guided.py.

    python tools/bench_match8.py --out profiles/match8.json [--reps 30] [--warmup 5]
    python tools/bench_match8.py --regs-into profiles/match8.json      # needs hipcc, no GPU
    python tools/bench_match8.py --trace-loop 32768 20                  # the kernel-trace run: nothing but the two calls

Two routes, in the same process, interleaved repetition by repetition (A, B, A, B, ...), after `warmup` rounds of both:
  A  cusift_match(s1, s2)              match_kernel (fp32-input MFMA), which this feature does not change
  B  cusift_match8(q1, q2)             match8_kernel (int8 MFMA) on the tables cusift_quantize_descriptors made of s1, s2
on n x n synthetic unit descriptors (two independent sets), L2 distance, n = 4096 and 32768.  One repetition is `inner`
back-to-back calls of the route between two stream synchronisations, timed with the host clock and divided by `inner`.  Per
route: median, min, 10th and 90th percentile; `spread_us` is p90 - p10 of that route's repetitions.  `B_over_A` is the ratio
of medians; `faster_beyond_spreads` says whether A's median minus B's exceeds the sum of the two spreads.  After the timing
route B's rows are compared with route A's: the share of equal `match` and the largest score difference (a record of how
far quantisation moves the result on this data, not an assertion).
The quantiser: cusift_quantize_descriptors over 64 x 4096 records, the same timing; GB/s against the bytes it must move,
512 in and 136 out per record.
--regs-into adds VGPRs, LDS bytes and waves per SIMD of the kernels of sift_match8.hip and of match_kernel to a record.
A record, not an assertion.  The C ABI only, no torch.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = ((4096, 10), (32768, 4))  # (n, inner calls per repetition)
QUANT = (64, 4096, 10)  # images, records per image, inner calls


def unit_descriptors(capi, n, seed):
    rng = np.random.default_rng(seed)
    p = np.zeros(n, dtype=capi.SIFT_POINT_DTYPE)
    d = np.abs(rng.normal(size=(n, 128))).astype(np.float32)
    p["data"] = d / np.linalg.norm(d, axis=1, keepdims=True)
    p["coords2D"] = rng.uniform(0, 1000, (n, 2)).astype(np.float32)
    return p


def stats(us):
    us = np.asarray(us)
    return {"median_us": round(float(np.median(us)), 1), "min_us": round(float(us.min()), 1),
            "p10_us": round(float(np.percentile(us, 10)), 1), "p90_us": round(float(np.percentile(us, 90)), 1),
            "spread_us": round(float(np.percentile(us, 90) - np.percentile(us, 10)), 1)}


def kernel_resources():
    rows = {}
    for unit, needles in (("sift_match8.hip", []), ("sift_match.hip", ["12match_kernel"])):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), unit] + needles,
                             capture_output=True, text=True, timeout=600)
        lines = out.stdout.splitlines()
        head = lines[0].split() if lines else []
        for line in lines[1:]:
            cells = line.split()
            if len(cells) == len(head):
                rows[cells[0]] = {k: int(v) for k, v in zip(head[1:], cells[1:])}
    return rows


class Pair:
    """Two record sets and their byte tables on the device."""

    def __init__(self, capi, ctx, n):
        self.capi, self.ctx, self.n = capi, ctx, n
        s1, s2 = unit_descriptors(capi, n, 5), unit_descriptors(capi, n, 6)
        B = capi.DeviceBuffer
        self.d2 = B.from_numpy(ctx, s2)
        self.d1 = {"A": B.from_numpy(ctx, s1), "B": B.from_numpy(ctx, s1)}
        self.q = [B(ctx, n * 128), B(ctx, n * 128)]
        self.s = [B(ctx, n * 8), B(ctx, n * 8)]
        ctx.quantize_descriptors(self.d1["B"].ptr, n, self.q[0].ptr, self.s[0].ptr)
        ctx.quantize_descriptors(self.d2.ptr, n, self.q[1].ptr, self.s[1].ptr)
        ctx.synchronize()

    def route(self, r):
        n = self.n
        if r == "A":
            self.ctx.match(self.d1[r].ptr, n, self.d2.ptr, n, 1)
        else:
            self.ctx.match8(self.d1[r].ptr, n, self.q[0].ptr, self.s[0].ptr, self.d2.ptr, n, self.q[1].ptr, self.s[1].ptr, 1)

    def free(self):
        for b in list(self.d1.values()) + [self.d2] + self.q + self.s:
            b.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--regs-into", default=None, help="add the kernels' VGPRs and LDS to this record (needs hipcc)")
    ap.add_argument("--trace-loop", nargs=2, type=int, metavar=("N", "CALLS"), default=None,
                    help="CALLS alternating calls of both routes at N x N and nothing else: the run to put under a kernel trace")
    a = ap.parse_args()
    if a.regs_into:
        rec = json.load(open(a.regs_into)) if os.path.exists(a.regs_into) else {
            "tool": "tools/bench_match8.py", "cases": "not measured yet: no timed run of this tool is recorded"}
        rec["kernel_resources"] = kernel_resources()
        with open(a.regs_into, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")
        print(json.dumps(rec["kernel_resources"], indent=1))
        return
    from cusift_amd import capi

    if a.trace_loop:
        with capi.Context(0) as ctx:
            pair = Pair(capi, ctx, a.trace_loop[0])
            for _ in range(a.trace_loop[1]):
                pair.route("A")
                pair.route("B")
            ctx.synchronize()
            pair.free()
        return
    assert a.reps >= 20 and a.warmup >= 3
    cases = {}
    with capi.Context(0) as ctx:
        for n, inner in SIZES:
            pair = Pair(capi, ctx, n)

            def once(call):
                ctx.synchronize()
                t0 = time.perf_counter()
                for _ in range(inner):
                    call()
                ctx.synchronize()
                return (time.perf_counter() - t0) * 1e6 / inner

            times = {"A": [], "B": []}
            for i in range(a.warmup + a.reps):
                for r in ("A", "B"):
                    t = once(lambda: pair.route(r))
                    if i >= a.warmup:
                        times[r].append(t)
            fa = pair.d1["A"].to_numpy(capi.SIFT_POINT_DTYPE, n)
            fb = pair.d1["B"].to_numpy(capi.SIFT_POINT_DTYPE, n)
            st = {r: stats(times[r]) for r in times}
            ops = 2.0 * n * n * 128
            cases["%d x %d" % (n, n)] = {
                "inner_calls_per_repetition": inner,
                "A_match_fp32": dict(st["A"], tflops=round(ops / st["A"]["median_us"] / 1e6, 1)),
                "B_match8_int8": dict(st["B"], tops=round(ops / st["B"]["median_us"] / 1e6, 1)),
                "B_over_A": round(st["B"]["median_us"] / st["A"]["median_us"], 3),
                "A_minus_B_us": round(st["A"]["median_us"] - st["B"]["median_us"], 1),
                "sum_of_spreads_us": round(st["A"]["spread_us"] + st["B"]["spread_us"], 1),
                "faster_beyond_spreads": bool(st["A"]["median_us"] - st["B"]["median_us"] >
                                              st["A"]["spread_us"] + st["B"]["spread_us"]),
                "share_of_rows_with_the_fp32_match": round(float((fa["match"] == fb["match"]).mean()), 4),
                "largest_score_difference": round(float(np.abs(fa["score"] - fb["score"]).max()), 5)}
            pair.free()
        # the quantiser
        n_img, per, inner = QUANT
        pts = capi.DeviceBuffer.from_numpy(ctx, unit_descriptors(capi, n_img * per, 7))
        dq, ds = capi.DeviceBuffer(ctx, n_img * per * 128), capi.DeviceBuffer(ctx, n_img * per * 8)
        tq = []
        for i in range(a.warmup + a.reps):
            ctx.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                ctx.quantize_descriptors(pts.ptr, per, dq.ptr, ds.ptr, n_images=n_img)
            ctx.synchronize()
            if i >= a.warmup:
                tq.append((time.perf_counter() - t0) * 1e6 / inner)
        sq = stats(tq)
        moved = n_img * per * (512 + 136)
        quant = dict(sq, images=n_img, records_per_image=per, inner_calls_per_repetition=inner, bytes_moved=moved,
                     gb_per_s=round(moved / sq["median_us"] / 1e3, 1))
        for b in (pts, dq, ds):
            b.free()
    rec = {"tool": "tools/bench_match8.py", "unit": "microseconds per call of the route (host clock around `inner` "
           "calls between two stream synchronisations, divided by `inner`)", "reps": a.reps, "warmup": a.warmup,
           "distance": "L2", "cases": cases, "quantize_descriptors": quant}
    if a.out and os.path.exists(a.out):  # keep what --regs-into and the trace left in the record
        old = json.load(open(a.out))
        for k in ("kernel_resources", "kernel_trace"):
            if k in old:
                rec[k] = old[k]
    text = json.dumps(rec, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
