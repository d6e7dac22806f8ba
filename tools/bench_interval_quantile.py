#!/usr/bin/env python3
"""Device time of the interval rank (vse_interval_rank) beside its yardstick, the interval composite (vse_interval_accumulate with a
reset + vse_interval_composite) over the same K frames, on the 1080p default subtitle band of tools/bench_interval_composite.py
(rows 842:1069, columns 96:1824), for K in 5, 15, 31, 63 in one process.  After a warm-up of both, blocks of `calls` calls of the one
and of the other alternate between device events, `rounds` times; the medians of the blocks are reported as ms per call, GB/s over the
area's pixels of the K frames (what either kernel has to read), and the ratio rank / yardstick.  The frames are seeded random bytes
on the device, the same for both.  --shift 1 moves the area one pixel to the right: its rows are no longer 4-byte (or 16-byte) aligned,
so both kernels' general loads are timed.  One JSON line per K.

usage: python tools/bench_interval_quantile.py [--shift 0] [--calls 200] [--rounds 15] [--height 1080] [--width 1920] [--samples 5,15,31,63]"""
import argparse
import json
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vse_amd import engine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shift", type=int, default=0, help="move the area this many pixels to the right (1: the general loads are timed)")
    ap.add_argument("--calls", type=int, default=200, help="calls per timed block")
    ap.add_argument("--rounds", type=int, default=15, help="timed blocks per kernel and K; the median is reported")
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--samples", default="5,15,31,63")
    a = ap.parse_args()
    ks = [int(k) for k in a.samples.split(",")]
    ctx = engine.Context(0)
    h, w = a.height, a.width
    y0, y1, x0, x1 = int(0.78 * h), int(0.99 * h), int(0.05 * w) + a.shift, int(0.95 * w) + a.shift
    area, ah, aw = (y0, y1, x0, x1), y1 - y0, x1 - x0
    gen = torch.Generator(device=ctx.tdev)
    gen.manual_seed(1)
    dev = torch.randint(0, 256, (max(ks), h, w, 3), dtype=torch.uint8, device=ctx.tdev, generator=gen)
    state = ctx.interval_state(ah, aw)
    out = torch.empty((ah, aw, 3), dtype=torch.uint8, device=ctx.tdev)

    def rank(k):
        ctx.interval_rank(dev[:k], area, k // 2, out=out)

    def yardstick(k):
        ctx.interval_accumulate(dev[:k], area, state, reset=True)
        ctx.interval_composite(state, ah, aw, k, "min", out=out)

    def block(fn, k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            fn(k)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.calls

    for k in ks:
        for _ in range(3):
            block(rank, k), block(yardstick, k)
        times = {"rank": [], "yardstick": []}
        for _ in range(a.rounds):
            times["rank"].append(block(rank, k))
            times["yardstick"].append(block(yardstick, k))
        ms = {name: statistics.median(v) for name, v in times.items()}
        read_bytes = k * ah * aw * 3
        print(json.dumps({"samples": k, "rank": k // 2, "frame": [h, w], "area": list(area), "shift": a.shift,
                          "rank_ms": round(ms["rank"], 4), "rank_ms_min": round(min(times["rank"]), 4),
                          "yardstick_ms": round(ms["yardstick"], 4), "yardstick_ms_min": round(min(times["yardstick"]), 4),
                          "rank_gb_per_s_area_pixels": round(read_bytes / ms["rank"] / 1e6, 1),
                          "yardstick_gb_per_s_area_pixels": round(read_bytes / ms["yardstick"] / 1e6, 1),
                          "ratio": round(ms["rank"] / ms["yardstick"], 2)}), flush=True)


if __name__ == "__main__":
    main()
