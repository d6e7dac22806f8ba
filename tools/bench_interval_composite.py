#!/usr/bin/env python3
"""Device time of the interval composite (vse_interval_accumulate + vse_interval_composite) per batch: the synthetic 1080p batch and the
default subtitle area of tools/bench_frame_change.py (rows 0.78-0.99 H, columns 0.05-0.95 W), so the two tools read the same area
bytes and their GB/s compare directly.  Times `iters` x (one accumulate of the whole batch continuing the state + one composite)
between two device events and reports GB/s over the area's pixels (what the kernel reads) and over the bytes of the area's rows
(what an area-rows-only upload holds).  The default batch (78 MB of area rows) stays resident in the 256 MiB Infinity Cache;
--batch 256 (312 MB) does not.  Kernel time alone: run it under `rocprofv3 --kernel-trace --stats` (interval_accumulate_kernel).

usage: python tools/bench_interval_composite.py [--batch 64] [--iters 200] [--height 1080] [--width 1920] [--mode min|max|mean] [--shift 0]"""
import argparse
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vse_amd import engine, synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--mode", choices=sorted(engine.INTERVAL_MODES), default="min")
    ap.add_argument("--shift", type=int, default=0, help="move the area this many pixels to the right (1: its rows are no longer 16-byte "
                    "aligned, so the general loads are timed)")
    a = ap.parse_args()
    ctx = engine.Context(0)
    h, w = a.height, a.width
    y0, y1, x0, x1 = int(0.78 * h), int(0.99 * h), int(0.05 * w) + a.shift, int(0.95 * w) + a.shift
    frames, _ = synth.make_clip([(None, a.batch // 4), ("the quick brown fox", a.batch // 4), ("the quick brown box", a.batch // 4),
                                 ("seven wizards", a.batch - 3 * (a.batch // 4))], h, w, seed=1)
    dev = torch.from_numpy(frames).to(ctx.tdev)
    del frames
    state = ctx.interval_state(y1 - y0, x1 - x0)
    out = torch.empty((y1 - y0, x1 - x0, 3), dtype=torch.uint8, device=ctx.tdev)
    for k in range(10):
        ctx.interval_accumulate(dev, (y0, y1, x0, x1), state, reset=(k == 0))
        ctx.interval_composite(state, y1 - y0, x1 - x0, a.batch, a.mode, out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        ctx.interval_accumulate(dev, (y0, y1, x0, x1), state)
        ctx.interval_composite(state, y1 - y0, x1 - x0, a.batch, a.mode, out=out)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.iters
    area_bytes = a.batch * (y1 - y0) * w * 3            # whole rows of the area
    read_bytes = a.batch * (y1 - y0) * (x1 - x0) * 3    # the pixels the kernel needs
    print(json.dumps({"batch": a.batch, "frame": [h, w], "area": [y0, y1, x0, x1], "mode": a.mode, "ms_per_batch": round(ms, 4),
                      "area_row_mb": round(area_bytes / 1e6, 1), "gb_per_s_area_rows": round(area_bytes / ms / 1e6, 1),
                      "gb_per_s_area_pixels": round(read_bytes / ms / 1e6, 1),
                      "state_mb": round(state.numel() / 1e6, 2), "composite_max": int(out.max())}), flush=True)


if __name__ == "__main__":
    main()
