#!/usr/bin/env python3
"""Device time of the subtitle-change counts (vse_frame_change) per batch: `batch` synthetic 1080p frames on the device, the
reference's default subtitle area (rows 0.78-0.99 H, columns 0.05-0.95 W; backend/config.py:49), batches chained through one
state as the selector runs them.  Times `iters` calls between two device events (memset of the counts + the kernel per call)
and reports GB/s over the bytes of the area's rows (whole rows are what an area-rows-only upload holds).  Kernel time alone:
run it under `rocprofv3 --kernel-trace --stats` (frame_change_kernel).

usage: python tools/bench_frame_change.py [--batch 64] [--iters 200] [--height 1080] [--width 1920]"""
import argparse
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from vse_amd import engine, synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--edge-thresh", type=int, default=128)
    a = ap.parse_args()
    ctx = engine.Context(0)
    h, w = a.height, a.width
    y0, y1, x0, x1 = int(0.78 * h), int(0.99 * h), int(0.05 * w), int(0.95 * w)
    frames, _ = synth.make_clip([(None, a.batch // 4), ("the quick brown fox", a.batch // 4), ("the quick brown box", a.batch // 4),
                                 ("seven wizards", a.batch - 3 * (a.batch // 4))], h, w, seed=1)
    dev = torch.from_numpy(frames).to(ctx.tdev)
    state = ctx.frame_change_state(y1 - y0, x1 - x0)
    for k in range(10):
        ctx.frame_change(dev, (y0, y1, x0, x1), a.edge_thresh, state, reset=(k == 0))
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        out = ctx.frame_change(dev, (y0, y1, x0, x1), a.edge_thresh, state)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.iters
    area_bytes = a.batch * (y1 - y0) * w * 3            # whole rows of the area
    read_bytes = a.batch * (y1 - y0) * (x1 - x0) * 3    # the pixels the kernel needs
    print(json.dumps({"batch": a.batch, "frame": [h, w], "area": [y0, y1, x0, x1], "ms_per_batch": round(ms, 4),
                      "area_row_mb": round(area_bytes / 1e6, 1), "gb_per_s_area_rows": round(area_bytes / ms / 1e6, 1),
                      "gb_per_s_area_pixels": round(read_bytes / ms / 1e6, 1),
                      "edges_per_frame": int(np.asarray(out.cpu())[:, 0].max())}), flush=True)


if __name__ == "__main__":
    main()
