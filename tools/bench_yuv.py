#!/usr/bin/env python3
"""vse_yuv420_to_bgr alone, and what staging a 4:2:0 batch saves against a BGR batch.

1. The kernel: `--frames` x 1080 x 1920 I420 and NV12 frames (the 16-byte kernel) into a contiguous output, HIP events over `--iters`
   launches after warm-up; bytes = 4.5 per pixel (1.5 read + 3 written).  Yardstick: torch copy_ moving the same number of bytes (read +
   written) in the same process, as tools/copy_ceiling.py does; kernel and copy alternate for `--rounds` rounds.  Also the general kernel
   at 1080 x 1918 and on an odd row parity.
2. The upload: the pinned -> device copy of the 1.5 bytes per pixel a 4:2:0 frame no longer sends, and staging.Uploader.stage of a whole
   batch (slab copy + upload + conversion) for BGR frames and for ingest.Yuv420Frames, per frame.
One JSON line per measurement."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from vse_amd import engine, ingest, staging


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    ctx = engine.Context(0)
    n = a.frames
    rng = np.random.default_rng(0)

    def kernel_row(name, h, w, layout, parity):
        frame = ctx.lib.vse_yuv420_frame_bytes(h, w, parity)
        stride = (frame + 15) & ~15
        packed = torch.from_numpy(rng.integers(0, 256, size=(n, stride), dtype=np.uint8)).to(ctx.tdev)
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=ctx.tdev)
        moved = n * h * w * 4.5
        x = torch.empty(int(moved) // 2, dtype=torch.uint8, device=ctx.tdev)
        y = torch.empty_like(x)
        for r in range(a.rounds):
            us = timed(lambda: ctx.yuv420_to_bgr(packed, n, h, w, layout, parity, out=out), a.iters)
            cp = timed(lambda: y.copy_(x), a.iters)
            print(json.dumps({"what": name, "round": r, "frames": n, "h": h, "w": w, "layout": layout, "row_parity": parity,
                              "us_per_batch": round(us, 1), "us_per_frame": round(us / n, 2), "mb_moved": round(moved / 1e6, 1),
                              "tb_per_s": round(moved / us / 1e6, 3), "copy_same_bytes_us": round(cp, 1),
                              "copy_tb_per_s": round(moved / cp / 1e6, 3), "kernel_over_copy_rate": round(cp / us, 3)}), flush=True)

    kernel_row("16-byte kernel", 1080, 1920, "i420", 0)
    kernel_row("16-byte kernel", 1080, 1920, "nv12", 0)
    kernel_row("general kernel (w % 16 != 0)", 1080, 1918, "i420", 0)
    kernel_row("general kernel (odd row parity)", 1079, 1920, "i420", 1)

    # ---- the upload a 4:2:0 frame no longer makes: 1.5 bytes per pixel ---------------------------------------------------------
    h, w = 1080, 1920
    half = h * w * 3 // 2
    pin = torch.empty((n, half), dtype=torch.uint8, pin_memory=True)
    dev = torch.empty((n, half), dtype=torch.uint8, device=ctx.tdev)
    for r in range(a.rounds):
        us = timed(lambda: dev.copy_(pin, non_blocking=True), 10)
        print(json.dumps({"what": "pinned -> device copy of the bytes no longer sent", "round": r, "frames": n, "mb_per_frame": round(half / 1e6, 2),
                          "us_per_batch": round(us, 1), "us_per_frame": round(us / n, 1), "gb_per_s": round(n * half / us / 1e3, 1)}), flush=True)
    bgr = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for _ in range(8)]
    yuv = [ingest.Yuv420Frame(tuple(np.ascontiguousarray(p) for p in ingest.bgr_to_yuv420(f)), h, w) for f in bgr]
    up = staging.Uploader(ctx.tdev, ctx=ctx)
    for r in range(a.rounds):
        for name, frames in (("bgr", bgr), ("i420", yuv)):
            batch = [frames[k % len(frames)] for k in range(n)]
            for _ in range(3):
                up.stage(batch).tensor()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5):
                up.stage(batch).tensor()
            torch.cuda.synchronize()
            us = (time.perf_counter() - t0) / 5 * 1e6
            print(json.dumps({"what": "Uploader.stage + wait, one batch at a time", "round": r, "source": name, "frames": n,
                              "us_per_batch": round(us, 1), "us_per_frame": round(us / n, 1)}), flush=True)
    up.close()


if __name__ == "__main__":
    main()
