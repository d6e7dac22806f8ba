#!/usr/bin/env python3
"""vse_yuv_to_bgr_format alone: achieved bytes per second, read plus written, of each new kernel path, with vse_yuv420_to_bgr's 16-byte
kernel as the yardstick on the same box and in the same run.

`--frames` x 1080 x 1920 device-resident frames of each format into a contiguous output, HIP events over `--iters` launches after warm-up;
bytes = the packed frame read once + 3 per pixel written.  The rows alternate for `--rounds` rounds, so the spread between a row's
repeats is the run's own noise: a new path counts as slower than the yardstick only if it falls below it by more than that.
  16-byte kernel, 8-bit I420              the yardstick (vse_yuv420_to_bgr)
  16-byte kernel, yuv420p10le / p010le    the new fast paths
  general kernel, yuv422p / yuv444p       the 8-bit formats that have no fast kernel: what one would have to beat
  general kernel, yuv420p10le at w=1918 / yuv444p10le / gray10le
One JSON line per measurement, then one summary line per row."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from vse_amd import engine, ingest


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
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    ctx = engine.Context(0)
    n = a.frames
    rng = np.random.default_rng(0)
    rows = [("16-byte kernel, 8-bit i420 (yardstick)", None, 1080, 1920), ("16-byte kernel", "yuv420p10le", 1080, 1920),
            ("16-byte kernel", "p010le", 1080, 1920), ("general kernel", "yuv422p", 1080, 1920), ("general kernel", "yuv444p", 1080, 1920),
            ("general kernel (w % 16 != 0)", "yuv420p10le", 1080, 1918), ("general kernel", "yuv444p10le", 1080, 1920),
            ("general kernel", "gray10le", 1080, 1920), ("general kernel", "yuvj420p", 1080, 1920)]
    runs = []
    for name, pix_fmt, h, w in rows:
        fmt = ingest.YuvFormat() if pix_fmt is None else ingest.YuvFormat.from_pix_fmt(pix_fmt, matrix="bt709")
        frame = fmt.frame_bytes(h, w)
        assert frame == ctx.lib.vse_yuv_frame_bytes(h, w, fmt.sub_x, fmt.sub_y, fmt.chroma, fmt.depth, 0)
        stride = (frame + 15) & ~15
        packed = torch.from_numpy(rng.integers(0, 256, size=(n, stride), dtype=np.uint8)).to(ctx.tdev)
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=ctx.tdev)
        if pix_fmt is None:
            fn = lambda packed=packed, out=out, h=h, w=w: ctx.yuv420_to_bgr(packed, n, h, w, "i420", 0, out=out)          # noqa: E731
        else:
            fn = lambda packed=packed, out=out, h=h, w=w, fmt=fmt: ctx.yuv_to_bgr(packed, n, h, w, fmt, 0, out=out)       # noqa: E731
        runs.append((name, pix_fmt or "yuv420p", h, w, n * (frame + 3 * h * w), fn, []))
    for r in range(a.rounds):
        for name, pix_fmt, h, w, moved, fn, rates in runs:
            us = timed(fn, a.iters)
            rates.append(moved / us / 1e6)
            print(json.dumps({"what": name, "pix_fmt": pix_fmt, "round": r, "frames": n, "h": h, "w": w, "us_per_batch": round(us, 1),
                              "us_per_frame": round(us / n, 2), "mb_moved": round(moved / 1e6, 1), "tb_per_s": round(rates[-1], 3)}), flush=True)
    base = runs[0][6]
    for name, pix_fmt, h, w, moved, _fn, rates in runs:
        print(json.dumps({"summary": name, "pix_fmt": pix_fmt, "w": w, "tb_per_s_median": round(float(np.median(rates)), 3),
                          "tb_per_s_min": round(min(rates), 3), "tb_per_s_max": round(max(rates), 3),
                          "median_over_yardstick": round(float(np.median(rates) / np.median(base)), 3)}), flush=True)


if __name__ == "__main__":
    main()
