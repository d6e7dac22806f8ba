#!/usr/bin/env python3
"""vse_yuv_deinterlace alone, and what it costs the host-fed selector pass.

Kernel: `--frames` x 1080 x W device-resident pictures, each with the one before it as its previous picture (one buffer, d_prev = d_yuv -
stride), into a second buffer; HIP events over `--iters` launches after warm-up.  Bytes = three packed pictures per frame (read C, read P,
write), the least the rule can move.  Each row is set against vse_yuv_to_bgr_format on the same frames in the same run (bytes = the packed
picture + 3 per pixel), and the rows alternate for `--rounds` rounds, so the spread between a row's repeats is the run's own noise.
  yuv420p, yuv420p10le at w = 1920        the 16-byte kernel
  yuv420p, yuv420p10le at w = 1918        the general kernel
Selector pass (`--pass-frames` > 0): the change selector on the engine over a 1080 x 1920 yuv420p clip held in host memory (`--pass-frames`
pictures, `--pass-repeats` times over), its lower quarter staged through staging.Uploader, as plain YuvFrames (the progressive pass: what
runs without --deinterlace), as InterlacedYuvFrames mode adaptive and mode interpolate; frames per second of the whole pass, alternating
for `--rounds` rounds.
One JSON line per measurement, then one summary line per row."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from vse_amd import engine, extractor, frame_select, ingest, staging


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


def summary(name, rates, unit, more):
    print(json.dumps({"summary": name, **more, f"{unit}_median": round(float(np.median(rates)), 3), f"{unit}_min": round(min(rates), 3),
                      f"{unit}_max": round(max(rates), 3)}), flush=True)


def kernels(ctx, a):
    n = a.frames
    rng = np.random.default_rng(0)
    runs = []
    for kernel, pix_fmt, w in (("16-byte", "yuv420p", 1920), ("16-byte", "yuv420p10le", 1920), ("general", "yuv420p", 1918), ("general", "yuv420p10le", 1918)):
        h = 1080
        fmt = ingest.YuvFormat.from_pix_fmt(pix_fmt, matrix="bt709")
        frame = fmt.frame_bytes(h, w)
        stride = (frame + 15) & ~15 if kernel == "16-byte" else frame
        buf = torch.from_numpy(rng.integers(0, 256, size=(n + 1) * stride, dtype=np.uint8)).to(ctx.tdev)
        cur = buf[stride:].as_strided((n, stride), (stride, 1))
        out = torch.empty((n, stride), dtype=torch.uint8, device=ctx.tdev)
        bgr = torch.empty((n, h, w, 3), dtype=torch.uint8, device=ctx.tdev)
        common = dict(pix_fmt=pix_fmt, w=w, kernel=kernel)
        runs.append(("vse_yuv_deinterlace", common, 3 * n * frame, [],
                     lambda cur=cur, buf=buf, out=out, h=h, w=w, fmt=fmt: ctx.yuv_deinterlace(cur, n, h, w, fmt, prev=buf, out=out)))
        runs.append(("vse_yuv_to_bgr_format (yardstick)", common, n * (frame + 3 * h * w), [],
                     lambda cur=cur, bgr=bgr, h=h, w=w, fmt=fmt: ctx.yuv_to_bgr(cur, n, h, w, fmt, 0, out=bgr)))
    for r in range(a.rounds):
        for name, common, moved, rates, fn in runs:
            us = timed(fn, a.iters)
            rates.append(moved / us / 1e6)
            print(json.dumps({"what": name, **common, "round": r, "frames": n, "us_per_batch": round(us, 1), "us_per_frame": round(us / n, 2),
                              "mb_moved": round(moved / 1e6, 1), "tb_per_s": round(rates[-1], 3)}), flush=True)
    for name, common, moved, rates, _fn in runs:
        summary(name, rates, "tb_per_s", {**common, "us_per_frame_median": round(moved / float(np.median(rates)) / 1e6 / n, 2)})


def selector_pass(ctx, a):
    h, w, n = 1080, 1920, a.pass_frames
    rng = np.random.default_rng(1)
    fmt = ingest.YuvFormat(matrix="bt709")
    base = [rng.integers(16, 236, size=shp, dtype=np.uint8) for shp in fmt.plane_shapes(h, w)]
    clip = []
    for k in range(n):                    # a still picture, a band of which changes every frame: both branches of the rule run
        planes = [p.copy() for p in base]
        planes[0][h - 200 + (k % 8) * 8:h - 200 + (k % 8) * 8 + 8] = rng.integers(16, 236, size=(8, w), dtype=np.uint8)
        clip.append(tuple(planes))
    area = extractor.SubtitleArea(ymin=int(0.75 * h), ymax=h, xmin=0, xmax=w)

    total = n * a.pass_repeats                # the pictures in turn, `--pass-repeats` times over: a pass long enough to time

    def frames_of(kind):
        if kind == "progressive":
            return [ingest.YuvFrame(clip[k % n], h, w, fmt) for k in range(total)]
        return [ingest.InterlacedYuvFrame(clip[k % n], h, w, fmt, clip[(k - 1) % n] if k else None, "tff", kind) for k in range(total)]
    kinds = {"progressive": [], "adaptive": [], "interpolate": []}
    up = staging.Uploader(ctx.tdev, ctx=ctx)
    try:
        for r in range(a.rounds + 1):                 # round 0 warms the slabs and the allocator up and is not counted
            for kind, rates in kinds.items():
                frames = frames_of(kind)
                sel = frame_select.ChangeFrameSelector(frame_select.EngineCounter(ctx), batch=a.batch)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sel.run(frames, area, uploader=up)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if r:
                    rates.append(total / dt)
                    print(json.dumps({"what": "selector pass, host-fed", "frames_as": kind, "round": r - 1, "frames": total, "seconds": round(dt, 4),
                                      "frames_per_s": round(total / dt, 1)}), flush=True)
    finally:
        up.close()
    for kind, rates in kinds.items():
        summary("selector pass, host-fed", rates, "frames_per_s", {"frames_as": kind, "over_progressive": round(
            float(np.median(rates) / np.median(kinds["progressive"])), 3)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--pass-frames", type=int, default=96, help="distinct pictures of the selector pass's clip; 0 skips it")
    ap.add_argument("--pass-repeats", type=int, default=64, help="how many times the selector pass goes through them")
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    ctx = engine.Context(0)
    kernels(ctx, a)
    if a.pass_frames > 0:
        selector_pass(ctx, a)


if __name__ == "__main__":
    main()
