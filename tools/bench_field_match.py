#!/usr/bin/env python3
"""vse_yuv_field_match alone, and what it costs the host-fed selector pass.

Kernel: `--frames` x 1080 x W device-resident pictures, each with the one before it as its previous picture (one buffer, d_prev = d_yuv -
stride), into a second buffer; HIP events over `--iters` calls after warm-up.  Two kinds of content: "film", smooth pictures dealt in 3:2
pulldown (every frame is matched: choices 0 and 1), and "video", random words (every frame combs and takes the adaptive fallback).  Byte
model of a matched frame: the count reads two luma planes, the weave reads one packed picture and writes one (2 luma + 2 pictures, about
3.3 pictures of 4:2:0); the fallback's weave reads two pictures (2 luma + 3 pictures).  The yardstick is vse_yuv_deinterlace, mode adaptive,
on the same film frames in the same job (3 pictures); the rows alternate for `--rounds` rounds, so the spread between a row's repeats is the
run's own noise.
  yuv420p, yuv420p10le at w = 1920        the 16-byte kernels
  yuv420p, yuv420p10le at w = 1918        the general kernels
Selector pass (`--pass-frames` > 0): the change selector on the engine over a telecined 1080 x 1920 yuv420p clip held in host memory
(`--pass-frames` pictures, `--pass-repeats` times over), its lower quarter staged through staging.Uploader, as plain YuvFrames (the
progressive pass: what runs without --deinterlace), as InterlacedYuvFrames mode adaptive and mode match; frames per second of the whole
pass, alternating for `--rounds` rounds.
One JSON line per measurement, then one summary line per row."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from vse_amd import engine, extractor, frame_select, ingest, staging, synth


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


def summary(name, values, unit, more):
    print(json.dumps({"summary": name, **more, f"{unit}_median": round(float(np.median(values)), 3), f"{unit}_min": round(min(values), 3),
                      f"{unit}_max": round(max(values), 3)}), flush=True)


def film_frames(rng, fmt, h, w, count):
    """`count` stored frames of a film of vertically smooth pictures (five levels 40 8-bit levels apart in turn, noise of 0..4 levels) in 3:2
    pulldown, top field first: a weave of one picture's fields combs nowhere, a weave of two pictures' fields everywhere."""
    unit = 1 << (fmt.depth - 8 + (16 - fmt.depth if fmt.msb else 0))
    base = [tuple(((30 + 40 * k) * unit + rng.integers(0, 5 * unit, size=shp)).astype(fmt.sample_dtype) for shp in fmt.plane_shapes(h, w)) for k in range(5)]
    film = [base[k % 5] for k in range((count + 4) // 5 * 4 + 4)]
    return synth.telecine(film, "32", "tff")[0][:count]


def packed_buffer(frames, fmt, stride, device):
    host = np.zeros(len(frames) * stride, np.uint8)
    for k, planes in enumerate(frames):
        h, w = planes[0].shape
        ingest.YuvFrame(planes, h, w, fmt).pack_into(host[k * stride:])
    return torch.from_numpy(host).to(device)


def kernels(ctx, a):
    n = a.frames
    rng = np.random.default_rng(0)
    runs = []
    for kernel, pix_fmt, w in (("16-byte", "yuv420p", 1920), ("16-byte", "yuv420p10le", 1920), ("general", "yuv420p", 1918), ("general", "yuv420p10le", 1918)):
        h = 1080
        fmt = ingest.YuvFormat.from_pix_fmt(pix_fmt, matrix="bt709")
        frame = fmt.frame_bytes(h, w)
        luma = h * w * fmt.sample_bytes
        stride = (frame + 15) & ~15 if kernel == "16-byte" else frame
        film = packed_buffer(film_frames(rng, fmt, h, w, n + 1), fmt, stride, ctx.tdev)
        video = torch.from_numpy(rng.integers(0, 256, size=(n + 1) * stride, dtype=np.uint8)).to(ctx.tdev)
        out = torch.empty((n, stride), dtype=torch.uint8, device=ctx.tdev)
        stats = torch.empty((n, 4), dtype=torch.int32, device=ctx.tdev)

        def view(buf, stride=stride):
            return buf[stride:].as_strided((n, stride), (stride, 1))
        common = dict(pix_fmt=pix_fmt, w=w, kernel=kernel)
        for content, buf, moved in (("film", film, 2 * luma + 2 * frame), ("video", video, 2 * luma + 3 * frame)):
            ctx.yuv_field_match(view(buf), n, h, w, fmt, prev=buf, out=out, stats=stats)
            choices = np.bincount(stats.cpu().numpy()[:, 3], minlength=4).tolist()
            runs.append(("vse_yuv_field_match", {**common, "content": content, "choices": choices}, n * moved, [],
                         lambda buf=buf, h=h, w=w, fmt=fmt, out=out, stats=stats, view=view: ctx.yuv_field_match(view(buf), n, h, w, fmt, prev=buf, out=out,
                                                                                                                    stats=stats)))
        runs.append(("vse_yuv_deinterlace adaptive (yardstick)", {**common, "content": "film"}, 3 * n * frame, [],
                     lambda buf=film, h=h, w=w, fmt=fmt, out=out, view=view: ctx.yuv_deinterlace(view(buf), n, h, w, fmt, prev=buf, out=out)))
    for r in range(a.rounds):
        for name, common, moved, us_frame, fn in runs:
            us = timed(fn, a.iters)
            us_frame.append(us / n)
            print(json.dumps({"what": name, **common, "round": r, "frames": n, "us_per_batch": round(us, 1), "us_per_frame": round(us / n, 2),
                              "mb_moved": round(moved / 1e6, 1), "tb_per_s": round(moved / us / 1e6, 3)}), flush=True)
    yard = {(c["pix_fmt"], c["w"]): float(np.median(v)) for name, c, _m, v, _f in runs if "yardstick" in name}
    for name, common, moved, us_frame, _fn in runs:
        med = float(np.median(us_frame))
        summary(name, us_frame, "us_per_frame", {**common, "tb_per_s_median": round(moved / n / med / 1e6, 3),
                                                 "over_adaptive": round(med / yard[common["pix_fmt"], common["w"]], 3)})


def selector_pass(ctx, a):
    h, w, n = 1080, 1920, a.pass_frames
    rng = np.random.default_rng(1)
    fmt = ingest.YuvFormat(matrix="bt709")
    clip = film_frames(rng, fmt, h, w, n)
    area = extractor.SubtitleArea(ymin=int(0.75 * h), ymax=h, xmin=0, xmax=w)
    total = n * a.pass_repeats                # the pictures in turn, `--pass-repeats` times over: a pass long enough to time

    def frames_of(kind):
        if kind == "progressive":
            return [ingest.YuvFrame(clip[k % n], h, w, fmt) for k in range(total)]
        return [ingest.InterlacedYuvFrame(clip[k % n], h, w, fmt, clip[(k - 1) % n] if k else None, "tff", kind) for k in range(total)]
    kinds = {"progressive": [], "adaptive": [], "match": []}
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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--pass-frames", type=int, default=95, help="distinct stored frames of the selector pass's clip (a multiple of 5 keeps the "
                    "cadence over the repeats); 0 skips it")
    ap.add_argument("--pass-repeats", type=int, default=32, help="how many times the selector pass goes through them")
    ap.add_argument("--batch", type=int, default=32)
    a = ap.parse_args()
    ctx = engine.Context(0)
    kernels(ctx, a)
    if a.pass_frames > 0:
        selector_pass(ctx, a)


if __name__ == "__main__":
    main()
