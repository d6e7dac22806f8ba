#!/usr/bin/env python3
"""Device time of the colour key (vse_colour_key) per batch, both forms, beside the selector's own pass (vse_frame_change) on the same
band in the same process, and the selector's host-fed pass with and without the key.  `batch` random 1080p frames on the device, two
cases: the band of rows 810:1080 and whole frames.  The fast form runs on packed frames (pitch 5760, 16-byte aligned); the general form
on the same bytes in buffers whose pitch is 5760 + 3 on both sides, so nothing is aligned.  The three alternate in `rounds` rounds of
`iters` calls each, every round timed between two device events; the general form's bytes are checked once against the fast form's.
Reports per-round ms, their medians and GB/s over the bytes read plus written (2 x 3 bytes per pixel for the key, 3 read for the
change pass).  The host-fed pass is ChangeFrameSelector over host frames through a staging.Uploader (band rows only), wall clock around
run(), alternating without / with EngineKey, `rounds` each.  No gate.  Kernel time alone: run it under `rocprofv3 --kernel-trace --stats`
(colour_key_fast_kernel, colour_key_general_kernel, frame_change_kernel).

usage: python tools/bench_colour_key.py [--batch 64] [--iters 200] [--rounds 5] [--height 1080] [--width 1920] [--clip-frames 1024]"""
import argparse
import json
import os
import statistics
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from vse_amd import engine, frame_select, staging


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def padded(ctx, n, h, w, pad):
    """An [n,h,w,3] view with row pitch 3 w + pad into a fresh buffer that starts one byte off."""
    pitch = 3 * w + pad
    buf = torch.empty(n * h * pitch + 1, dtype=torch.uint8, device=ctx.tdev)
    return buf[1:].as_strided((n, h, w, 3), (h * pitch, pitch, 3, 1))


def case(ctx, name, dev, area, key, iters, rounds):
    n, h, w, _ = dev.shape
    y0, y1, x0, x1 = area
    out = torch.empty_like(dev)
    slow_in, slow_out = padded(ctx, n, h, w, 3), padded(ctx, n, h, w, 3)
    slow_in.copy_(dev)
    state = ctx.frame_change_state(y1 - y0, x1 - x0)
    fns = {"key_fast": lambda: ctx.colour_key(dev, area, key, out=out),
           "key_general": lambda: ctx.colour_key(slow_in, area, key, out=slow_out),
           "frame_change": lambda: ctx.frame_change(dev, area, 128, state, reset=False)}
    for fn in fns.values():
        timed(fn, 3)
    assert torch.equal(out[:, y0:y1, x0:x1], slow_out[:, y0:y1, x0:x1]), "the two forms disagree"
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ms[k].append(timed(fn, iters))
    pixels = n * (y1 - y0) * (x1 - x0)
    moved = {"key_fast": 6 * pixels, "key_general": 6 * pixels, "frame_change": 3 * pixels}
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"case": name, "batch": n, "frame": [h, w], "area": list(area), "mb_read_plus_written": {k: round(v / 1e6, 1) for k, v in moved.items()},
            "ms_per_call": {k: [round(x, 4) for x in v] for k, v in ms.items()}, "median_ms": {k: round(v, 4) for k, v in med.items()},
            "gb_per_s_read_plus_written": {k: round(moved[k] / med[k] / 1e6, 1) for k in med},
            "key_fast_over_frame_change": round(med["key_fast"] / med["frame_change"], 3)}


def host_fed(ctx, frames, band, key, rounds, batch):
    """Wall clock of ChangeFrameSelector.run over host frames through an uploader, without and with the key, alternating."""
    s = {"plain": [], "keyed": []}
    up = staging.Uploader(ctx.tdev)
    frame_select.ChangeFrameSelector(frame_select.EngineCounter(ctx), batch=batch).run(frames[:2 * batch], band, 25.0, uploader=up)      # warm-up: pinned slabs
    for _ in range(rounds):
        for name, key_fn in (("plain", None), ("keyed", frame_select.EngineKey(ctx, key))):
            sel = frame_select.ChangeFrameSelector(frame_select.EngineCounter(ctx), batch=batch, key_fn=key_fn)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sel.run(frames, band, 25.0, uploader=up)
            torch.cuda.synchronize()
            s[name].append(time.perf_counter() - t0)
    up.close()
    med = {k: statistics.median(v) for k, v in s.items()}
    nbytes = len(frames) * (band.ymax - band.ymin) * frames[0].shape[1] * 3
    return {"case": "host-fed ChangeFrameSelector pass", "frames": len(frames), "band_rows": [band.ymin, band.ymax],
            "seconds": {k: [round(x, 4) for x in v] for k, v in s.items()}, "median_seconds": {k: round(v, 4) for k, v in med.items()},
            "gb_per_s_band_bytes_uploaded": {k: round(nbytes / v / 1e9, 2) for k, v in med.items()},
            "keyed_over_plain": round(med["keyed"] / med["plain"], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--clip-frames", type=int, default=1024, help="frames of the host-fed pass (0: skip it)")
    a = ap.parse_args()
    ctx = engine.Context(0)
    h, w, n = a.height, a.width, a.batch
    key = frame_select.ColourKey("yellow", 48)
    rng = np.random.default_rng(1)
    host = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    dev = torch.from_numpy(host).to(ctx.tdev)
    y0 = h * 810 // 1080
    print(json.dumps(case(ctx, "band", dev, (y0, h, 0, w), key, a.iters, a.rounds)), flush=True)
    print(json.dumps(case(ctx, "whole frames", dev, (0, h, 0, w), key, a.iters, a.rounds)), flush=True)
    if a.clip_frames:
        from vse_amd.extractor import SubtitleArea
        frames = [host[i % n] for i in range(a.clip_frames)]
        print(json.dumps(host_fed(ctx, frames, SubtitleArea(y0, h, 0, w), key, a.rounds, a.batch)), flush=True)


if __name__ == "__main__":
    main()
