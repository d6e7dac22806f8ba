#!/usr/bin/env python3
"""Device time of the streaming composite (vse_interval_stream) per batch, beside tools/bench_interval_composite.py: the same synthetic
1080p batch and default subtitle area, `iters` identical calls between two device events (nothing advances implicitly, so a call can
be repeated as it is).  Three steady-state calls of frame_select.StreamingCompositor's plan, with T = --trim frames:
  open     a long open run under the change selector (lag 0, ring of T + 1): one CONTINUEd fold of the batch's 64 frames' worth (the
           first T + 1 of them from the ring), the last T + 1 batch frames stored;
  closings the same batch with two subtitles ending in it: two EMITs and the open fold;
  lagged   a selector whose rows trail by --lag frames (ring of lag + T + 1): the whole batch stored, 64 frames folded from the ring alone.
GB/s is over the area's pixels of the frames folded, as the other tool's gb_per_s_area_pixels.  The yardstick is that tool run in the
same job, alternating with this one; this tool prints no ratio of its own.

usage: python tools/bench_interval_stream.py [--batch 64] [--iters 200] [--height 1080] [--width 1920] [--mode min|max|mean] [--shift 0]
                                             [--trim 6] [--lag 64]"""
import argparse
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vse_amd import engine, synth

CONT, EMIT = engine.INTERVAL_SEG_CONTINUE, engine.INTERVAL_SEG_EMIT


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--mode", choices=sorted(engine.INTERVAL_MODES), default="min")
    ap.add_argument("--shift", type=int, default=0, help="move the area this many pixels to the right (1: its rows are no longer 16-byte "
                    "aligned, so the general loads are timed)")
    ap.add_argument("--trim", type=int, default=6, help="T, the frames left out at either end of a subtitle")
    ap.add_argument("--lag", type=int, default=64, help="the frames by which the rows trail in the `lagged` case")
    a = ap.parse_args()
    ctx = engine.Context(0)
    h, w, n, T = a.height, a.width, a.batch, a.trim
    y0, y1, x0, x1 = int(0.78 * h), int(0.99 * h), int(0.05 * w) + a.shift, int(0.95 * w) + a.shift
    area = (y0, y1, x0, x1)
    frames, _ = synth.make_clip([(None, n // 4), ("the quick brown fox", n // 4), ("the quick brown box", n // 4),
                                 ("seven wizards", n - 3 * (n // 4))], h, w, seed=1)
    dev = torch.from_numpy(frames).to(ctx.tdev)
    del frames
    fed = 10 * n                                        # somewhere inside a clip
    out = torch.empty((2, y1 - y0, x1 - x0, 3), dtype=torch.uint8, device=ctx.tdev)
    third = n // 3
    cases = [
        ("open", T + 1, [(fed - T, fed + n - T - 1, CONT, 0)], fed + n - T),
        ("closings", T + 1, [(fed - T, fed + third, CONT | EMIT, 200), (fed + third + 4, fed + 2 * third, EMIT, 2 * third - third - 3),
                             (fed + 2 * third + 4, fed + n - T - 1, 0, 0)], fed + n - T),
        ("lagged", a.lag + T + 1, [(fed - a.lag - T, fed - a.lag - T + n - 1, CONT, 0)], fed + 1),
    ]
    for name, cap, segs, store_from in cases:
        state = ctx.interval_stream_state(y1 - y0, x1 - x0, cap)
        # the ring as the calls before would have left it: the last min(cap, batch) frames of a batch ending at `fed`, then a fold to CONTINUE
        for back in range((cap + n - 1) // n, 0, -1):
            ctx.interval_stream(dev, area, state, cap, fed - back * n, [], 0, a.mode, out=out)
        ctx.interval_stream(dev, area, state, cap, fed, [(fed + 1, fed + 1, 0, 0)], fed + n + 1, a.mode, out=out)
        for _ in range(10):
            ctx.interval_stream(dev, area, state, cap, fed, segs, store_from, a.mode, out=out)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            ctx.interval_stream(dev, area, state, cap, fed, segs, store_from, a.mode, out=out)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.iters
        folded = sum(last - first + 1 for first, last, _f, _c in segs)
        stored = max(0, fed + n - max(store_from, fed + 1) + 1)
        read_bytes = folded * (y1 - y0) * (x1 - x0) * 3
        print(json.dumps({"case": name, "batch": n, "frame": [h, w], "area": list(area), "mode": a.mode, "trim": T, "cap": cap,
                          "frames_folded": folded, "frames_from_ring": sum(max(0, min(last, fed) - first + 1) for first, last, _f, _c in segs),
                          "frames_stored": stored, "emits": sum(1 for g in segs if g[2] & EMIT), "ms_per_batch": round(ms, 4),
                          "gb_per_s_area_pixels": round(read_bytes / ms / 1e6, 1), "state_mb": round(state.numel() / 1e6, 2)}), flush=True)
        del state


if __name__ == "__main__":
    main()
