#!/usr/bin/env python3
"""Device time of the focus pass (vse_frame_focus) per batch, beside the selector's own pass over the same bytes (vse_frame_change):
`batch` synthetic 1080p frames on the device (synth.make_clip: held subtitles over noise that is drawn afresh per frame), both kernels
over the same band (rows 810:1060, full width: the same bytes read once), batches chained through their states as a clip that never
ends.  The two alternate in `rounds` rounds of `iters` calls each, every round timed between two device events; the rows of both are
checked once against each other's definition (kept <= the edges of the frame and of the one before).  Reports per-round ms, their
medians, GB/s over the band's bytes and the ratio focus / change per round.  No gate.  Kernel time alone: run it under
`rocprofv3 --kernel-trace --stats` (frame_focus_kernel, frame_change_kernel).

usage: python tools/bench_frame_focus.py [--batch 64] [--iters 50] [--rounds 7] [--height 1080] [--width 1920]"""
import argparse
import json
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vse_amd import engine, synth


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    a = ap.parse_args()
    ctx = engine.Context(0)
    h, w, n = a.height, a.width, a.batch
    y0, y1 = h * 810 // 1080, h * 1060 // 1080
    area = (y0, y1, 0, w)
    q = max(1, n // 4)
    frames, _ = synth.make_clip([(None, q), ("the quick brown fox", q), ("seven wizards box", q), ("near frozen lakes", max(1, n - 3 * q))],
                                h, w, seed=1)
    dev = torch.from_numpy(frames[:n]).to(ctx.tdev)
    states = {k: ctx.frame_change_state(y1 - y0, w) for k in ("focus", "change")}
    last = {}

    def focus():
        last["focus"] = ctx.frame_focus(dev, area, 128, states["focus"], reset=False)

    def change():
        last["change"] = ctx.frame_change(dev, area, 128, states["change"], reset=False)

    for fn in (focus, change):
        timed(fn, 5)
    kept, edges = last["focus"][:, 0].cpu(), last["change"][:, 0].cpu()
    assert bool((kept[1:] <= torch.minimum(edges[1:], edges[:-1])).all()) and int(kept.max()) > 0, "the two kernels disagree about the edge masks"
    ms = {"focus": [], "change": []}
    for _ in range(a.rounds):
        ms["focus"].append(timed(focus, a.iters))
        ms["change"].append(timed(change, a.iters))
    nbytes = n * (y1 - y0) * w * 3
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({"batch": n, "frame": [h, w], "band_rows": [y0, y1], "band_mb": round(nbytes / 1e6, 1),
                      "ms_per_batch": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                      "median_ms": {k: round(v, 4) for k, v in med.items()},
                      "gb_per_s_band_bytes": {k: round(nbytes / v / 1e6, 1) for k, v in med.items()},
                      "focus_over_change": [round(f / c, 3) for f, c in zip(ms["focus"], ms["change"])],
                      "focus_over_change_median": round(med["focus"] / med["change"], 3),
                      "kept_mean": round(float(last["focus"][:, 0].float().mean()), 1),
                      "edges_mean": round(float(last["change"][:, 0].float().mean()), 1)}), flush=True)


if __name__ == "__main__":
    main()
