#!/usr/bin/env python3
"""Device time of the held-edge selector's pass (vse_frame_hold, hold = 8) per batch, beside the pass it extends (vse_frame_change):
`batch` synthetic 1080p frames on the device (synth.make_moving_clip: a textured background that pans, with held subtitles), both
kernels over the same band (rows 810:1060, full width: the same bytes read once), batches chained through their states as a clip
that never ends.  With --pan 0 0 the background stands still: all its edges are held, so both kernels count about as many pixels per
frame (with the default pan the held counts are small and most blocks skip their atomic adds).  The two alternate in `rounds` rounds
of `iters` calls each, every round timed between two device events.  Reports per-round ms, GB/s over the band's bytes and the ratio hold / change.  Kernel time alone: run it under
`rocprofv3 --kernel-trace --stats` (frame_hold_kernel, frame_change_kernel).

usage: python tools/bench_frame_hold.py [--batch 64] [--iters 50] [--rounds 4] [--hold 8] [--height 1080] [--width 1920] [--pan 2 3]"""
import argparse
import json
import os
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
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--hold", type=int, default=8)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--pan", type=int, nargs=2, default=(2, 3), metavar=("DY", "DX"),
                    help="background motion per frame; 0 0 is a static busy shot, where every background edge is held and counted")
    a = ap.parse_args()
    ctx = engine.Context(0)
    h, w, n, hold = a.height, a.width, a.batch, a.hold
    y0, y1 = h * 810 // 1080, h * 1060 // 1080
    area = (y0, y1, 0, w)
    q = n // 4
    frames, _ = synth.make_moving_clip([(None, q), ("the quick brown fox", q), ("seven wizards box", q), ("near frozen lakes", n - 3 * q)],
                                       h, w, pan=tuple(a.pan), seed=1)
    dev = torch.from_numpy(frames).to(ctx.tdev)
    hold_state = ctx.frame_hold_state(y1 - y0, w, hold)
    change_state = ctx.frame_change_state(y1 - y0, w)
    fed = [0]
    last = {}

    def held():
        last["hold"] = ctx.frame_hold(dev, area, 128, hold, hold_state, fed[0])
        fed[0] += n

    def change():
        last["change"] = ctx.frame_change(dev, area, 128, change_state, reset=False)

    for fn in (held, change):
        timed(fn, 5)
    ms = {"hold": [], "change": []}
    for _ in range(a.rounds):
        ms["hold"].append(timed(held, a.iters))
        ms["change"].append(timed(change, a.iters))
    nbytes = n * (y1 - y0) * w * 3
    best = {k: min(v) for k, v in ms.items()}
    print(json.dumps({"batch": n, "frame": [h, w], "band_rows": [y0, y1], "hold": hold, "pan": list(a.pan), "band_mb": round(nbytes / 1e6, 1),
                      "ms_per_batch": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                      "gb_per_s_band_bytes": {k: round(nbytes / v / 1e6, 1) for k, v in best.items()},
                      "hold_over_change": [round(c / g, 3) for c, g in zip(ms["hold"], ms["change"])],
                      "hold_frames_per_s": round(n / best["hold"] * 1e3),
                      "edges_mean": {k: round(float(v[:, 0].float().mean()), 1) for k, v in last.items()}}), flush=True)


if __name__ == "__main__":
    main()
