#!/usr/bin/env python3
"""Device time of the bounded held-edge pass (vse_frame_hold_bounded, hold 8, max_hold 360) per batch, beside the pass it extends
(vse_frame_hold, hold 8, unchanged code: the baseline), on the same build and over the same band (rows 810:1060 of `batch` synthetic
1080p frames on the device, full width: the same bytes read once), batches chained through their states as a clip that never ends.
Two inputs: `clean`, subtitles that change every quarter of the batch over a background without edges (synth.make_clip: the runs that
end are the subtitles', all of one length per change), and `busy`, the same subtitles over a textured background that stands still
(synth.make_moving_clip with pan 0 0 and --noise levels of fresh noise per frame: the background's own edges never end, and the pixels
whose gradient the noise carries across the threshold end runs of every length in every frame).  The two kernels alternate in `rounds`
rounds of `iters` calls each, every round timed between two device events.  Reports per-round ms, the ratio bounded / hold per round,
and per input the mean rows (edges, appeared, vanished: `vanished` is the runs that end in range per frame, each of which the
per-length loop and its atomics see).  Kernel time alone: run it under `rocprofv3 --kernel-trace --stats` (frame_hold_bounded_kernel,
frame_hold_rows_kernel, frame_hold_kernel).

usage: python tools/bench_frame_hold_bounded.py [--batch 64] [--iters 50] [--rounds 4] [--hold 8] [--max-hold 360] [--noise 3]
                                                [--height 1080] [--width 1920] [--inputs clean busy]"""
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
    ap.add_argument("--max-hold", type=int, default=360)
    ap.add_argument("--noise", type=int, default=3, help="busy: levels of fresh noise per frame; more makes more pixels flicker")
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--inputs", nargs="+", default=["clean", "busy"], choices=("clean", "busy"))
    a = ap.parse_args()
    ctx = engine.Context(0)
    h, w, n, hold, max_hold = a.height, a.width, a.batch, a.hold, a.max_hold
    y0, y1 = h * 810 // 1080, h * 1060 // 1080
    area = (y0, y1, 0, w)
    q = n // 4
    schedule = [(None, q), ("the quick brown fox", q), ("seven wizards box", q), ("near frozen lakes", n - 3 * q)]
    nbytes = n * (y1 - y0) * w * 3
    for name in a.inputs:
        if name == "clean":
            frames, _ = synth.make_clip(schedule, h, w, seed=1)
        else:
            frames, _ = synth.make_moving_clip(schedule, h, w, pan=(0, 0), noise=a.noise, seed=1)
        dev = torch.from_numpy(frames).to(ctx.tdev)
        del frames
        hold_state = ctx.frame_hold_state(y1 - y0, w, hold)
        bounded_state = ctx.frame_hold_bounded_state(y1 - y0, w, max_hold)
        fed = {"hold": 0, "bounded": 0}
        last = {}

        def held():
            last["hold"] = ctx.frame_hold(dev, area, 128, hold, hold_state, fed["hold"])
            fed["hold"] += n

        def bounded():
            last["bounded"] = ctx.frame_hold_bounded(dev, area, 128, hold, max_hold, bounded_state, fed["bounded"])
            fed["bounded"] += n

        # warm up beyond max_hold frames: from then on every call writes a full batch of rows
        for fn in (held, bounded):
            timed(fn, max(5, max_hold // n + 2))
        ms = {"hold": [], "bounded": []}
        for _ in range(a.rounds):
            ms["hold"].append(timed(held, a.iters))
            ms["bounded"].append(timed(bounded, a.iters))
        best = {k: min(v) for k, v in ms.items()}
        print(json.dumps({"input": name, "batch": n, "frame": [h, w], "band_rows": [y0, y1], "hold": hold, "max_hold": max_hold,
                          "noise": a.noise if name == "busy" else None, "band_mb": round(nbytes / 1e6, 1),
                          "ms_per_batch": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                          "gb_per_s_band_bytes": {k: round(nbytes / v / 1e6, 1) for k, v in best.items()},
                          "bounded_over_hold": [round(b / g, 3) for b, g in zip(ms["bounded"], ms["hold"])],
                          "bounded_over_hold_best": round(best["bounded"] / best["hold"], 3),
                          "rows_mean": {k: [round(float(x), 1) for x in v.float().mean(0)] for k, v in last.items()}}), flush=True)
        del dev


if __name__ == "__main__":
    main()
