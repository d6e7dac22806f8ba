#!/usr/bin/env python3
"""What the locator's cells cost on held edges: `batch` synthetic 1080p frames resident on the device, the WHOLE frame as the region,
one job at a time.  Four things alternate in one process, each repetition timed between two device events:
  hold1    one vse_frame_cells_hold call, one threshold (128), hold 8,
  single   one vse_frame_cells call at 128 (its parent),
  hold8    one vse_frame_cells_hold call with the eight default thresholds, hold 8,
  multi    one vse_frame_cells_multi call with the same eight thresholds (its parent).
Every timed call starts a clip and flushes it (fed = 0 / reset, flush), so the hold calls include their hold - 1 drain steps.  Reports
the medians over `reps` repetitions of `iters` calls with their minimum and maximum, GB/s over the frame bytes, and the ratios hold1 /
single and hold8 / multi.  At hold 1 the hold call's totals are checked against vse_frame_cells_multi's first.

With --host-frames N it then times the locator's whole pass as the extractor runs it on the same clip: AreaLocator.run over N
host-resident frames through a staging.Uploader (host clock around work that ends in the read-back of the totals), automaton "change"
and "hold" alternating, at edge_thresh 128 and at "auto".

usage: python tools/bench_cells_hold.py [--batch 64] [--iters 20] [--reps 20] [--height 1080] [--width 1920] [--hold 8] [--host-frames 0]"""
import argparse
import json
import os
import statistics
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vse_amd import area_locator, engine, staging, synth


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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--hold", type=int, default=8)
    ap.add_argument("--host-frames", type=int, default=0)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: medians over at least 20 repetitions")
    ctx = engine.Context(0)
    h, w, n, hold = a.height, a.width, a.batch, a.hold
    area = (0, h, 0, w)
    q = n // 4
    frames, _ = synth.make_clip([(None, q), ("the quick brown fox", q), ("the quick brown box", q), ("seven wizards", n - 3 * q)], h, w, seed=1)
    dev = torch.from_numpy(frames).to(ctx.tdev)
    fps = 24.0
    params = area_locator.AreaLocator().params(fps)
    ths = area_locator.AUTO_THRESHOLDS
    hold1_state = ctx.frame_cells_hold_state(h, w, 1, hold)
    hold8_state = ctx.frame_cells_hold_state(h, w, len(ths), hold)
    check_state = ctx.frame_cells_hold_state(h, w, len(ths), 1)
    multi_state = ctx.frame_cells_multi_state(h, w, len(ths))
    one_state = ctx.frame_cells_state(h, w)
    fns = {"hold1": lambda: ctx.frame_cells_hold(dev, area, (params.edge_thresh,), hold, params, hold1_state, 0, flush=True),
           "single": lambda: ctx.frame_cells(dev, area, params, one_state, reset=True, flush=True),
           "hold8": lambda: ctx.frame_cells_hold(dev, area, ths, hold, params, hold8_state, 0, flush=True),
           "multi": lambda: ctx.frame_cells_multi(dev, area, ths, params, multi_state, reset=True, flush=True)}

    fns["multi"]()
    ctx.frame_cells_hold(dev, area, ths, 1, params, check_state, 0, flush=True)
    same = bool(torch.equal(check_state.totals, multi_state.totals))
    if not same:
        print(json.dumps({"error": "vse_frame_cells_hold's totals at hold 1 differ from vse_frame_cells_multi's"}), flush=True)
        return 1
    for fn in fns.values():
        timed(fn, 3)
    ms = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, fn in fns.items():
            ms[k].append(timed(fn, a.iters))
    nbytes = n * h * w * 3
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({"batch": n, "frame": [h, w], "hold": hold, "thresholds": list(ths), "frame_mb": round(nbytes / 1e6, 1), "reps": a.reps,
                      "iters": a.iters, "hold_one_equals_multi": same,
                      "median_ms": {k: round(v, 4) for k, v in med.items()},
                      "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
                      "gb_per_s_frame_bytes": {k: round(nbytes / v / 1e6, 1) for k, v in med.items()},
                      "hold1_over_single": round(med["hold1"] / med["single"], 3),
                      "hold8_over_multi": round(med["hold8"] / med["multi"], 3),
                      "ratio_min_max": {"hold1_over_single": [round(min(x / y for x, y in zip(ms["hold1"], ms["single"])), 3),
                                                              round(max(x / y for x, y in zip(ms["hold1"], ms["single"])), 3)],
                                        "hold8_over_multi": [round(min(x / y for x, y in zip(ms["hold8"], ms["multi"])), 3),
                                                             round(max(x / y for x, y in zip(ms["hold8"], ms["multi"])), 3)]}}), flush=True)
    if a.host_frames:
        host = [frames[k % n] for k in range(a.host_frames)]
        up = staging.Uploader(ctx.tdev, ctx=ctx)
        secs = {(auto, et): [] for et in (128, "auto") for auto in ("change", "hold")}
        found = {}
        try:
            for rep in range(4):                        # the first repetition warms everything up and is not counted
                for auto, et in secs:
                    loc = area_locator.AreaLocator(area_locator.EngineCells(ctx), batch=n, edge_thresh=et, automaton=auto, hold_frames=hold)
                    torch.cuda.synchronize()
                    t0 = time.time()
                    got = loc.run(host, fps, uploader=up)
                    dt = time.time() - t0
                    if rep:
                        secs[auto, et].append(dt)
                    found[f"{auto}/{et}"] = (None if got is None else [got.ymin, got.ymax, got.xmin, got.xmax], loc.edge_thresh)
        finally:
            up.close()
        med = {k: statistics.median(v) for k, v in secs.items()}
        print(json.dumps({"host_fed_pass": "bgr", "frames": len(host), "hold": hold,
                          "seconds": {f"{k[0]}/{k[1]}": [round(x, 3) for x in v] for k, v in secs.items()},
                          "frames_per_s": {f"{k[0]}/{k[1]}": round(len(host) / v, 1) for k, v in med.items()},
                          "hold_over_change_at_128": round(med["hold", 128] / med["change", 128], 3),
                          "hold_over_change_at_auto": round(med["hold", "auto"] / med["change", "auto"], 3),
                          "area_and_threshold": found}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
