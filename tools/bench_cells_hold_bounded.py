#!/usr/bin/env python3
"""What the locator's cells cost on bounded runs: `batch` synthetic 1080p frames resident on the device, the WHOLE frame as the region,
one job at a time.  Four things alternate in one process, each repetition timed between two device events:
  bounded1  one vse_frame_cells_hold_bounded call, one threshold (128), hold 8, max_hold 300,
  hold1     one vse_frame_cells_hold call at 128, hold 8 (its parent),
  bounded8  one vse_frame_cells_hold_bounded call with the eight default thresholds, hold 8, max_hold 300,
  hold8     one vse_frame_cells_hold call with the same eight thresholds (its parent).
Every timed call starts a clip and flushes it (fed = 0, flush): the bounded calls include the clear of their pending rows (the ring of
max_hold + 64 slots per cell and threshold) and the flush's pass over all of them, the hold calls their hold - 1 drain steps.  Reports
the medians over `reps` repetitions of `iters` calls with their minimum and maximum, GB/s over the frame bytes, and the ratios
bounded1 / hold1 and bounded8 / hold8.  First, on the same frames, the bounded call's per-cell counts summed over the cells are checked
against vse_frame_hold_bounded's rows, its totals in batches of 23 frames against its totals in one call, and its totals at max_hold
4000 against vse_frame_cells_hold's.

With --host-frames N it then times the locator's whole pass as the extractor runs it on the same clip: AreaLocator.run over N
host-resident frames through a staging.Uploader (host clock around work that ends in the read-back of the totals), automaton "hold"
without and with max_hold_frames alternating, at edge_thresh 128 and at "auto".

usage: python tools/bench_cells_hold_bounded.py [--batch 64] [--iters 20] [--reps 20] [--height 1080] [--width 1920] [--hold 8]
                                                [--max-hold 300] [--host-frames 0]"""
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
    ap.add_argument("--max-hold", type=int, default=300)
    ap.add_argument("--host-frames", type=int, default=0)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: medians over at least 20 repetitions")
    ctx = engine.Context(0)
    h, w, n, hold, max_hold = a.height, a.width, a.batch, a.hold, a.max_hold
    area = (0, h, 0, w)
    q = n // 4
    frames, _ = synth.make_clip([(None, q), ("the quick brown fox", q), ("the quick brown box", q), ("seven wizards", n - 3 * q)], h, w, seed=1)
    dev = torch.from_numpy(frames).to(ctx.tdev)
    fps = 24.0
    params = area_locator.AreaLocator().params(fps)
    ths = area_locator.AUTO_THRESHOLDS
    bounded1_state = ctx.frame_cells_hold_bounded_state(h, w, 1, max_hold)
    bounded8_state = ctx.frame_cells_hold_bounded_state(h, w, len(ths), max_hold)
    hold1_state = ctx.frame_cells_hold_state(h, w, 1, hold)
    hold8_state = ctx.frame_cells_hold_state(h, w, len(ths), hold)
    fns = {"bounded1": lambda: ctx.frame_cells_hold_bounded(dev, area, (params.edge_thresh,), hold, max_hold, params, bounded1_state, 0, flush=True),
           "hold1": lambda: ctx.frame_cells_hold(dev, area, (params.edge_thresh,), hold, params, hold1_state, 0, flush=True),
           "bounded8": lambda: ctx.frame_cells_hold_bounded(dev, area, ths, hold, max_hold, params, bounded8_state, 0, flush=True),
           "hold8": lambda: ctx.frame_cells_hold(dev, area, ths, hold, params, hold8_state, 0, flush=True)}

    # the kernel at the size that is timed, against the device's other entry points
    short = min(max_hold, 12)             # a bound that cuts runs off inside the clip
    chold = min(hold, short)
    check = ctx.frame_cells_hold_bounded_state(h, w, len(ths), short)
    whole, counts = ctx.frame_cells_hold_bounded(dev, area, ths, chold, short, params, check, 0, flush=True, want_counts=True)
    whole = whole.clone()
    rows_state = ctx.frame_hold_bounded_state(h, w, short)
    sums_ok = all(bool(torch.equal(counts[k].sum((1, 2)), ctx.frame_hold_bounded(dev, area, th, chold, short, rows_state, 0, flush=True)))
                  for k, th in enumerate(ths))
    fed = 0
    while fed < n:
        ctx.frame_cells_hold_bounded(dev[fed:fed + 23], area, ths, chold, short, params, check, fed, flush=fed + 23 >= n)
        fed += 23
    batches_ok = bool(torch.equal(check.totals, whole))
    big = ctx.frame_cells_hold_bounded_state(h, w, len(ths), 4000)
    ctx.frame_cells_hold_bounded(dev, area, ths, hold, 4000, params, big, 0, flush=True)
    fns["hold8"]()
    unbounded_ok = bool(torch.equal(big.totals, hold8_state.totals))
    del big, check, counts
    if not (sums_ok and batches_ok and unbounded_ok):
        print(json.dumps({"error": "vse_frame_cells_hold_bounded disagrees with the device's other entry points",
                          "counts_sum_to_frame_hold_bounded_rows": sums_ok, "batches_equal_one_call": batches_ok,
                          "max_hold_4000_equals_frame_cells_hold": unbounded_ok}), flush=True)
        return 1
    for fn in fns.values():
        timed(fn, 3)
    ms = {k: [] for k in fns}
    for _ in range(a.reps):
        for k, fn in fns.items():
            ms[k].append(timed(fn, a.iters))
    nbytes = n * h * w * 3
    med = {k: statistics.median(v) for k, v in ms.items()}
    ratios = {"bounded1_over_hold1": ("bounded1", "hold1"), "bounded8_over_hold8": ("bounded8", "hold8")}
    print(json.dumps({"batch": n, "frame": [h, w], "hold": hold, "max_hold": max_hold, "thresholds": list(ths), "frame_mb": round(nbytes / 1e6, 1),
                      "state_mb": {"bounded1": round(bounded1_state.words.numel() / 1e6, 1), "bounded8": round(bounded8_state.words.numel() / 1e6, 1),
                                   "hold1": round(hold1_state.words.numel() / 1e6, 1), "hold8": round(hold8_state.words.numel() / 1e6, 1)},
                      "reps": a.reps, "iters": a.iters, "counts_sum_to_frame_hold_bounded_rows": sums_ok, "batches_equal_one_call": batches_ok,
                      "max_hold_4000_equals_frame_cells_hold": unbounded_ok,
                      "median_ms": {k: round(v, 4) for k, v in med.items()},
                      "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
                      "gb_per_s_frame_bytes": {k: round(nbytes / v / 1e6, 1) for k, v in med.items()},
                      **{name: round(med[x] / med[y], 3) for name, (x, y) in ratios.items()},
                      "ratio_min_max": {name: [round(min(p / r for p, r in zip(ms[x], ms[y])), 3), round(max(p / r for p, r in zip(ms[x], ms[y])), 3)]
                                        for name, (x, y) in ratios.items()}}), flush=True)
    if a.host_frames:
        host = [frames[k % n] for k in range(a.host_frames)]
        up = staging.Uploader(ctx.tdev, ctx=ctx)
        secs = {(kind, et): [] for et in (128, "auto") for kind in ("hold", "bounded")}
        found = {}
        try:
            for rep in range(4):                        # the first repetition warms everything up and is not counted
                for kind, et in secs:
                    loc = area_locator.AreaLocator(area_locator.EngineCells(ctx), batch=n, edge_thresh=et, automaton="hold", hold_frames=hold,
                                                   max_hold_frames=max_hold if kind == "bounded" else None)
                    torch.cuda.synchronize()
                    t0 = time.time()
                    got = loc.run(host, fps, uploader=up)
                    dt = time.time() - t0
                    if rep:
                        secs[kind, et].append(dt)
                    found[f"{kind}/{et}"] = (None if got is None else [got.ymin, got.ymax, got.xmin, got.xmax], loc.edge_thresh)
        finally:
            up.close()
        med = {k: statistics.median(v) for k, v in secs.items()}
        print(json.dumps({"host_fed_pass": "bgr", "frames": len(host), "hold": hold, "max_hold": max_hold,
                          "seconds": {f"{k[0]}/{k[1]}": [round(x, 3) for x in v] for k, v in secs.items()},
                          "frames_per_s": {f"{k[0]}/{k[1]}": round(len(host) / v, 1) for k, v in med.items()},
                          "bounded_over_hold_at_128": round(med["bounded", 128] / med["hold", 128], 3),
                          "bounded_over_hold_at_auto": round(med["bounded", "auto"] / med["hold", "auto"], 3),
                          "area_and_threshold": found}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
