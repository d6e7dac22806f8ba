#!/usr/bin/env python3
"""What the edge-threshold calibration costs on the device: `batch` synthetic 1080p frames resident on the device, the WHOLE frame as
the region, one job at a time.  Three things alternate in one process, each repetition timed between two device events:
  multi    one vse_frame_cells_multi call with the eight default thresholds (the frame bytes read once),
  eight    eight vse_frame_cells calls, one per threshold (what a person does today: the bytes read eight times),
  single   one vse_frame_cells call at 128.
Reports the medians over `reps` repetitions of `iters` calls, GB/s over the frame bytes (multi and single: the bytes once; eight: the
bytes of ONE pass over its time, so the three rates compare as frames per second do), and the ratios multi / eight and multi / single.
The totals of the multi call are checked against the eight single calls first: faster and different is not faster.

With --host-frames N it then times the locator's whole pass as the extractor runs it on tools/bench_area_locator.py's clip:
AreaLocator.run over N host-resident frames through a staging.Uploader (host clock around work that ends in the read-back of the
totals), edge_thresh 128 and "auto" alternating.

usage: python tools/bench_edge_calibrate.py [--batch 64] [--iters 20] [--reps 20] [--height 1080] [--width 1920] [--host-frames 0]"""
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
    ap.add_argument("--host-frames", type=int, default=0)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: medians over at least 20 repetitions")
    ctx = engine.Context(0)
    h, w, n = a.height, a.width, a.batch
    area = (0, h, 0, w)
    q = n // 4
    frames, _ = synth.make_clip([(None, q), ("the quick brown fox", q), ("the quick brown box", q), ("seven wizards", n - 3 * q)], h, w, seed=1)
    dev = torch.from_numpy(frames).to(ctx.tdev)
    fps = 24.0
    params = area_locator.AreaLocator().params(fps)
    ths = area_locator.AUTO_THRESHOLDS
    multi_state = ctx.frame_cells_multi_state(h, w, len(ths))
    single_states = [ctx.frame_cells_state(h, w) for _ in ths]
    one_state = ctx.frame_cells_state(h, w)

    def multi(**kw):
        return ctx.frame_cells_multi(dev, area, ths, params, multi_state, **kw)

    def eight(**kw):
        for th, st in zip(ths, single_states):
            ctx.frame_cells(dev, area, params._replace(edge_thresh=th), st, **kw)

    def single(**kw):
        return ctx.frame_cells(dev, area, params, one_state, **kw)

    multi(reset=True, flush=True)
    eight(reset=True, flush=True)
    same = all(torch.equal(multi_state.totals[k], st.totals) for k, st in enumerate(single_states))
    if not same:
        print(json.dumps({"error": "vse_frame_cells_multi's totals differ from vse_frame_cells'"}), flush=True)
        return 1
    single(reset=True)
    for fn in (multi, eight, single):
        timed(fn, 3)
    ms = {"multi": [], "eight": [], "single": []}
    for _ in range(a.reps):
        ms["multi"].append(timed(multi, a.iters))
        ms["eight"].append(timed(eight, a.iters))
        ms["single"].append(timed(single, a.iters))
    nbytes = n * h * w * 3
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({"batch": n, "frame": [h, w], "thresholds": list(ths), "frame_mb": round(nbytes / 1e6, 1), "reps": a.reps, "iters": a.iters,
                      "totals_equal": same,
                      "median_ms": {k: round(v, 4) for k, v in med.items()},
                      "min_max_ms": {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms.items()},
                      "gb_per_s_frame_bytes_of_one_pass": {k: round(nbytes / v / 1e6, 1) for k, v in med.items()},
                      "multi_over_eight": round(med["multi"] / med["eight"], 3),
                      "multi_over_single": round(med["multi"] / med["single"], 3)}), flush=True)
    if a.host_frames:
        host = [frames[k % n] for k in range(a.host_frames)]
        up = staging.Uploader(ctx.tdev, ctx=ctx)
        secs = {"128": [], "auto": []}
        found = {}
        try:
            for rep in range(4):                        # the first repetition warms both up and is not counted
                for name in secs:
                    loc = area_locator.AreaLocator(area_locator.EngineCells(ctx), batch=n, edge_thresh="auto" if name == "auto" else 128)
                    torch.cuda.synchronize()
                    t0 = time.time()
                    got = loc.run(host, fps, uploader=up)
                    dt = time.time() - t0
                    if rep:
                        secs[name].append(dt)
                    found[name] = (None if got is None else [got.ymin, got.ymax, got.xmin, got.xmax], loc.edge_thresh)
        finally:
            up.close()
        med = {k: statistics.median(v) for k, v in secs.items()}
        print(json.dumps({"host_fed_pass": "bgr", "frames": len(host), "seconds": {k: [round(x, 3) for x in v] for k, v in secs.items()},
                          "frames_per_s": {k: round(len(host) / v, 1) for k, v in med.items()},
                          "auto_over_128": round(med["auto"] / med["128"], 3),
                          "area_and_threshold": found}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
