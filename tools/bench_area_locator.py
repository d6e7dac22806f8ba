#!/usr/bin/env python3
"""Device time of the subtitle-area locator's pass (vse_frame_cells) per batch, beside the pass it is modelled on (vse_frame_change)
: `batch` synthetic 1080p frames on the device, both kernels over the WHOLE frame as their area (the same bytes read once), batches
chained through their states.  The two alternate in `rounds` rounds of `iters` calls each, every round timed between two device
events.  Reports per-round ms, GB/s over the frame bytes and the ratio cells / change; what a plain read reaches on the box is
tools/copy_ceiling.py's read-only figure, run in the same job.  Kernel time alone: run it under `rocprofv3 --kernel-trace --stats`
(frame_cells_kernel, frame_change_kernel).

With --host-frames N it then times the locator's whole extra pass as the extractor runs it: AreaLocator.run over N host-resident
frames through a staging.Uploader (host clock around work that ends in the read-back of the totals), BGR and YUV 4:2:0.

usage: python tools/bench_area_locator.py [--batch 64] [--iters 50] [--rounds 4] [--height 1080] [--width 1920] [--host-frames 0]"""
import argparse
import json
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vse_amd import area_locator, engine, ingest, staging, synth


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
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--host-frames", type=int, default=0)
    a = ap.parse_args()
    ctx = engine.Context(0)
    h, w, n = a.height, a.width, a.batch
    area = (0, h, 0, w)
    q = n // 4
    frames, _ = synth.make_clip([(None, q), ("the quick brown fox", q), ("the quick brown box", q), ("seven wizards", n - 3 * q)], h, w, seed=1)
    dev = torch.from_numpy(frames).to(ctx.tdev)
    fps = 24.0
    params = area_locator.AreaLocator().params(fps)
    cells_state = ctx.frame_cells_state(h, w)
    change_state = ctx.frame_change_state(h, w)

    def cells():
        return ctx.frame_cells(dev, area, params, cells_state)

    def change():
        return ctx.frame_change(dev, area, params.edge_thresh, change_state)

    ctx.frame_cells(dev, area, params, cells_state, reset=True)
    ctx.frame_change(dev, area, params.edge_thresh, change_state, reset=True)
    for fn in (cells, change):
        timed(fn, 5)
    ms = {"cells": [], "change": []}
    for _ in range(a.rounds):
        ms["cells"].append(timed(cells, a.iters))
        ms["change"].append(timed(change, a.iters))
    nbytes = n * h * w * 3
    best = {k: min(v) for k, v in ms.items()}
    totals = ctx.frame_cells(dev[:0], area, params, cells_state, flush=True).cpu().numpy()
    print(json.dumps({"batch": n, "frame": [h, w], "cells": list(totals.shape[:2]), "frame_mb": round(nbytes / 1e6, 1),
                      "ms_per_batch": {k: [round(x, 4) for x in v] for k, v in ms.items()},
                      "gb_per_s_frame_bytes": {k: round(nbytes / v / 1e6, 1) for k, v in best.items()},
                      "cells_over_change": [round(c / g, 3) for c, g in zip(ms["cells"], ms["change"])],
                      "cells_frames_per_s": round(n / best["cells"] * 1e3), "covered_max": int(totals[..., 0].max())}), flush=True)
    if a.host_frames:
        host = [frames[k % n] for k in range(a.host_frames)]
        yuv = [ingest.Yuv420Frame(ingest.bgr_to_yuv420(f), h, w, "i420") for f in frames]
        up = staging.Uploader(ctx.tdev, ctx=ctx)
        for name, clip in (("bgr", host), ("i420", [yuv[k % n] for k in range(a.host_frames)])):
            loc = area_locator.AreaLocator(area_locator.EngineCells(ctx), batch=n)
            loc.run(clip[:3 * n], fps, uploader=up)
            torch.cuda.synchronize()
            t0 = time.time()
            found = loc.run(clip, fps, uploader=up)
            dt = time.time() - t0
            print(json.dumps({"host_fed_pass": name, "frames": len(clip), "seconds": round(dt, 3), "frames_per_s": round(len(clip) / dt, 1),
                              "frame_mb": round(h * w * (3 if name == "bgr" else 1.5) / 1e6, 2),
                              "area": None if found is None else [found.ymin, found.ymax, found.xmin, found.xmax]}), flush=True)
        up.close()


if __name__ == "__main__":
    main()
