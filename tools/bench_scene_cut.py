#!/usr/bin/env python3
"""Device time of the scene-cut counts (vse_scene_change) per batch: `batch` synthetic 1080p frames on the device (generator
scenes: pans, holds, cuts), scale 3 and search radius 8 as the keyframe finder runs them, batches chained through one state.
Times `iters` calls between two device events (memset of the counts + three kernels per call) and reports GB/s over the frame
bytes, which pass 1 reads once.  The passes alone: run it under `rocprofv3 --kernel-trace --stats` (scene_plane_kernel,
scene_search_kernel, scene_state_kernel).

usage: python tools/bench_scene_cut.py [--batch 64] [--iters 100] [--height 1080] [--width 1920] [--scale 3] [--search 8]"""
import argparse
import json
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from vse_amd import engine, synth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--scale", type=int, default=3)
    ap.add_argument("--search", type=int, default=8)
    ap.add_argument("--bias", type=int, default=1024)
    a = ap.parse_args()
    ctx = engine.Context(0)
    h, w, n = a.height, a.width, a.batch
    q = max(n // 4, 1)
    frames, _ = synth.make_scenes([dict(frames=q, pan=(0, 7)), dict(frames=q, pan=(5, -3), hold=[2]), dict(frames=q),
                                   dict(frames=max(n - 3 * q, 1), pan=(-9, 0))], h, w, seed=1)
    frames = frames[:n]
    dev = torch.from_numpy(frames).to(ctx.tdev)
    state = ctx.scene_change_state(h, w, a.scale)
    ws = torch.empty(ctx.lib.vse_scene_change_workspace_bytes(n, h, w, a.scale), dtype=torch.uint8, device=ctx.tdev)
    for k in range(5):
        ctx.scene_change(dev, a.scale, a.search, a.bias, state, reset=(k == 0), workspace=ws)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        out = ctx.scene_change(dev, a.scale, a.search, a.bias, state, workspace=ws)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.iters
    nbytes = n * h * w * 3
    ah, aw = h // a.scale, w // a.scale
    print(json.dumps({"batch": n, "frame": [h, w], "scale": a.scale, "search": a.search, "plane": [ah, aw],
                      "blocks": (ah // 16) * (aw // 16), "ms_per_batch": round(ms, 4), "frame_mb": round(nbytes / 1e6, 1),
                      "gb_per_s_frame_bytes": round(nbytes / ms / 1e6, 1), "frames_per_s": round(n / ms * 1e3),
                      "changed_max_after_first": int(np.asarray(out.cpu())[1:, 0].max()) if n > 1 else 0}), flush=True)


if __name__ == "__main__":
    main()
