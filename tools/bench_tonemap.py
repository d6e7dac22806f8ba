#!/usr/bin/env python3
"""vse_yuv_to_bgr_tonemap beside the unchanged vse_yuv_to_bgr_format on the same buffers, in one job: what the two table gathers and the
gamut matrix cost on top of the plain conversion, and whether the tone-mapped conversion still hides under the upload it rides on.

64 x 1080p and 16 x 2160p device-resident frames, P010 and yuv420p10le, of a synthetic clip (synth.make_frames) graded as PQ BT.2020 by
synth.hdr_grade, so that the table addresses are a picture's and not constants (`--distinct` frames are graded on the host and repeated;
2160p is the 1080p grade with every sample doubled in both directions).  Per size and format three rows alternate for `--rounds` rounds,
HIP events over `--iters` launches after warm-up each time, so the spread between a row's repeats is the job's own noise:
  plain     vse_yuv_to_bgr_format, 16-byte kernel
  tonemap   vse_yuv_to_bgr_tonemap, 16-byte kernel
  general   vse_yuv_to_bgr_tonemap from a base one sample off its alignment: the kernel without conditions on the same pictures
bytes moved = the packed frame read once + 3 per pixel written.  One JSON line per measurement, then one summary line per row with the
median time per frame, GB/s, the ratio to the plain conversion and the frame's time on the link (--link-gbs, EXPERIMENTS.md L)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from vse_amd import engine, ingest, synth


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # us


def packed_frames(graded, pix_fmt, scale):
    """(Y, U, V) 10-bit plane triples -> [distinct, frame bytes] uint8 of the pixel format, every sample repeated `scale` times both ways."""
    out = []
    for y, u, v in graded:
        y, u, v = (np.repeat(np.repeat(p, scale, 0), scale, 1).astype("<u2") for p in (y, u, v))
        if pix_fmt == "p010le":
            planes = (y << 6, np.stack([u, v], axis=2).reshape(u.shape[0], -1) << 6)
        else:
            planes = (y, u, v)
        out.append(np.concatenate([np.ascontiguousarray(p).reshape(-1).view(np.uint8) for p in planes]))
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=4, help="frames graded on the host, repeated to fill a batch")
    ap.add_argument("--link-gbs", type=float, default=57.1, help="host-to-device rate of pinned uploads, GB/s")
    a = ap.parse_args()
    ctx = engine.Context(0)
    tone = ingest.ToneMap("pq")
    graded = synth.hdr_grade(synth.make_frames(a.distinct, 1080, 1920, seed=1), depth=10, sub=(1, 1))
    runs = []
    for n, h, w, scale in ((64, 1080, 1920, 1), (16, 2160, 3840, 2)):
        for pix_fmt in ("p010le", "yuv420p10le"):
            fmt = ingest.YuvFormat.from_pix_fmt(pix_fmt, matrix="bt2020")
            frame = fmt.frame_bytes(h, w)
            assert frame % 16 == 0
            host = packed_frames(graded, pix_fmt, scale)
            assert host.shape == (a.distinct, frame)
            flat = torch.from_numpy(np.concatenate([host[np.arange(n) % a.distinct].reshape(-1), np.zeros(16, np.uint8)])).to(ctx.tdev)
            packed, shifted = flat[:n * frame].view(n, frame), flat.clone()[2:2 + n * frame].view(n, frame)
            shifted.copy_(packed)
            assert packed.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 2
            out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=ctx.tdev)
            ref = ctx.yuv_to_bgr(packed, n, h, w, fmt, 0, tone=tone)
            assert torch.equal(ref, ctx.yuv_to_bgr(shifted, n, h, w, fmt, 0, tone=tone))                     # both kernels, the same bytes
            assert np.array_equal(ref[0, :64].cpu().numpy(), ingest.YuvFrame(
                ingest._planes_at(host[0], 0, h, w, fmt), h, w, fmt, tone=tone)[:64].to_bgr())               # ... and the host's
            del ref
            calls = {"plain": lambda p=packed, o=out, n=n, h=h, w=w, f=fmt: ctx.yuv_to_bgr(p, n, h, w, f, 0, out=o),
                     "tonemap": lambda p=packed, o=out, n=n, h=h, w=w, f=fmt: ctx.yuv_to_bgr(p, n, h, w, f, 0, out=o, tone=tone),
                     "general": lambda p=shifted, o=out, n=n, h=h, w=w, f=fmt: ctx.yuv_to_bgr(p, n, h, w, f, 0, out=o, tone=tone)}
            for what, fn in calls.items():
                runs.append(dict(what=what, pix_fmt=pix_fmt, n=n, h=h, w=w, frame=frame, moved=frame + 3 * h * w, fn=fn, us=[]))
    for r in range(a.rounds):
        for run in runs:
            us = timed(run["fn"], a.iters) / run["n"]
            run["us"].append(us)
            print(json.dumps({"what": run["what"], "pix_fmt": run["pix_fmt"], "h": run["h"], "w": run["w"], "frames": run["n"], "round": r,
                              "us_per_frame": round(us, 2), "gb_per_s": round(run["moved"] / us / 1e3, 1)}), flush=True)
    plain = {(run["pix_fmt"], run["h"]): float(np.median(run["us"])) for run in runs if run["what"] == "plain"}
    for run in runs:
        med = float(np.median(run["us"]))
        link_us = run["frame"] / a.link_gbs / 1e3
        print(json.dumps({"summary": run["what"], "pix_fmt": run["pix_fmt"], "h": run["h"], "w": run["w"], "us_per_frame_median": round(med, 2),
                          "us_per_frame_min": round(min(run["us"]), 2), "us_per_frame_max": round(max(run["us"]), 2),
                          "gb_per_s_median": round(run["moved"] / med / 1e3, 1), "over_plain": round(med / plain[run["pix_fmt"], run["h"]], 3),
                          "link_us_per_frame": round(link_us, 1), "hides_under_the_upload": bool(max(run["us"]) < link_us)}), flush=True)


if __name__ == "__main__":
    main()
