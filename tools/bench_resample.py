#!/usr/bin/env python3
"""vse_yuv_resample beside the unchanged vse_yuv_to_bgr_format on the same frames, in one job: what the horizontal resample to square
pixels costs in front of the conversion it feeds, and whether it still hides under the upload it rides on.

Device-resident frames of a synthetic clip (synth.make_frames through ingest.bgr_to_yuv420; `--distinct` frames repeated), three cases:
  dvd     64 x 720 x 480 yuv420p -> 854 columns (NTSC 16:9 DVD, 32:27): 854-byte rows, so the kernel without conditions
  hdv     64 x 1440 x 1080 yuv420p -> 1920 columns (4:3): every row 16-byte aligned, the one-store kernel
  p010    32 x 1920 x 1080 p010le -> 1920 columns through a table that is not the identity (the filter a quarter column off its
          centres): the cost of 2-byte interleaved samples at the width of the conversion's own benchmark, for cost only
each with every filter (bilinear 2 taps, bicubic 4, lanczos 6).  Per case the rows alternate for `--rounds` rounds, HIP events over
`--iters` launches after warm-up each time, so the spread between a row's repeats is the job's own noise:
  plain      vse_yuv_to_bgr_format of the stored frames (the parent's kernels, unchanged)
  <filter>   vse_yuv_resample of the same frames
bytes moved by a resample = the packed frame read once + the packed output written.  One JSON line per measurement, then one summary
line per row with the median time per frame, GB/s, the ratio to the plain conversion and the frame's time on the link (--link-gbs,
EXPERIMENTS.md L)."""
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


class ShiftedFilter(ingest.Resample):
    """A Resample of equal widths whose centres lie a quarter column to the right: every tap carries weight (for cost only)."""
    __slots__ = ()

    def tables(self, fmt):
        def table(pw):
            support = {"bicubic": 2, "bilinear": 1, "lanczos": 3}[self.filter]
            c = np.arange(pw, dtype=np.float64) + 0.25
            left = np.floor(c - support).astype(np.int64) + 1
            w = ingest._filter_kernel(self.filter, left[:, None] + np.arange(2 * support)[None, :] - c[:, None])
            q = np.rint(w / w.sum(axis=1, keepdims=True) * 16384.0).astype(np.int64)
            q[np.arange(pw), np.argmax(w, axis=1)] += 16384 - q.sum(axis=1)
            ingest.check_resample_table(left, q)
            return left.astype(np.int32), q.astype(np.int16)
        return table(self.out_width), (table(fmt.chroma_size(1, self.out_width)[1]) if fmt.chroma else None)


def packed_frames(frames, fmt, w):
    """BGR frames -> [distinct, frame bytes] uint8 of `fmt` (8-bit planar 4:2:0 or P010), the luma cut or repeated to w columns."""
    out = []
    for f in frames:
        reps = -(-w // f.shape[1])
        y, u, v = ingest.bgr_to_yuv420(np.tile(f, (1, reps, 1))[:, :w])
        if fmt.chroma == 2:
            planes = (y.astype("<u2") << 8, np.stack([u, v], axis=2).reshape(u.shape[0], -1).astype("<u2") << 8)
        else:
            planes = (y, u, v)
        out.append(np.concatenate([np.ascontiguousarray(p).reshape(-1).view(np.uint8) for p in planes]))
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=2, help="frames made on the host, repeated to fill a batch")
    ap.add_argument("--link-gbs", type=float, default=57.1, help="host-to-device rate of pinned uploads, GB/s")
    a = ap.parse_args()
    ctx = engine.Context(0)
    runs = []
    for case, n, h, w, w_out, pix_fmt in (("dvd", 64, 480, 720, 854, "yuv420p"), ("hdv", 64, 1080, 1440, 1920, "yuv420p"),
                                          ("p010", 32, 1080, 1920, 1920, "p010le")):
        fmt = ingest.YuvFormat.from_pix_fmt(pix_fmt, matrix="bt709")
        frame, frame_out = fmt.frame_bytes(h, w), fmt.frame_bytes(h, w_out)
        host = packed_frames(synth.make_frames(a.distinct, h, min(w, 1280), seed=1), fmt, w)
        assert host.shape == (a.distinct, frame)
        stride = (frame + 15) & ~15
        packed = torch.zeros((n, stride), dtype=torch.uint8, device=ctx.tdev)
        packed[:, :frame] = torch.from_numpy(host[np.arange(n) % a.distinct]).to(ctx.tdev)
        bgr = torch.empty((n, h, w, 3), dtype=torch.uint8, device=ctx.tdev)
        out = torch.empty((n, (frame_out + 15) & ~15), dtype=torch.uint8, device=ctx.tdev)
        runs.append(dict(case=case, what="plain", n=n, h=h, w=w, w_out=w, frame=frame, moved=frame + 3 * h * w, us=[],
                         fn=lambda p=packed, o=bgr, n=n, h=h, w=w, f=fmt: ctx.yuv_to_bgr(p, n, h, w, f, 0, out=o)))
        for name in ("bilinear", "bicubic", "lanczos"):
            r = ShiftedFilter(w, w_out, name) if w == w_out else ingest.Resample(w, w_out, name)
            got = ctx.yuv_resample(packed, n, h, w, fmt, r, out=out)
            planes = r.planes(fmt, tuple(p[:16] for p in ingest._planes_at(host[0], 0, h, w, fmt)))          # the host's integers, 16 rows
            dev = ingest._planes_at(got[0].cpu().numpy(), 0, h, w_out, fmt)
            assert all(np.array_equal(d[:len(p)], p) for d, p in zip(dev, planes)), (case, name)
            runs.append(dict(case=case, what=name, n=n, h=h, w=w, w_out=w_out, frame=frame, moved=frame + frame_out, us=[],
                             taps=int(r.tables(fmt)[0][1].shape[1]),
                             fn=lambda p=packed, o=out, n=n, h=h, w=w, f=fmt, r=r: ctx.yuv_resample(p, n, h, w, f, r, out=o)))
    for rnd in range(a.rounds):
        for run in runs:
            us = timed(run["fn"], a.iters) / run["n"]
            run["us"].append(us)
            print(json.dumps({"case": run["case"], "what": run["what"], "h": run["h"], "w": run["w"], "w_out": run["w_out"], "frames": run["n"],
                              "round": rnd, "us_per_frame": round(us, 2), "gb_per_s": round(run["moved"] / us / 1e3, 1)}), flush=True)
    plain = {run["case"]: float(np.median(run["us"])) for run in runs if run["what"] == "plain"}
    for run in runs:
        med = float(np.median(run["us"]))
        link_us = run["frame"] / a.link_gbs / 1e3
        print(json.dumps({"summary": run["what"], "case": run["case"], "h": run["h"], "w": run["w"], "w_out": run["w_out"], "taps": run.get("taps"),
                          "us_per_frame_median": round(med, 2), "us_per_frame_min": round(min(run["us"]), 2),
                          "us_per_frame_max": round(max(run["us"]), 2), "gb_per_s_median": round(run["moved"] / med / 1e3, 1),
                          "over_plain": round(med / plain[run["case"]], 3), "link_us_per_frame": round(link_us, 1),
                          "hides_under_the_upload": bool(max(run["us"]) < link_us)}), flush=True)


if __name__ == "__main__":
    main()
