#!/usr/bin/env python3
"""vse_yuv_vscale beside the unchanged vse_yuv_to_bgr_format on the same frames, in one job: what scaling UHD and other oversized YUV down
costs in front of the conversion, and whether the scaled route still hides under the upload it rides on.

Device-resident frames of a synthetic clip (synth.make_frames through ingest.bgr_to_yuv420, tiled to the size; `--distinct` frames
repeated), three cases:
  uhd      16 x 3840 x 2160 yuv420p -> 1920 x 1080
  uhd-p010 16 x 3840 x 2160 p010le  -> 1920 x 1080 (2-byte samples, interleaved chroma)
  hd       32 x 1920 x 1080 yuv420p -> 1280 x 720
each with every filter (at 2 : 1 bilinear 4 taps, bicubic 8, lanczos 12; at 3 : 2 4, 6, 10).  Per case the rows alternate for `--rounds`
rounds, HIP events over `--iters` launches after warm-up each time, so the spread between a row's repeats is the job's own noise:
  plain          vse_yuv_to_bgr_format of the stored, unscaled frames (the parent's kernels, unchanged)
  <filter> v     vse_yuv_vscale of the same frames, whole pictures
  <filter> v+h   ... and vse_yuv_resample of its output to the output width
  <filter> route ... and vse_yuv_to_bgr_format of that: everything the Uploader runs behind the copy
bytes moved by the vertical pass = the packed frame read once + the packed output written once.  One JSON line per measurement, then one
summary line per row with the median time per frame and min - max, GB/s (vertical pass only), the ratio to the plain conversion and the
frame's time on the link (--link-gbs, EXPERIMENTS.md L)."""
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


def packed_frames(frames, fmt, h, w):
    """BGR frames -> [distinct, frame bytes] uint8 of `fmt` (8-bit planar 4:2:0 or P010), tiled to h x w."""
    out = []
    for f in frames:
        y, u, v = ingest.bgr_to_yuv420(np.tile(f, (-(-h // f.shape[0]), -(-w // f.shape[1]), 1))[:h, :w])
        if fmt.chroma == 2:
            planes = (y.astype("<u2") << 8, np.stack([u, v], axis=2).reshape(u.shape[0], -1).astype("<u2") << 8)
        else:
            planes = (y, u, v)
        out.append(np.concatenate([np.ascontiguousarray(p).reshape(-1).view(np.uint8) for p in planes]))
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--distinct", type=int, default=2, help="frames made on the host, repeated to fill a batch")
    ap.add_argument("--link-gbs", type=float, default=57.1, help="host-to-device rate of pinned uploads, GB/s")
    a = ap.parse_args()
    ctx = engine.Context(0)
    runs = []
    for case, n, h, w, h_out, w_out, pix_fmt in (("uhd", 16, 2160, 3840, 1080, 1920, "yuv420p"), ("uhd-p010", 16, 2160, 3840, 1080, 1920, "p010le"),
                                                 ("hd", 32, 1080, 1920, 720, 1280, "yuv420p")):
        fmt = ingest.YuvFormat.from_pix_fmt(pix_fmt, matrix="bt709")
        frame, frame_mid, frame_out = fmt.frame_bytes(h, w), fmt.frame_bytes(h_out, w), fmt.frame_bytes(h_out, w_out)
        host = packed_frames(synth.make_frames(a.distinct, 360, 640, seed=1), fmt, h, w)
        assert host.shape == (a.distinct, frame)
        stride = (frame + 15) & ~15
        packed = torch.zeros((n, stride), dtype=torch.uint8, device=ctx.tdev)
        packed[:, :frame] = torch.from_numpy(host[np.arange(n) % a.distinct]).to(ctx.tdev)
        bgr = torch.empty((n, h, w, 3), dtype=torch.uint8, device=ctx.tdev)
        small = torch.empty((n, h_out, w_out, 3), dtype=torch.uint8, device=ctx.tdev)
        mid = torch.empty((n, (frame_mid + 15) & ~15), dtype=torch.uint8, device=ctx.tdev)
        out = torch.empty((n, (frame_out + 15) & ~15), dtype=torch.uint8, device=ctx.tdev)
        common = dict(case=case, n=n, h=h, w=w, h_out=h_out, w_out=w_out, frame=frame)
        runs.append(dict(common, what="plain", moved=frame + 3 * h * w, us=[],
                         fn=lambda p=packed, o=bgr, n=n, h=h, w=w, f=fmt: ctx.yuv_to_bgr(p, n, h, w, f, 0, out=o)))
        for name in ("bilinear", "bicubic", "lanczos"):
            v, r = ingest.VScale(h, h_out, name), ingest.Resample(w, w_out, name)
            assert v.source_rows(fmt, 0, h_out) == (0, h)

            def vertical(p=packed, o=mid, n=n, h=h, w=w, f=fmt, v=v, h_out=h_out):
                return ctx.yuv_vscale(p, n, h, w, f, v, 0, h, 0, h_out, out=o)

            def both(o=out, n=n, w=w, f=fmt, r=r, h_out=h_out, vertical=vertical):
                return ctx.yuv_resample(vertical(), n, h_out, w, f, r, out=o)

            def route(o=small, n=n, f=fmt, h_out=h_out, w_out=w_out, both=both):
                return ctx.yuv_to_bgr(both(), n, h_out, w_out, f, 0, out=o)
            got = vertical()
            planes = v.planes(fmt, ingest._planes_at(host[0], 0, h, w, fmt), 0, 16)                          # the host's integers, 16 rows
            dev = ingest._planes_at(got[0].cpu().numpy(), 0, h_out, w, fmt)
            assert all(np.array_equal(d[:len(p)], p) for d, p in zip(dev, planes)), (case, name)
            taps = int(v.tables(fmt)[0][1].shape[1])
            runs.append(dict(common, what=name + " v", taps=taps, moved=frame + frame_mid, us=[], fn=vertical))
            runs.append(dict(common, what=name + " v+h", taps=taps, moved=None, us=[], fn=both))
            runs.append(dict(common, what=name + " route", taps=taps, moved=None, us=[], fn=route))
    for rnd in range(a.rounds):
        for run in runs:
            us = timed(run["fn"], a.iters) / run["n"]
            run["us"].append(us)
            print(json.dumps({"case": run["case"], "what": run["what"], "h": run["h"], "w": run["w"], "h_out": run["h_out"], "w_out": run["w_out"],
                              "frames": run["n"], "round": rnd, "us_per_frame": round(us, 2),
                              "gb_per_s": None if run["moved"] is None else round(run["moved"] / us / 1e3, 1)}), flush=True)
    plain = {run["case"]: float(np.median(run["us"])) for run in runs if run["what"] == "plain"}
    for run in runs:
        med = float(np.median(run["us"]))
        link_us = run["frame"] / a.link_gbs / 1e3
        print(json.dumps({"summary": run["what"], "case": run["case"], "h": run["h"], "w": run["w"], "h_out": run["h_out"], "w_out": run["w_out"],
                          "taps": run.get("taps"), "us_per_frame_median": round(med, 2), "us_per_frame_min": round(min(run["us"]), 2),
                          "us_per_frame_max": round(max(run["us"]), 2),
                          "gb_per_s_median": None if run["moved"] is None else round(run["moved"] / med / 1e3, 1),
                          "over_plain": round(med / plain[run["case"]], 3), "link_us_per_frame": round(link_us, 1),
                          "hides_under_the_upload": bool(max(run["us"]) < link_us)}), flush=True)


if __name__ == "__main__":
    main()
