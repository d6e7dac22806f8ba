#!/usr/bin/env python3
"""Cost of interval fusion (SubtitleExtractor(interval_text="fused")), in two parts, one JSON line per measurement.

(a) --kernel: vse_ctc_fuse alone at ncls 6625, t 40 and 240, K 3 and 5, 32 groups, on random probabilities: microseconds per call
    between two device events and bytes read per second (g * K * t * ncls * 4; the eight bytes written per step do not count).  The
    t = 40 tensors (102 / 170 MB) stay resident in the 256 MiB Infinity Cache, the t = 240 ones (0.6 / 1.0 GB) do not.  --stride adds
    floats to row_stride: 0 is the recogniser's own layout (ncls odd: one step in four takes the 16-byte loads), 3 aligns every row.
    Put tools/copy_ceiling.py's numbers of the same session next to it; there is no pass mark, the kernel is a small share of (b).
(b) --extract: extractor.SubtitleExtractor.run() on a synthetic 1080p clip held in HOST memory (every frame's upload is inside the
    timed region), frame_selector="change", staged upload: interval_text "single" and "fused" with 3 and 5 samples, `--runs` timed
    runs each after one warm-up run, frames/s and milliseconds per interval.  The clip holds each subtitle for --hold frames with as
    many dark frames between, so fused samples show the same pixels: this times the plumbing and the recogniser running K times,
    not a recognition gain (no real clips, stand-in recogniser weights).  --modes single runs on a checkout without the feature
    too (--root: the checkout whose vse_amd is timed), which is how "single" is compared with the parent commit on one box.

usage: python tools/bench_interval_fuse.py --kernel [--iters 50] [--stride 0]
       python tools/bench_interval_fuse.py --extract [--frames 1152] [--hold 24] [--runs 3] [--modes single,fused3,fused5] [--rec V4_ch_rec_fast]"""
import argparse
import json
import os
import sys
import time


def kernel_rows(a):
    import torch
    from vse_amd import engine
    ctx = engine.Context(0)
    ncls, g = 6625, 32
    for t in (40, 240):
        for k in (3, 5):
            b = g * k
            stride = ncls + a.stride
            buf = torch.rand((b * t, stride), dtype=torch.float32, device=ctx.tdev)
            probs = buf[:, :ncls].view(b, 1, t, ncls) if a.stride == 0 else torch.as_strided(buf, (b, 1, t, ncls), (t * stride, t * stride, stride, 1))
            group = list(range(0, b + 1, k))
            for _ in range(3):
                out = ctx.ctc_fuse(probs, group)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                out = ctx.ctc_fuse(probs, group)
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / a.iters
            nbytes = b * t * ncls * 4
            print(json.dumps({"what": "vse_ctc_fuse", "ncls": ncls, "t": t, "K": k, "groups": g, "row_stride": stride, "us_per_call": round(us, 1),
                              "read_mb": round(nbytes / 1e6, 1), "read_tb_per_s": round(nbytes / us / 1e6, 3),
                              "argmax_checksum": int(out.view(torch.int32)[..., 0].sum())}), flush=True)
            del buf, probs, out


def extract_rows(a):
    import numpy as np
    import torch
    from vse_amd import engine, extractor, frame_select, modelzoo, pipeline, shim, staging, synth
    ctx = engine.Context(0)
    det = modelzoo.get_model("V3_ch_det_fast", seed=0)
    rec = modelzoo.get_model(a.rec, seed=1)
    charset = shim.en_charset() if a.rec == "V4_en_rec_fast" else shim.standin_charset("ch", shim._ncls(rec[0]))
    pipe = pipeline.OcrPipeline(ctx, det, rec, charset)
    n_sub = (a.frames + 2 * a.hold - 1) // (2 * a.hold)
    lit = synth.make_frames(min(n_sub, 48), a.height, a.width, seed=9)
    dark = np.full((a.height, a.width, 3), 40, np.uint8)
    clip = []
    for k in range(n_sub):
        clip += [lit[k % len(lit)]] * a.hold + [dark] * a.hold
    clip = clip[:a.frames]
    fps = 24.0

    class Ocr(shim.OcrRecogniser):
        """The shim's recogniser object over this tool's pipeline (no model files needed)."""

        def __init__(self):
            super().__init__()
            self.recogniser = shim.PaddleOCR.__new__(shim.PaddleOCR)
            self.recogniser.pipe = pipe

    area = extractor.SubtitleArea(ymin=int(0.75 * a.height), ymax=a.height, xmin=0, xmax=a.width)
    up = staging.Uploader(ctx.tdev)
    modes = {"single": {}, "fused3": dict(interval_text="fused", fuse_params={"samples": 3}),
             "fused5": dict(interval_text="fused", fuse_params={"samples": 5})}
    for name in a.modes.split(","):
        def run(frames):
            ex = extractor.SubtitleExtractor(extractor.ArraySource(frames, fps), Ocr(), sub_area=area, mode="fast", frame_selector="change",
                                             change_counter=frame_select.EngineCounter(ctx), uploader=up, drop_score=0.0, batch=a.batch,
                                             **modes[name])
            torch.cuda.synchronize()
            t0 = time.time()
            text = ex.run()
            torch.cuda.synchronize()
            return time.time() - t0, ex, text
        run(clip)                                           # warm-up: every plan the timed runs use is compiled and its workspace allocated
        for k in range(a.runs):
            dt, ex, text = run(clip)
            print(json.dumps({"what": "extract", "mode": name, "run": k, "rec": a.rec, "frames": len(clip), "frame": [a.height, a.width],
                              "intervals": len(ex.intervals), "seconds": round(dt, 3), "frames_per_s": round(len(clip) / dt, 1),
                              "ms_per_interval": round(dt * 1e3 / max(len(ex.intervals), 1), 2), "srt_blocks": text.count(" --> "),
                              "root": a.root}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--extract", action="store_true")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--stride", type=int, default=0, help="floats added to row_stride = ncls")
    ap.add_argument("--frames", type=int, default=1152)
    ap.add_argument("--hold", type=int, default=24, help="frames one subtitle stays on screen")
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--modes", default="single,fused3,fused5")
    ap.add_argument("--rec", default="V4_ch_rec_fast", help="recogniser model id (stand-in weights)")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose vse_amd is measured")
    a = ap.parse_args()
    sys.path.insert(0, a.root)
    if a.kernel:
        kernel_rows(a)
    if a.extract:
        extract_rows(a)


if __name__ == "__main__":
    main()
