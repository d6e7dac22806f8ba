#!/usr/bin/env python3
"""Cost of the edge threshold chosen in the selector's own pass (vse_frame_cells_counts, vse_frame_cells_export_state,
frame_select.CalibratingChangeSelector), one JSON line per figure, in one process.

    a   one vse_frame_cells_counts over 64 frames of 1080p, rows 810:1080 (the band alone is on the device, as the selector stages it),
        at nt = 8 (thresholds 24 32 48 64 96 128 160 192) against the two launches it replaces, vse_frame_cells_multi with the same
        thresholds plus vse_frame_change at 128, and at nt = 1 (threshold 128) against vse_frame_change alone.  Two pictures: `text`
        (synth.make_frames, a few thousand edge pixels per frame) and `noise` (random bytes: every pixel an edge at the low
        thresholds, the most the atomics can be asked for).  Counts and totals are first held equal to the existing entries'.  After
        a warm-up, blocks of `calls` calls of the one and of the other alternate between device events, `rounds` times; the medians
        are reported as ms per call, and their ratio.
    b   vse_frame_cells_export_state on that band's state: its own time, ms per call.
    c   end to end on tools/bench_one_pass.py's clip (synthetic 1080p at 24 fps held as YUV 4:2:0 in host memory, area rows 810:1080,
        staged upload, mobile models, the change selector, edge_thresh="auto"): several passes without the key (calibration pass,
        selector pass), several passes with it, one pass with it (calibrate_seconds = `--calibrate-seconds`), and the plain one-pass
        run at the constant 128 for its peak_retained; `--runs` timed runs each after one warm-up run.  `decodes`: how often the clip
        was read from its start.

No decoder runs here (the frames are in host memory, so a saved pass saves an upload and a conversion, not a decode), and how the choice
or a window of 300 s behaves on real footage is not measured by this tool.

usage: python tools/bench_streaming_calibration.py [--parts a,b,c] [--calls 50] [--rounds 5] [--frames 9216] [--hold 24]
                                                   [--calibrate-seconds 20] [--runs 5]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from vse_amd import area_locator, engine, frame_select  # noqa: E402

BATCH = 64
T8 = area_locator.AUTO_THRESHOLDS


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def kernels(a, ctx):
    from vse_amd import synth
    h, w = 1080, 1920
    y0 = int(0.75 * h)
    ah = h - y0
    area = (0, ah, 0, w)                                  # in a band of the area's rows alone
    params = area_locator.AreaLocator(edge_thresh="auto").params(24.0)
    gen = torch.Generator(device=ctx.tdev)
    gen.manual_seed(1)
    lit = synth.make_frames(8, h, w, seed=9)[:, y0:]
    pictures = {"text": torch.from_numpy(lit).to(ctx.tdev).repeat(BATCH // 8, 1, 1, 1).contiguous(),
                "noise": torch.randint(0, 256, (BATCH, ah, w, 3), dtype=torch.uint8, device=ctx.tdev, generator=gen)}
    for name, band in pictures.items():
        for ths in (T8, (128,)):
            nt = len(ths)
            fused_state = ctx.frame_cells_multi_state(ah, w, nt)
            multi_state = ctx.frame_cells_multi_state(ah, w, nt)
            change_state = ctx.frame_change_state(ah, w)
            totals, counts = ctx.frame_cells_counts(band, area, ths, params, fused_state, reset=True, flush=True)
            want_totals = ctx.frame_cells_multi(band, area, ths, params, multi_state, reset=True, flush=True)
            assert torch.equal(totals, want_totals) and torch.equal(fused_state.words, multi_state.words), (name, nt)
            for q, th in enumerate(ths):
                assert torch.equal(counts[:, q], ctx.frame_change(band, area, th, change_state, reset=True)), (name, nt, th)

            def fused():
                ctx.frame_cells_counts(band, area, ths, params, fused_state, reset=True, flush=True)

            def two():
                if nt > 1:
                    ctx.frame_cells_multi(band, area, ths, params, multi_state, reset=True, flush=True)
                ctx.frame_change(band, area, 128, change_state, reset=True)
            for _ in range(2):
                timed(fused, a.calls), timed(two, a.calls)
            times = {"fused": [], "two": []}
            for _ in range(a.rounds):
                times["fused"].append(timed(fused, a.calls))
                times["two"].append(timed(two, a.calls))
            ms = {n: statistics.median(v) for n, v in times.items()}
            print(json.dumps({"what": "cells_counts", "picture": name, "nt": nt, "frames": BATCH, "area": [ah, w],
                              "edges_per_frame_at_128": int(counts[:, ths.index(128), 0].float().mean()),
                              "against": "frame_cells_multi + frame_change" if nt > 1 else "frame_change",
                              "fused_ms": round(ms["fused"], 4), "fused_ms_min": round(min(times["fused"]), 4),
                              "replaced_ms": round(ms["two"], 4), "replaced_ms_min": round(min(times["two"]), 4),
                              "ratio": round(ms["fused"] / ms["two"], 3),
                              "fused_gb_per_s_frame_bytes": round(BATCH * ah * w * 3 / ms["fused"] / 1e6, 1)}), flush=True)
            if "b" in a.parts and nt == 8 and name == "text":
                out = ctx.frame_change_state(ah, w)

                def export():
                    ctx.frame_cells_export_state(fused_state, ah, w, 3, out=out)
                for _ in range(2):
                    timed(export, a.calls)
                ms = [timed(export, a.calls) for _ in range(a.rounds)]
                print(json.dumps({"what": "export_state", "area": [ah, w], "state_bytes": out.numel(), "ms": round(statistics.median(ms), 4),
                                  "ms_min": round(min(ms), 4)}), flush=True)


def end_to_end(a, ctx):
    import numpy as np
    from bench_one_pass import Yuv420ArraySource, schedule
    from vse_amd import extractor, ingest, modelzoo, pipeline, shim, staging, synth
    det = modelzoo.get_model("V3_ch_det_fast", seed=0)
    rec = modelzoo.get_model("V4_ch_rec_fast", seed=1)
    pipe = pipeline.OcrPipeline(ctx, det, rec, shim.standin_charset("ch", shim._ncls(rec[0])))
    h, w, fps = 1080, 1920, 24.0
    n_sub = (a.frames + 2 * a.hold - 1) // (2 * a.hold)
    lit = synth.make_frames(min(n_sub, 48), h, w, seed=9)
    pictures = [ingest.bgr_to_yuv420(f) for f in lit] + [ingest.bgr_to_yuv420(np.full((h, w, 3), 40, np.uint8))]
    raw = [ingest.Yuv420Frame(p, h, w, "i420") for p in pictures]
    clip = [raw[k] for k in schedule(a.frames, a.hold, len(pictures))]

    class Ocr(shim.OcrRecogniser):
        """The shim's recogniser object over this tool's pipeline (no model files needed)."""

        def __init__(self):
            super().__init__()
            self.recogniser = shim.PaddleOCR.__new__(shim.PaddleOCR)
            self.recogniser.pipe = pipe

    class Counting(Yuv420ArraySource):
        """... that counts how often the clip is read from its start."""
        decodes = 0

        def raw_frames(self):
            self.decodes += 1
            return super().raw_frames()

        def frames(self):
            self.decodes += 1
            return super().frames()

    area = extractor.SubtitleArea(ymin=int(0.75 * h), ymax=h, xmin=0, xmax=w)
    up = staging.Uploader(ctx.tdev)
    auto = {"edge_thresh": "auto"}
    rows = {"multi_auto": dict(change_params=auto, area_params={"cells_fn": area_locator.EngineCells(ctx)}),
            "multi_auto_streaming": dict(change_params=auto, area_params={"streaming": True}),
            "onepass_auto_streaming": dict(one_pass=True, change_params=auto,
                                           area_params={"streaming": True, "calibrate_seconds": a.calibrate_seconds}),
            "onepass_128": dict(one_pass=True)}

    def run(kw):
        src = Counting(clip, fps)
        if kw.get("area_params", {}).get("streaming"):
            kw = {**kw, "area_params": {**kw["area_params"], "cells_counts_fn": frame_select.EngineCellsCounts(ctx)}}
        ex = extractor.SubtitleExtractor(src, Ocr(), sub_area=area, mode="fast", frame_selector="change",
                                         change_counter=frame_select.EngineCounter(ctx), uploader=up, drop_score=0.0, batch=BATCH, **kw)
        torch.cuda.synchronize()
        t0 = time.time()
        text = ex.run()
        torch.cuda.synchronize()
        return time.time() - t0, ex, text, src
    try:
        for name, kw in rows.items():
            run(kw)
            for k in range(a.runs):
                dt, ex, text, src = run(kw)
                print(json.dumps({"what": "end_to_end", "row": name, "run": k, "frames": a.frames, "hold": a.hold, "intervals": len(ex.intervals),
                                  "seconds": round(dt, 3), "frames_per_s": round(a.frames / dt, 1), "one_pass": ex.one_pass,
                                  "decodes": src.decodes, "edge_thresh": ex.edge_thresh, "frames_calibrated": ex.frames_calibrated,
                                  "peak_retained": ex.peak_retained, "clamped_intervals": ex.clamped_intervals,
                                  "srt_blocks": text.count(" --> ")}), flush=True)
    finally:
        up.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--calls", type=int, default=50, help="calls per timed block")
    ap.add_argument("--rounds", type=int, default=5, help="timed blocks per figure; the median is reported")
    ap.add_argument("--frames", type=int, default=9216)
    ap.add_argument("--hold", type=int, default=24, help="part c: frames one subtitle stays on screen")
    ap.add_argument("--calibrate-seconds", type=float, default=20.0, help="part c: the one-pass window")
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    a.parts = a.parts.split(",")
    ctx = engine.Context(0)
    if "a" in a.parts or "b" in a.parts:
        kernels(a, ctx)
    if "c" in a.parts:
        end_to_end(a, ctx)


if __name__ == "__main__":
    main()
