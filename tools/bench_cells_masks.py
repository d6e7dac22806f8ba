#!/usr/bin/env python3
"""Cost of the subtitle area found in the selector's own pass (vse_frame_cells_masks, vse_frame_masks_replay,
frame_select.LocatingChangeSelector), one JSON line per figure, in one process.

    a   one vse_frame_cells_masks over 64 whole frames of 1080p at nt = 1 (threshold 128) and nt = 8 (thresholds 24 32 48 64 96 128 160
        192) against vse_frame_cells_multi at the same, the kernel it copies, which writes no masks.  Two pictures: `text`
        (synth.make_frames) and `noise` (random bytes).  Totals, state and the kept words are first held equal to the existing entry's
        and to each other.  After a warm-up, blocks of `calls` calls of the one and of the other alternate between device events,
        `rounds` times; the medians are reported as ms per call, and their ratio.  The masks kernel writes nt bits per 24 bits it reads:
        +4 % bytes at one threshold, +33 % at eight.
    b   vse_frame_masks_replay of a window of `--window` slots (1440: a minute at 24 fps) on a band-sized rectangle, rows 810:1080 of
        the frame, at nt = 1 and nt = 8 (the slots are as far apart as the thresholds are many): its own time, ms per call.
    c   end to end on tools/bench_one_pass.py's clip (synthetic 1080p at 24 fps held as YUV 4:2:0 in host memory, staged upload, mobile
        models, the change selector at 128): one pass with the key (locate_seconds = `--locate-seconds`) against the plain one-pass run
        with the located box typed in, and several passes with the key against several passes with the locator's own pass over the
        same window (probe); `--runs` timed runs each after one warm-up run.  `decodes`: how often the clip was read from its start;
        `peak_retained`: the most frames a one-pass run held at once.

No decoder runs here (the frames are in host memory, so a saved pass saves an upload and a conversion, not a decode), and whether a
minute of a real film finds its band is not measured by this tool.

usage: python tools/bench_cells_masks.py [--parts a,b,c] [--calls 20] [--rounds 5] [--window 1440] [--frames 9216] [--hold 24]
                                         [--locate-seconds 20] [--runs 5]"""
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
H, W = 1080, 1920


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def pictures(ctx):
    from vse_amd import synth
    gen = torch.Generator(device=ctx.tdev)
    gen.manual_seed(1)
    lit = synth.make_frames(8, H, W, seed=9)
    return {"text": torch.from_numpy(lit).to(ctx.tdev).repeat(BATCH // 8, 1, 1, 1).contiguous(),
            "noise": torch.randint(0, 256, (BATCH, H, W, 3), dtype=torch.uint8, device=ctx.tdev, generator=gen)}


def kernels(a, ctx):
    region = (0, H, 0, W)
    params = area_locator.AreaLocator(edge_thresh="auto").params(24.0)
    for name, frames in pictures(ctx).items():
        for ths in ((128,), T8):
            nt = len(ths)
            masks_state = ctx.frame_cells_multi_state(H, W, nt)
            multi_state = ctx.frame_cells_multi_state(H, W, nt)
            masks = ctx.frame_masks_buffer(H, W, nt, BATCH)
            totals = ctx.frame_cells_masks(frames, region, ths, params, masks_state, masks, 0, reset=True, flush=True)
            want = ctx.frame_cells_multi(frames, region, ths, params, multi_state, reset=True, flush=True)
            assert torch.equal(totals, want) and torch.equal(masks_state.words, multi_state.words), (name, nt)
            # the kept words against vse_frame_change on a rectangle, through the replay
            counts, _state = ctx.frame_masks_replay(masks, nt - 1, 0, BATCH, (810, H, 0, W))
            assert torch.equal(counts, ctx.frame_change(frames, (810, H, 0, W), ths[-1], ctx.frame_change_state(H - 810, W), reset=True))

            def kept():
                ctx.frame_cells_masks(frames, region, ths, params, masks_state, masks, 0, reset=True, flush=True)

            def plain():
                ctx.frame_cells_multi(frames, region, ths, params, multi_state, reset=True, flush=True)
            for _ in range(2):
                timed(kept, a.calls), timed(plain, a.calls)
            times = {"masks": [], "multi": []}
            for _ in range(a.rounds):
                times["masks"].append(timed(kept, a.calls))
                times["multi"].append(timed(plain, a.calls))
            ms = {n: statistics.median(v) for n, v in times.items()}
            read, written = BATCH * H * W * 3, masks.words.numel()
            print(json.dumps({"what": "cells_masks", "picture": name, "nt": nt, "frames": BATCH, "region": [H, W],
                              "masks_ms": round(ms["masks"], 4), "masks_ms_min": round(min(times["masks"]), 4),
                              "multi_ms": round(ms["multi"], 4), "multi_ms_min": round(min(times["multi"]), 4),
                              "ratio": round(ms["masks"] / ms["multi"], 3), "bytes_ratio": round((read + written) / read, 3),
                              "masks_gb_per_s_read_and_written": round((read + written) / ms["masks"] / 1e6, 1)}), flush=True)


def replay(a, ctx):
    region = (0, H, 0, W)
    params = area_locator.AreaLocator(edge_thresh="auto").params(24.0)
    frames = pictures(ctx)["text"]
    rect = (810, H, 0, W)
    for ths in ((128,), T8):
        nt = len(ths)
        state = ctx.frame_cells_multi_state(H, W, nt)
        masks = ctx.frame_masks_buffer(H, W, nt, a.window)
        for slot0 in range(0, a.window, BATCH):
            n = min(BATCH, a.window - slot0)
            ctx.frame_cells_masks(frames[:n], region, ths, params, state, masks, slot0, reset=slot0 == 0, flush=False)
        out = ctx.frame_change_state(rect[1] - rect[0], rect[3] - rect[2])

        def call():
            ctx.frame_masks_replay(masks, nt - 1, 0, a.window, rect, reset=True, out=out)
        for _ in range(2):
            timed(call, a.calls)
        ms = [timed(call, a.calls) for _ in range(a.rounds)]
        touched = a.window * (rect[1] - rect[0] - 2) * ((W - 2 + 63) // 64) * 8
        print(json.dumps({"what": "masks_replay", "nt": nt, "slots": a.window, "rect": list(rect), "buffer_bytes": masks.words.numel(),
                          "ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4),
                          "gb_per_s_words_of_the_rectangle_read_twice": round(2 * touched / statistics.median(ms) / 1e6, 1)}), flush=True)
        del masks


def end_to_end(a, ctx):
    import numpy as np
    from bench_one_pass import Yuv420ArraySource, schedule
    from vse_amd import extractor, ingest, modelzoo, pipeline, shim, staging, synth
    det = modelzoo.get_model("V3_ch_det_fast", seed=0)
    rec = modelzoo.get_model("V4_ch_rec_fast", seed=1)
    pipe = pipeline.OcrPipeline(ctx, det, rec, shim.standin_charset("ch", shim._ncls(rec[0])))
    fps = 24.0
    n_sub = (a.frames + 2 * a.hold - 1) // (2 * a.hold)
    lit = synth.make_frames(min(n_sub, 48), H, W, seed=9)
    planes = [ingest.bgr_to_yuv420(f) for f in lit] + [ingest.bgr_to_yuv420(np.full((H, W, 3), 40, np.uint8))]
    raw = [ingest.Yuv420Frame(p, H, W, "i420") for p in planes]
    clip = [raw[k] for k in schedule(a.frames, a.hold, len(planes))]
    window = int(round(a.locate_seconds * fps))

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

    up = staging.Uploader(ctx.tdev)
    key = {"streaming_locate": True, "locate_seconds": a.locate_seconds}
    rows = {"multi_locator_pass": dict(sub_area="auto", area_params={"cells_fn": area_locator.EngineCells(ctx), "probe": (1, window)}),
            "multi_locate_key": dict(sub_area="auto", area_params=key),
            "onepass_locate_key": dict(sub_area="auto", one_pass=True, area_params=key),
            "onepass_box_typed_in": dict(one_pass=True)}
    located = [None]

    def run(kw):
        src = Counting(clip, fps)
        if kw.get("area_params", {}).get("streaming_locate"):
            kw = {**kw, "area_params": {**kw["area_params"], "cells_masks_fn": frame_select.EngineCellsMasks(ctx)}}
        if "sub_area" not in kw:
            kw = {**kw, "sub_area": located[0]}
        ex = extractor.SubtitleExtractor(src, Ocr(), mode="fast", frame_selector="change", change_counter=frame_select.EngineCounter(ctx),
                                         uploader=up, drop_score=0.0, batch=BATCH, **kw)
        torch.cuda.synchronize()
        t0 = time.time()
        text = ex.run()
        torch.cuda.synchronize()
        if ex.located_area is not None:
            located[0] = ex.located_area
        return time.time() - t0, ex, text, src
    try:
        for name, kw in rows.items():
            run(kw)
            for k in range(a.runs):
                dt, ex, text, src = run(kw)
                area = ex.sub_area
                print(json.dumps({"what": "end_to_end", "row": name, "run": k, "frames": a.frames, "hold": a.hold, "window": window,
                                  "area": None if area is None else [area.ymin, area.ymax, area.xmin, area.xmax],
                                  "intervals": None if ex.intervals is None else len(ex.intervals), "seconds": round(dt, 3),
                                  "frames_per_s": round(a.frames / dt, 1), "one_pass": ex.one_pass, "decodes": src.decodes,
                                  "peak_retained": ex.peak_retained, "clamped_intervals": ex.clamped_intervals,
                                  "srt_blocks": text.count(" --> ")}), flush=True)
    finally:
        up.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--calls", type=int, default=20, help="calls per timed block")
    ap.add_argument("--rounds", type=int, default=5, help="timed blocks per figure; the median is reported")
    ap.add_argument("--window", type=int, default=1440, help="part b: slots replayed")
    ap.add_argument("--frames", type=int, default=9216)
    ap.add_argument("--hold", type=int, default=24, help="part c: frames one subtitle stays on screen")
    ap.add_argument("--locate-seconds", type=float, default=20.0, help="part c: the window that decides")
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    a.parts = a.parts.split(",")
    ctx = engine.Context(0)
    if "a" in a.parts:
        kernels(a, ctx)
    if "b" in a.parts:
        replay(a, ctx)
    if "c" in a.parts:
        end_to_end(a, ctx)


if __name__ == "__main__":
    main()
