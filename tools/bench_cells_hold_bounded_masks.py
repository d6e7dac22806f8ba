#!/usr/bin/env python3
"""Cost of the subtitle area found in the pass of the hold selector with BOUNDED runs (vse_frame_cells_hold_bounded_masks,
vse_frame_masks_replay_hold_bounded, frame_select.LocatingBoundedHoldSelector), one JSON line per figure.
tools/bench_cells_hold_masks.py for the bounded entries.  Each part runs in a child process of its own under a time limit of its own
(`--limit`), one after the other; the first that fails or runs out of time ends the tool with its exit status.

    a   one vse_frame_cells_hold_bounded_masks over 64 whole frames of 1080p at nt = 1 (threshold 128) and nt = 8 (thresholds 24 32 48 64
        96 128 160 192), hold 8, max_hold 300, against (1) vse_frame_cells_hold_bounded at the same, the kernel it extends, which keeps no
        masks, and (2) the two-call sequence vse_frame_cells_masks + vse_frame_cells_hold_bounded, which leaves the same buffer and totals
        without new kernel code.  Two pictures: `text` (synth.make_frames) and `noise` (random bytes).  Totals, state and the kept words
        are first held equal to the existing entries'.  After a warm-up, blocks of `calls` calls of each alternate between device events,
        `rounds` times; the medians are reported as ms per call, and their ratios.  The masks kernel writes nt bits per 24 bits it reads:
        +4 % bytes at one threshold, +33 % at eight.
    b   vse_frame_masks_replay_hold_bounded of a window of `--window` slots (1440: a minute at 24 fps) on a band-sized rectangle, rows
        810:1080 of the frame, at nt = 1 and nt = 8, hold 8, max_hold 300, against vse_frame_hold_bounded over the same frames' band in
        calls of 64 (the rows are first held equal): ms per call of each.
    c   end to end on tools/bench_one_pass.py's clip (synthetic 1080p at 24 fps held as YUV 4:2:0 in host memory, staged upload, mobile
        models, the hold selector at 128 with max_hold 300): one pass with the key (locate_seconds = `--locate-seconds`) against the plain
        one-pass run with the located box typed in, and several passes with the key against several passes with the bounded locator's own
        pass over the same window (probe); `--runs` timed runs each after one warm-up run, with `peak_retained`.

No decoder runs here (the frames are in host memory, so a saved pass saves an upload and a conversion, not a decode), and whether a
minute of a real film finds its band, or 12.5 s is the right bound, is not measured by this tool.

usage: python tools/bench_cells_hold_bounded_masks.py [--parts a,b,c] [--limit 420] [--calls 20] [--rounds 5] [--window 1440]
                                                      [--frames 9216] [--hold 24] [--locate-seconds 20] [--runs 5]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

HOLD, MAX_HOLD = 8, 300   # the selectors' hold at 24 fps (0.3 s), and 12.5 s
H, W = 1080, 1920
BAND = (810, H, 0, W)


def kernels(a, ctx):
    import torch
    from bench_cells_masks import BATCH, T8, pictures, timed
    from vse_amd import area_locator
    region = (0, H, 0, W)
    params = area_locator.AreaLocator(edge_thresh="auto", automaton="hold", max_hold_frames=MAX_HOLD).params(24.0)
    for name, frames in pictures(ctx).items():
        for ths in ((128,), T8):
            nt = len(ths)
            kept_state, plain_state = (ctx.frame_cells_hold_bounded_state(H, W, nt, MAX_HOLD) for _ in range(2))
            multi_state = ctx.frame_cells_multi_state(H, W, nt)
            masks, change_masks = ctx.frame_masks_buffer(H, W, nt, BATCH), ctx.frame_masks_buffer(H, W, nt, BATCH)
            totals = ctx.frame_cells_hold_bounded_masks(frames, region, ths, HOLD, MAX_HOLD, params, kept_state, masks, 0, 0, flush=True)
            want = ctx.frame_cells_hold_bounded(frames, region, ths, HOLD, MAX_HOLD, params, plain_state, 0, flush=True)
            ctx.frame_cells_masks(frames, region, ths, params, multi_state, change_masks, 0, reset=True, flush=True)
            assert torch.equal(totals, want) and torch.equal(kept_state.words, plain_state.words), (name, nt)
            assert torch.equal(masks.words, change_masks.words), (name, nt)

            def fused():
                ctx.frame_cells_hold_bounded_masks(frames, region, ths, HOLD, MAX_HOLD, params, kept_state, masks, 0, 0, flush=True)

            def plain():
                ctx.frame_cells_hold_bounded(frames, region, ths, HOLD, MAX_HOLD, params, plain_state, 0, flush=True)

            def two_calls():
                ctx.frame_cells_masks(frames, region, ths, params, multi_state, change_masks, 0, reset=True, flush=True)
                ctx.frame_cells_hold_bounded(frames, region, ths, HOLD, MAX_HOLD, params, plain_state, 0, flush=True)
            fns = {"bounded_masks": fused, "bounded": plain, "masks_then_bounded": two_calls}
            for _ in range(2):
                for fn in fns.values():
                    timed(fn, a.calls)
            times = {n: [] for n in fns}
            for _ in range(a.rounds):
                for n, fn in fns.items():
                    times[n].append(timed(fn, a.calls))
            ms = {n: statistics.median(v) for n, v in times.items()}
            read, written = BATCH * H * W * 3, masks.words.numel()
            print(json.dumps({"what": "cells_hold_bounded_masks", "picture": name, "nt": nt, "hold": HOLD, "max_hold": MAX_HOLD,
                              "frames": BATCH, "region": [H, W],
                              **{f"{n}_ms": round(v, 4) for n, v in ms.items()},
                              **{f"{n}_ms_min": round(min(v), 4) for n, v in times.items()},
                              "ratio_to_bounded": round(ms["bounded_masks"] / ms["bounded"], 3),
                              "ratio_to_two_calls": round(ms["bounded_masks"] / ms["masks_then_bounded"], 3),
                              "bytes_ratio": round((read + written) / read, 3)}), flush=True)
            del masks, change_masks, kept_state, plain_state


def replay(a, ctx):
    import torch
    from bench_cells_masks import BATCH, T8, pictures, timed
    from vse_amd import area_locator
    region = (0, H, 0, W)
    params = area_locator.AreaLocator(edge_thresh="auto", automaton="hold", max_hold_frames=MAX_HOLD).params(24.0)
    frames = pictures(ctx)["text"]
    band = frames[:, BAND[0]:BAND[1]]
    area = (0, BAND[1] - BAND[0], 0, W)
    for ths in ((128,), T8):
        nt = len(ths)
        state = ctx.frame_cells_hold_bounded_state(H, W, nt, MAX_HOLD)
        masks = ctx.frame_masks_buffer(H, W, nt, a.window)
        for slot0 in range(0, a.window, BATCH):
            n = min(BATCH, a.window - slot0)
            ctx.frame_cells_hold_bounded_masks(frames[:n], region, ths, HOLD, MAX_HOLD, params, state, masks, slot0, slot0)
        out, direct = (ctx.frame_hold_bounded_state(area[1], W, MAX_HOLD) for _ in range(2))

        def call():
            return ctx.frame_masks_replay_hold_bounded(masks, nt - 1, 0, a.window, BAND, HOLD, MAX_HOLD, out, 0, flush=True)

        def frames_call():
            rows, fed = [], 0
            while fed < a.window:
                n = min(BATCH, a.window - fed)
                rows.append(ctx.frame_hold_bounded(band[:n], area, ths[-1], HOLD, MAX_HOLD, direct, fed, flush=fed + n == a.window))
                fed += n
            return torch.cat(rows)
        assert torch.equal(call(), frames_call()), nt
        for _ in range(2):
            timed(call, a.calls), timed(frames_call, max(1, a.calls // 4))
        ms = [timed(call, a.calls) for _ in range(a.rounds)]
        ms_frames = [timed(frames_call, max(1, a.calls // 4)) for _ in range(a.rounds)]
        touched = a.window * (BAND[1] - BAND[0] - 2) * ((W - 2 + 63) // 64) * 8
        print(json.dumps({"what": "masks_replay_hold_bounded", "nt": nt, "hold": HOLD, "max_hold": MAX_HOLD, "slots": a.window,
                          "rect": list(BAND), "buffer_bytes": masks.words.numel(), "ms": round(statistics.median(ms), 4),
                          "ms_min": round(min(ms), 4), "frame_hold_bounded_ms": round(statistics.median(ms_frames), 4),
                          "frame_hold_bounded_ms_min": round(min(ms_frames), 4),
                          "gb_per_s_words_of_the_rectangle": round(touched / statistics.median(ms) / 1e6, 1)}), flush=True)
        del masks


def end_to_end(a, ctx):
    import numpy as np
    import torch
    from bench_cells_masks import BATCH
    from bench_one_pass import Yuv420ArraySource, schedule
    from vse_amd import area_locator, extractor, frame_select, ingest, modelzoo, pipeline, shim, staging, synth
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
    bound = {"max_hold_frames": MAX_HOLD}
    key = {"streaming_locate_bounded": True, "locate_seconds": a.locate_seconds, **bound}
    rows = {"multi_locator_pass": dict(sub_area="auto", area_params={"cells_fn": area_locator.EngineCells(ctx), "automaton": "hold",
                                                                     "probe": (1, window), **bound}),
            "multi_locate_key": dict(sub_area="auto", area_params=key),
            "onepass_locate_key": dict(sub_area="auto", one_pass=True, area_params=key),
            "onepass_box_typed_in": dict(one_pass=True)}
    located = [None]

    def run(kw):
        src = Counting(clip, fps)
        if kw.get("area_params", {}).get("streaming_locate_bounded"):
            kw = {**kw, "area_params": {**kw["area_params"], "cells_bounded_masks_fn": frame_select.EngineCellsHoldBoundedMasks(ctx)}}
        if "sub_area" not in kw:
            kw = {**kw, "sub_area": located[0]}
        ex = extractor.SubtitleExtractor(src, Ocr(), mode="fast", frame_selector="hold", change_counter=frame_select.EngineBoundedHoldCounter(ctx),
                                         change_params=dict(bound), uploader=up, drop_score=0.0, batch=BATCH, **kw)
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
                print(json.dumps({"what": "end_to_end", "row": name, "run": k, "frames": a.frames, "hold": a.hold, "max_hold": MAX_HOLD,
                                  "window": window, "area": None if area is None else [area.ymin, area.ymax, area.xmin, area.xmax],
                                  "intervals": None if ex.intervals is None else len(ex.intervals), "seconds": round(dt, 3),
                                  "frames_per_s": round(a.frames / dt, 1), "one_pass": ex.one_pass, "decodes": src.decodes,
                                  "peak_retained": ex.peak_retained, "clamped_intervals": ex.clamped_intervals,
                                  "srt_blocks": text.count(" --> ")}), flush=True)
    finally:
        up.close()


PARTS = {"a": kernels, "b": replay, "c": end_to_end}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--part", default=None, choices=sorted(PARTS), help="run this part alone, in this process (what the tool starts per part)")
    ap.add_argument("--limit", type=float, default=420.0, help="seconds a part may take; it is ended behind them")
    ap.add_argument("--calls", type=int, default=20, help="calls per timed block")
    ap.add_argument("--rounds", type=int, default=5, help="timed blocks per figure; the median is reported")
    ap.add_argument("--window", type=int, default=1440, help="part b: slots replayed")
    ap.add_argument("--frames", type=int, default=9216)
    ap.add_argument("--hold", type=int, default=24, help="part c: frames one subtitle stays on screen")
    ap.add_argument("--locate-seconds", type=float, default=20.0, help="part c: the window that decides")
    ap.add_argument("--runs", type=int, default=5)
    a = ap.parse_args()
    if a.part is not None:
        from vse_amd import engine
        PARTS[a.part](a, engine.Context(0))
        return 0
    passed = sys.argv[1:]
    for part in a.parts.split(","):
        # a fresh child per part, so that a part that faults or hangs ends there and nothing is started behind it
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--part", part] + passed, timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print(json.dumps({"what": "time_limit", "part": part, "seconds": a.limit}), flush=True)
            return 124
        if rc != 0:
            print(json.dumps({"what": "failed", "part": part, "exit": rc}), flush=True)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
