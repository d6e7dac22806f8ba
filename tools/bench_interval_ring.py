#!/usr/bin/env python3
"""Cost of the streaming quantile (vse_interval_ring_rank, frame_select.StreamingQuantile), one JSON line per figure, in one process.

    a   one vse_interval_ring_rank with 1 and with 8 groups at K = 5 / 15 / 31 / 63 samples against its yardstick, vse_interval_rank on
        the same samples laid out contiguously (one call per group), on the 1080p default subtitle band of
        tools/bench_interval_quantile.py (rows 842:1069, columns 96:1824).  The ring is the one `--ring-seconds` at `--fps` makes
        (60 s at 24 fps: 1511 slots), filled completely; a group samples an interval of `--interval` frames as fuse_samples does, the
        groups lie spread over the ring (how many of them lie across its wrap is reported).  After a warm-up of both, blocks of `calls`
        calls of the one and of the other alternate between device events, `rounds` times; the medians are reported as ms per call
        and their ratio.
    b   the ring store of one batch of 64 such bands (vse_interval_stream without segments, store_from = fed + 1), `fed` advancing so
        that the slots move through the ring: ms per batch and GB/s over the area's pixels (each read once and written once).
    c   end to end on tools/bench_one_pass.py's clip (synthetic 1080p at 24 fps held as YUV 4:2:0 in host memory, area rows 810:1080,
        staged upload, mobile models, the change selector): one pass with the streaming quantile, one pass with
        interval_image="middle", the several-pass quantile run, and several passes with the streaming quantile; `--runs` timed runs
        each after one warm-up run.

Also printed: the state's size at `--ring-seconds` for 24 and 60 fps.  No decoder runs here, and what the pictures gain in recognition
on real footage is not measured by this tool.

usage: python tools/bench_interval_ring.py [--parts a,b,c] [--calls 100] [--rounds 11] [--samples 5,15,31,63] [--ring-seconds 60]
                                           [--fps 24] [--interval 120] [--frames 9216] [--hold 24] [--runs 3]"""
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
from vse_amd import engine, frame_select  # noqa: E402

BATCH = 64


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def kernels(a, ctx):
    h, w = 1080, 1920
    y0, y1, x0, x1 = int(0.78 * h), int(0.99 * h), int(0.05 * w), int(0.95 * w)
    ah, aw = y1 - y0, x1 - x0
    area = (0, ah, x0, x1)                                # in a band of the area's rows alone
    cap = int(round(a.ring_seconds * a.fps)) + int(round(0.25 * a.fps)) + BATCH + 1
    for fps in (24, 60):
        c = int(round(a.ring_seconds * fps)) + int(round(0.25 * fps)) + BATCH + 1
        print(json.dumps({"what": "state", "ring_seconds": a.ring_seconds, "fps": fps, "cap": c, "area": [ah, aw],
                          "state_mb": round(ctx.lib.vse_interval_stream_state_bytes(ah, aw, c) / 1e6, 1)}), flush=True)
    gen = torch.Generator(device=ctx.tdev)
    gen.manual_seed(1)
    band = torch.randint(0, 256, (BATCH, ah, w, 3), dtype=torch.uint8, device=ctx.tdev, generator=gen)
    state = ctx.interval_stream_state(ah, aw, cap)
    fed = 0
    while fed < cap + BATCH:                              # frame f is band[(f - 1) % 64]; every slot is written
        ctx.interval_stream(band, area, state, cap, fed, [], fed + 1, "min")
        fed += BATCH
    if "b" in a.parts:
        at = [fed]

        def store():
            ctx.interval_stream(band, area, state, cap, at[0], [], at[0] + 1, "min")
            at[0] += BATCH
        for _ in range(3):
            timed(store, a.calls)
        ms = [timed(store, a.calls) for _ in range(a.rounds)]
        fed = at[0]
        med = statistics.median(ms)
        print(json.dumps({"what": "ring_store", "frames": BATCH, "cap": cap, "ms": round(med, 4), "ms_min": round(min(ms), 4),
                          "gb_per_s_area_pixels": round(BATCH * ah * aw * 3 / med / 1e6, 1)}), flush=True)
    if "a" not in a.parts:
        return
    oldest = fed - cap + 1
    out_ring = torch.empty((8, ah, aw, 3), dtype=torch.uint8, device=ctx.tdev)
    out_flat = torch.empty((ah, aw, 3), dtype=torch.uint8, device=ctx.tdev)
    for k in [int(v) for v in a.samples.split(",")]:
        length = max(a.interval, k)
        assert 8 * length <= cap, "the ring is too short for 8 disjoint intervals of this length"
        starts = [oldest + g * ((cap - length) // 7) for g in range(8)]
        starts[-1] = fed - length + 1                     # the last one ends at `fed`
        groups, stacks = [], []
        for s in starts:
            nos, _pos = frame_select.fuse_samples(s, s + length - 1, s, a.fps, k, 0.0)
            groups.append((nos, k // 2))
            stacks.append(band[[(f - 1) % BATCH for f in nos]].contiguous())
        wraps = sum(1 for nos, _r in groups if nos[0] % cap > nos[-1] % cap)
        for g, (nos, r) in enumerate(groups):             # the two give the same bytes
            ctx.interval_ring_rank(state, ah, aw, cap, fed, [(nos, r)], out=out_ring[:1])
            ctx.interval_rank(stacks[g], area, r, out=out_flat)
            assert torch.equal(out_ring[0], out_flat), (k, g)
        for ng in (1, 8):
            part = groups[-ng:]

            def ring():
                ctx.interval_ring_rank(state, ah, aw, cap, fed, part, out=out_ring)

            def flat():
                for g in range(8 - ng, 8):
                    ctx.interval_rank(stacks[g], area, k // 2, out=out_flat)
            for _ in range(3):
                timed(ring, a.calls), timed(flat, a.calls)
            times = {"ring": [], "flat": []}
            for _ in range(a.rounds):
                times["ring"].append(timed(ring, a.calls))
                times["flat"].append(timed(flat, a.calls))
            ms = {n: statistics.median(v) for n, v in times.items()}
            print(json.dumps({"what": "ring_rank", "samples": k, "groups": ng, "interval": length, "cap": cap, "groups_across_the_wrap": wraps,
                              "ring_ms": round(ms["ring"], 4), "ring_ms_min": round(min(times["ring"]), 4),
                              "rank_ms": round(ms["flat"], 4), "rank_ms_min": round(min(times["flat"]), 4),
                              "ratio": round(ms["ring"] / ms["flat"], 3)}), flush=True)


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

    area = extractor.SubtitleArea(ymin=int(0.75 * h), ymax=h, xmin=0, xmax=w)
    up = staging.Uploader(ctx.tdev)
    rows = {"onepass_streaming_quantile": dict(one_pass=True, interval_image="quantile",
                                               composite_params={"streaming": True, "ring_seconds": a.ring_seconds}),
            "onepass_middle": dict(one_pass=True),
            "multi_quantile": dict(interval_image="quantile"),
            "multi_streaming_quantile": dict(interval_image="quantile", composite_params={"streaming": True, "ring_seconds": a.ring_seconds})}

    def run(kw):
        ex = extractor.SubtitleExtractor(Yuv420ArraySource(clip, fps), Ocr(), sub_area=area, mode="fast", frame_selector="change",
                                         change_counter=frame_select.EngineCounter(ctx), uploader=up, drop_score=0.0, batch=BATCH, **kw)
        torch.cuda.synchronize()
        t0 = time.time()
        text = ex.run()
        torch.cuda.synchronize()
        return time.time() - t0, ex, text
    try:
        for name, kw in rows.items():
            run(kw)
            for k in range(a.runs):
                dt, ex, text = run(kw)
                print(json.dumps({"what": "end_to_end", "row": name, "run": k, "frames": a.frames, "hold": a.hold, "intervals": len(ex.intervals),
                                  "seconds": round(dt, 3), "frames_per_s": round(a.frames / dt, 1), "one_pass": ex.one_pass,
                                  "clamped_quantiles": ex.clamped_quantiles, "srt_blocks": text.count(" --> ")}), flush=True)
    finally:
        up.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="a,b,c")
    ap.add_argument("--calls", type=int, default=100, help="calls per timed block")
    ap.add_argument("--rounds", type=int, default=11, help="timed blocks per figure; the median is reported")
    ap.add_argument("--samples", default="5,15,31,63")
    ap.add_argument("--ring-seconds", type=float, default=60.0)
    ap.add_argument("--fps", type=float, default=24.0)
    ap.add_argument("--interval", type=int, default=120, help="frames of the intervals sampled in part a")
    ap.add_argument("--frames", type=int, default=9216)
    ap.add_argument("--hold", type=int, default=24, help="part c: frames one subtitle stays on screen")
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    a.parts = a.parts.split(",")
    ctx = engine.Context(0)
    if "a" in a.parts or "b" in a.parts:
        kernels(a, ctx)
    if "c" in a.parts:
        end_to_end(a, ctx)


if __name__ == "__main__":
    main()
