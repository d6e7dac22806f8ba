#!/usr/bin/env python3
"""Whole-clip throughput of the callers' row: extractor.SubtitleExtractor.run() (frame selection -> batched OCR -> raw.txt
filters -> SRT) on a synthetic 1080p clip held in HOST memory (so the PCIe upload of every frame is inside the timed
region), real-weight detector (V3_ch_det_fast) + stand-in en recogniser, fully data-driven boxes.

usage: python tools/bench_extract.py [--frames 1024] [--batch 64] [--hold 12] [--source bgr|i420]
--source i420 holds the same clip as unconverted YUV 4:2:0 planes (ingest.Yuv420Frame, 1.5 bytes per pixel): the staged rows then
pack and upload half the bytes and convert on the device (vse_yuv420_to_bgr); both sources time upload + OCR, not a disk.
Prints one JSON line per mode: fps sampler looking at every frame, batched and frame by frame (the reference's order of
work), and the accurate mode (detector loop over every frame + OCR of the selected ones).  First, fast mode with an area both
ways: the fps sampler at the default extract_frequency (what that run fell back to) and the subtitle-change selector
(frame_selector="change", VideoSubFinder's role); `ocr_frames` is the number of frames each run sent to OCR."""
import argparse
import json
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from vse_amd import engine, extractor, frame_select, ingest, modelzoo, pipeline, shim, staging, synth


class Yuv420ArraySource:
    """extractor.ArraySource over ingest.Yuv420Frames held in host memory: read_raw / raw_frames hand out the planes (the staged
    routes), read / frames the host conversion (every other route)."""

    def __init__(self, raw, fps):
        self._raw = raw
        self.frame_count = len(raw)
        self.fps = float(fps)

    def read_raw(self, frame_no):
        return self._raw[frame_no - 1] if 1 <= frame_no <= self.frame_count else None

    def read(self, frame_no):
        raw = self.read_raw(frame_no)
        return None if raw is None else raw.to_bgr()

    def raw_frames(self):
        return iter(self._raw)

    def frames(self):
        return (f.to_bgr() for f in self._raw)

    pos_msec = None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--hold", type=int, default=12, help="frames one subtitle stays on screen")
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--single", type=int, default=96, help="frames of the frame-by-frame run (slow)")
    ap.add_argument("--workers", type=int, default=4, help="copy threads of the pinned-slab uploader")
    ap.add_argument("--staged-only", action="store_true")
    ap.add_argument("--source", choices=("bgr", "i420"), default="bgr", help="what the host holds: BGR frames or YUV 4:2:0 planes")
    ap.add_argument("--change-only", action="store_true", help="only the two fast-mode-with-area rows (fps sampler / change selector)")
    a = ap.parse_args()
    ctx = engine.Context(0)
    det = modelzoo.get_model("V3_ch_det_fast", seed=0)
    rec = modelzoo.get_model("V4_en_rec_fast", seed=1)
    pipe = pipeline.OcrPipeline(ctx, det, rec, shim.en_charset(), rec_mode="bucketed")
    n_sub = (a.frames + 2 * a.hold - 1) // (2 * a.hold)
    lit = synth.make_frames(min(n_sub, 48), a.height, a.width, seed=9)
    dark = np.full((a.height, a.width, 3), 40, np.uint8)
    if a.source == "i420":
        def raw(frame):
            return ingest.Yuv420Frame(ingest.bgr_to_yuv420(frame), a.height, a.width, "i420")
        lit, dark = [raw(f) for f in lit], raw(dark)
    make_source = extractor.ArraySource if a.source == "bgr" else Yuv420ArraySource
    clip = []
    for k in range(n_sub):                                  # subtitle k for `hold` frames, then `hold` dark frames
        clip += [lit[k % len(lit)]] * a.hold + [dark] * a.hold
    clip = clip[:a.frames]
    fps = 24.0

    class Ocr:
        frames = 0                                    # frames sent to OCR

        def predict(self, frame):
            self.frames += 1
            b, r = pipe.ocr(torch.from_numpy(np.ascontiguousarray(frame)).to(ctx.tdev)[None])[0]
            return shim.OcrRecogniser.arrange(b, r)

    class OcrBatched(Ocr):
        def predict_batch(self, frames):
            self.frames += len(frames)
            return [shim.OcrRecogniser.arrange(b, r) for b, r in pipe.ocr(frames)]

    def detect_stream(batches):
        for dets in pipe.detect_stream(batches):
            yield [np.asarray(b, np.float32).reshape(-1, 4, 2) for b in dets]

    class OcrStreamed(OcrBatched):
        def predict_with_dets(self, frames, dets):
            return [shim.OcrRecogniser.arrange(b, r) for b, r in pipe.ocr_from_det(frames, dets)]

        def predict_stream(self, batches):
            def counted():
                for x in batches:
                    self.frames += x.shape[0]
                    yield x
            for out in pipe.ocr_stream(counted()):
                yield [shim.OcrRecogniser.arrange(b, r) for b, r in out]

    def detect(frames):
        dev = frames if torch.is_tensor(frames) else torch.from_numpy(np.stack(frames)).to(ctx.tdev)
        return [np.asarray(b, np.float32).reshape(-1, 4, 2) for b in pipe.detect(dev)]

    area = extractor.SubtitleArea(ymin=int(0.75 * a.height), ymax=a.height, xmin=0, xmax=a.width)
    up = staging.Uploader(ctx.tdev, workers=a.workers)
    runs = [
        ("fast mode + area: fps sampler at extract_frequency 3, staged upload + streamed detector", clip, OcrStreamed(),
         dict(sub_area=area, mode="fast", extract_frequency=3, uploader=up)),
        ("fast mode + area: subtitle-change selector, staged upload + streamed detector", clip, OcrStreamed(),
         dict(sub_area=area, mode="fast", frame_selector="change", change_counter=frame_select.EngineCounter(ctx), uploader=up)),
        ("fps sampler, every frame, staged upload + streamed detector", clip, OcrStreamed(),
         dict(sub_area=None, mode="fast", extract_frequency=fps, uploader=up)),
        ("fps sampler, every frame, batched, staged upload", clip, OcrBatched(),
         dict(sub_area=None, mode="fast", extract_frequency=fps, uploader=up)),
        ("accurate mode, staged upload + streamed detector, boxes reused", clip, OcrStreamed(),
         dict(sub_area=area, mode="accurate", uploader=up, detect_stream=detect_stream)),
        ("accurate mode, batched, staged upload", clip, OcrBatched(), dict(sub_area=area, mode="accurate", uploader=up)),
        ("fps sampler, every frame, batched", clip, OcrBatched(), dict(sub_area=None, mode="fast", extract_frequency=fps)),
        ("fps sampler, every frame, frame by frame", clip[:a.single], Ocr(), dict(sub_area=None, mode="fast", extract_frequency=fps)),
        ("accurate mode, batched", clip, OcrBatched(), dict(sub_area=area, mode="accurate")),
    ]
    if a.change_only:
        runs = runs[:2]
    elif a.staged_only:
        runs = runs[:6]
    for name, frames, ocr, kw in runs:
        src = make_source(frames, fps)
        ex = extractor.SubtitleExtractor(src, ocr, detect_batch=detect, drop_score=0.0, batch=a.batch, **kw)
        ex_warm = extractor.SubtitleExtractor(make_source(frames[:5 * a.batch], fps), ocr, detect_batch=detect,
                                              drop_score=0.0, batch=a.batch, **kw)
        ex_warm.run()
        torch.cuda.synchronize()
        ocr.frames = 0
        t0 = time.time()
        text = ex.run()
        torch.cuda.synchronize()
        dt = time.time() - t0
        print(json.dumps({"mode": name, "frames": len(frames), "seconds": round(dt, 3), "frames_per_s": round(len(frames) / dt, 1),
                          "ocr_frames": ocr.frames, "raw_lines": len(ex.raw_lines), "srt_blocks": text.count(" --> "),
                          "source": a.source, "frame_mb": round(a.height * a.width * (3 if a.source == "bgr" else 1.5) / 1e6, 2)}), flush=True)


if __name__ == "__main__":
    main()
