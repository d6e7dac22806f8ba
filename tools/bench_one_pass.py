#!/usr/bin/env python3
"""Cost of one pass (SubtitleExtractor(one_pass=True), ingest.Y4mStream) against the multi-pass run(), one JSON line per timed run.

The clip is EXPERIMENTS.md §Q's: a synthetic 1080p clip at 24 fps, each subtitle of synth.make_frames held for --hold frames with as
many dark frames between, area rows 810:1080, staged upload, mobile models (V3_ch_det_fast with its real weights, a stand-in
V4_ch_rec_fast).  It is held in HOST memory as YUV 4:2:0 planes (ingest.Yuv420Frame, 1.5 bytes per pixel), so every frame's packing,
upload and conversion on the device is inside the timed region.  Rows, each `--runs` timed runs after one warm-up run, all in one job:

    multi     run() over the seekable source (selector pass, then the middle frames read again for OCR)
    onepass   the same source with one_pass=True
    pipe      the same bytes as YUV4MPEG2 through an OS pipe from a child process that only writes them (this file with --writer),
              read by ingest.Y4mStream: what `decoder | python -m vse_amd.extractor -` costs on the reading side

for frame_selector "change" and "hold", and for each of --interval-frames (middle: the default; sharpest: every frame scored by
vse_frame_focus in the selector's pass, the sharpest of each interval recognised).  `peak_retained` is the largest number of frames a one-pass run held at once.  The run-to-run
spread is to be read from the multi rows themselves (the machine's other work shares the host).  No decoder runs here: how a real
`ffmpeg` pipe compares is not measured by this tool.

usage: python tools/bench_one_pass.py [--frames 9216] [--hold 24] [--runs 4] [--selectors change,hold] [--rows multi,onepass,pipe]
                                      [--interval-frames middle]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def schedule(frames, hold, distinct):
    """Index into the distinct pictures (the last one is the dark frame) for every frame of the clip."""
    n_sub = (frames + 2 * hold - 1) // (2 * hold)
    idx = []
    for k in range(n_sub):
        idx += [k % (distinct - 1)] * hold + [distinct - 1] * hold
    return idx[:frames]


def writer(a):
    """The child: the distinct pictures' bytes from a .npy file [k, frame bytes], written as YUV4MPEG2 to standard output."""
    import numpy as np
    blobs = [b"FRAME\n" + row.tobytes() for row in np.load(a.writer)]
    out = sys.stdout.buffer
    out.write(b"YUV4MPEG2 W%d H%d F24:1 Ip A1:1 C420jpeg\n" % (a.width, a.height))
    try:
        for k in schedule(a.frames, a.hold, len(blobs)):
            out.write(blobs[k])
        out.flush()
    except BrokenPipeError:
        pass


class Yuv420ArraySource:
    """extractor.ArraySource over ingest.Yuv420Frames held in host memory."""

    def __init__(self, raw, fps):
        self._raw, self.frame_count, self.fps = raw, len(raw), float(fps)

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
    ap.add_argument("--frames", type=int, default=9216)
    ap.add_argument("--hold", type=int, default=24, help="frames one subtitle stays on screen")
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--selectors", default="change,hold")
    ap.add_argument("--rows", default="multi,onepass,pipe")
    ap.add_argument("--interval-frames", default="middle", help="comma-separated: middle, sharpest")
    ap.add_argument("--rec", default="V4_ch_rec_fast", help="recogniser model id (stand-in weights)")
    ap.add_argument("--writer", default=None, metavar="NPY", help="(the pipe rows' child) write the clip of these pictures to standard output")
    a = ap.parse_args()
    if a.writer:
        return writer(a)
    import tempfile
    import numpy as np
    import torch
    from vse_amd import engine, extractor, frame_select, ingest, modelzoo, pipeline, shim, staging, synth
    ctx = engine.Context(0)
    det = modelzoo.get_model("V3_ch_det_fast", seed=0)
    rec = modelzoo.get_model(a.rec, seed=1)
    charset = shim.en_charset() if a.rec == "V4_en_rec_fast" else shim.standin_charset("ch", shim._ncls(rec[0]))
    pipe = pipeline.OcrPipeline(ctx, det, rec, charset)
    n_sub = (a.frames + 2 * a.hold - 1) // (2 * a.hold)
    lit = synth.make_frames(min(n_sub, 48), a.height, a.width, seed=9)
    pictures = [ingest.bgr_to_yuv420(f) for f in lit] + [ingest.bgr_to_yuv420(np.full((a.height, a.width, 3), 40, np.uint8))]
    order = schedule(a.frames, a.hold, len(pictures))
    raw = [ingest.Yuv420Frame(p, a.height, a.width, "i420") for p in pictures]
    clip = [raw[k] for k in order]
    fps = 24.0

    class Ocr(shim.OcrRecogniser):
        """The shim's recogniser object over this tool's pipeline (no model files needed)."""

        def __init__(self):
            super().__init__()
            self.recogniser = shim.PaddleOCR.__new__(shim.PaddleOCR)
            self.recogniser.pipe = pipe

    area = extractor.SubtitleArea(ymin=int(0.75 * a.height), ymax=a.height, xmin=0, xmax=a.width)
    up = staging.Uploader(ctx.tdev)
    tmp = tempfile.mkdtemp()
    npy = os.path.join(tmp, "pictures.npy")
    np.save(npy, np.stack([np.concatenate([np.ascontiguousarray(p).reshape(-1) for p in tr]) for tr in pictures]))

    def run(row, selector, frames, interval_frame="middle"):
        counter = frame_select.EngineCounter(ctx) if selector == "change" else frame_select.EngineHoldCounter(ctx)
        child = None
        if row == "pipe":
            child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--writer", npy, "--frames", str(frames), "--hold", str(a.hold),
                                      "--height", str(a.height), "--width", str(a.width)], stdout=subprocess.PIPE)
            source = ingest.Y4mStream(child.stdout)
        else:
            source = Yuv420ArraySource(clip[:frames], fps)
        ex = extractor.SubtitleExtractor(source, Ocr(), sub_area=area, mode="fast", frame_selector=selector, change_counter=counter,
                                         uploader=up, drop_score=0.0, batch=a.batch, one_pass=None if row != "onepass" else True,
                                         **({} if interval_frame == "middle" else {"interval_frame": interval_frame}))
        torch.cuda.synchronize()
        t0 = time.time()
        text = ex.run()
        torch.cuda.synchronize()
        dt = time.time() - t0
        if child is not None:
            child.stdout.close()
            child.wait()
        return dt, ex, text

    try:
        for selector in a.selectors.split(","):
            for row, interval_frame in ((r, f) for r in a.rows.split(",") for f in a.interval_frames.split(",")):
                # warm-up: every plan the timed runs use is compiled and its workspace allocated (the pipe rows: on the clip's first batches)
                run(row, selector, a.frames if row != "pipe" else min(a.frames, 5 * a.batch), interval_frame)
                for k in range(a.runs):
                    dt, ex, text = run(row, selector, a.frames, interval_frame)
                    print(json.dumps({"what": "one_pass", "row": row, "selector": selector, "interval_frame": interval_frame, "run": k, "rec": a.rec, "frames": a.frames,
                                      "frame": [a.height, a.width], "intervals": len(ex.intervals), "seconds": round(dt, 3),
                                      "frames_per_s": round(a.frames / dt, 1), "one_pass": ex.one_pass, "peak_retained": ex.peak_retained,
                                      "clamped_intervals": ex.clamped_intervals, "srt_blocks": text.count(" --> ")}), flush=True)
    finally:
        up.close()
        os.remove(npy)
        os.rmdir(tmp)


if __name__ == "__main__":
    main()
