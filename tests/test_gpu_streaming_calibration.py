"""The edge threshold chosen in the selector's own pass, on the MI355X: frame_select.CalibratingChangeSelector on the engine against
the numpy callables, SubtitleExtractor with area_params={"streaming": True} in several passes (E1) and in one pass over an OS pipe (E2)
against the several-pass run without the key (engine cells and counters, staging.Uploader, the engine's recogniser with the stand-in
models), and `python -m vse_amd.extractor - --streaming-calibration` as a fresh child process reading a pipe.  A few dozen frames of
the synthetic clip at little contrast, where the constant 128 finds nothing."""
import os
import subprocess
import sys

import numpy as np
import pytest

from edge_calibrate_ref import low_contrast
from frame_change_ref import NumpyCounter
from test_gpu_one_pass import EngineOcr, pipe_ocr          # noqa: F401  (a fixture)
from test_one_pass import piped
from test_streaming_calibration import NumpyCellsCounts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, FPS = 360, 640, 12
SCHEDULE = [(None, 3), ("the quick brown fox", 9), ("seven wizards quietly box", 7), (None, 4), ("near frozen lakes", 8), (None, 2)]
LOCATOR = dict(min_seconds=0.5, max_seconds=4.0)           # runs of 6 .. 48 frames at 12 fps
SECONDS, WINDOW = 1.5, 18                                  # the decision falls inside the third batch of 8


@pytest.fixture(scope="module")
def material(tmp_path_factory):
    """The clip as a YUV4MPEG2 file -> (path, its bytes, the frames a reader decodes from them, truth, the subtitle area)."""
    from vse_amd import extractor, ingest, synth
    frames, truth = synth.make_clip(SCHEDULE, H, W, seed=6)
    path = str(tmp_path_factory.mktemp("calib") / "low.y4m")
    ingest.write_y4m(path, [ingest.bgr_to_yuv420(f) for f in low_contrast(frames)], FPS)
    src = ingest.Y4mSource(path)
    decoded = list(src.frames())
    src.close()
    with open(path, "rb") as fp:
        data = fp.read()
    return path, data, decoded, truth, extractor.SubtitleArea(ymin=int(0.75 * H), ymax=H, xmin=0, xmax=W)


def test_selector_on_the_engine_equals_the_numpy_callables(ctx, material):
    from vse_amd import frame_select
    _path, _data, decoded, truth, area = material
    assert frame_select.ChangeFrameSelector(frame_select.EngineCounter(ctx), batch=8).run(list(decoded), area, FPS) == []      # 128: nothing
    for window in (WINDOW, None):
        host = frame_select.CalibratingChangeSelector(NumpyCounter(), NumpyCellsCounts(), window=window, locator_params=LOCATOR, batch=8)
        host.run(list(decoded), area, FPS)
        dev = frame_select.CalibratingChangeSelector(frame_select.EngineCounter(ctx), frame_select.EngineCellsCounts(ctx), window=window,
                                                     locator_params=LOCATOR, batch=8)
        dev.run(list(decoded), area, FPS)
        assert dev.edge_thresh == host.edge_thresh and dev.edge_thresh < 128 and dev.scores == host.scores
        assert np.array_equal(dev.totals, host.totals) and dev.frames_scanned == host.frames_scanned == (window or len(decoded))
        assert dev.intervals == host.intervals and np.array_equal(dev.counts, host.counts)
        assert [(s, e) for s, e, _r in dev.intervals] == [(s, e) for s, e, _t in truth]


def run_extractor(ctx, ocr_pipe, up, source, decoded, area, key, **area_params):
    from vse_amd import area_locator, extractor, frame_select
    ocr = EngineOcr(ocr_pipe, decoded)
    own = {"streaming": True, "cells_counts_fn": frame_select.EngineCellsCounts(ctx)} if key else {"cells_fn": area_locator.EngineCells(ctx)}
    ex = extractor.SubtitleExtractor(source, ocr, sub_area=area, mode="auto", drop_score=0.0, batch=8, uploader=up, frame_selector="change",
                                     change_counter=frame_select.EngineCounter(ctx), change_params={"edge_thresh": "auto"},
                                     area_params={**own, **LOCATOR, **area_params})
    text = ex.run()
    return ex, (ex.edge_thresh, ex.intervals, ocr.seen, ex.raw_lines, text)


def test_e1_and_e2_on_the_engine(ctx, pipe_ocr, material):          # noqa: F811
    from vse_amd import ingest, staging
    path, data, decoded, truth, area = material
    up = staging.Uploader(ctx.tdev, ctx=ctx)
    src = ingest.Y4mSource(path)
    try:
        # E1: several passes, the whole clip decides
        _ex, want = run_extractor(ctx, pipe_ocr, up, src, decoded, area, key=False)
        ex, got = run_extractor(ctx, pipe_ocr, up, src, decoded, area, key=True)
        assert not ex.one_pass and got == want and got[0] < 128 and ex.frames_calibrated == len(decoded)
        assert [(s, e) for s, e, _r in got[1]] == [(s, e) for s, e, _t in truth] and got[2] == [(s + e) // 2 for s, e, _t in truth]
        assert got[4].count(" --> ") >= 1
        # E2: one pass over a pipe, the first WINDOW frames decide
        _ex, want = run_extractor(ctx, pipe_ocr, up, src, decoded, area, key=False, probe=(1, WINDOW))
        fp, th = piped(data, 1 << 16)
        stream = ingest.Y4mStream(fp)
        ex, got = run_extractor(ctx, pipe_ocr, up, stream, decoded, area, key=True, calibrate_seconds=SECONDS)
        th.join()
        fp.close()
        assert ex.one_pass and got == want and got[0] < 128 and ex.frames_calibrated == WINDOW
        assert ex.clamped_intervals == 0 and stream.frame_count == len(decoded) and 0 < ex.peak_retained <= len(decoded)
        assert [(s, e) for s, e, _r in got[1]] == [(s, e) for s, e, _t in truth]
    finally:
        up.close()
        src.close()


def test_command_line_in_a_fresh_process_reading_a_pipe(ctx, material, tmp_path, monkeypatch):
    """`python -m vse_amd.extractor - --edge-thresh auto --streaming-calibration` as a child of its own (this process has the GPU open),
    the Y4M bytes on its standard input: exit status 0 and the SRT of the several-pass run with that probe in this process."""
    from vse_amd import extractor, ingest, shim, staging
    path, _data, _decoded, truth, area = material
    out = str(tmp_path / "out.srt")
    args = [sys.executable, "-m", "vse_amd.extractor", "-", "--allow-standin-weights", "--area", f"{area.ymin},{area.ymax},{area.xmin},{area.xmax}",
            "--selector", "change", "--batch", "8", "--edge-thresh", "auto", "-o", out]
    with open(path, "rb") as fp:
        r = subprocess.run(args + ["--streaming-calibration", "--calibrate-seconds", str(SECONDS)], cwd=ROOT, stdin=fp, capture_output=True,
                           text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    child = open(out).read()
    for name, value in (("language", "ch"), ("mode", "fast"), ("allow_standin_weights", True), ("weights_dir", None)):
        monkeypatch.setattr(shim.config, name, value)
    src = ingest.Y4mSource(path)
    up = staging.default_uploader()
    try:
        ex = extractor.SubtitleExtractor(src, shim.OcrRecogniser(), sub_area=area, mode="fast", batch=8, uploader=up, frame_selector="change",
                                         change_params={"edge_thresh": "auto"}, area_params={"probe": (1, WINDOW)})
        here = ex.run()
    finally:
        up.close()
        src.close()
    assert ex.edge_thresh < 128 and [(s, e) for s, e, _r in ex.intervals] == [(s, e) for s, e, _t in truth]
    # (the stand-in recogniser's confidences lie below the default drop_score: the SRTs may both be empty, as in tests/test_gpu_one_pass.py)
    assert child.count(" --> ") == here.count(" --> ") and child == here
