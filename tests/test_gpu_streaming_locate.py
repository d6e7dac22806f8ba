"""The subtitle area found in the selector's own pass, on the MI355X: frame_select.LocatingChangeSelector on the engine against the
numpy callables, SubtitleExtractor with area_params={"streaming_locate": True} in several passes (E1) and in one pass over an OS pipe
(E2) against the several-pass run with that probe (engine cells and counters, staging.Uploader, the engine's recogniser with the
stand-in models), and `python -m vse_amd.extractor - --area auto --streaming-locate` as a fresh child process reading a pipe.  A few
dozen frames of the synthetic clip."""
import os
import subprocess
import sys

import numpy as np
import pytest

from frame_change_ref import NumpyCounter
from frame_masks_ref import NumpyCellsMasks
from test_gpu_one_pass import EngineOcr, pipe_ocr          # noqa: F401  (a fixture)
from test_one_pass import piped

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W, FPS = 360, 640, 12
SCHEDULE = [(None, 3), ("the quick brown fox", 9), ("seven wizards quietly box", 7), (None, 4), ("near frozen lakes", 8), (None, 2)]
LOCATOR = dict(min_seconds=0.5, max_seconds=4.0)           # runs of 6 .. 48 frames at 12 fps
SECONDS, WINDOW = 1.5, 18                                  # the decision falls inside the third batch of 8, and inside the second subtitle


@pytest.fixture(scope="module")
def material(tmp_path_factory):
    """The clip as a YUV4MPEG2 file -> (path, its bytes, the frames a reader decodes from them, truth)."""
    from vse_amd import ingest, synth
    frames, truth = synth.make_clip(SCHEDULE, H, W, seed=6)
    path = str(tmp_path_factory.mktemp("locate") / "clip.y4m")
    ingest.write_y4m(path, [ingest.bgr_to_yuv420(f) for f in frames], FPS)
    src = ingest.Y4mSource(path)
    decoded = list(src.frames())
    src.close()
    with open(path, "rb") as fp:
        data = fp.read()
    return path, data, decoded, truth


def as_tuple(area):
    return None if area is None else (area.ymin, area.ymax, area.xmin, area.xmax)


@pytest.mark.parametrize("edge_thresh", [128, "auto"])
def test_selector_on_the_engine_equals_the_numpy_callables(ctx, material, edge_thresh):
    from vse_amd import frame_select, staging
    _path, _data, decoded, truth = material
    up = staging.Uploader(ctx.tdev, ctx=ctx)
    try:
        for window, uploader in ((WINDOW, None), (100, None), (WINDOW, up)):
            host = frame_select.LocatingChangeSelector(NumpyCounter(), NumpyCellsMasks(), window=window, locator_params=LOCATOR,
                                                       edge_thresh=edge_thresh, batch=8)
            host.run(iter(list(decoded)), None, FPS)
            dev = frame_select.LocatingChangeSelector(frame_select.EngineCounter(ctx), frame_select.EngineCellsMasks(ctx), window=window,
                                                      locator_params=LOCATOR, edge_thresh=edge_thresh, batch=8)
            dev.run(iter(list(decoded)), None, FPS, uploader)
            assert dev.area is not None and as_tuple(dev.area) == as_tuple(host.area) and dev.edge_thresh == host.edge_thresh
            assert dev.scores == host.scores and np.array_equal(dev.totals, host.totals)
            assert dev.frames_scanned == host.frames_scanned == min(window, len(decoded))
            assert dev.intervals == host.intervals and np.array_equal(dev.counts, host.counts)
            assert [(s, e) for s, e, _r in dev.intervals] == [(s, e) for s, e, _t in truth]
            assert dev.area.ymin % 8 == 1 and dev.area.xmin % 64 == 1 and dev.area.xmin > 0          # off the cell grid, and not the clamp
    finally:
        up.close()


def run_extractor(ctx, ocr_pipe, up, source, decoded, key, edge_thresh=128, **area_params):
    from vse_amd import area_locator, extractor, frame_select
    ocr = EngineOcr(ocr_pipe, decoded)
    own = {"streaming_locate": True, "cells_masks_fn": frame_select.EngineCellsMasks(ctx)} if key else {"cells_fn": area_locator.EngineCells(ctx)}
    ex = extractor.SubtitleExtractor(source, ocr, sub_area="auto", mode="auto", drop_score=0.0, batch=8, uploader=up, frame_selector="change",
                                     change_counter=frame_select.EngineCounter(ctx),
                                     change_params=None if edge_thresh == 128 else {"edge_thresh": edge_thresh},
                                     area_params={**own, **LOCATOR, **area_params})
    text = ex.run()
    return ex, (as_tuple(ex.located_area), ex.edge_thresh, ex.intervals, ocr.seen, ex.raw_lines, text)


@pytest.mark.parametrize("edge_thresh", [128, "auto"])
def test_e1_and_e2_on_the_engine(ctx, pipe_ocr, material, edge_thresh):          # noqa: F811
    from vse_amd import ingest, staging
    path, data, decoded, truth = material
    up = staging.Uploader(ctx.tdev, ctx=ctx)
    src = ingest.Y4mSource(path)
    try:
        _ex, want = run_extractor(ctx, pipe_ocr, up, src, decoded, key=False, edge_thresh=edge_thresh, probe=(1, WINDOW))
        assert want[0] is not None and [(s, e) for s, e, _r in want[2]] == [(s, e) for s, e, _t in truth]
        assert want[3] == [(s + e) // 2 for s, e, _t in truth]
        # E1: several passes with the key
        ex, got = run_extractor(ctx, pipe_ocr, up, src, decoded, key=True, edge_thresh=edge_thresh, locate_seconds=SECONDS)
        assert not ex.one_pass and got == want and ex.frames_located == WINDOW
        # E2: one pass over a pipe
        fp, th = piped(data, 1 << 16)
        stream = ingest.Y4mStream(fp)
        ex, got = run_extractor(ctx, pipe_ocr, up, stream, decoded, key=True, edge_thresh=edge_thresh, locate_seconds=SECONDS)
        th.join()
        fp.close()
        assert ex.one_pass and got == want and ex.frames_located == WINDOW
        assert ex.clamped_intervals == 0 and stream.frame_count == len(decoded) and WINDOW <= ex.peak_retained <= len(decoded)
    finally:
        up.close()
        src.close()


def test_command_line_in_a_fresh_process_reading_a_pipe(ctx, material, tmp_path, monkeypatch):
    """`python -m vse_amd.extractor - --area auto --streaming-locate` as a child of its own (this process has the GPU open), the Y4M
    bytes on its standard input: exit status 0 and the SRT of the several-pass run with that probe in this process."""
    from vse_amd import extractor, ingest, shim, staging
    path, _data, _decoded, truth = material
    out = str(tmp_path / "out.srt")
    args = [sys.executable, "-m", "vse_amd.extractor", "-", "--allow-standin-weights", "--area", "auto", "--selector", "change", "--batch", "8",
            "-o", out]
    with open(path, "rb") as fp:
        r = subprocess.run(args + ["--streaming-locate", "--locate-seconds", str(SECONDS)], cwd=ROOT, stdin=fp, capture_output=True,
                           text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    child = open(out).read()
    for name, value in (("language", "ch"), ("mode", "fast"), ("allow_standin_weights", True), ("weights_dir", None)):
        monkeypatch.setattr(shim.config, name, value)
    src = ingest.Y4mSource(path)
    up = staging.default_uploader()
    try:
        ex = extractor.SubtitleExtractor(src, shim.OcrRecogniser(), sub_area="auto", mode="fast", batch=8, uploader=up, frame_selector="change",
                                         area_params={"probe": (1, WINDOW)})
        here = ex.run()
    finally:
        up.close()
        src.close()
    assert ex.located_area is not None and [(s, e) for s, e, _r in ex.intervals] == [(s, e) for s, e, _t in truth]
    # (the stand-in recogniser's confidences lie below the default drop_score: the SRTs may both be empty, as in tests/test_gpu_one_pass.py)
    assert child.count(" --> ") == here.count(" --> ") and child == here
