"""The subtitle area found in the pass of the hold selector with bounded runs, on the MI355X:
frame_select.LocatingBoundedHoldSelector on the engine (vse_frame_cells_hold_bounded_masks, vse_frame_masks_replay_hold_bounded,
vse_frame_hold_bounded) against the numpy callables, and SubtitleExtractor with area_params={"streaming_locate_bounded": True} in several
passes and in one pass over an OS pipe against the several-pass run with area_params={"automaton": "hold", "max_hold_frames": 30, "probe":
(1, window)} (engine cells and counters, staging.Uploader, the engine's recogniser with the stand-in models).  The clips are
tests/test_area_locator_hold_bounded.py's, 90 frames of 120 x 320 whose busy background stands still; window 70 lies beyond the kernels'
chunk of 64 frames and beyond max_hold."""
import numpy as np
import pytest

from frame_hold_bounded_ref import NumpyBoundedHoldCounter
from frame_masks_hold_bounded_ref import NumpyCellsHoldBoundedMasks
from test_area_locator_hold_bounded import FPS, STATIC, TRUE, as_tuple, contains_text, static_clip
from test_gpu_one_pass import EngineOcr, pipe_ocr          # noqa: F401  (a fixture)
from test_one_pass import piped

pytestmark = pytest.mark.gpu

BOUNDS = {"hold_frames": 3, "max_hold_frames": 30}
WINDOW = 70


@pytest.fixture(scope="module", params=sorted(STATIC))
def material(request, tmp_path_factory):
    """A clip as a YUV4MPEG2 file -> (path, its bytes, the frames a reader decodes from them, truth)."""
    from vse_amd import ingest
    frames, truth = static_clip(request.param)
    path = str(tmp_path_factory.mktemp("locate_bounded") / f"{request.param}.y4m")
    ingest.write_y4m(path, [ingest.bgr_to_yuv420(f) for f in frames], FPS)
    src = ingest.Y4mSource(path)
    decoded = list(src.frames())
    src.close()
    with open(path, "rb") as fp:
        data = fp.read()
    return path, data, decoded, truth


@pytest.mark.parametrize("edge_thresh,window,staged", [(64, 20, False), (64, WINDOW, True), ("auto", WINDOW, False), (64, 200, False)])
def test_selector_on_the_engine_equals_the_numpy_callables(ctx, material, edge_thresh, window, staged):
    from vse_amd import frame_select, staging
    _path, _data, decoded, _truth = material
    up = staging.Uploader(ctx.tdev, ctx=ctx) if staged else None
    try:
        host = frame_select.LocatingBoundedHoldSelector(NumpyBoundedHoldCounter(), NumpyCellsHoldBoundedMasks(), window=window,
                                                        edge_thresh=edge_thresh, batch=8, locator_params=dict(BOUNDS), **BOUNDS)
        host.run(iter(list(decoded)), None, FPS)
        dev = frame_select.LocatingBoundedHoldSelector(frame_select.EngineBoundedHoldCounter(ctx), frame_select.EngineCellsHoldBoundedMasks(ctx),
                                                       window=window, edge_thresh=edge_thresh, batch=8, locator_params=dict(BOUNDS), **BOUNDS)
        dev.run(iter(list(decoded)), None, FPS, up)
        assert as_tuple(dev.area) == as_tuple(host.area) and dev.edge_thresh == host.edge_thresh
        assert dev.scores == host.scores and np.array_equal(dev.totals, host.totals)
        assert dev.frames_scanned == host.frames_scanned == min(window, len(decoded))
        assert dev.intervals == host.intervals and np.array_equal(dev.counts, host.counts)
        if window >= WINDOW:
            assert contains_text(dev.area) and set(TRUE) <= {(s, e) for s, e, _r in dev.intervals}
            assert dev.area.ymin % 8 == 1 or dev.area.xmin % 64 == 1       # off the cell grid: what the kept words exist for
    finally:
        if up is not None:
            up.close()


def run_extractor(ctx, ocr_pipe, up, source, decoded, key, **area_params):
    from vse_amd import area_locator, extractor, frame_select
    ocr = EngineOcr(ocr_pipe, decoded)
    own = ({"streaming_locate_bounded": True, "cells_bounded_masks_fn": frame_select.EngineCellsHoldBoundedMasks(ctx)} if key else
           {"cells_fn": area_locator.EngineCells(ctx), "automaton": "hold"})
    ex = extractor.SubtitleExtractor(source, ocr, sub_area="auto", mode="auto", drop_score=0.0, batch=8, uploader=up, frame_selector="hold",
                                     change_counter=frame_select.EngineBoundedHoldCounter(ctx),
                                     change_params={**BOUNDS, "edge_thresh": "auto"},
                                     area_params={**own, "max_hold_frames": BOUNDS["max_hold_frames"], **area_params})
    text = ex.run()
    return ex, (as_tuple(ex.located_area), ex.edge_thresh, ex.intervals, ocr.seen, ex.raw_lines, text)


def test_the_keys_runs_on_the_engine_equal_several_passes_with_that_probe(ctx, pipe_ocr, material):          # noqa: F811
    from vse_amd import ingest, staging
    path, data, decoded, _truth = material
    up = staging.Uploader(ctx.tdev, ctx=ctx)
    src = ingest.Y4mSource(path)
    try:
        _ex, want = run_extractor(ctx, pipe_ocr, up, src, decoded, key=False, probe=(1, WINDOW))
        assert want[0] is not None and set(TRUE) <= {(s, e) for s, e, _r in want[2]} and want[3] == [r for _s, _e, r in want[2]]
        # several passes with the key
        ex, got = run_extractor(ctx, pipe_ocr, up, src, decoded, key=True, locate_seconds=WINDOW / FPS)
        assert not ex.one_pass and got == want and ex.frames_located == WINDOW
        # one pass over a pipe
        fp, th = piped(data, 1 << 16)
        stream = ingest.Y4mStream(fp)
        ex, got = run_extractor(ctx, pipe_ocr, up, stream, decoded, key=True, locate_seconds=WINDOW / FPS)
        th.join()
        fp.close()
        assert ex.one_pass and got == want and ex.frames_located == WINDOW
        assert ex.clamped_intervals == 0 and stream.frame_count == len(decoded) and WINDOW <= ex.peak_retained <= len(decoded)
    finally:
        up.close()
        src.close()
