"""The subtitle area found in the hold selector's own pass, on the MI355X: frame_select.LocatingHoldSelector on the engine
(vse_frame_cells_hold_masks, vse_frame_masks_replay_hold, vse_frame_hold) against the numpy callables, and SubtitleExtractor with
area_params={"streaming_locate_hold": True} in several passes and in one pass over an OS pipe against the several-pass run with
area_params={"automaton": "hold", "probe": (1, window)} (engine cells and counters, staging.Uploader, the engine's recogniser with the
stand-in models).  The clip is tests/test_area_locator_hold.py's, 95 frames of 120 x 320 whose textured background moves; window 40
falls inside the second subtitle, window 70 lies beyond the kernels' chunk of 64 frames."""
import numpy as np
import pytest

from frame_hold_ref import NumpyHoldCounter
from frame_masks_hold_ref import NumpyCellsHoldMasks
from test_area_locator_hold import FPS, as_tuple, busy_clip
from test_gpu_one_pass import EngineOcr, pipe_ocr          # noqa: F401  (a fixture)
from test_one_pass import piped

pytestmark = pytest.mark.gpu

WINDOWS = (40, 70)


@pytest.fixture(scope="module")
def material(tmp_path_factory):
    """The clip as a YUV4MPEG2 file -> (path, its bytes, the frames a reader decodes from them, truth)."""
    from vse_amd import ingest
    frames, truth = busy_clip()
    path = str(tmp_path_factory.mktemp("locate_hold") / "clip.y4m")
    ingest.write_y4m(path, [ingest.bgr_to_yuv420(f) for f in frames], FPS)
    src = ingest.Y4mSource(path)
    decoded = list(src.frames())
    src.close()
    with open(path, "rb") as fp:
        data = fp.read()
    return path, data, decoded, truth


@pytest.mark.parametrize("edge_thresh,window,staged", [(128, 40, False), (128, 70, True), ("auto", 70, False), (128, 200, False)])
def test_selector_on_the_engine_equals_the_numpy_callables(ctx, material, edge_thresh, window, staged):
    from vse_amd import frame_select, staging
    _path, _data, decoded, _truth = material
    up = staging.Uploader(ctx.tdev, ctx=ctx) if staged else None
    try:
        host = frame_select.LocatingHoldSelector(NumpyHoldCounter(), NumpyCellsHoldMasks(), window=window, edge_thresh=edge_thresh, batch=8)
        host.run(iter(list(decoded)), None, FPS)
        dev = frame_select.LocatingHoldSelector(frame_select.EngineHoldCounter(ctx), frame_select.EngineCellsHoldMasks(ctx), window=window,
                                                edge_thresh=edge_thresh, batch=8)
        dev.run(iter(list(decoded)), None, FPS, up)
        assert dev.area is not None and as_tuple(dev.area) == as_tuple(host.area) and dev.edge_thresh == host.edge_thresh
        assert dev.scores == host.scores and np.array_equal(dev.totals, host.totals)
        assert dev.frames_scanned == host.frames_scanned == min(window, len(decoded))
        assert dev.intervals == host.intervals and np.array_equal(dev.counts, host.counts) and len(dev.intervals) >= 2
        assert dev.area.ymin % 8 == 1 and dev.area.xmin % 64 == 1          # off the cell grid: what the kept words exist for
    finally:
        if up is not None:
            up.close()


def run_extractor(ctx, ocr_pipe, up, source, decoded, key, edge_thresh=128, **area_params):
    from vse_amd import area_locator, extractor, frame_select
    ocr = EngineOcr(ocr_pipe, decoded)
    own = ({"streaming_locate_hold": True, "cells_hold_masks_fn": frame_select.EngineCellsHoldMasks(ctx)} if key else
           {"cells_fn": area_locator.EngineCells(ctx), "automaton": "hold"})
    ex = extractor.SubtitleExtractor(source, ocr, sub_area="auto", mode="auto", drop_score=0.0, batch=8, uploader=up, frame_selector="hold",
                                     change_counter=frame_select.EngineHoldCounter(ctx),
                                     change_params=None if edge_thresh == 128 else {"edge_thresh": edge_thresh},
                                     area_params={**own, **area_params})
    text = ex.run()
    return ex, (as_tuple(ex.located_area), ex.edge_thresh, ex.intervals, ocr.seen, ex.raw_lines, text)


@pytest.mark.parametrize("edge_thresh,window", [(128, 40), ("auto", 70)])
def test_the_keys_runs_on_the_engine_equal_several_passes_with_that_probe(ctx, pipe_ocr, material, edge_thresh, window):          # noqa: F811
    from vse_amd import ingest, staging
    path, data, decoded, truth = material
    up = staging.Uploader(ctx.tdev, ctx=ctx)
    src = ingest.Y4mSource(path)
    try:
        _ex, want = run_extractor(ctx, pipe_ocr, up, src, decoded, key=False, edge_thresh=edge_thresh, probe=(1, window))
        assert want[0] is not None and len(want[2]) >= 2 and want[3] == [r for _s, _e, r in want[2]]
        if edge_thresh == 128:
            assert [(s, e) for s, e, _r in want[2]] == [(s, e) for s, e, _t in truth]
        # several passes with the key
        ex, got = run_extractor(ctx, pipe_ocr, up, src, decoded, key=True, edge_thresh=edge_thresh, locate_seconds=window / FPS)
        assert not ex.one_pass and got == want and ex.frames_located == window
        # one pass over a pipe
        fp, th = piped(data, 1 << 16)
        stream = ingest.Y4mStream(fp)
        ex, got = run_extractor(ctx, pipe_ocr, up, stream, decoded, key=True, edge_thresh=edge_thresh, locate_seconds=window / FPS)
        th.join()
        fp.close()
        assert ex.one_pass and got == want and ex.frames_located == window
        assert ex.clamped_intervals == 0 and stream.frame_count == len(decoded) and window <= ex.peak_retained <= len(decoded)
    finally:
        up.close()
        src.close()
