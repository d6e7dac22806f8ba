"""The subtitle area found in the selector's own pass, on the host: frame_select.LocatingChangeSelector against AreaLocator's pass over
the window followed by ChangeFrameSelector on what it found, a clip whose located area lies off the cell grid by the one pixel the kept
masks exist for, how many frames the selector reads before it decides, SubtitleExtractor with area_params={"streaming_locate": True} in
several passes (E1) and in one pass over a pipe (E2) against the several-pass run with that probe, a clip without subtitles, every
refusal, and the command line.  CPU only: the numpy cells, masks and counters (tests/edge_calibrate_ref.py, tests/frame_masks_ref.py,
tests/frame_change_ref.py) and a scripted recogniser."""
import logging
from types import SimpleNamespace

import numpy as np
import pytest

import frame_change_ref as FC
import frame_masks_ref as FM
from area_clip import FPS, H, LOCATOR, W, as_tuple, decorated_clip
from edge_calibrate_ref import NumpyCellsMulti
from frame_change_ref import NumpyCounter
from frame_masks_ref import NumpyCellsMasks
from test_one_pass import LookupOcr, piped
from vse_amd import area_locator, extractor, frame_select, ingest, synth

BATCH = 8
KEY = "area_params={'streaming_locate': True}"
TEXT_BOX = [[240, 330], [400, 330], [400, 346], [240, 346]]      # inside the text rows of area_clip's clip
SHOWN = [(7, 20), (21, 32), (38, 53), (54, 62)]                  # area_clip.SCHEDULE: when a subtitle is shown
FOUR = dict(LOCATOR, thresholds=(48, 96, 128, 192))              # the selector's tests choose among four thresholds: half the numpy work


@pytest.fixture(scope="module")
def clip():
    frames, truth = decorated_clip()
    frames.setflags(write=False)
    return frames, truth


@pytest.fixture
def host_stack(monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)          # the scripted recogniser takes the list of host frames


# ---- the numpy restatement itself ------------------------------------------------------------------------------------------------------
def test_the_numpy_replay_is_frame_change_on_the_rectangle():
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, size=(5, 23, 150, 3), dtype=np.uint8)
    region, ths = (1, 22, 3, 149), (40, 90)
    words = FM.mask_words(frames, region, ths)
    assert words.shape == (5, 2) + FM.dims(21, 146) + (8,) and words.dtype == np.uint64
    for rect in ((0, 21, 0, 146), (1, 12, 1, 68), (9, 21, 63, 146), (2, 5, 64, 67)):
        area = (region[0] + rect[0], region[0] + rect[1], region[2] + rect[2], region[2] + rect[3])
        for q, th in enumerate(ths):
            want, last = FC.counts(frames, area, th)
            got, mask, state = FM.replay(words, 21, 146, q, 0, 5, rect)
            assert np.array_equal(got, want) and np.array_equal(mask, last) and np.array_equal(state, FM.pack_rows(last).reshape(-1))
            head, _m, _s = FM.replay(words, 21, 146, q, 0, 2, rect)
            tail, mask, _s = FM.replay(words, 21, 146, q, 2, 5, rect, reset=False)
            assert np.array_equal(np.concatenate([head, tail]), want) and np.array_equal(mask, last)


# ---- the selector ----------------------------------------------------------------------------------------------------------------------
_two_passes = {}


def two_passes(name, frames, window, edge_thresh):
    """AreaLocator over the first `window` frames, then the plain selector on its area at its threshold -> (locator, selector | None)."""
    key = (name, window, edge_thresh)
    if key not in _two_passes:
        loc = area_locator.AreaLocator(NumpyCellsMulti(), edge_thresh=edge_thresh, probe=(1, window), batch=BATCH, **FOUR)
        area = loc.run(list(frames), FPS)
        sel = None
        if area is not None:
            sel = frame_select.ChangeFrameSelector(NumpyCounter(), edge_thresh=loc.edge_thresh, batch=BATCH)
            sel.run(list(frames), area, FPS)
        _two_passes[key] = (loc, sel)
    return _two_passes[key]


def compare(sel, loc, plain):
    assert sel.decided and as_tuple(sel.area) == as_tuple(loc.area) and sel.edge_thresh == loc.edge_thresh
    assert sel.scores == loc.scores and sel.frames_scanned == loc.frames_scanned
    assert sel.totals.shape == loc.totals.shape and np.array_equal(sel.totals, loc.totals)
    if plain is not None:
        assert sel.intervals == plain.intervals and np.array_equal(sel.counts, plain.counts)


@pytest.mark.parametrize("batch", [1, 7, 64])
@pytest.mark.parametrize("window", [100, 45, 27])            # beyond the clip; inside the third subtitle; inside the second, and no multiple of 7
@pytest.mark.parametrize("edge_thresh", [128, "auto"])
def test_selector_equals_the_locator_pass_and_the_plain_selector(clip, edge_thresh, window, batch):
    frames, truth = clip
    assert window >= len(frames) or any(s < window < e for s, e in SHOWN)
    loc, plain = two_passes("decorated", frames, window, edge_thresh)
    cells, counter = NumpyCellsMasks(), NumpyCounter()
    sel = frame_select.LocatingChangeSelector(counter, cells, window=window, locator_params=FOUR, edge_thresh=edge_thresh, batch=batch)
    seen, yielded, decided_at = 0, [], min(window, len(frames))
    for items, closed in sel.iter_run(iter(list(frames)), None, FPS):
        seen += len(items)
        if seen < decided_at or (window > len(frames) and items):
            assert closed == [] and sel.tracker is None and not sel.decided and sel.area is None
        yielded += closed
    compare(sel, loc, plain)
    assert loc.area is not None and sel.frames_scanned == decided_at == cells.frames and seen == len(frames)
    assert sel.intervals == yielded and len(sel.intervals) == len(truth)
    assert cells.replayed == [(0 if edge_thresh == 128 else loc.thresholds.index(loc.edge_thresh), as_tuple(loc.area))]
    # the plain counter ran on the frames behind the window only, and never with reset
    assert counter.calls == -(-(len(frames) - decided_at) // batch)
    # the offsets the kept masks exist for: the located area's interior starts one row and one column off the cell grid
    assert sel.area.ymin % 8 == 1 and sel.area.xmin % 64 == 1


def test_a_short_line_away_from_the_left_edge_is_located_off_the_cell_grid():
    frames, truth = synth.make_clip([(None, 6), ("fox", 14), (None, 5), ("owl", 12), (None, 4)], H, W, seed=3)
    loc, plain = two_passes("short", frames, 100, 128)
    sel = frame_select.LocatingChangeSelector(NumpyCounter(), NumpyCellsMasks(), window=100, locator_params=FOUR, batch=BATCH)
    sel.run(iter(list(frames)), None, FPS)
    compare(sel, loc, plain)
    # not the clamp to 0: the rectangle starts inside the picture, one pixel behind a cell boundary both ways, and ends inside it too
    assert sel.area.xmin % 64 == 1 and sel.area.ymin % 8 == 1 and sel.area.xmin > 64 and sel.area.ymin > 8
    assert sel.area.xmax < W and [(s, e) for s, e, _r in sel.intervals] == [(s, e) for s, e, _t in truth]


class StubUploader:
    """What staging.prefetch asks of an uploader, on the host: the batches are staged by its producer thread."""

    def bind_thread(self):
        pass

    def stage(self, frames):
        data = np.stack([np.asarray(f) for f in frames])
        return SimpleNamespace(tensor=lambda: data)


@pytest.mark.parametrize("uploader", [None, "stub"])
@pytest.mark.parametrize("kind", ["text", "bare"])
def test_exactly_the_window_is_read_before_the_decision(clip, kind, uploader):
    frames = clip[0] if kind == "text" else synth.make_clip([(None, 40)], H, W, seed=3)[0]
    read = [0]

    def counting():
        for f in frames:
            read[0] += 1
            yield f
    window = 27
    sel = frame_select.LocatingChangeSelector(NumpyCounter(), NumpyCellsMasks(), window=window, locator_params=LOCATOR, batch=7)
    at_decision = None
    for _items, _closed in sel.iter_run(counting(), None, FPS, StubUploader() if uploader else None):
        assert read[0] <= window or sel.decided
        if sel.decided and at_decision is None:
            at_decision = read[0]
    assert sel.decided and at_decision == window
    if kind == "bare":
        assert sel.area is None and read[0] == window and sel.intervals == [] and sel.tracker is None
    else:
        assert sel.area is not None and read[0] == len(frames)


def test_selector_arguments():
    with pytest.raises(ValueError, match="window"):
        frame_select.LocatingChangeSelector(NumpyCounter(), NumpyCellsMasks())
    with pytest.raises(ValueError, match="window"):
        frame_select.LocatingChangeSelector(NumpyCounter(), NumpyCellsMasks(), window=0)
    for params, word in (({"automaton": "hold"}, "automaton='hold'"), ({"max_hold_seconds": 3}, "max_hold_seconds"),
                         ({"max_hold_frames": 30}, "max_hold_frames"), ({"search_area": (0, 8, 0, 8)}, "search_area"),
                         ({"probe": (1, 5)}, "probe")):
        with pytest.raises(ValueError, match="does not take") as e:
            frame_select.LocatingChangeSelector(NumpyCounter(), NumpyCellsMasks(), window=5, locator_params=params)
        assert word in str(e.value)
    sel = frame_select.LocatingChangeSelector(NumpyCounter(), NumpyCellsMasks(), window=5)
    with pytest.raises(ValueError, match="takes none"):
        sel.run([], (0, 8, 0, 8), FPS)
    assert sel.run([], None, FPS) == [] and sel.area is None and not sel.decided


# ---- the extractor ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def y4m(clip, tmp_path_factory):
    """The clip as a YUV4MPEG2 file -> (its path, its bytes, the frames a reader decodes from them)."""
    path = str(tmp_path_factory.mktemp("locate") / "clip.y4m")
    ingest.write_y4m(path, [ingest.bgr_to_yuv420(f) for f in clip[0]], FPS)
    src = ingest.Y4mSource(path)
    decoded = list(src.frames())
    src.close()
    with open(path, "rb") as fp:
        return path, fp.read(), decoded


def make(source, decoded, truth, key, edge_thresh=128, one_pass=None, **area_params):
    ocr = LookupOcr(decoded, truth, TEXT_BOX)
    own = {"streaming_locate": True, "cells_masks_fn": NumpyCellsMasks()} if key else {"cells_fn": NumpyCellsMulti()}
    ex = extractor.SubtitleExtractor(source, ocr, sub_area="auto", mode="fast", frame_selector="change", change_counter=NumpyCounter(),
                                     drop_score=0.0, batch=BATCH, one_pass=one_pass,
                                     change_params=None if edge_thresh == 128 else {"edge_thresh": edge_thresh},
                                     area_params={**own, **LOCATOR, **area_params})
    return ex, ocr


def results(ex, ocr):
    text = ex.run()
    return as_tuple(ex.located_area), ex.edge_thresh, ex.intervals, ocr.seen, ex.raw_lines, text


@pytest.mark.parametrize("edge_thresh,window", [(128, 27), (128, 100), ("auto", 45)])
def test_e1_e2_equal_several_passes_with_that_probe(host_stack, clip, y4m, edge_thresh, window):
    path, data, decoded = y4m
    truth = clip[1]
    src = ingest.Y4mSource(path)
    want = results(*make(src, decoded, truth, key=False, edge_thresh=edge_thresh, probe=(1, window)))
    assert want[0] is not None and len(want[2]) == len(truth) and want[5].count(" --> ") == len(truth)
    # E1: several passes with the key
    ex, ocr = make(src, decoded, truth, key=True, edge_thresh=edge_thresh, locate_seconds=window / FPS)
    assert not ex.one_pass and results(ex, ocr) == want and ex.frames_located == min(window, len(decoded))
    src.close()
    # E2: one pass over a pipe
    pipe, th = piped(data, 65536)
    stream = ingest.Y4mStream(pipe)
    ex, ocr = make(stream, decoded, truth, key=True, edge_thresh=edge_thresh, locate_seconds=window / FPS)
    got = results(ex, ocr)
    th.join()
    pipe.close()
    assert ex.one_pass and stream.frame_count == len(decoded) and got == want
    assert ex.clamped_intervals == 0 and ex.peak_retained >= min(window, len(decoded)) and ex.frames_located == min(window, len(decoded))
    # a seekable source forced into one pass takes the same road
    ex, ocr = make(extractor.ArraySource(list(decoded), FPS), decoded, truth, key=True, edge_thresh=edge_thresh, one_pass=True,
                   locate_seconds=window / FPS)
    assert results(ex, ocr)[:5] == want[:5]                      # (the SRT's times: an array source has no timestamps of its own)


def test_several_passes_without_locate_seconds_decide_on_the_whole_clip(host_stack, clip):
    frames, truth = clip

    class CountingSource(extractor.ArraySource):
        passes = 0

        def frames(self):
            self.passes += 1
            return super().frames()
    src = CountingSource(list(frames), FPS)
    want = results(*make(src, frames, truth, key=False))
    passes_without = src.passes
    src = CountingSource(list(frames), FPS)
    ex, ocr = make(src, frames, truth, key=True)
    assert results(ex, ocr) == want and ex.frames_located == len(frames)
    assert src.passes == passes_without - 1 == 1                 # the locator's pass is folded into the selector's


@pytest.mark.parametrize("one_pass", [None, True])
def test_no_area_found_warns_and_goes_on_as_the_run_without_one(host_stack, one_pass, caplog):
    frames, truth = synth.make_clip([(None, 40)], H, W, seed=3)
    want_ex, ocr = make(extractor.ArraySource(list(frames), FPS), frames, truth, key=False, probe=(1, 20))
    want = results(want_ex, ocr)
    assert want[0] is None and want[2] is None and len(want[3]) > 0
    caplog.clear()
    ex, ocr = make(extractor.ArraySource(list(frames), FPS), frames, truth, key=True, one_pass=one_pass, locate_seconds=2.0)
    with caplog.at_level(logging.WARNING):
        got = results(ex, ocr)
    assert got == want and ex.sub_area is None and ex.frames_located == 20
    warned = [r for r in caplog.records if "no subtitle area found in 20 frames" in r.getMessage()]
    assert len(warned) == 1
    if one_pass:
        assert ex.peak_retained >= 20


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def build(one_pass=None, area_params=None, **kw):
    frames = np.zeros((4, 16, 16, 3), np.uint8)
    args = dict(sub_area="auto", frame_selector="change", one_pass=one_pass, area_params={"streaming_locate": True, **(area_params or {})})
    args.update(kw)
    return extractor.SubtitleExtractor(extractor.ArraySource(list(frames), FPS), LookupOcr([], [], None), **args)


@pytest.mark.parametrize("names,kw", [
    (["frame_selector='hold'"], dict(frame_selector="hold")),
    (["automaton='hold'"], dict(area_params={"automaton": "hold"})),
    (["max_hold_seconds"], dict(area_params={"automaton": "change", "max_hold_seconds": 12})),
    (["max_hold_frames"], dict(area_params={"max_hold_frames": 100})),
    (["search_area"], dict(area_params={"search_area": extractor.SubtitleArea(0, 8, 0, 8)})),
    (["probe"], dict(area_params={"probe": (1, 20)})),
    (["area_params={'streaming': True}"], dict(area_params={"streaming": True}, change_params={"edge_thresh": "auto"})),
    (["interval_frame='sharpest'"], dict(interval_frame="sharpest")),
    (["composite_params={'streaming': True}"], dict(interval_image="min", composite_params={"streaming": True})),
    (["shard=(0, 2)"], dict(shard=(0, 2))),
    (["mode='accurate'"], dict(mode="accurate")),
    (["sub_area=SubtitleArea", "sub_area='auto'"], dict(sub_area=extractor.SubtitleArea(300, H, 0, W))),
    (["sub_area=None"], dict(sub_area=None)),
])
def test_the_key_refuses_what_needs_the_area_from_the_first_frame(names, kw):
    with pytest.raises(ValueError) as e:
        build(**kw)
    assert KEY in str(e.value) and "does not combine with" in str(e.value) and all(n in str(e.value) for n in names)


def test_the_keys_parameters_mean_nothing_alone_and_one_pass_needs_the_window():
    for own in ("locate_seconds", "mask_gib", "cells_masks_fn", "replay_fn"):
        with pytest.raises(ValueError, match=rf"area_params: \['{own}'\] belong to area_params=\{{'streaming_locate': True\}} and mean nothing without it"):
            build(area_params={"streaming_locate": False, own: 3.0})
    with pytest.raises(ValueError, match="locate_seconds must be positive"):
        build(area_params={"locate_seconds": 0})
    with pytest.raises(ValueError, match="mask_gib must be positive"):
        build(area_params={"mask_gib": 0})
    with pytest.raises(ValueError, match="in one pass needs locate_seconds"):
        build(one_pass=True)
    build(one_pass=True, area_params={"locate_seconds": 5})                          # accepted
    build(one_pass=True, area_params={"locate_seconds": 5}, change_params={"edge_thresh": "auto"})       # "auto" is decided in the same pass
    build()                                                                          # several passes: the whole clip decides


def test_the_window_must_fit_what_keeps_it(host_stack, clip):
    frames, truth = clip
    per = frames[0].nbytes
    ex, ocr = make(extractor.ArraySource(list(frames), FPS), frames, truth, key=True, one_pass=True, locate_seconds=3.0)
    ex.retain_bytes = 30 * per - 1
    with pytest.raises(ValueError) as e:
        ex.run()
    msg = str(e.value)
    assert KEY in msg and f"{30 * per} bytes" in msg and f"retain_bytes={30 * per - 1}" in msg and "shorter locate_seconds" in msg
    assert "--retain-gib" in msg and ocr.seen == []
    ex.retain_bytes = 30 * per                                                       # exactly enough
    ex.run()
    assert ex.located_area is not None and ex.clamped_intervals == 0
    gy, gx = area_locator.cells_dims(H, W)
    need = 30 * gy * gx * 64
    for one_pass in (None, True):
        ex, ocr = make(extractor.ArraySource(list(frames), FPS), frames, truth, key=True, one_pass=one_pass, locate_seconds=3.0,
                       mask_gib=(need - 1) / (1 << 30))
        with pytest.raises(ValueError) as e:
            ex.run()
        msg = str(e.value)
        assert KEY in msg and f"{need} bytes" in msg and "mask_gib" in msg and "shorter locate_seconds" in msg and "--mask-gib" in msg
        assert ocr.seen == []
    ex, ocr = make(extractor.ArraySource(list(frames), FPS), frames, truth, key=True, edge_thresh="auto", locate_seconds=3.0,
                   mask_gib=(8 * need - 1) / (1 << 30))
    with pytest.raises(ValueError, match="8 thresholds"):
        ex.run()


def test_without_the_key_the_old_refusals_stay_word_for_word():
    frames = np.zeros((4, 16, 16, 3), np.uint8)
    src = extractor.ArraySource(list(frames), FPS)
    for area_params in (None, {}, {"streaming_locate": False}, {"min_seconds": 0.5}):
        with pytest.raises(ValueError, match=r"sub_area='auto' is not available in one pass \(a sequential source, or one_pass=True\): "
                                             "it needs a second look at frames already gone"):
            extractor.SubtitleExtractor(src, LookupOcr([], [], None), sub_area="auto", frame_selector="change", one_pass=True,
                                        area_params=area_params)
    with pytest.raises(ValueError, match=r"area_params=\{'streaming': True\} .* does not combine with sub_area='auto'"):
        extractor.SubtitleExtractor(src, LookupOcr([], [], None), sub_area="auto", frame_selector="change",
                                    change_params={"edge_thresh": "auto"}, area_params={"streaming": True})


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def test_command_line(host_stack, clip, y4m, monkeypatch, capsys, caplog):
    path, data, decoded = y4m
    truth = clip[1]
    common = ["--area", "auto", "--selector", "change", "--batch", str(BATCH)]

    def main(args, stdin=True):
        pipe, th = piped(data if stdin else b"", 4099)
        monkeypatch.setattr("sys.stdin", type("Stdin", (), {"buffer": pipe})())
        ocr = LookupOcr(decoded, truth, TEXT_BOX)
        rc = extractor.main(args, ocr=ocr, counter=NumpyCounter(), cells_fn=NumpyCellsMulti(), cells_masks_fn=NumpyCellsMasks())
        pipe.close()
        th.join()
        return rc, ocr, capsys.readouterr()
    src = ingest.Y4mSource(path)
    want = results(*make(src, decoded, truth, key=False, probe=(1, 27)))[5]
    src.close()
    rc, ocr, out = main(["-"] + common + ["--streaming-locate", "--locate-seconds", "2.7"])
    assert rc == 0 and out.out == want and want.count(" --> ") == len(truth) and len(ocr.seen) == len(truth)
    rc, _ocr, several = main([path] + common, stdin=False)                            # the locator's own pass, then the selector's
    assert rc == 0 and several.out.count(" --> ") == len(truth)
    with caplog.at_level(logging.INFO, logger="vse_amd.extractor"):
        rc, _ocr, out = main(["-"] + common + ["--streaming-locate"])                 # a pipe: what fits, at most 300 s, beyond this clip
    assert rc == 0 and out.out == several.out
    assert [r.getMessage() for r in caplog.records if "--streaming-locate" in r.getMessage()] == [
        "--streaming-locate: the area is found on the first 300 seconds (what fits --retain-gib 4 and --mask-gib 8, at most 300)"]
    rc, _ocr, out = main([path] + common + ["--streaming-locate"], stdin=False)       # a file: the whole clip
    assert rc == 0 and out.out == several.out
    rc, _ocr, out = main(["-"] + common + ["--streaming-locate", "--edge-thresh", "auto", "--locate-seconds", "10"])
    assert rc == 0 and out.out.count(" --> ") == len(truth)
    for bad, word in ((["-"] + common, "sub_area='auto' is not available in one pass"),
                      (["-"] + common + ["--locate-seconds", "3"], "--locate-seconds"),
                      (["-"] + common + ["--mask-gib", "3"], "--mask-gib"),
                      (["-"] + common + ["--streaming-locate", "--locate-seconds", "0"], "locate_seconds"),
                      (["-"] + common + ["--streaming-locate", "--locate-seconds", "6", "--mask-gib", "0.001"], "mask_gib"),
                      (["-"] + common + ["--streaming-locate", "--locate-seconds", "6", "--retain-gib", "0.001"], "--retain-gib"),
                      (["-"] + common + ["--streaming-locate", "--retain-gib", "0.0001"], "not one second"),
                      (["-", "--area", "auto", "--selector", "hold", "--streaming-locate"], "frame_selector='hold'"),
                      (["-", "--area", "300,360,0,640", "--selector", "change", "--streaming-locate"], "sub_area=")):
        rc, ocr, out = main(bad)
        assert rc == 2 and out.err.startswith("extractor: ") and word in out.err and ocr.seen == [], bad
    with pytest.raises(SystemExit):
        extractor.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--streaming-locate" in text and "--locate-seconds" in text and "--mask-gib" in text
    assert "a policy, not a measurement: nobody has tried whether a minute of a real film finds its band" in text


def test_the_default_window_of_a_pipe_is_what_fits():
    film = SimpleNamespace(height=1080, width=1920, fps=24.0, fmt=None)
    assert extractor.default_locate_seconds(film, True, False, 4 << 30, 8.0) == 57.0          # 4 GiB of 4:2:0 frames
    assert extractor.default_locate_seconds(film, False, False, 4 << 30, 8.0) == 28.0         # ... of BGR frames
    assert extractor.default_locate_seconds(film, True, True, 64 << 30, 8.0) == 172.0         # 4142 frames of masks at eight thresholds
    assert extractor.default_locate_seconds(film, True, False, 64 << 30, 8.0) == 300.0        # the cap
    assert 33140 == (8 << 30) // (135 * 30 * 64) and 4142 == (8 << 30) // (8 * 135 * 30 * 64)
    with pytest.raises(ValueError, match="not one second"):
        extractor.default_locate_seconds(film, True, False, 1 << 20, 8.0)
