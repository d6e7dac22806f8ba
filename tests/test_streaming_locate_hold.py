"""The subtitle area found in the HOLD selector's own pass, on the host: the numpy restatement of the replay against frame_hold_ref,
frame_select.LocatingHoldSelector against AreaLocator(automaton="hold")'s pass over the window followed by HoldFrameSelector on what it
found, SubtitleExtractor with area_params={"streaming_locate_hold": True} in several passes and in one pass over a pipe against the
several-pass run with that probe, a clip without subtitles, every refusal, and the command line.  The clip is
tests/test_area_locator_hold.py's: a textured background that moves behind the subtitles, on which the change automaton finds neither an
area nor a threshold.  The expectation is equality with the several-pass run, not with the truth: with edge_thresh="auto" both merge the
back-to-back subtitles, as tests/test_area_locator_hold.py describes.  CPU only: the numpy cells, masks and counters
(tests/area_cells_hold_ref.py, tests/frame_masks_hold_ref.py, tests/frame_hold_ref.py) and a scripted recogniser."""
import logging

import numpy as np
import pytest

import frame_masks_hold_ref as FMH
import frame_masks_ref as FM
from area_cells_hold_ref import NumpyCellsHold
from frame_hold_ref import NumpyHoldCounter, counts as hold_counts
from frame_masks_hold_ref import NumpyCellsHoldMasks
from test_area_locator_hold import FPS, HELD_AREA, as_tuple, busy_clip
from test_one_pass import LookupOcr, piped
from vse_amd import area_locator, extractor, frame_select, ingest, synth
from vse_amd.frame_select import LocatingHoldSelector

BATCH = 8
HOLD = 8                  # the selectors' default at 25 fps
KEY = "area_params={'streaming_locate_hold': True}"
TEXT_BOX = [[40, 92], [280, 92], [280, 112], [40, 112]]          # inside the text rows of the 120 x 320 clip
SHOWN = [(8, 27), (28, 45), (52, 76), (77, 90)]                  # test_frame_hold.MOVING: when a subtitle is shown
WINDOWS = (40, 70, 200)   # inside the second subtitle; beyond the 64-frame chunk; the clip (95 frames) ends inside it


def test_the_clip_is_what_the_windows_were_chosen_for():
    frames, truth = busy_clip()
    assert frames.shape == (95, 120, 320, 3) and [(s, e) for s, e, _t in truth] == SHOWN
    assert SHOWN[1][0] < 40 < SHOWN[1][1] and 64 < 70 < len(frames) < 200


# ---- the numpy restatement itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", [1, 3, 8])
def test_the_numpy_replay_is_frame_hold_on_the_rectangle(hold):
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, size=(20, 23, 150, 3), dtype=np.uint8)
    frames[6:17, 4:20, 30:120] = frames[5, 4:20, 30:120]         # a patch that holds still for twelve frames
    region, ths = (1, 22, 3, 149), (40, 90)
    words = FM.mask_words(frames, region, ths)
    for rect in ((0, 21, 0, 146), (1, 12, 1, 68), (9, 21, 63, 146), (2, 5, 64, 67)):
        area = (region[0] + rect[0], region[0] + rect[1], region[2] + rect[2], region[2] + rect[3])
        for q, th in enumerate(ths):
            want = hold_counts(frames, area, th, hold)
            assert rect[3] - rect[2] < 10 or want.min(0).max() > 0           # (every column counts something)
            assert np.array_equal(FMH.replay_hold(words, 21, 146, q, 0, 20, rect, hold), want)
            assert np.array_equal(FMH.replay_hold(words, 21, 146, q, 0, 20, rect, hold, flush=False), want[:20 - hold + 1])
            # the host callable leaves a NumpyHoldCounter where it would stand after those frames
            cells, counter = NumpyCellsHoldMasks(), NumpyHoldCounter()
            cells.words, cells.frames = words[:13], 13
            head = cells.replay(region, q, rect, counter, hold, False)
            tail = counter(frames[13:], area, th, hold, 13, True)
            assert np.array_equal(np.concatenate([head, tail]), want), (rect, th)


# ---- the selector ----------------------------------------------------------------------------------------------------------------------
_two_passes = {}


def two_passes(frames, window, edge_thresh, **locator):
    """AreaLocator(automaton="hold") over the first `window` frames, then the plain hold selector on its area at its threshold
    -> (locator, selector | None)."""
    key = (id(frames), window, edge_thresh, tuple(sorted(locator.items())))
    if key not in _two_passes:
        loc = area_locator.AreaLocator(NumpyCellsHold(), automaton="hold", edge_thresh=edge_thresh, probe=(1, window), batch=BATCH, **locator)
        area = loc.run(list(frames), FPS)
        sel = None
        if area is not None:
            sel = frame_select.HoldFrameSelector(NumpyHoldCounter(), edge_thresh=loc.edge_thresh, batch=BATCH)
            sel.run(list(frames), area, FPS)
        _two_passes[key] = (loc, sel)
    return _two_passes[key]


@pytest.mark.parametrize("batch", [7, 64])
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("edge_thresh", [128, "auto"])
def test_selector_equals_the_locator_pass_and_the_plain_selector(edge_thresh, window, batch):
    frames, truth = busy_clip()
    loc, plain = two_passes(frames, window, edge_thresh)
    assert as_tuple(loc.area) == HELD_AREA and loc.hold == HOLD
    cells, counter = NumpyCellsHoldMasks(), NumpyHoldCounter()
    sel = LocatingHoldSelector(counter, cells, window=window, edge_thresh=edge_thresh, batch=batch)
    seen, yielded, decided_at = 0, [], min(window, len(frames))
    for items, closed in sel.iter_run(iter(list(frames)), None, FPS):
        seen += len(items)
        if seen < decided_at or (window > len(frames) and items):
            assert closed == [] and sel.tracker is None and not sel.decided and sel.area is None
        elif items and seen - len(items) < decided_at:           # the deciding batch: the tracker has seen the rows 1 .. window - hold + 1
            assert sel.decided and sel.tracker.fed == decided_at - HOLD + 1 and sel.hold == HOLD
        yielded += closed
    assert sel.decided and as_tuple(sel.area) == as_tuple(loc.area) and sel.edge_thresh == loc.edge_thresh
    assert sel.scores == loc.scores and sel.frames_scanned == loc.frames_scanned == decided_at == cells.frames and seen == len(frames)
    assert sel.totals.shape == loc.totals.shape and np.array_equal(sel.totals, loc.totals)
    assert sel.intervals == plain.intervals == yielded and np.array_equal(sel.counts, plain.counts) and len(sel.counts) == len(frames)
    assert sel.tracker.min_frames == HOLD
    if edge_thresh == 128:
        assert [(s, e) for s, e, _r in sel.intervals] == SHOWN
    else:
        assert sel.edge_thresh == 64 and 2 <= len(sel.intervals) <= len(truth)
    q = 0 if edge_thresh == 128 else loc.thresholds.index(loc.edge_thresh)
    assert cells.replayed == [(q, as_tuple(loc.area), HOLD, window > len(frames))] and set(cells.cells.holds) == {HOLD}
    # the plain counter ran on the frames behind the window and for the flush only, and never with fed = 0
    assert counter.calls == (0 if window > len(frames) else -(-(len(frames) - window) // batch) + 1)


def test_the_locators_hold_and_the_selectors_are_two_numbers():
    frames, _truth = busy_clip()
    cells, counter = NumpyCellsHoldMasks(), NumpyHoldCounter()
    sel = LocatingHoldSelector(counter, cells, window=70, hold_frames=5, locator_params={"hold_frames": 3}, batch=BATCH)
    sel.run(iter(list(frames)), None, FPS)
    assert set(cells.cells.holds) == {3} and cells.replayed[0][2:] == (5, False) and sel.hold == 5
    loc, _plain = two_passes(frames, 70, 128, hold_frames=3)
    plain = frame_select.HoldFrameSelector(NumpyHoldCounter(), hold_frames=5, batch=BATCH)
    plain.run(list(frames), loc.area, FPS)
    assert as_tuple(sel.area) == as_tuple(loc.area) and sel.intervals == plain.intervals and np.array_equal(sel.counts, plain.counts)


def test_a_clip_of_exactly_the_window_is_flushed_through_the_counter():
    frames, _truth = busy_clip()
    loc, plain = two_passes(frames[:70], 70, 128)
    counter = NumpyHoldCounter()
    sel = LocatingHoldSelector(counter, NumpyCellsHoldMasks(), window=70, batch=BATCH)
    assert sel.run(iter(list(frames[:70])), None, FPS) == plain.intervals and np.array_equal(sel.counts, plain.counts)
    assert counter.calls == 1 and len(sel.counts) == 70


def test_selector_arguments():
    for bad in (dict(window=None), dict(window=0), dict(window=5, locator_params={"automaton": "change"}),
                dict(window=5, locator_params={"max_hold_seconds": 12}), dict(window=5, locator_params={"max_hold_frames": 100}),
                dict(window=5, locator_params={"search_area": extractor.SubtitleArea(0, 8, 0, 8)}),
                dict(window=5, locator_params={"probe": (1, 5)}), dict(window=5, max_hold_seconds=12), dict(window=5, max_hold_frames=100)):
        with pytest.raises(ValueError, match="LocatingHoldSelector"):
            LocatingHoldSelector(NumpyHoldCounter(), NumpyCellsHoldMasks(), **bad)
    sel = LocatingHoldSelector(NumpyHoldCounter(), NumpyCellsHoldMasks(), window=5, locator_params={"automaton": "hold"})
    with pytest.raises(ValueError, match="finds the area itself"):
        sel.run([np.zeros((16, 16, 3), np.uint8)], extractor.SubtitleArea(0, 8, 0, 8), FPS)
    assert sel.run([], None, FPS) == [] and sel.area is None and not sel.decided


# ---- the extractor ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def host_stack(monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)          # the scripted recogniser takes the list of host frames


@pytest.fixture(scope="module")
def y4m(tmp_path_factory):
    """The clip as a YUV4MPEG2 file -> (its path, its bytes, the frames a reader decodes from them)."""
    path = str(tmp_path_factory.mktemp("locate_hold") / "clip.y4m")
    ingest.write_y4m(path, [ingest.bgr_to_yuv420(f) for f in busy_clip()[0]], FPS)
    src = ingest.Y4mSource(path)
    decoded = list(src.frames())
    src.close()
    with open(path, "rb") as fp:
        return path, fp.read(), decoded


def make(source, decoded, truth, key, edge_thresh=128, one_pass=None, change_params=None, **area_params):
    ocr = LookupOcr(decoded, truth, TEXT_BOX)
    own = {"streaming_locate_hold": True, "cells_hold_masks_fn": NumpyCellsHoldMasks()} if key else {"cells_fn": NumpyCellsHold(), "automaton": "hold"}
    params = {**({} if edge_thresh == 128 else {"edge_thresh": edge_thresh}), **(change_params or {})}
    ex = extractor.SubtitleExtractor(source, ocr, sub_area="auto", mode="fast", frame_selector="hold", change_counter=NumpyHoldCounter(),
                                     drop_score=0.0, batch=BATCH, one_pass=one_pass, change_params=params or None,
                                     area_params={**own, **area_params})
    return ex, ocr


def results(ex, ocr):
    text = ex.run()
    return as_tuple(ex.located_area), ex.edge_thresh, ex.intervals, ocr.seen, ex.raw_lines, text


@pytest.mark.parametrize("edge_thresh,window", [(128, 40), (128, 200), ("auto", 70), ("auto", 40)])
def test_several_passes_and_one_pass_equal_several_passes_with_that_probe(host_stack, y4m, edge_thresh, window):
    path, data, decoded = y4m
    truth = busy_clip()[1]
    src = ingest.Y4mSource(path)
    want_ex, ocr = make(src, decoded, truth, key=False, edge_thresh=edge_thresh, probe=(1, window))
    want = results(want_ex, ocr)
    assert want[0] is not None and len(want[2]) >= 2 and want[5].count(" --> ") >= 2
    if edge_thresh == 128:
        assert [(s, e) for s, e, _r in want[2]] == SHOWN
    # several passes with the key
    ex, ocr = make(src, decoded, truth, key=True, edge_thresh=edge_thresh, locate_seconds=window / FPS)
    assert not ex.one_pass and results(ex, ocr) == want and ex.frames_located == min(window, len(decoded))
    assert ex.edge_scores is None if edge_thresh == 128 else len(ex.edge_scores) == 8
    src.close()
    # one pass over a pipe
    pipe, th = piped(data, 65536)
    stream = ingest.Y4mStream(pipe)
    ex, ocr = make(stream, decoded, truth, key=True, edge_thresh=edge_thresh, locate_seconds=window / FPS)
    got = results(ex, ocr)
    th.join()
    pipe.close()
    assert ex.one_pass and stream.frame_count == len(decoded) and got == want
    assert ex.clamped_intervals == 0 and ex.peak_retained >= min(window, len(decoded)) and ex.frames_located == min(window, len(decoded))
    # a seekable source forced into one pass takes the same road; giving the implied automaton is accepted
    ex, ocr = make(extractor.ArraySource(list(decoded), FPS), decoded, truth, key=True, edge_thresh=edge_thresh, one_pass=True,
                   locate_seconds=window / FPS, automaton="hold")
    assert results(ex, ocr)[:5] == want[:5]                      # (the SRT's times: an array source has no timestamps of its own)


def test_the_locators_hold_follows_the_selectors_unless_area_params_sets_its_own(host_stack):
    frames, truth = busy_clip()
    for change, own, want_locator, want_selector in (({"hold_frames": 3}, {}, 3, 3), ({"hold_frames": 3}, {"hold_frames": 5}, 5, 3),
                                                     ({"hold_seconds": 0.2}, {}, 5, 5), ({}, {"hold_seconds": 0.16}, 4, 8)):
        ex, ocr = make(extractor.ArraySource(list(frames), FPS), frames, truth, key=True, change_params=change, locate_seconds=2.0, **own)
        cells = ex._locate_fns[0]
        ex.run()
        assert set(cells.cells.holds) == {want_locator} and cells.replayed[0][2] == want_selector, (change, own)


def test_several_passes_without_locate_seconds_decide_on_the_whole_clip(host_stack):
    frames, truth = busy_clip()

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
    assert results(ex, ocr) == want and ex.frames_located == len(frames) and want[0] == HELD_AREA
    assert src.passes == passes_without - 1 == 1                 # the locator's pass is folded into the selector's


@pytest.mark.parametrize("one_pass", [None, True])
def test_no_area_found_warns_and_goes_on_as_the_run_without_one(host_stack, one_pass, caplog):
    frames, truth = synth.make_moving_clip([(None, 40)], amp=(120, 120))
    want_ex, ocr = make(extractor.ArraySource(list(frames), FPS), frames, truth, key=False, probe=(1, 20))
    want = results(want_ex, ocr)
    assert want[0] is None and want[2] is None and len(want[3]) > 0
    caplog.clear()
    ex, ocr = make(extractor.ArraySource(list(frames), FPS), frames, truth, key=True, one_pass=one_pass, locate_seconds=0.8)
    with caplog.at_level(logging.WARNING):
        got = results(ex, ocr)
    assert got == want and ex.sub_area is None and ex.frames_located == 20
    assert len([r for r in caplog.records if "no subtitle area found in 20 frames" in r.getMessage()]) == 1
    if one_pass:
        assert ex.peak_retained >= 20


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def build(one_pass=None, area_params=None, **kw):
    frames = np.zeros((4, 16, 16, 3), np.uint8)
    args = dict(sub_area="auto", frame_selector="hold", one_pass=one_pass, area_params={"streaming_locate_hold": True, **(area_params or {})})
    args.update(kw)
    return extractor.SubtitleExtractor(extractor.ArraySource(list(frames), FPS), LookupOcr([], [], None), **args)


@pytest.mark.parametrize("names,kw", [
    (["streaming_locate"], dict(area_params={"streaming_locate": True})),
    (["frame_selector='change'"], dict(frame_selector="change")),
    (["frame_selector='fps'"], dict(frame_selector="fps")),
    (["automaton='change'"], dict(area_params={"automaton": "change"})),
    (["max_hold_seconds in area_params"], dict(area_params={"max_hold_seconds": 12})),
    (["max_hold_frames in area_params"], dict(area_params={"automaton": "hold", "max_hold_frames": 100})),
    (["max_hold_seconds in change_params"], dict(change_params={"max_hold_seconds": 12})),
    (["max_hold_frames in change_params"], dict(change_params={"max_hold_frames": 100})),
    (["search_area"], dict(area_params={"search_area": extractor.SubtitleArea(0, 8, 0, 8)})),
    (["probe"], dict(area_params={"probe": (1, 20)})),
    (["area_params={'streaming': True}"], dict(area_params={"streaming": True}, change_params={"edge_thresh": "auto"})),
    (["interval_frame='sharpest'"], dict(interval_frame="sharpest")),
    (["composite_params={'streaming': True}"], dict(interval_image="min", composite_params={"streaming": True})),
    (["shard=(0, 2)"], dict(shard=(0, 2))),
    (["mode='accurate'"], dict(mode="accurate")),
    (["sub_area=SubtitleArea", "sub_area='auto'"], dict(sub_area=extractor.SubtitleArea(80, 120, 0, 320))),
    (["sub_area=None"], dict(sub_area=None)),
])
def test_the_key_refuses_by_name(names, kw):
    with pytest.raises(ValueError) as e:
        build(**kw)
    assert KEY in str(e.value) and "does not combine with" in str(e.value) and all(n in str(e.value) for n in names)


def test_the_keys_parameters_and_the_two_keys_callables():
    frames = np.zeros((4, 16, 16, 3), np.uint8)

    def plain(**area_params):
        return extractor.SubtitleExtractor(extractor.ArraySource(list(frames), FPS), LookupOcr([], [], None), sub_area="auto",
                                           frame_selector="hold", area_params=area_params)
    for own in ("cells_hold_masks_fn", "replay_hold_fn"):
        for other in ({}, {"streaming_locate_hold": False}, {"streaming_locate": True}):
            with pytest.raises(ValueError, match=rf"area_params: \['{own}'\] belong to area_params=\{{'streaming_locate_hold': True\}} and mean nothing"):
                plain(**{own: 3.0}, **other)
    for own in ("cells_masks_fn", "replay_fn"):                  # the other key's callables
        with pytest.raises(ValueError, match=rf"area_params: \['{own}'\] belong to area_params=\{{'streaming_locate': True\}} and mean nothing"):
            build(area_params={own: 3.0})
    for own in ("locate_seconds", "mask_gib"):                   # they go with either key, and mean nothing with neither, as before
        with pytest.raises(ValueError, match=rf"area_params: \['{own}'\] belong to area_params=\{{'streaming_locate': True\}} and mean nothing"):
            plain(**{own: 3.0})
    with pytest.raises(ValueError, match="locate_seconds must be positive"):
        build(area_params={"locate_seconds": 0})
    with pytest.raises(ValueError, match="mask_gib must be positive"):
        build(area_params={"mask_gib": 0})
    with pytest.raises(ValueError, match="in one pass needs locate_seconds") as e:
        build(one_pass=True)
    assert KEY in str(e.value)
    build(one_pass=True, area_params={"locate_seconds": 5})                          # accepted
    build(one_pass=True, area_params={"locate_seconds": 5, "automaton": "hold"}, change_params={"edge_thresh": "auto"})
    build()                                                                          # several passes: the whole clip decides
    with pytest.raises(ValueError, match=r"sub_area='auto' is not available in one pass"):       # without the key nothing changed
        extractor.SubtitleExtractor(extractor.ArraySource(list(frames), FPS), LookupOcr([], [], None), sub_area="auto", frame_selector="hold",
                                    one_pass=True, area_params={"automaton": "hold"})


def test_the_window_must_fit_what_keeps_it(host_stack):
    frames, truth = busy_clip()
    per = frames[0].nbytes
    ex, ocr = make(extractor.ArraySource(list(frames), FPS), frames, truth, key=True, one_pass=True, locate_seconds=1.6)
    ex.retain_bytes = 40 * per - 1
    with pytest.raises(ValueError) as e:
        ex.run()
    msg = str(e.value)
    assert KEY in msg and f"{40 * per} bytes" in msg and f"retain_bytes={40 * per - 1}" in msg and "shorter locate_seconds" in msg
    assert "--retain-gib" in msg and ocr.seen == []
    ex.retain_bytes = 40 * per                                                       # exactly enough
    ex.run()
    assert as_tuple(ex.located_area) == HELD_AREA and ex.clamped_intervals == 0
    gy, gx = area_locator.cells_dims(120, 320)
    need = 40 * gy * gx * 64
    for one_pass in (None, True):
        ex, ocr = make(extractor.ArraySource(list(frames), FPS), frames, truth, key=True, one_pass=one_pass, locate_seconds=1.6,
                       mask_gib=(need - 1) / (1 << 30))
        with pytest.raises(ValueError) as e:
            ex.run()
        msg = str(e.value)
        assert KEY in msg and f"{need} bytes" in msg and "mask_gib" in msg and "shorter locate_seconds" in msg and "--mask-gib" in msg
        assert ocr.seen == []
    ex, ocr = make(extractor.ArraySource(list(frames), FPS), frames, truth, key=True, edge_thresh="auto", locate_seconds=1.6,
                   mask_gib=(8 * need - 1) / (1 << 30))
    with pytest.raises(ValueError, match="8 thresholds"):
        ex.run()


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def test_command_line(host_stack, y4m, monkeypatch, capsys, caplog):
    path, data, decoded = y4m
    truth = busy_clip()[1]
    common = ["--area", "auto", "--selector", "hold", "--batch", str(BATCH)]

    def main(args, stdin=True):
        pipe, th = piped(data if stdin else b"", 4099)
        monkeypatch.setattr("sys.stdin", type("Stdin", (), {"buffer": pipe})())
        ocr = LookupOcr(decoded, truth, TEXT_BOX)
        rc = extractor.main(args, ocr=ocr, counter=NumpyHoldCounter(), cells_fn=NumpyCellsHold(), cells_hold_masks_fn=NumpyCellsHoldMasks())
        pipe.close()
        th.join()
        return rc, ocr, capsys.readouterr()
    src = ingest.Y4mSource(path)
    want = results(*make(src, decoded, truth, key=False, probe=(1, 40)))[5]
    src.close()
    rc, ocr, out = main(["-"] + common + ["--streaming-locate-hold", "--locate-seconds", "1.6"])
    assert rc == 0 and out.out == want and want.count(" --> ") == len(truth) and len(ocr.seen) == len(truth)
    rc, _ocr, several = main([path] + common + ["--locator-automaton", "hold"], stdin=False)          # the locator's own pass, then the selector's
    assert rc == 0 and several.out.count(" --> ") == len(truth)
    with caplog.at_level(logging.INFO, logger="vse_amd.extractor"):
        rc, _ocr, out = main(["-"] + common + ["--streaming-locate-hold"])            # a pipe: what fits, at most 300 s, beyond this clip
    assert rc == 0 and out.out == several.out
    assert [r.getMessage() for r in caplog.records if "--streaming-locate" in r.getMessage()] == [
        "--streaming-locate-hold: the area is found on the first 300 seconds (what fits --retain-gib 4 and --mask-gib 8, at most 300)"]
    rc, _ocr, out = main([path] + common + ["--streaming-locate-hold", "--mask-gib", "1"], stdin=False)     # a file: the whole clip
    assert rc == 0 and out.out == several.out
    for bad, word in ((["-"] + common, "sub_area='auto' is not available in one pass"),
                      (["-"] + common + ["--locate-seconds", "3"], "--locate-seconds"),
                      (["-"] + common + ["--streaming-locate-hold", "--streaming-locate"], "give one of them"),
                      (["-"] + common + ["--streaming-locate-hold", "--locate-seconds", "0"], "locate_seconds"),
                      (["-"] + common + ["--streaming-locate-hold", "--locate-seconds", "2", "--mask-gib", "0.0001"], "mask_gib"),
                      (["-"] + common + ["--streaming-locate-hold", "--locate-seconds", "2", "--retain-gib", "0.001"], "--retain-gib"),
                      (["-"] + common + ["--streaming-locate-hold", "--max-hold-seconds", "12"], "max_hold_seconds in change_params"),
                      (["-"] + common + ["--streaming-locate-hold", "--locator-max-hold-seconds", "12", "--locator-automaton", "hold"],
                       "max_hold_seconds in area_params"),
                      (["-", "--area", "auto", "--selector", "change", "--streaming-locate-hold"], "frame_selector='change'"),
                      (["-", "--area", "auto", "--selector", "hold", "--streaming-locate"], "frame_selector='hold'"),
                      (["-", "--area", "80,120,0,320", "--selector", "hold", "--streaming-locate-hold"], "sub_area=")):
        rc, ocr, out = main(bad)
        assert rc == 2 and out.err.startswith("extractor: ") and word in out.err and ocr.seen == [], bad
    with pytest.raises(SystemExit):
        extractor.main(["--help"])
    assert "--streaming-locate-hold" in " ".join(capsys.readouterr().out.split())
