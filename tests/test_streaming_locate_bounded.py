"""The subtitle area found in the pass of the HOLD selector with BOUNDED runs, on the host: the numpy restatement of the replay against
frame_hold_bounded_ref, frame_select.LocatingBoundedHoldSelector against AreaLocator(automaton="hold", max_hold_frames=M)'s pass over the
window followed by HoldFrameSelector(max_hold_frames=S) on what it found, SubtitleExtractor with area_params={"streaming_locate_bounded":
True} in several passes and in one pass over a pipe against the several-pass run with that probe, every refusal, and the command line.
The clips are tests/test_area_locator_hold_bounded.py's: a busy background that STANDS STILL behind the subtitles, on which the held
automaton finds no area (or a wrong one) and the unbounded hold selector merges the subtitles.  CPU only: the numpy cells, masks and
counters (tests/area_cells_hold_bounded_ref.py, tests/frame_masks_hold_bounded_ref.py, tests/frame_hold_bounded_ref.py) and a scripted
recogniser."""
import logging

import numpy as np
import pytest

import frame_masks_hold_bounded_ref as FMB
import frame_masks_ref as FM
from area_cells_hold_bounded_ref import NumpyCellsHoldBounded
from frame_change_ref import edge_mask
from frame_hold_bounded_ref import NumpyBoundedHoldCounter, counts as bounded_counts
from frame_masks_hold_bounded_ref import NumpyCellsHoldBoundedMasks
from frame_masks_hold_ref import NumpyCellsHoldMasks
from test_area_locator_hold_bounded import FPS, STATIC, TRUE, as_tuple, contains_text, static_clip
from test_one_pass import LookupOcr, piped
from vse_amd import area_locator, extractor, frame_select, ingest
from vse_amd.frame_select import LocatingBoundedHoldSelector, LocatingHoldSelector

BATCH = 8
HOLD, MAX_HOLD = 3, 30        # the runs that count, for the locator and for the selector: a subtitle of the clips is shown 20 frames
KEY = "area_params={'streaming_locate_bounded': True}"
TEXT_BOX = [[40, 92], [280, 92], [280, 112], [40, 112]]          # inside the text rows of the 120 x 320 clips
CHANGE = {"hold_frames": HOLD, "max_hold_frames": MAX_HOLD}
LOCATOR = {"hold_frames": HOLD, "max_hold_frames": MAX_HOLD}
CLIP = 90


def test_the_clips_are_what_the_windows_were_chosen_for():
    for name in STATIC:
        frames, truth = static_clip(name)
        assert frames.shape == (CLIP, 120, 320, 3) and [(s, e) for s, e, _t in truth] == TRUE


# ---- the numpy restatement itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold,max_hold", [(1, 1), (2, 5), (3, 30), (8, 70), (3, 4000)])
def test_the_numpy_replay_is_frame_hold_bounded_on_the_rectangle(hold, max_hold):
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, size=(24, 23, 150, 3), dtype=np.uint8)
    frames[6:17, 4:20, 30:120] = frames[5, 4:20, 30:120]         # a patch that holds still for twelve frames, and one for four
    frames[19:22, 2:12, 60:140] = frames[18, 2:12, 60:140]
    n = len(frames)
    region, ths = (1, 22, 3, 149), (40, 90)
    words = FM.mask_words(frames, region, ths)
    for rect in ((0, 21, 0, 146), (1, 12, 1, 68), (9, 21, 63, 146), (2, 5, 64, 67)):
        area = (region[0] + rect[0], region[0] + rect[1], region[2] + rect[2], region[2] + rect[3])
        for q, th in enumerate(ths):
            want = bounded_counts(frames, area, th, hold, max_hold)
            rows, runs = FMB.replay_hold_bounded(words, 21, 146, q, 0, n, rect, hold, max_hold)
            assert np.array_equal(rows, want) and len(rows) == n
            assert np.array_equal(runs, FMB.run_lengths(edge_mask(frames, area, th), max_hold)) and runs.max() <= max_hold + 1
            head, _runs = FMB.replay_hold_bounded(words, 21, 146, q, 0, n, rect, hold, max_hold, flush=False)
            assert len(head) == max(0, n - max_hold)
            if len(head) and max_hold > 1:
                # rows that are final before the clip ends are the whole clip's (at max_hold 1 a run that reaches the last frame fed
                # is cut off there and counts, which the device's pending state knows and a cut-off stack does not)
                assert np.array_equal(head, want[:len(head)])
            # the host callable leaves a NumpyBoundedHoldCounter where it would stand after those frames
            cells, counter = NumpyCellsHoldBoundedMasks(), NumpyBoundedHoldCounter()
            cells.words, cells.frames = words[:13], 13
            head = cells.replay(region, q, rect, counter, hold, max_hold, False)
            tail = counter(frames[13:], area, th, hold, max_hold, 13, True)
            assert np.array_equal(np.concatenate([head, tail]), want), (rect, th)
    whole = bounded_counts(frames, (1, 22, 3, 149), 40, hold, max_hold)
    assert whole[:, 0].max() > 0 and whole[:, 1].max() > 0 and whole[:, 2].max() > 0          # (the clip counts something in range)


# ---- the selector ----------------------------------------------------------------------------------------------------------------------
_two_passes = {}


def two_passes(name, window, edge_thresh, selector=None, **locator):
    """AreaLocator(automaton="hold", max_hold_frames=M) over the first `window` frames, then the plain bounded hold selector on its area
    at its threshold -> (locator, selector | None)."""
    frames, _truth = static_clip(name)
    selector = dict(CHANGE) if selector is None else selector
    key = (name, window, edge_thresh, tuple(sorted(selector.items())), tuple(sorted(locator.items())))
    if key not in _two_passes:
        loc = area_locator.AreaLocator(NumpyCellsHoldBounded(), automaton="hold", edge_thresh=edge_thresh, probe=(1, window), batch=BATCH,
                                       **{**LOCATOR, **locator})
        area = loc.run(list(frames), FPS)
        sel = None
        if area is not None:
            sel = frame_select.HoldFrameSelector(NumpyBoundedHoldCounter(), edge_thresh=loc.edge_thresh, batch=BATCH, **selector)
            sel.run(list(frames), area, FPS)
        _two_passes[key] = (loc, sel)
    return _two_passes[key]


# windows shorter than, equal to and longer than the selector's max_hold (30) and the clip (90); batches that do and do not divide them
@pytest.mark.parametrize("name,edge_thresh,window,batch", [
    ("loud", 64, 20, 7), ("loud", 64, 30, 10), ("loud", 64, 64, 8), ("loud", 64, 64, 7), ("loud", 64, 90, 64), ("loud", 64, 200, 9),
    ("loud", "auto", 64, 7), ("busier", "auto", 90, 30), ("busier", "auto", 200, 64)])
def test_selector_equals_the_locator_pass_and_the_plain_selector(name, edge_thresh, window, batch):
    frames, truth = static_clip(name)
    loc, plain = two_passes(name, window, edge_thresh)
    assert (loc.hold, loc.max_hold) == (HOLD, MAX_HOLD)
    cells, counter = NumpyCellsHoldBoundedMasks(), NumpyBoundedHoldCounter()
    sel = LocatingBoundedHoldSelector(counter, cells, window=window, edge_thresh=edge_thresh, batch=batch, locator_params=dict(LOCATOR),
                                      **CHANGE)
    seen, yielded, decided_at = 0, [], min(window, CLIP)
    for items, closed in sel.iter_run(iter(list(frames)), None, FPS):
        seen += len(items)
        if seen < decided_at or (window > CLIP and items):
            assert closed == [] and sel.tracker is None and not sel.decided and sel.area is None
        elif items and seen - len(items) < decided_at and sel.area is not None:
            # the deciding batch: without a flush the tracker has seen the rows 1 .. max(0, W - max_hold)
            assert sel.decided and sel.tracker.fed == max(0, decided_at - MAX_HOLD) and (sel.hold, sel.max_hold) == (HOLD, MAX_HOLD)
        yielded += closed
    assert sel.decided and as_tuple(sel.area) == as_tuple(loc.area) and sel.edge_thresh == loc.edge_thresh
    assert sel.scores == loc.scores and sel.frames_scanned == loc.frames_scanned == decided_at == cells.frames
    assert sel.totals.shape == loc.totals.shape and np.array_equal(sel.totals, loc.totals)
    assert set(cells.cells.holds) == {(HOLD, MAX_HOLD)}
    if window < 64:
        return                                                    # (whatever so short a window decides, both roads decided it alike)
    assert contains_text(sel.area) and seen == CLIP and sel._lag() == MAX_HOLD
    assert sel.intervals == plain.intervals == yielded and np.array_equal(sel.counts, plain.counts) and len(sel.counts) == CLIP
    assert set(TRUE) <= {(s, e) for s, e, _r in sel.intervals}
    q = 0 if edge_thresh != "auto" else loc.thresholds.index(loc.edge_thresh)
    assert cells.replayed == [(q, as_tuple(loc.area), HOLD, MAX_HOLD, window > CLIP)]
    # the plain counter ran on the frames behind the window and for the flush only, and never with fed = 0
    assert counter.calls == (0 if window > CLIP else -(-(CLIP - window) // batch) + 1)


def test_short_windows_decide_as_the_locator_pass_does():
    """Windows of 20 and 30 frames: what they find is the locator pass's, and when it is an area the selector goes on as the plain one."""
    frames, _truth = static_clip("loud")
    for window in (20, 30):
        loc, plain = two_passes("loud", window, 64)
        sel = LocatingBoundedHoldSelector(NumpyBoundedHoldCounter(), NumpyCellsHoldBoundedMasks(), window=window, edge_thresh=64, batch=BATCH,
                                          locator_params=dict(LOCATOR), **CHANGE)
        got = sel.run(iter(list(frames)), None, FPS)
        assert as_tuple(sel.area) == as_tuple(loc.area)
        if plain is not None:
            assert got == plain.intervals and np.array_equal(sel.counts, plain.counts)


def test_the_locators_bounds_and_the_selectors_are_four_numbers():
    frames, _truth = static_clip("loud")
    cells, counter = NumpyCellsHoldBoundedMasks(), NumpyBoundedHoldCounter()
    sel = LocatingBoundedHoldSelector(counter, cells, window=70, edge_thresh=64, hold_frames=5, max_hold_frames=40, batch=BATCH,
                                      locator_params={"hold_frames": 3, "max_hold_seconds": 1.2})
    sel.run(iter(list(frames)), None, FPS)
    assert set(cells.cells.holds) == {(3, 30)} and cells.replayed[0][2:] == (5, 40, False) and (sel.hold, sel.max_hold) == (5, 40)
    assert sel.tracker.min_frames == 5
    loc, plain = two_passes("loud", 70, 64, selector={"hold_frames": 5, "max_hold_frames": 40})
    assert as_tuple(sel.area) == as_tuple(loc.area) and sel.intervals == plain.intervals and np.array_equal(sel.counts, plain.counts)


def test_a_clip_of_exactly_the_window_is_flushed_through_the_counter():
    frames, _truth = static_clip("loud")
    loc = area_locator.AreaLocator(NumpyCellsHoldBounded(), automaton="hold", edge_thresh=64, batch=BATCH, **LOCATOR)
    area = loc.run(list(frames[:70]), FPS)
    plain = frame_select.HoldFrameSelector(NumpyBoundedHoldCounter(), edge_thresh=64, batch=BATCH, **CHANGE)
    plain.run(list(frames[:70]), area, FPS)
    counter = NumpyBoundedHoldCounter()
    sel = LocatingBoundedHoldSelector(counter, NumpyCellsHoldBoundedMasks(), window=70, edge_thresh=64, batch=BATCH,
                                      locator_params=dict(LOCATOR), **CHANGE)
    assert sel.run(iter(list(frames[:70])), None, FPS) == plain.intervals and np.array_equal(sel.counts, plain.counts)
    assert counter.calls == 1 and len(sel.counts) == 70


def test_selector_arguments():
    ok = dict(window=5, locator_params=dict(LOCATOR), **CHANGE)
    for bad, word in ((dict(ok, window=None), "window"), (dict(ok, window=0), "window"),
                      (dict(ok, locator_params={**LOCATOR, "automaton": "change"}), "automaton='change'"),
                      (dict(ok, locator_params={**LOCATOR, "search_area": extractor.SubtitleArea(0, 8, 0, 8)}), "search_area"),
                      (dict(ok, locator_params={**LOCATOR, "probe": (1, 5)}), "probe"),
                      (dict(window=5, locator_params=dict(LOCATOR), hold_frames=3), "the selector's max_hold_seconds or max_hold_frames is required"),
                      (dict(window=5, locator_params={"hold_frames": 3}, **CHANGE), "locator_params' max_hold_seconds or max_hold_frames is required"),
                      (dict(window=5, **CHANGE), "locator_params' max_hold_seconds or max_hold_frames is required")):
        with pytest.raises(ValueError, match="LocatingBoundedHoldSelector") as e:
            LocatingBoundedHoldSelector(NumpyBoundedHoldCounter(), NumpyCellsHoldBoundedMasks(), **bad)
        assert word in str(e.value), bad
    assert issubclass(LocatingBoundedHoldSelector, LocatingHoldSelector)
    assert LocatingBoundedHoldSelector.iter_run is LocatingHoldSelector.iter_run          # the hooks, not a third copy
    sel = LocatingBoundedHoldSelector(NumpyBoundedHoldCounter(), NumpyCellsHoldBoundedMasks(), window=5,
                                      locator_params={**LOCATOR, "automaton": "hold"}, max_hold_seconds=1.2)
    with pytest.raises(ValueError, match="finds the area itself"):
        sel.run([np.zeros((16, 16, 3), np.uint8)], extractor.SubtitleArea(0, 8, 0, 8), FPS)
    assert sel.run([], None, FPS) == [] and sel.area is None and not sel.decided
    # a bound below the hold or beyond the device's is refused once the frame rate is known, before any frame is counted
    for kw in (dict(CHANGE, max_hold_frames=2), dict(CHANGE, max_hold_frames=4001)):
        cells = NumpyCellsHoldBoundedMasks()
        sel = LocatingBoundedHoldSelector(NumpyBoundedHoldCounter(), cells, window=5, locator_params=dict(LOCATOR), **kw)
        with pytest.raises(ValueError, match="max_hold"):
            sel.run([np.zeros((16, 16, 3), np.uint8)] * 6, None, FPS)
        assert cells.frames == 0
    # the unbounded selector keeps refusing the bounds, word for word
    for bad in (dict(locator_params={"max_hold_seconds": 12}), dict(max_hold_frames=100)):
        with pytest.raises(ValueError, match="LocatingHoldSelector: the locator in the selector's pass counts whole frames with the held "
                                             "automaton, the kept words are replayed with unbounded runs"):
            LocatingHoldSelector(None, NumpyCellsHoldMasks(), window=5, **bad)


# ---- the extractor ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def host_stack(monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)          # the scripted recogniser takes the list of host frames


@pytest.fixture(scope="module", params=sorted(STATIC))
def y4m(request, tmp_path_factory):
    """A clip as a YUV4MPEG2 file -> (its name, its path, its bytes, the frames a reader decodes from them)."""
    path = str(tmp_path_factory.mktemp("locate_bounded") / f"{request.param}.y4m")
    ingest.write_y4m(path, [ingest.bgr_to_yuv420(f) for f in static_clip(request.param)[0]], FPS)
    src = ingest.Y4mSource(path)
    decoded = list(src.frames())
    src.close()
    with open(path, "rb") as fp:
        return request.param, path, fp.read(), decoded


def make(source, decoded, truth, key, edge_thresh="auto", one_pass=None, change_params=None, **area_params):
    ocr = LookupOcr(decoded, truth, TEXT_BOX)
    own = ({"streaming_locate_bounded": True, "cells_bounded_masks_fn": NumpyCellsHoldBoundedMasks()} if key else
           {"cells_fn": NumpyCellsHoldBounded(), "automaton": "hold"})
    params = {**CHANGE, **({} if edge_thresh == 128 else {"edge_thresh": edge_thresh}), **(change_params or {})}
    ex = extractor.SubtitleExtractor(source, ocr, sub_area="auto", mode="fast", frame_selector="hold", change_counter=NumpyBoundedHoldCounter(),
                                     drop_score=0.0, batch=BATCH, one_pass=one_pass, change_params=params,
                                     area_params={**own, "max_hold_frames": MAX_HOLD, **area_params})
    return ex, ocr


def three_true_lines(text, truth):
    """Three blocks, each a true line (their frames are checked on `intervals`, which the SRT's times are made of)."""
    return text.count(" --> ") == len(TRUE) and all(line in text for _s, _e, line in truth)


def results(ex, ocr):
    text = ex.run()
    return as_tuple(ex.located_area), ex.edge_thresh, ex.intervals, ocr.seen, ex.raw_lines, text


@pytest.mark.parametrize("window", [70, 200])
def test_several_passes_and_one_pass_equal_several_passes_with_that_probe(host_stack, y4m, window):
    name, path, data, decoded = y4m
    truth = static_clip(name)[1]
    src = ingest.Y4mSource(path)
    want_ex, ocr = make(src, decoded, truth, key=False, probe=(1, window))
    want = results(want_ex, ocr)
    # the result is the three true intervals, area and threshold found and nothing typed in (the gaps are shorter than max_hold, so
    # the background's runs that the text cut make them intervals too, as in the several-pass run: OCR calls without text, no line)
    assert want[0] is not None and want[1] in area_locator.AUTO_THRESHOLDS and set(TRUE) <= {(s, e) for s, e, _r in want[2]}
    assert three_true_lines(want[5], truth)
    # several passes with the key
    ex, ocr = make(src, decoded, truth, key=True, locate_seconds=window / FPS)
    assert not ex.one_pass and results(ex, ocr) == want and ex.frames_located == min(window, CLIP) and len(ex.edge_scores) == 8
    src.close()
    # one pass over a pipe
    pipe, th = piped(data, 65536)
    stream = ingest.Y4mStream(pipe)
    ex, ocr = make(stream, decoded, truth, key=True, locate_seconds=window / FPS)
    got = results(ex, ocr)
    th.join()
    pipe.close()
    assert ex.one_pass and stream.frame_count == CLIP and got == want
    assert ex.clamped_intervals == 0 and ex.peak_retained >= min(window, CLIP) and ex.frames_located == min(window, CLIP)
    # the same call with the unbounded key is still refused, and without any key sub_area="auto" in one pass is still refused
    with pytest.raises(ValueError, match="streaming_locate_hold.*max_hold_frames in area_params"):
        extractor.SubtitleExtractor(extractor.ArraySource(list(decoded), FPS), ocr, sub_area="auto", frame_selector="hold", one_pass=True,
                                    change_params=dict(CHANGE), area_params={"streaming_locate_hold": True, "max_hold_frames": MAX_HOLD,
                                                                            "locate_seconds": window / FPS})
    with pytest.raises(ValueError, match="sub_area='auto' is not available in one pass"):
        extractor.SubtitleExtractor(extractor.ArraySource(list(decoded), FPS), ocr, sub_area="auto", frame_selector="hold", one_pass=True,
                                    change_params=dict(CHANGE), area_params={"automaton": "hold", "max_hold_frames": MAX_HOLD})


def test_one_threshold_and_a_seekable_source_forced_into_one_pass(host_stack):
    frames, truth = static_clip("loud")
    want = results(*make(extractor.ArraySource(list(frames), FPS), frames, truth, key=False, edge_thresh=64, probe=(1, 70)))
    assert set(TRUE) <= {(s, e) for s, e, _r in want[2]} and three_true_lines(want[5], truth)
    ex, ocr = make(extractor.ArraySource(list(frames), FPS), frames, truth, key=True, edge_thresh=64, one_pass=True, locate_seconds=2.8,
                   automaton="hold")                              # (giving the implied automaton is accepted)
    assert results(ex, ocr) == want and ex.edge_scores is None and ex.peak_retained >= 70


def test_the_locators_hold_follows_the_selectors_and_its_bound_does_not(host_stack):
    frames, truth = static_clip("loud")
    for change, own, want_locator, want_selector in (({}, {}, (3, 30), (3, 30)), ({"hold_frames": 4}, {"max_hold_frames": 25}, (4, 25), (4, 30)),
                                                     ({"max_hold_frames": 40}, {"hold_frames": 2}, (2, 30), (3, 40))):
        ex, _ocr = make(extractor.ArraySource(list(frames), FPS), frames, truth, key=True, edge_thresh=64, change_params=change,
                        locate_seconds=2.8, **own)
        cells = ex._locate_fns[0]
        ex.run()
        assert set(cells.cells.holds) == {want_locator} and cells.replayed[0][2:4] == want_selector, (change, own)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def build(one_pass=None, area_params=None, change_params=None, **kw):
    frames = np.zeros((4, 16, 16, 3), np.uint8)
    args = dict(sub_area="auto", frame_selector="hold", one_pass=one_pass, change_params={"max_hold_seconds": 12, **(change_params or {})},
                area_params={"streaming_locate_bounded": True, "max_hold_seconds": 12, **(area_params or {})})
    args.update(kw)
    return extractor.SubtitleExtractor(extractor.ArraySource(list(frames), FPS), LookupOcr([], [], None), **args)


@pytest.mark.parametrize("names,kw", [
    (["frame_selector='change'"], dict(frame_selector="change")),
    (["frame_selector='fps'"], dict(frame_selector="fps")),
    (["automaton='change'"], dict(area_params={"automaton": "change"})),
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


def test_the_key_refuses_the_other_two_keys_and_they_refuse_the_bounds():
    for other in ("streaming_locate", "streaming_locate_hold"):
        with pytest.raises(ValueError) as e:
            build(area_params={other: True})
        assert KEY in str(e.value) and f"does not combine with {other}, give one of them" in str(e.value)
    frames = np.zeros((4, 16, 16, 3), np.uint8)

    def other_key(key, selector, **kw):
        return extractor.SubtitleExtractor(extractor.ArraySource(list(frames), FPS), LookupOcr([], [], None), sub_area="auto",
                                           frame_selector=selector, **{"area_params": {key: True}, **kw})
    # exactly as before this key existed
    with pytest.raises(ValueError, match=r"streaming_locate_hold.*does not combine with max_hold_seconds in area_params"):
        other_key("streaming_locate_hold", "hold", area_params={"streaming_locate_hold": True, "max_hold_seconds": 12})
    with pytest.raises(ValueError, match=r"streaming_locate_hold.*does not combine with max_hold_frames in change_params"):
        other_key("streaming_locate_hold", "hold", change_params={"max_hold_frames": 100})
    with pytest.raises(ValueError, match=r"streaming_locate'.*does not combine with max_hold_seconds in area_params"):
        other_key("streaming_locate", "change", area_params={"streaming_locate": True, "max_hold_seconds": 12})
    with pytest.raises(ValueError, match=r"streaming_locate_hold.*it does not combine with streaming_locate, give one of them"):
        other_key("streaming_locate", "hold", area_params={"streaming_locate": True, "streaming_locate_hold": True})


def test_both_bounds_are_required_each_in_its_own_place():
    frames = np.zeros((4, 16, 16, 3), np.uint8)

    def plain(change_params, area_params):
        return extractor.SubtitleExtractor(extractor.ArraySource(list(frames), FPS), LookupOcr([], [], None), sub_area="auto",
                                           frame_selector="hold", change_params=change_params,
                                           area_params={"streaming_locate_bounded": True, **area_params})
    for change, area, where in ((None, {"max_hold_seconds": 12}, "change_params"), ({"hold_frames": 3}, {"max_hold_frames": 100}, "change_params"),
                                ({"max_hold_seconds": 12}, {}, "area_params"), ({"max_hold_frames": 100}, {"hold_frames": 3}, "area_params")):
        with pytest.raises(ValueError) as e:
            plain(change, area)
        assert KEY in str(e.value) and f"needs max_hold_seconds or max_hold_frames in {where}" in str(e.value) and "inherited" in str(e.value)
    plain({"max_hold_frames": 100}, {"max_hold_seconds": 12})     # accepted: frames for one, seconds for the other


def test_the_keys_parameters_and_the_three_keys_callables():
    frames = np.zeros((4, 16, 16, 3), np.uint8)

    def plain(**area_params):
        return extractor.SubtitleExtractor(extractor.ArraySource(list(frames), FPS), LookupOcr([], [], None), sub_area="auto",
                                           frame_selector="hold", area_params=area_params)
    for own in ("cells_bounded_masks_fn", "replay_bounded_fn"):
        for other in ({}, {"streaming_locate_bounded": False}, {"streaming_locate": True}, {"streaming_locate_hold": True}):
            with pytest.raises(ValueError, match=rf"area_params: \['{own}'\] belong to area_params=\{{'streaming_locate_bounded': True\}} and mean nothing"):
                plain(**{own: 3.0}, **other)
    for own, key in (("cells_masks_fn", "streaming_locate"), ("replay_fn", "streaming_locate"), ("cells_hold_masks_fn", "streaming_locate_hold"),
                     ("replay_hold_fn", "streaming_locate_hold")):           # the other keys' callables
        with pytest.raises(ValueError, match=rf"area_params: \['{own}'\] belong to area_params=\{{'{key}': True\}} and mean nothing"):
            build(area_params={own: 3.0})
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


def test_the_window_must_fit_what_keeps_it(host_stack):
    frames, truth = static_clip("loud")
    per = frames[0].nbytes
    ex, ocr = make(extractor.ArraySource(list(frames), FPS), frames, truth, key=True, edge_thresh=64, one_pass=True, locate_seconds=2.8)
    ex.retain_bytes = 70 * per - 1
    with pytest.raises(ValueError) as e:
        ex.run()
    msg = str(e.value)
    assert KEY in msg and f"{70 * per} bytes" in msg and f"retain_bytes={70 * per - 1}" in msg and "shorter locate_seconds" in msg
    assert "--retain-gib" in msg and ocr.seen == []
    gy, gx = area_locator.cells_dims(120, 320)
    need = 70 * gy * gx * 64
    for one_pass in (None, True):
        ex, ocr = make(extractor.ArraySource(list(frames), FPS), frames, truth, key=True, edge_thresh=64, one_pass=one_pass, locate_seconds=2.8,
                       mask_gib=(need - 1) / (1 << 30))
        with pytest.raises(ValueError) as e:
            ex.run()
        msg = str(e.value)
        assert KEY in msg and f"{need} bytes" in msg and "mask_gib" in msg and "shorter locate_seconds" in msg and "--mask-gib" in msg
        assert ocr.seen == []


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def test_command_line(host_stack, y4m, monkeypatch, capsys, caplog):
    name, path, data, decoded = y4m
    truth = static_clip(name)[1]
    common = ["--area", "auto", "--selector", "hold", "--batch", str(BATCH), "--edge-thresh", "auto", "--max-hold-seconds", "1.2"]

    def main(args, stdin=True):
        pipe, th = piped(data if stdin else b"", 4099)
        monkeypatch.setattr("sys.stdin", type("Stdin", (), {"buffer": pipe})())
        ocr = LookupOcr(decoded, truth, TEXT_BOX)
        cells = NumpyCellsHoldBoundedMasks()
        rc = extractor.main(args, ocr=ocr, counter=NumpyBoundedHoldCounter(), cells_fn=NumpyCellsHoldBounded(), cells_bounded_masks_fn=cells)
        pipe.close()
        th.join()
        return rc, ocr, capsys.readouterr(), cells
    # the default hold of 0.3 s is 8 frames at 25 fps, 1.2 s are 30 frames: no box and no threshold typed in, the three true intervals
    with caplog.at_level(logging.INFO, logger="vse_amd.extractor"):
        rc, ocr, out, cells = main(["-"] + common + ["--streaming-locate-bounded", "--locate-seconds", "2.8"])
    assert rc == 0 and three_true_lines(out.out, truth) and len(ocr.seen) >= len(TRUE)
    assert set(cells.cells.holds) == {(8, 30)} and cells.replayed[0][2:] == (8, 30, False)
    assert [r.getMessage() for r in caplog.records if "--streaming-locate-bounded" in r.getMessage()] == [
        "--streaming-locate-bounded: the locator bounds its runs as the selector does, --max-hold-seconds 1.2 (a policy; "
        "--locator-max-hold-seconds sets it apart)"]
    piped_text = out.out
    # the locator's own bound, and the several-pass run it equals
    rc, _ocr, out, cells = main(["-"] + common + ["--streaming-locate-bounded", "--locate-seconds", "2.8", "--locator-max-hold-seconds", "1.0"])
    assert rc == 0 and set(cells.cells.holds) == {(8, 25)} and cells.replayed[0][2:] == (8, 30, False)
    rc, _ocr, several, _cells = main([path] + common + ["--locator-automaton", "hold", "--locator-max-hold-seconds", "1.2"], stdin=False)
    assert rc == 0 and several.out.count(" --> ") == len(TRUE)
    caplog.clear()
    with caplog.at_level(logging.INFO, logger="vse_amd.extractor"):
        rc, _ocr, out, _cells = main(["-"] + common + ["--streaming-locate-bounded"])   # a pipe: what fits, at most 300 s, beyond this clip
    assert rc == 0 and out.out == several.out
    assert "--streaming-locate-bounded: the area is found on the first 300 seconds (what fits --retain-gib 4 and --mask-gib 8, at most 300)" in [
        r.getMessage() for r in caplog.records]
    rc, _ocr, out, _cells = main([path] + common + ["--streaming-locate-bounded", "--mask-gib", "1"], stdin=False)     # a file: the whole clip
    assert rc == 0 and out.out == several.out and piped_text.count(" --> ") == several.out.count(" --> ")
    no_bound = [a for a in common if a not in ("--max-hold-seconds", "1.2")]
    for bad, word in ((["-"] + common, "sub_area='auto' is not available in one pass"),
                      (["-"] + common + ["--locate-seconds", "3"], "--locate-seconds"),
                      (["-"] + common + ["--streaming-locate-bounded", "--streaming-locate"], "--streaming-locate-bounded finds the area for"),
                      (["-"] + common + ["--streaming-locate-bounded", "--streaming-locate"], "and --streaming-locate for"),
                      (["-"] + common + ["--streaming-locate-bounded", "--streaming-locate-hold"], "and --streaming-locate-hold for"),
                      (["-"] + common + ["--streaming-locate-bounded", "--streaming-locate-hold"], "give one of them"),
                      (["-"] + common + ["--streaming-locate-bounded", "--locate-seconds", "0"], "locate_seconds"),
                      (["-"] + common + ["--streaming-locate-bounded", "--locate-seconds", "2", "--mask-gib", "0.0001"], "mask_gib"),
                      (["-"] + common + ["--streaming-locate-bounded", "--locate-seconds", "2", "--retain-gib", "0.001"], "--retain-gib"),
                      (["-"] + no_bound + ["--streaming-locate-bounded"], "needs max_hold_seconds or max_hold_frames in change_params"),
                      (["-"] + no_bound + ["--streaming-locate-bounded", "--locator-max-hold-seconds", "1.2"],
                       "needs max_hold_seconds or max_hold_frames in change_params"),
                      (["-"] + common + ["--streaming-locate-hold"], "max_hold_seconds in change_params"),       # (the unbounded flag, as before)
                      (["-", "--area", "auto", "--selector", "change", "--streaming-locate-bounded"], "frame_selector='change'"),
                      (["-", "--area", "80,120,0,320"] + common[2:] + ["--streaming-locate-bounded"], "sub_area=")):
        rc, ocr, out, _cells = main(bad)
        assert rc == 2 and out.err.startswith("extractor: ") and word in out.err and ocr.seen == [], bad
    with pytest.raises(SystemExit):
        extractor.main(["--help"])
    assert "--streaming-locate-bounded" in " ".join(capsys.readouterr().out.split())
