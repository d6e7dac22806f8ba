"""Held-edge frame selection on the host: the numpy restatement of vse_frame_hold (tests/frame_hold_ref.py) whole and streamed,
frame_select.HoldFrameSelector on a clip whose textured background moves (synth.make_moving_clip), where the change selector finds
nothing, and SubtitleExtractor(frame_selector="hold") with a scripted recogniser.  CPU only."""
import numpy as np
import pytest

from frame_change_ref import NumpyCounter, counts as change_counts
from frame_hold_ref import NumpyHoldCounter, counts as hold_counts
from test_change_select import AREA, H, SCHEDULE, ScriptedOcr, W, stamped
from vse_amd import extractor, frame_select, srt, synth

A, B, C = "the quick brown fox", "seven wizards box", "near frozen lakes"
MOVING = [(None, 7), (A, 20), (B, 18), (None, 6), (C, 25), (A, 14), (None, 5)]
BAND = extractor.SubtitleArea(ymin=60, ymax=120, xmin=0, xmax=320)
HOLDS = (2, 3, 5, 8)
_cache = {}


def moving_clip():
    if "moving" not in _cache:
        _cache["moving"] = synth.make_moving_clip(MOVING)
    return _cache["moving"]


def spans(intervals):
    return [(s, e) for s, e, _r in intervals]


# ---- the reference against itself -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", (1,) + HOLDS + (32,))
def test_streaming_counter_equals_whole_clip(hold):
    frames, _ = moving_clip()
    area = (60, 120, 0, 320)
    whole = hold_counts(frames, area, 128, hold)
    assert whole.shape == (len(frames), 3)
    counter, out, fed = NumpyHoldCounter(), [], 0
    for n in (1, 2, 3, 64, len(frames) - 70):
        out.append(counter(frames[fed:fed + n], area, 128, hold, fed, False))
        assert len(out[-1]) == max(0, fed + n - hold + 1) - max(0, fed - hold + 1)
        fed += n
    assert fed == len(frames)
    out.append(counter(frames[:0], area, 128, hold, fed, True))
    assert np.array_equal(np.concatenate(out), whole)


def test_hold_one_is_the_change_selector_count():
    frames, _ = moving_clip()
    area = (60, 120, 0, 320)
    assert np.array_equal(hold_counts(frames, area, 128, 1), change_counts(frames, area, 128)[0])


def test_runs_are_cut_at_both_ends_of_the_clip():
    """One pixel, by hand: a 2-frame run at the start, a 3-frame run in the middle and a 2-frame run at the end, hold 3."""
    e = np.array([1, 1, 0, 1, 1, 1, 0, 0, 1, 1], bool).reshape(-1, 1, 1)
    from frame_hold_ref import held_masks, rows_of
    held = held_masks(e, 3)
    assert held.ravel().tolist() == [0, 0, 0, 1, 1, 1, 0, 0, 0, 0]
    assert rows_of(held).tolist() == [[0, 0, 0]] * 3 + [[1, 1, 0], [1, 0, 0], [1, 0, 0], [0, 0, 1]] + [[0, 0, 0]] * 3


# ---- the selector on a moving background ------------------------------------------------------------------------------------
def test_change_selector_finds_nothing_on_a_moving_background():
    """Why the held-edge selector exists."""
    frames, truth = moving_clip()
    assert [(s, e) for s, e, _t in truth] == [(8, 27), (28, 45), (52, 76), (77, 90)]
    assert frame_select.ChangeFrameSelector(NumpyCounter()).run(list(frames), BAND) == []


@pytest.mark.parametrize("hold", HOLDS)
def test_hold_selector_finds_the_truth_on_a_moving_background(hold):
    frames, truth = moving_clip()
    counter = NumpyHoldCounter()
    sel = frame_select.HoldFrameSelector(counter, hold_frames=hold, batch=16)
    got = sel.run(list(frames), BAND, 25.0)
    assert spans(got) == [(s, e) for s, e, _t in truth]
    assert all(r == (s + e) // 2 for s, e, r in got)
    assert sel.intervals == got and sel.counts.shape == (len(frames), 3) and sel.hold == hold
    assert counter.calls == (len(frames) + 15) // 16 + 1          # every batch once, then the flush without frames


def test_hold_frames_default_comes_from_the_frame_rate():
    frames, truth = moving_clip()
    for fps, want in ((25.0, 8), (10.0, 3), (1.0, 1), (200.0, 32)):
        sel = frame_select.HoldFrameSelector(NumpyHoldCounter())
        sel.run(list(frames[:40]), BAND, fps)
        assert sel.hold == want, fps
    with pytest.raises(ValueError):
        frame_select.HoldFrameSelector(NumpyHoldCounter(), hold_frames=33).run(list(frames[:4]), BAND, 25.0)
    assert frame_select.HoldFrameSelector(NumpyHoldCounter()).run([], BAND, 25.0) == []


@pytest.mark.parametrize("hold", (1, 2, 3, 5))
def test_hold_selector_equals_change_selector_on_a_quiet_background(hold):
    frames, _ = synth.make_clip(SCHEDULE, H, W, seed=5)
    if "quiet" not in _cache:
        _cache["quiet"] = frame_select.ChangeFrameSelector(NumpyCounter()).run(list(frames), AREA)
    assert len(_cache["quiet"]) >= 6
    assert frame_select.HoldFrameSelector(NumpyHoldCounter(), hold_frames=hold).run(list(frames), AREA, 25.0) == _cache["quiet"]


def test_a_subtitle_shorter_than_hold_is_not_found():
    """On a background without edges, where a run is as long as the subtitle.  (Over the moving texture a text edge that falls on a
    background edge of the neighbouring gap frame makes a run one frame longer: the same schedule on make_moving_clip at hold 5
    holds 75-122 pixels over frames 9..13, above the 64 of default_min_edges, and reports (9, 13) for the subtitle at 10..13.)"""
    frames, truth = synth.make_clip([(None, 9), (A, 4), (None, 9), (B, 12), (None, 6)], 120, 320, seed=1)
    both = [(s, e) for s, e, _t in truth]
    assert both[0] == (10, 13)
    for hold, want in ((3, both), (4, both), (5, both[1:])):
        assert spans(frame_select.HoldFrameSelector(NumpyHoldCounter(), hold_frames=hold).run(list(frames), BAND, 25.0)) == want, hold


def test_hold_intervals_is_change_intervals_with_the_longer_minimum():
    rows = np.array([(50, 50, 0), (50, 0, 0), (0, 0, 50), (50, 50, 0), (50, 0, 0), (50, 0, 0), (0, 0, 50)], np.int32)
    assert frame_select.hold_intervals(rows, 10, 2) == frame_select.change_intervals(rows, 10, 0.5, 2) == [(1, 2, 1), (4, 6, 5)]
    assert frame_select.hold_intervals(rows, 10, 3) == [(4, 6, 5)]
    assert frame_select.hold_intervals(rows, 10, 1, min_frames=3) == [(4, 6, 5)]


# ---- the extractor --------------------------------------------------------------------------------------------------------
class BandOcr(ScriptedOcr):
    """test_change_select's scripted recogniser with its box inside the band of the 120 x 320 clip."""

    def predict(self, img):
        boxes, res = super().predict(img)
        return ([[[40, 92], [280, 92], [280, 112], [40, 112]]] if res else []), res


@pytest.mark.parametrize("image", ["middle", "min"])
def test_extractor_hold_selector(image, monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    frames, truth = moving_clip()
    src = extractor.ArraySource(list(stamped(frames)), 25.0)
    ocr = BandOcr(truth, True)
    kw = {}
    if image != "middle":
        from interval_ref import NumpyCompositor
        kw = dict(interval_image=image, composite_params={"accumulate_fn": NumpyCompositor()})
    ex = extractor.SubtitleExtractor(src, ocr, sub_area=BAND, mode="fast", frame_selector="hold", change_counter=NumpyHoldCounter(),
                                     change_params={"hold_frames": 5}, drop_score=0.0, batch=8, **kw)
    text = ex.run()
    want = [(s, e, (s + e) // 2) for s, e, _t in truth]
    assert ex.intervals == want
    assert sorted(ocr.seen) == [r for _s, _e, r in want]                 # exactly one OCR call per interval, on its middle frame
    lines = sum((extractor.frame_lines(r, *BandOcr(truth, False).predict(src.read(r)), BAND, "ch", 0.0, 0.0) for _s, _e, r in want), [])
    assert len(lines) == len(truth)
    assert text == srt.generate_subtitle_file_intervals(lines, want, 25.0)[0]
    assert text.count(" --> ") == 4
    for s, e, _t in truth:
        assert f"{srt.frame_to_timecode(s, 25.0)} --> {srt.frame_to_timecode(e, 25.0)}" in text
    assert (ex.interval_patches is None) == (image == "middle")


def test_other_selectors_are_unchanged():
    frames, truth = moving_clip()
    src = extractor.ArraySource(list(frames), 25.0)
    with pytest.raises(ValueError):
        extractor.SubtitleExtractor(src, ScriptedOcr(truth, True), frame_selector="vsf")
    with pytest.raises(ValueError):
        extractor.SubtitleExtractor(src, ScriptedOcr(truth, True), frame_selector="fps", interval_image="min")
    ex = extractor.SubtitleExtractor(src, ScriptedOcr(truth, True), sub_area=BAND, mode="fast", change_counter=NumpyHoldCounter())
    assert ex.frame_selector == "fps" and len(ex.select_tasks()) < len(frames) and ex.intervals is None
