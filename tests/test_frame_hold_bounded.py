"""Held-edge selection with bounded runs on the host: the numpy restatement of vse_frame_hold_bounded (tests/frame_hold_bounded_ref.py)
in its mask form, its difference form and streamed; frame_select.HoldFrameSelector(max_hold_*) on clips whose busy background
stands still (synth.make_moving_clip with pan (0, 0)), where the hold selector merges subtitles and loses them; one pass against
several; the refusals and the command line.  CPU only."""
import numpy as np
import pytest

from frame_change_ref import edge_mask
from frame_hold_bounded_ref import NumpyBoundedHoldCounter, bounded_masks, counts as bounded_counts, difference_rows, emitted
from frame_hold_ref import NumpyHoldCounter, counts as hold_counts, rows_of
from test_one_pass import LookupOcr
from vse_amd import extractor, frame_select, synth

SCHEDULE = [(None, 10), ("FIRST LINE", 20), (None, 10), ("SECOND ONE", 20), ("THIRD TEXT", 20), (None, 10)]
TRUE = [(11, 30), (41, 60), (61, 80)]
BAND = extractor.SubtitleArea(ymin=75, ymax=120, xmin=0, xmax=320)       # the bottom 45 rows of the 120 x 320 clip
AREA = (75, 120, 0, 320)
# name -> (make_moving_clip's background, edge pixels of a gap frame / a frame with text, the hold selector's intervals today)
STATIC = {
    "busy": (dict(amp=(110, 60), cells=(16, 4)), (589, 1583), [(1, 10), (11, 30), (31, 40), (41, 80), (81, 90)]),
    "busier": (dict(amp=(120, 120), cells=(8, 3)), (3230, 3821), [(1, 90)]),
}
MAX_HOLD = 30
_cache = {}


def static_clip(name):
    if name not in _cache:
        frames, truth = synth.make_moving_clip(SCHEDULE, pan=(0, 0), seed=1, **STATIC[name][0])
        frames.setflags(write=False)
        _cache[name] = frames, truth
    return _cache[name]


def spans(intervals):
    return [(s, e) for s, e, _r in intervals]


# ---- the reference against itself -----------------------------------------------------------------------------------------
def test_bounded_masks_by_hand():
    """One pixel: runs of 2, 3, 5 and (cut off by the clip's end) 2 frames; hold 3, max_hold 4 keeps the run of 3 alone."""
    e = np.array([1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 1, 1, 0, 1, 1], bool).reshape(-1, 1, 1)
    assert bounded_masks(e, 3, 4).ravel().tolist() == [0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    assert bounded_masks(e, 2, 5).ravel().tolist() == [1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 1, 1, 0, 1, 1]
    assert bounded_masks(e, 1, 2).ravel().tolist() == [1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1]
    rows = rows_of(bounded_masks(e, 3, 4)).tolist()
    assert rows[3:7] == [[1, 1, 0], [1, 0, 0], [1, 0, 0], [0, 0, 1]] and not np.any(rows[:3]) and not np.any(rows[7:])
    assert emitted(0, 10, 4, False) == (0, 6) and emitted(10, 3, 4, False) == (6, 9) and emitted(13, 0, 4, True) == (9, 13)
    assert emitted(0, 3, 4, False) == (0, 0) and emitted(3, 0, 4, True) == (0, 3)


@pytest.mark.parametrize("name", list(STATIC))
@pytest.mark.parametrize("hold,max_hold", [(1, 1), (1, 30), (3, 3), (3, 30), (3, 19), (3, 20)])
def test_difference_form_equals_mask_form(name, hold, max_hold):
    """What the device computes (a difference array over the rows, filled in as runs end) is what the definition says."""
    frames, _ = static_clip(name)
    e = edge_mask(frames, AREA, 128)
    want = bounded_counts(frames, AREA, 128, hold, max_hold)
    assert np.array_equal(difference_rows(e, hold, max_hold), want)
    assert want[:, 0].max() > 0


@pytest.mark.parametrize("name", list(STATIC))
@pytest.mark.parametrize("hold", [1, 3, 8])
def test_unbounded_is_the_hold_counter(name, hold):
    frames, _ = static_clip(name)
    want = hold_counts(frames, AREA, 128, hold)
    for max_hold in (len(frames), len(frames) + 7, 4000):
        assert np.array_equal(bounded_counts(frames, AREA, 128, hold, max_hold), want)
    assert not np.array_equal(bounded_counts(frames, AREA, 128, hold, len(frames) - 1), want)       # the background's runs are the clip


@pytest.mark.parametrize("hold,max_hold", [(1, 1), (3, 5), (3, 30), (2, 200)])
def test_streaming_counter_equals_whole_clip(hold, max_hold):
    frames, _ = static_clip("busy")
    whole = bounded_counts(frames, AREA, 128, hold, max_hold)
    for sizes in ((len(frames),), (1, 2, 3, 64, 20), (7,) * 12 + (6,), (33, 57), (1,) * len(frames)):
        counter, out, fed = NumpyBoundedHoldCounter(), [], 0
        for n in sizes:
            out.append(counter(frames[fed:fed + n], AREA, 128, hold, max_hold, fed, False))
            assert len(out[-1]) == max(0, fed + n - max_hold) - max(0, fed - max_hold)
            fed += n
        assert fed == len(frames)
        out.append(counter(frames[:0], AREA, 128, hold, max_hold, fed, True))
        assert np.array_equal(np.concatenate(out), whole), sizes


# ---- the selector over a background that stands still -------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(STATIC))
@pytest.mark.parametrize("hold", [1, 3])
def test_hold_selector_loses_subtitles_over_a_static_background(name, hold):
    """The hole the option closes: static edges sit in the denominator of the cut ratio and in neither numerator."""
    frames, truth = static_clip(name)
    assert [(s, e) for s, e, _t in truth] == TRUE
    e = edge_mask(frames, AREA, 128)
    assert (int(e[0].sum()), int(e[15].sum())) == STATIC[name][1]
    got = spans(frame_select.HoldFrameSelector(NumpyHoldCounter(), hold_frames=hold).run(list(frames), BAND, 25.0))
    assert got == STATIC[name][2]
    assert len([t for t in TRUE if t in got]) < len(TRUE)


@pytest.mark.parametrize("batch", [16, 64])
@pytest.mark.parametrize("name", list(STATIC))
@pytest.mark.parametrize("hold", [1, 3])
def test_bounded_runs_find_every_true_interval(name, hold, batch):
    frames, _ = static_clip(name)
    counter = NumpyBoundedHoldCounter()
    sel = frame_select.HoldFrameSelector(counter, hold_frames=hold, max_hold_frames=MAX_HOLD, batch=batch)
    got = sel.run(list(frames), BAND, 25.0)
    for t in TRUE:
        assert t in spans(got), (t, got)                   # every true interval appears exactly
    if name == "busy":
        assert spans(got) == TRUE
    else:
        assert set(spans(got)) - set(TRUE) <= {(1, 10), (31, 40), (81, 90)}          # flicker in the gaps: OCR calls, no subtitle lost
    assert all(r == (s + e) // 2 for s, e, r in got)
    assert (sel.hold, sel.max_hold) == (hold, MAX_HOLD) and sel.intervals == got
    assert np.array_equal(sel.counts, bounded_counts(frames, AREA, 128, hold, MAX_HOLD))
    assert counter.calls == (len(frames) + batch - 1) // batch + 1          # every batch once, then the flush without frames


def test_max_hold_comes_from_the_frame_rate_or_the_frames():
    frames, _ = static_clip("busy")
    for kw, fps, want in ((dict(max_hold_seconds=12), 25.0, 300), (dict(max_hold_seconds=1.2), 25.0, 30), (dict(max_hold_seconds=15), 24.0, 360),
                          (dict(max_hold_seconds=99, max_hold_frames=30), 25.0, 30), (dict(max_hold_frames=4000), 25.0, 4000),
                          (dict(max_hold_frames=8), 25.0, 8)):
        sel = frame_select.HoldFrameSelector(NumpyBoundedHoldCounter(), **kw)
        sel.run(list(frames[:20]), BAND, fps)
        assert (sel.hold, sel.max_hold) == (round(0.3 * fps), want), kw
    sel = frame_select.HoldFrameSelector(NumpyHoldCounter())                # neither: today's path and today's count_fn contract
    sel.run(list(frames[:20]), BAND, 25.0)
    assert sel.max_hold is None and sel.engine_count_fn is frame_select.EngineHoldCounter
    assert frame_select.HoldFrameSelector(max_hold_frames=30).engine_count_fn is frame_select.EngineBoundedHoldCounter
    assert frame_select.HoldFrameSelector(NumpyBoundedHoldCounter(), max_hold_frames=30).run([], BAND, 25.0) == []


@pytest.mark.parametrize("kw", [dict(max_hold_frames=7), dict(max_hold_frames=4001), dict(max_hold_seconds=0.2), dict(max_hold_seconds=161),
                                dict(hold_frames=3, max_hold_frames=2), dict(max_hold_frames=0), dict(hold_frames=33, max_hold_frames=40)])
def test_max_hold_out_of_range_is_a_value_error(kw):
    frames, _ = static_clip("busy")
    with pytest.raises(ValueError):
        frame_select.HoldFrameSelector(NumpyBoundedHoldCounter(), **kw).run(list(frames[:4]), BAND, 25.0)


def test_change_selector_does_not_take_the_option():
    with pytest.raises(TypeError):
        frame_select.ChangeFrameSelector(max_hold_frames=30)


# ---- one pass -------------------------------------------------------------------------------------------------------------------
BOX = [[40, 79], [280, 79], [280, 116], [40, 116]]


def extract(source, frames, truth, batch, one_pass, **more):
    ocr = LookupOcr(frames, truth, BOX)
    ex = extractor.SubtitleExtractor(source, ocr, mode="fast", drop_score=0.0, batch=batch, one_pass=one_pass, sub_area=BAND,
                                     frame_selector="hold", change_counter=NumpyBoundedHoldCounter(),
                                     change_params={"hold_frames": 3, "max_hold_frames": MAX_HOLD}, **more)
    text = ex.run()
    return ex, (ex.intervals, ocr.seen, ex.raw_lines, text)


@pytest.mark.parametrize("batch", [1, 7, 64])
@pytest.mark.parametrize("name", list(STATIC))
def test_one_pass_equals_multi_pass(monkeypatch, name, batch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)          # the scripted recogniser takes the list of host frames
    frames, truth = static_clip(name)
    src = extractor.ArraySource(list(frames), 25.0)
    _, want = extract(src, frames, truth, batch, None)
    ex, got = extract(src, frames, truth, batch, True)
    assert got == want and ex.clamped_intervals == 0
    for t in TRUE:
        assert t in spans(got[0])
    assert sorted(got[1]) == [r for _s, _e, r in got[0]] and got[3].count(" --> ") == 3
    # the rows trail the frames by max_hold, and that many more frames are kept
    assert ex.peak_retained <= MAX_HOLD + 10 + 2 * batch


def test_extractor_seconds_reach_the_selector(monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    frames, truth = static_clip("busy")
    ocr = LookupOcr(frames, truth, BOX)
    ex = extractor.SubtitleExtractor(extractor.ArraySource(list(frames), 25.0), ocr, mode="fast", drop_score=0.0, sub_area=BAND,
                                     frame_selector="hold", change_counter=NumpyBoundedHoldCounter(),
                                     change_params={"hold_frames": 3, "max_hold_seconds": 1.2})
    ex.run()
    assert spans(ex.intervals) == TRUE


# ---- the command line -----------------------------------------------------------------------------------------------------------
def test_command_line_flag(monkeypatch, tmp_path, capsys):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    frames, truth = static_clip("busy")
    path, out = str(tmp_path / "clip.npy"), str(tmp_path / "out.srt")
    np.save(path, frames)                                  # a frame stack: the clip's own bytes, no colour conversion in between
    decoded = frames
    common = [path, "--fps", "25", "--area", "75,120,0,320", "--batch", "16", "-o", out]
    # at 25 fps the default hold is 8 frames; 1.2 s are 30
    ocr = LookupOcr(decoded, truth, BOX)
    assert extractor.main(common + ["--selector", "hold", "--max-hold-seconds", "1.2"], ocr=ocr, counter=NumpyBoundedHoldCounter()) == 0
    bounded = open(out).read()
    assert bounded.count(" --> ") == 3 and sorted(ocr.seen) == [(s + e) // 2 for s, e in TRUE]
    ocr = LookupOcr(decoded, truth, BOX)
    assert extractor.main(common + ["--selector", "hold"], ocr=ocr, counter=NumpyHoldCounter()) == 0           # without it: one merged
    assert open(out).read() != bounded
    capsys.readouterr()
    for bad in (["--max-hold-seconds", "1.2"], ["--selector", "change", "--max-hold-seconds", "1.2"],
                ["--selector", "hold", "--max-hold-seconds", "0.1"], ["--selector", "hold", "--max-hold-seconds", "200"]):
        ocr = LookupOcr(decoded, truth, BOX)
        assert extractor.main(common + bad, ocr=ocr, counter=NumpyBoundedHoldCounter()) == 2, bad
        assert capsys.readouterr().err.startswith("extractor: ") and ocr.seen == []
    with pytest.raises(SystemExit):
        extractor.main(["--help"])
    assert "--max-hold-seconds" in capsys.readouterr().out
