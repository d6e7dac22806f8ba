"""interval_frame="sharpest" on the host: frame_select.sharpest_rep, the selectors' focus_fn (tests/frame_focus_ref.py restates
vse_frame_focus in numpy), SubtitleExtractor in several passes on a clip whose middle frame is degraded, one pass against several passes
(intervals, frames recognised, raw.txt lines, SRT), what one pass keeps of a long run, the refused combinations and the command line.
CPU only: numpy counters and a scripted recogniser."""
import logging

import numpy as np
import pytest

from frame_change_ref import NumpyCounter
from frame_focus_ref import NumpyFocus, focus as ref_focus
from frame_hold_ref import NumpyHoldCounter
from test_one_pass import AREA, FPS, HOLD, LookupOcr, clip, piped, text_box
from test_frame_hold import BAND
from vse_amd import extractor, frame_select, ingest, synth

TRIM = 3                      # round(0.25 s * 12 fps)
_cache = {}


def degraded_clip():
    """test_one_pass's change clip (intervals of 9, 7 and 8 frames) with the middle frame of the first interval at 70 % contrast inside the
    subtitle area: the text's 255 against its black outline becomes 178, still an edge at the threshold of 128.
    -> (frames, truth, number of the degraded frame)."""
    if "degraded" not in _cache:
        frames, truth = clip("change")
        frames = frames.copy()
        s, e, _text = truth[0]
        mid = (s + e) // 2
        band = frames[mid - 1, AREA.ymin:AREA.ymax].astype(np.float32) * 0.7
        frames[mid - 1, AREA.ymin:AREA.ymax] = band.astype(np.uint8)
        _cache["degraded"] = (frames, truth, mid)
    return _cache["degraded"]


def area_of(a, frames):
    return frame_select.clip_area(a, *frames.shape[1:3])


# ---- sharpest_rep ---------------------------------------------------------------------------------------------------------------
def rows_of(column):
    return np.stack([np.zeros(len(column), np.int64), np.asarray(column, np.int64)], 1)


def test_sharpest_rep_trims_both_ends():
    col = [0] * 40
    col[9], col[12], col[28], col[30] = 900, 50, 70, 800          # frames 10, 13, 29, 31
    # interval 10..31 at 12 fps: the candidates are 13..28, so the two sharpest frames, inside the trim, do not count
    assert frame_select.trim_range(10, 31, FPS, 0.25) == (13, 28)
    assert frame_select.sharpest_rep(10, 31, rows_of(col), FPS) == 13
    col[27] = 60                                                   # frame 28, the last candidate
    assert frame_select.sharpest_rep(10, 31, rows_of(col), FPS) == 28
    assert frame_select.sharpest_rep(10, 31, rows_of(col), FPS, trim_seconds=0) == 10
    assert frame_select.sharpest_rep(10, 31, rows_of(col), FPS, trim_seconds=0.1) == 29         # a trim of one frame: 11..30
    assert frame_select.sharpest_rep(10, 31, col, FPS) == 28                                     # the focus column alone


def test_sharpest_rep_of_a_short_run_is_its_middle():
    col = [5, 90, 10, 20, 30, 95, 7]
    # 2..6: shorter than two trims of 3 frames, an even span: the middle frame alone remains, whatever the others score
    assert frame_select.trim_range(2, 6, FPS, 0.25) == (4, 4)
    assert frame_select.sharpest_rep(2, 6, rows_of(col), FPS) == 4 == (2 + 6) // 2
    # 2..5: an odd span leaves the two frames around the middle, the sharper of which is taken
    assert frame_select.trim_range(2, 5, FPS, 0.25) == (3, 4)
    assert frame_select.sharpest_rep(2, 5, rows_of(col), FPS) == 4
    assert frame_select.sharpest_rep(1, 2, rows_of(col), FPS) == 2


def test_sharpest_rep_ties_zero_and_one_frame():
    col = [0, 0, 7, 9, 9, 9, 3, 0, 0, 0]
    assert frame_select.sharpest_rep(1, 10, rows_of(col), FPS) == 4                  # candidates 4..7: the earliest of the equals
    assert frame_select.sharpest_rep(1, 10, rows_of([0] * 10), FPS) == 4            # every focus 0: the first candidate
    assert frame_select.sharpest_rep(1, 10, rows_of([0] * 10), FPS, trim_seconds=0) == 1
    assert frame_select.sharpest_rep(6, 6, rows_of(col), FPS) == 6                   # an interval of one frame
    assert frame_select.sharpest_rep(8, 8, rows_of(col), FPS) == 8


# ---- the selectors' focus_fn ------------------------------------------------------------------------------------------------------
def selector(kind, batch, focus_fn):
    if kind == "hold":
        return frame_select.HoldFrameSelector(NumpyHoldCounter(), hold_frames=HOLD, batch=batch, focus_fn=focus_fn), BAND
    return frame_select.ChangeFrameSelector(NumpyCounter(), batch=batch, focus_fn=focus_fn), AREA


@pytest.mark.parametrize("kind", ["change", "hold"])
def test_selector_focus_has_one_row_per_frame_fed(kind):
    frames, _truth = clip(kind)
    whole = None
    for batch in (64, 7, 1):
        nf = NumpyFocus()
        sel, area = selector(kind, batch, nf)
        plain, _ = selector(kind, batch, None)
        want_intervals = plain.run(list(frames), area, FPS)
        if whole is None:
            whole, _ = ref_focus(frames, area_of(area, frames), 128)
            assert whole[:, 1].max() > 0 and whole.dtype == np.int64
        fed = 0
        for items, _closed in sel.iter_run(list(frames), area, FPS):
            fed += len(items)
            assert sel.focus.shape == (fed, 2) and sel.focus.dtype == np.int64          # focus rows do not trail the frames ...
            assert np.array_equal(sel.focus, whole[:fed])
            if kind == "hold" and items:
                assert sel.tracker.fed == max(0, fed - (HOLD - 1))                       # ... as the hold selector's counts do
        assert np.array_equal(sel.focus, whole) and fed == len(frames)                    # batch splits give the same rows
        assert sel.intervals == want_intervals and np.array_equal(sel.counts, plain.counts)
        n = len(frames)
        assert nf.calls == [(min(batch, n - i), i == 0) for i in range(0, n, batch)]      # once per batch, reset on the first


def test_without_focus_fn_no_call_is_made(monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    frames, truth = clip("change")
    sel = frame_select.ChangeFrameSelector(NumpyCounter(), batch=8)
    sel.run(list(frames), AREA, FPS)
    assert sel.focus_fn is None and not hasattr(sel, "focus")
    nf = NumpyFocus()
    ex = extractor.SubtitleExtractor(extractor.ArraySource(list(frames), FPS), LookupOcr(frames, truth, text_box(AREA)), sub_area=AREA,
                                     frame_selector="change", change_counter=NumpyCounter(), drop_score=0.0, frame_params={"focus_fn": nf})
    ex.run()
    assert ex.interval_frame == "middle" and nf.calls == [] and ex.focus is None
    assert [r for _s, _e, r in ex.intervals] == [(s + e) // 2 for s, e, _t in truth]


# ---- the extractor ----------------------------------------------------------------------------------------------------------------
def kwargs_of(kind):
    if kind == "hold":
        return dict(sub_area=BAND, frame_selector="hold", change_counter=NumpyHoldCounter(), change_params={"hold_frames": HOLD})
    return dict(sub_area=AREA, frame_selector="change", change_counter=NumpyCounter())


def run(source, frames, truth, kind, batch, one_pass, interval_frame="sharpest", **more):
    kw = {**kwargs_of(kind), **more}
    ocr = LookupOcr(frames, truth, text_box(kw["sub_area"]))
    ex = extractor.SubtitleExtractor(source, ocr, mode="fast", drop_score=0.0, batch=batch, one_pass=one_pass, interval_frame=interval_frame,
                                     frame_params={"focus_fn": NumpyFocus()}, **kw)
    text = ex.run()
    return ex, (ex.intervals, ocr.seen, ex.raw_lines, text)


@pytest.fixture
def host_stack(monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)          # the scripted recogniser takes the list of host frames


def test_extractor_avoids_the_degraded_middle_frame(host_stack):
    frames, truth, bad = degraded_clip()
    clean, _ = clip("change")
    src = extractor.ArraySource(list(frames), FPS)
    # preconditions: the degraded frame changes no interval, and its focus is strictly the smallest of its trimmed range
    want_intervals = frame_select.ChangeFrameSelector(NumpyCounter()).run(list(clean), AREA)
    assert frame_select.ChangeFrameSelector(NumpyCounter()).run(list(frames), AREA) == want_intervals
    assert [(s, e) for s, e, _r in want_intervals] == [(s, e) for s, e, _t in truth] and want_intervals[0][2] == bad
    whole, _ = ref_focus(frames, area_of(AREA, frames), 128)
    s, e, _text = truth[0]
    first, last = frame_select.trim_range(s, e, FPS, 0.25)
    assert (first, last) == (s + TRIM, e - TRIM) and first < bad < last
    assert all(whole[bad - 1, 1] < whole[k - 1, 1] for k in range(first, last + 1) if k != bad)

    _, (intervals, seen, _raw, text) = run(src, frames, truth, "change", 8, False, "middle")
    assert intervals == want_intervals and seen[0] == bad
    ex, (intervals, seen, raw, text2) = run(src, frames, truth, "change", 8, False)
    assert np.array_equal(ex.focus, whole)
    assert [(s, e) for s, e, _r in intervals] == [(s, e) for s, e, _r in want_intervals]
    assert [r for _s, _e, r in intervals] == [frame_select.sharpest_rep(s, e, whole, FPS, 0.25) for s, e, _r in intervals] == seen
    assert seen[0] != bad and first <= seen[0] <= last
    assert text2 == text and text.count(" --> ") == len(truth)                          # the scripted recogniser reads every frame alike
    # trim_seconds travels through frame_params
    ex = extractor.SubtitleExtractor(src, LookupOcr(frames, truth, text_box(AREA)), drop_score=0.0, interval_frame="sharpest",
                                     frame_params={"focus_fn": NumpyFocus(), "trim_seconds": 0.0}, **kwargs_of("change"))
    ex.run()
    assert [r for _s, _e, r in ex.intervals] == [frame_select.sharpest_rep(s, e, whole, FPS, 0.0) for s, e, _r in ex.intervals]


def test_auto_edge_thresh_reaches_the_focus_in_several_passes(host_stack):
    from edge_calibrate_ref import NumpyCellsMulti
    frames, truth, _bad = degraded_clip()
    nf = NumpyFocus()
    seen = []
    ex = extractor.SubtitleExtractor(extractor.ArraySource(list(frames), FPS), LookupOcr(frames, truth, text_box(AREA)), sub_area=AREA,
                                     frame_selector="change", change_counter=NumpyCounter(), drop_score=0.0, interval_frame="sharpest",
                                     change_params={"edge_thresh": "auto"}, area_params={"cells_fn": NumpyCellsMulti()},
                                     frame_params={"focus_fn": lambda f, a, th, r: (seen.append(th), nf(f, a, th, r))[1]})
    ex.run()
    assert isinstance(ex.edge_thresh, int) and ex.edge_thresh != 128 and set(seen) == {ex.edge_thresh}
    whole, _ = ref_focus(frames, area_of(AREA, frames), ex.edge_thresh)
    assert np.array_equal(ex.focus, whole)


@pytest.mark.parametrize("batch", [1, 3, 4, 8])
@pytest.mark.parametrize("route", ["one_pass", "pipe"])
@pytest.mark.parametrize("kind", ["change", "hold"])
def test_one_pass_equals_several_passes(host_stack, tmp_path, kind, route, batch):
    frames, truth = degraded_clip()[:2] if kind == "change" else clip("hold")
    if route == "one_pass":
        src = extractor.ArraySource(list(frames), FPS)
        decoded = frames
        _, want = run(src, decoded, truth, kind, batch, False)
        ex, got = run(src, decoded, truth, kind, batch, True)
    else:
        path = str(tmp_path / "clip.y4m")
        ingest.write_y4m(path, [ingest.bgr_to_yuv420(f) for f in frames], FPS)
        src = ingest.Y4mSource(path)
        decoded = list(src.frames())
        _, want = run(src, decoded, truth, kind, batch, None)
        with open(path, "rb") as fp:
            data = fp.read()
        pipe, th = piped(data, 65536)
        ex, got = run(ingest.Y4mStream(pipe), decoded, truth, kind, batch, None)
        th.join()
        pipe.close()
        src.close()
    assert ex.one_pass and got == want and ex.clamped_intervals == 0
    intervals, seen, _raw, text = got
    assert [(s, e) for s, e, _r in intervals] == [(s, e) for s, e, _t in truth] and text.count(" --> ") >= 2
    assert seen == [r for _s, _e, r in intervals] == [frame_select.sharpest_rep(s, e, ex.focus, FPS, 0.25) for s, e, _r in intervals]
    assert seen != [(s + e) // 2 for s, e, _r in intervals]                             # the choice does differ from the middle frames


# ---- what one pass keeps ----------------------------------------------------------------------------------------------------------
def test_a_long_run_keeps_two_trims_and_the_batches_not_half_the_run(host_stack, caplog):
    batch, run_len = 4, 200
    frames, truth = synth.make_clip([(None, 2), ("the quick brown fox", run_len), (None, 3)], 120, 320, seed=3)
    (s, e, _t), = truth
    src = extractor.ArraySource(list(frames), FPS)
    area = extractor.SubtitleArea(60, 120, 0, 320)
    _, want = run(src, frames, truth, "change", batch, False, sub_area=area)
    ex, got = run(src, frames, truth, "change", batch, True, sub_area=area)
    assert got == want and ex.clamped_intervals == 0
    assert ex.peak_retained <= 2 * TRIM + 1 + 2 * batch, ex.peak_retained
    ex, _ = run(src, frames, truth, "change", batch, True, "middle", sub_area=area)
    assert ex.peak_retained > 50 and ex.clamped_intervals == 0                          # about half the run
    # room for 40 frames clamps the middle frame and not the sharpest one
    room = 40 * frames[0].nbytes
    with caplog.at_level(logging.WARNING, logger="vse_amd.extractor"):
        ex, got = run(src, frames, truth, "change", batch, True, sub_area=area, retain_bytes=room)
    assert got == want and ex.clamped_intervals == 0 and not [r for r in caplog.records if "retain_bytes" in r.getMessage()]
    with caplog.at_level(logging.WARNING, logger="vse_amd.extractor"):
        ex, got = run(src, frames, truth, "change", batch, True, "middle", sub_area=area, retain_bytes=room)
    assert ex.clamped_intervals == 1 and ex.intervals[0][2] > (s + e) // 2
    assert len([r for r in caplog.records if "retain_bytes" in r.getMessage()]) == 1


class ScriptedRows:
    """A count_fn or focus_fn that hands out prepared rows, as many as it is given frames."""

    def __init__(self, rows):
        self.rows, self.at = np.asarray(rows), 0

    def __call__(self, frames, area, edge_thresh, reset):
        self.at = 0 if reset else self.at
        out = self.rows[self.at:self.at + len(frames)]
        self.at += len(frames)
        return out


def test_retention_keeps_the_offline_choice_on_random_runs(host_stack):
    """Random runs, gaps, cuts, focus columns with many ties, trims and batch sizes, scripted through the selector: one pass recognises the
    frames the several-pass run chooses, never clamps, and never holds more than two trims, one frame and two batches."""
    rng = np.random.default_rng(2024)
    area = extractor.SubtitleArea(0, 5, 0, 5)
    longest = 0
    for case in range(300):
        fps = float(rng.choice([1, 4, 12, 24]))                                  # trims of 0, 1, 3 and 6 frames
        trim = int(round(0.25 * fps))
        batch = int(rng.integers(1, 10))
        rows = []
        while len(rows) < 150:
            run_len = int(rng.choice([1, 2, 3, 2 * trim, 2 * trim + 1, int(rng.integers(1, 70))]))
            rows += [(100, 100, 100)] + [(100, 0, 0)] * max(0, run_len - 1)          # a cut (everything changed), then a run that holds
            rows += [(0, 0, 100)] * int(rng.choice([0, 0, 1, 3]))                    # back to back, or a gap
        n = len(rows)
        focus = np.stack([np.zeros(n, np.int64), rng.integers(0, int(rng.choice([2, 4, 1000])), size=n)], 1)
        frames = np.zeros((n, 5, 5, 3), np.uint8)
        frames[:, 0, 0, 0], frames[:, 0, 0, 1] = np.arange(n) % 256, np.arange(n) // 256          # every frame its own bytes
        src = extractor.ArraySource(list(frames), fps)
        runs = []
        for one_pass in (False, True):
            ocr = LookupOcr(frames, [(1, n, "text")], text_box(extractor.SubtitleArea(0, 12, 0, 300)))
            ex = extractor.SubtitleExtractor(src, ocr, sub_area=area, frame_selector="change", change_counter=ScriptedRows(rows), drop_score=0.0,
                                             batch=batch, one_pass=one_pass, interval_frame="sharpest", frame_params={"focus_fn": ScriptedRows(focus)})
            ex.run()
            runs.append((ex.intervals, ocr.seen))
        assert runs[0] == runs[1], case
        assert runs[0][1] == [frame_select.sharpest_rep(s, e, focus, fps) for s, e, _r in runs[0][0]]
        assert ex.clamped_intervals == 0 and ex.peak_retained <= 2 * trim + 1 + 2 * batch, (case, ex.peak_retained, trim, batch)
        longest = max(longest, max(e - s + 1 for s, e, _r in runs[0][0]))
    assert longest > 60


# ---- refusals and the command line ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option,kw", [("frame_selector", dict(frame_selector="fps")),
                                        ("interval_image", dict(frame_selector="change", interval_image="min")),
                                        ("interval_image", dict(frame_selector="hold", interval_image="quantile")),
                                        ("interval_text", dict(frame_selector="change", interval_text="fused"))])
def test_refused_combinations_name_both_options(option, kw):
    frames, truth = clip("change")
    src = extractor.ArraySource(list(frames), FPS)
    with pytest.raises(ValueError) as e:
        extractor.SubtitleExtractor(src, LookupOcr([], truth, None), sub_area=AREA, interval_frame="sharpest", **kw)
    assert "interval_frame" in str(e.value) and option in str(e.value)
    extractor.SubtitleExtractor(src, LookupOcr([], truth, None), sub_area=AREA, **kw)             # accepted with the middle frame, as before
    with pytest.raises(ValueError, match="interval_frame"):
        extractor.SubtitleExtractor(src, LookupOcr([], truth, None), sub_area=AREA, frame_selector="change", interval_frame="best")
    with pytest.raises(ValueError, match="frame_params"):
        extractor.SubtitleExtractor(src, LookupOcr([], truth, None), sub_area=AREA, frame_selector="change", interval_frame="sharpest",
                                    frame_params={"samples": 3})


def test_command_line_flag(host_stack, tmp_path, monkeypatch, capsys):
    frames, truth, bad = degraded_clip()
    path, out = str(tmp_path / "clip.y4m"), str(tmp_path / "out.srt")
    ingest.write_y4m(path, [ingest.bgr_to_yuv420(f) for f in frames], FPS)
    src = ingest.Y4mSource(path)
    decoded = list(src.frames())
    _, want = run(src, decoded, truth, "change", 8, None)
    with open(path, "rb") as fp:
        data = fp.read()
    area = f"{AREA.ymin},{AREA.ymax},{AREA.xmin},{AREA.xmax}"

    def main(args):
        pipe, th = piped(data, 4099)
        monkeypatch.setattr("sys.stdin", type("Stdin", (), {"buffer": pipe})())
        ocr = LookupOcr(decoded, truth, text_box(AREA))
        rc = extractor.main(args, ocr=ocr, counter=NumpyCounter(), focus_fn=NumpyFocus())
        pipe.close()
        th.join()
        return rc, ocr
    rc, ocr = main(["-", "--area", area, "--selector", "change", "--batch", "8", "--interval-frame", "sharpest", "-o", out])
    assert rc == 0 and ocr.seen == want[1] and open(out).read() == want[3]
    assert ocr.seen != [(s + e) // 2 for s, e, _t in truth]
    rc, ocr = main(["-", "--area", area, "--selector", "change", "--batch", "8", "--interval-frame", "middle", "-o", out])
    assert rc == 0 and ocr.seen == [(s + e) // 2 for s, e, _t in truth]
    capsys.readouterr()
    for bad_args in (["--selector", "fps"], ["--selector", "change", "--interval-image", "min"],
                     ["--selector", "hold", "--interval-image", "quantile"]):
        rc, ocr = main([path, "--area", area, "--interval-frame", "sharpest"] + bad_args)
        err = capsys.readouterr().err
        assert rc == 2 and err.startswith("extractor: ") and "interval_frame" in err and ocr.seen == [], bad_args
    with pytest.raises(SystemExit):
        extractor.main(["-", "--interval-frame", "best"])
    assert "--interval-frame" in capsys.readouterr().err
    src.close()
