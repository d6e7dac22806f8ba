"""The streaming quantile on the host: frame_select.StreamingQuantile, driven by the numpy restatement of the ring and of
vse_interval_ring_rank (tests/interval_ring_ref.py, whose ring raises on a frame that is not there), gives the patches of
IntervalQuantile.run under every selector lag, batch, quantile and sample count; the rule for an interval that reaches back beyond the
ring, with its sample numbers written out; SubtitleExtractor with interval_image="quantile" and composite_params={"streaming": True,
"ring_seconds": S} (the ring is granted explicitly: the streaming key alone stays the error tests/test_interval_stream.py holds it to be)
equals the several-pass quantile run in several passes, in one pass and over a pipe; what it refuses; the command line.  CPU only:
numpy counters and a scripted recogniser."""
import logging

import numpy as np
import pytest

import interval_rank_ref
import interval_ring_ref
from frame_change_ref import NumpyCounter
from frame_hold_bounded_ref import NumpyBoundedHoldCounter
from frame_hold_ref import NumpyHoldCounter
from test_frame_hold import BAND
from test_interval_stream import AreaOcr, ScriptedRows, extract, host_stack, kind_kwargs, same_pictures  # noqa: F401 (host_stack: a fixture)
from test_one_pass import AREA, FPS, clip, piped
from vse_amd import engine, extractor, frame_select, ingest

SMALL = extractor.SubtitleArea(ymin=2, ymax=6, xmin=1, xmax=9)
QUANTILES, SAMPLES, TRIM = (0, 0.5, 1), (1, 2, 5, 15, 63), 0.2


def test_the_reference_speaks_the_library_s_numbers():
    assert (interval_ring_ref.MAX_GROUPS, interval_ring_ref.RANK_MAX) == (engine.INTERVAL_RING_MAX_GROUPS, engine.INTERVAL_RANK_MAX)
    ring = interval_ring_ref.Ring(3)
    frames = np.arange(5 * 2 * 2 * 3, dtype=np.uint8).reshape(5, 2, 2, 3)
    ring.store(frames, 0)                                  # frames 1..5 pass; 3, 4, 5 remain
    assert np.array_equal(ring.rank([([3, 4, 5], 1)], 5)[0], frames[3])
    assert np.array_equal(ring.rank([([3, 5], 0, 2)], 5)[2], frames[2])
    for bad in ([([2, 3], 0)], [([3, 3], 0)], [([4, 3], 0)], [([5, 6], 0)], [([3], 1)], [([3], -1)], [([], 0)], [([3], 0, -1)]):
        with pytest.raises(ValueError):
            ring.rank(bad, 5)
    with pytest.raises(LookupError):
        ring.rank([([6], 0)], 6)                           # inside the window, but never stored


# ---- the planner against the second pass ----------------------------------------------------------------------------------------
class FanOut:
    """A selector's `compositor` that hands every call to several: one selector run serves all quantiles and sample counts."""

    def __init__(self, comps):
        self.comps = comps

    def begin(self, fps, lag):
        for c in self.comps:
            c.begin(fps, lag)

    def __call__(self, *args):
        for c in self.comps:
            c(*args)


def selector(kind, batch, comp):
    if kind == "change":
        return frame_select.ChangeFrameSelector(NumpyCounter(), batch=batch, compositor=comp), AREA, 0
    if kind == "hold":
        return frame_select.HoldFrameSelector(NumpyHoldCounter(), hold_frames=3, batch=batch, compositor=comp), BAND, 2
    return frame_select.HoldFrameSelector(NumpyBoundedHoldCounter(), hold_frames=3, max_hold_frames=30, batch=batch, compositor=comp), BAND, 30


_second_pass = {}


def second_pass(kind, intervals, frames, area, quantile, samples):
    """IntervalQuantile.run over NumpyRanker: computed once per case and shared between the batch sizes (the intervals are the same)."""
    key = (kind, quantile, samples)
    if key not in _second_pass:
        want = frame_select.IntervalQuantile(interval_rank_ref.NumpyRanker(), quantile=quantile, samples=samples, trim_seconds=TRIM,
                                             batch=64).run(list(frames), area, intervals, FPS)
        for p in want.values():
            p.setflags(write=False)
        _second_pass[key] = (list(intervals), want)
    assert _second_pass[key][0] == list(intervals)
    return _second_pass[key][1]


@pytest.mark.parametrize("batch", [1, 7, 64, 100])
@pytest.mark.parametrize("kind", ["change", "hold", "bounded"])
def test_streamed_quantiles_equal_the_second_pass(kind, batch):
    frames, truth = clip("change" if kind == "change" else "hold")
    cases = [(q, k) for q in QUANTILES for k in SAMPLES]
    fns = [interval_ring_ref.NumpyRingRanker() for _ in cases]
    comps = [frame_select.StreamingQuantile(fn, quantile=q, samples=k, trim_seconds=TRIM, ring_seconds=5.0, batch=batch)
             for fn, (q, k) in zip(fns, cases)]
    sel, area, lag = selector(kind, batch, FanOut(comps))
    intervals = sel.run(list(frames), area, fps=FPS)
    assert len(intervals) >= 3 and sel._lag() == lag
    for (q, k), comp, fn in zip(cases, comps, fns):
        want = second_pass(kind, intervals, frames, area, q, k)
        assert sorted(comp.patches) == sorted(want) == [r for _s, _e, r in intervals], (kind, batch, q, k)
        for r in want:
            assert comp.patches[r].dtype == np.uint8 and np.array_equal(comp.patches[r], want[r]), (kind, batch, q, k, r)
        assert comp.cap == int(round(5.0 * FPS)) + int(round(TRIM * FPS)) + lag + batch + 1
        assert 0 < comp.peak_ring <= comp.cap and comp.clamped == 0
        assert sum(n for n, _g in fn.calls) == len(frames) and fn.max_groups <= engine.INTERVAL_RING_MAX_GROUPS
        y0, y1, x0, x1 = comp.area
        assert (y0, y1 - y0, x0, x1) == (0, int(area.ymax - area.ymin), int(area.xmin), int(area.xmax))


def short_subtitles(n, every):
    rows = np.tile(np.array([[120, 0, 0]], np.int32), (n, 1))
    rows[::every, 1:] = 100                                # a cut before every `every`-th frame
    return rows


@pytest.mark.parametrize("kind", ["change", "bounded"])
def test_more_closings_in_a_batch_than_one_call_takes(kind):
    rng = np.random.default_rng(11)
    n = 150
    rows = short_subtitles(n, 3)
    frames = rng.integers(0, 256, size=(n, 7, 10, 3), dtype=np.uint8)
    fn = interval_ring_ref.NumpyRingRanker()
    comp = frame_select.StreamingQuantile(fn, quantile=0.5, samples=5, trim_seconds=0.0, ring_seconds=4.0, batch=100)
    kw = dict(min_edges=40, change_ratio=0.5, min_frames=1, batch=100, compositor=comp)
    if kind == "change":
        sel = frame_select.ChangeFrameSelector(ScriptedRows(rows, 0), **kw)
    else:
        sel = frame_select.HoldFrameSelector(ScriptedRows(rows, 20), hold_frames=2, max_hold_frames=20, **kw)
    intervals = sel.run(list(frames), SMALL, fps=1.0)
    assert len(intervals) == n // 3 and all(e - s == 2 for s, e, _r in intervals)
    want = frame_select.IntervalQuantile(interval_rank_ref.NumpyRanker(), quantile=0.5, samples=5, trim_seconds=0.0).run(
        list(frames), SMALL, intervals, 1.0)
    assert sorted(comp.patches) == sorted(want) and all(np.array_equal(comp.patches[r], want[r]) for r in want)
    # the first batch closes far more than 8 intervals: they go in calls of 8 groups, of which only the first stores
    per_batch = [c for c in fn.calls if c[0]]
    assert [c[0] for c in per_batch] == [100, 50] and fn.max_groups == 8 and len(fn.calls) >= 2 + (n // 3) // 8
    assert all(g for k, (stored, g) in enumerate(fn.calls) if not stored) and comp.peak_ring <= comp.cap and comp.clamped == 0


# ---- an interval that reaches back beyond the ring ------------------------------------------------------------------------------
def long_subtitle_rows():
    """35 frames: a gap, 3..6, a gap, 8..27 (longer than the ring), a gap, 29..33, a gap."""
    rows = np.zeros((35, 3), np.int32)
    for s, e in ((3, 6), (8, 27), (29, 33)):
        rows[s - 1:e, 0] = 120
    return rows, [(3, 6, 4), (8, 27, 17), (29, 33, 31)]


@pytest.mark.parametrize("samples, named", [(5, [19, 21, 23, 25, 27]), (1, [19]), (63, list(range(19, 28)))])
def test_an_interval_longer_than_the_ring_is_sampled_over_what_is_left(samples, named, caplog):
    """Change selector (no lag), batch 4, no trim, ring_seconds 5 at 1 fps: cap = 5 + 0 + 0 + 4 + 1 = 10.  The subtitle 8..27 closes with
    the row of frame 28, in the batch 25..28, after which the ring holds 19..28: its 20 frames are sampled over 19..27 instead,
    K = min(samples, 9) frames 19 + (i * 8) // (K - 1); with one sample, the ring frame nearest to the middle frame 17."""
    rows, truth = long_subtitle_rows()
    rng = np.random.default_rng(3)
    frames = rng.integers(0, 256, size=(len(rows), 7, 10, 3), dtype=np.uint8)
    fn = interval_ring_ref.NumpyRingRanker()
    comp = frame_select.StreamingQuantile(fn, quantile=0.5, samples=samples, trim_seconds=0.0, ring_seconds=5.0, batch=4)
    sel = frame_select.ChangeFrameSelector(ScriptedRows(rows, 0), min_edges=40, change_ratio=0.5, min_frames=2, batch=4, compositor=comp)
    with caplog.at_level(logging.WARNING, logger=frame_select.__name__):
        assert sel.run(list(frames), SMALL, fps=1.0) == truth
    assert comp.cap == 10 and comp.clamped == 1 and comp.peak_ring == 10
    warnings = [r for r in caplog.records if r.levelno == logging.WARNING]
    assert len(warnings) == 1 and "8..27" in warnings[0].getMessage() and "ring" in warnings[0].getMessage()
    box = (2, 6, 1, 9)
    rank = frame_select.quantile_rank(0.5, len(named))
    assert np.array_equal(comp.patches[17], interval_rank_ref.rank(frames[[f - 1 for f in named]], box, rank))
    want = frame_select.IntervalQuantile(interval_rank_ref.NumpyRanker(), quantile=0.5, samples=samples, trim_seconds=0.0).run(
        list(frames), SMALL, truth, 1.0)
    assert np.array_equal(comp.patches[4], want[4]) and np.array_equal(comp.patches[31], want[31])       # the others are exact
    if samples > 1:
        assert not np.array_equal(comp.patches[17], want[17])
    # a second clip through the same object starts afresh: the count, and the warning
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger=frame_select.__name__):
        sel.run(list(frames), SMALL, fps=1.0)
    assert comp.clamped == 1 and len([r for r in caplog.records if r.levelno == logging.WARNING]) == 1


def test_two_clamped_intervals_make_one_warning(caplog):
    rows = np.zeros((60, 3), np.int32)
    rows[2:25, 0] = rows[27:55, 0] = 120
    frames = np.random.default_rng(4).integers(0, 256, size=(60, 7, 10, 3), dtype=np.uint8)
    comp = frame_select.StreamingQuantile(interval_ring_ref.NumpyRingRanker(), samples=5, trim_seconds=0.0, ring_seconds=5.0, batch=4)
    sel = frame_select.ChangeFrameSelector(ScriptedRows(rows, 0), min_edges=40, min_frames=2, batch=4, compositor=comp)
    with caplog.at_level(logging.WARNING, logger=frame_select.__name__):
        assert [(s, e) for s, e, _r in sel.run(list(frames), SMALL, fps=1.0)] == [(3, 25), (28, 55)]
    assert comp.clamped == 2 and len([r for r in caplog.records if r.levelno == logging.WARNING]) == 1


def test_value_errors_and_asserts():
    fn = interval_ring_ref.NumpyRingRanker()
    for kw in (dict(quantile=-0.01), dict(quantile=1.01), dict(samples=0), dict(samples=64), dict(ring_seconds=-1.0)):
        with pytest.raises(ValueError, match="StreamingQuantile"):
            frame_select.StreamingQuantile(fn, **kw)
    frame_select.StreamingQuantile(fn, quantile=1, samples=63, batch=8, ring_seconds=0)          # the limits themselves
    # a selector whose batches are larger than the ring was sized for is a mistake of the caller's, caught on the first batch
    comp = frame_select.StreamingQuantile(fn, batch=4)
    sel = frame_select.ChangeFrameSelector(ScriptedRows(np.zeros((9, 3), np.int32), 0), min_edges=40, batch=8, compositor=comp)
    with pytest.raises(AssertionError, match="StreamingQuantile"):
        sel.run(list(np.zeros((9, 7, 10, 3), np.uint8)), SMALL, fps=1.0)
    # rows that trail by more than the lag the compositor was told
    comp = frame_select.StreamingQuantile(fn, batch=8)
    sel = frame_select.ChangeFrameSelector(ScriptedRows(np.zeros((30, 3), np.int32), 2), min_edges=40, batch=8, compositor=comp)
    with pytest.raises(AssertionError, match="StreamingQuantile"):
        sel.run(list(np.zeros((30, 7, 10, 3), np.uint8)), SMALL, fps=1.0)


# ---- the extractor ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [7, 64])
@pytest.mark.parametrize("kind", ["change", "hold"])
def test_extractor_streaming_quantile_equals_the_quantile_pass(host_stack, kind, batch):  # noqa: F811
    frames, truth = clip(kind)
    src = extractor.ArraySource(list(frames), FPS)
    want_ex, want_ocr, want = extract(src, frames, truth, kind, batch, None, "quantile",
                                      {"rank_fn": interval_rank_ref.NumpyRanker(), "samples": 5, "trim_seconds": 0.2})
    assert [(s, e) for s, e, _r in want[0]] == [(s, e) for s, e, _t in truth] and want[3].count(" --> ") >= 2
    assert any(not np.array_equal(want_ocr.shown[r], frames[r - 1][want_ocr.y0:want_ocr.y1]) for _s, _e, r in want[0])
    for one_pass in (False, True):
        fn = interval_ring_ref.NumpyRingRanker()
        ex, ocr, got = extract(src, frames, truth, kind, batch, one_pass, "quantile",
                               {"streaming": True, "ring_fn": fn, "samples": 5, "trim_seconds": 0.2, "ring_seconds": 10.0, "keep_patches": True})
        assert ex.one_pass == one_pass and ex.streaming and got == want and fn.calls
        assert ex.clamped_intervals == 0 and ex.clamped_quantiles == 0
        same_pictures(ex, ocr, want_ex, want_ocr)
    # one pass drops a picture once its frame has been recognised, unless told to keep it; several passes keep them
    params = {"streaming": True, "ring_fn": interval_ring_ref.NumpyRingRanker(), "samples": 5, "trim_seconds": 0.2, "ring_seconds": 60}
    ex, ocr, got = extract(src, frames, truth, kind, batch, True, "quantile", params)
    assert got == want and ex.interval_patches is None and all(np.array_equal(ocr.shown[r], want_ocr.shown[r]) for r in ocr.shown)
    ex, ocr, got = extract(src, frames, truth, kind, batch, False, "quantile", params)
    assert got == want
    same_pictures(ex, ocr, want_ex, want_ocr)


def test_extractor_counts_the_clamped_quantiles(host_stack):  # noqa: F811
    """ring_seconds 0 at batch 1: cap = 0 + 3 + 0 + 1 + 1 = 5 frames, shorter than the clip's subtitles (7 to 9 frames, 3 to 5 trimmed)."""
    frames, truth = clip("change")
    src = extractor.ArraySource(list(frames), FPS)
    ex, _ocr, got = extract(src, frames, truth, "change", 1, True, "quantile",
                            {"streaming": True, "ring_fn": interval_ring_ref.NumpyRingRanker(), "samples": 15, "ring_seconds": 0})
    _want_ex, _want_ocr, want = extract(src, frames, truth, "change", 1, True, "middle", None)
    assert ex.clamped_quantiles >= 1 and got[0] == want[0] and got[1] == want[1]          # intervals and frames recognised are untouched


@pytest.mark.parametrize("kind", ["change", "hold"])
def test_extractor_streaming_quantile_over_a_piped_stream(host_stack, tmp_path, kind):  # noqa: F811
    frames, truth = clip(kind)
    path = str(tmp_path / "clip.y4m")
    ingest.write_y4m(path, [ingest.bgr_to_yuv420(f) for f in frames], FPS)
    src = ingest.Y4mSource(path)
    decoded = list(src.frames())
    want_ex, want_ocr, want = extract(src, decoded, truth, kind, 7, None, "quantile", {"rank_fn": interval_rank_ref.NumpyRanker(), "samples": 5})
    with open(path, "rb") as fp:
        data = fp.read()
    pipe, th = piped(data, 65536)
    stream = ingest.Y4mStream(pipe)
    ex, ocr, got = extract(stream, decoded, truth, kind, 7, None, "quantile",
                           {"streaming": True, "ring_fn": interval_ring_ref.NumpyRingRanker(), "samples": 5, "ring_seconds": 60, "keep_patches": True})
    th.join()
    pipe.close()
    src.close()
    assert ex.one_pass and got == want and stream.frame_count == len(frames) and got[3].count(" --> ") >= 2
    same_pictures(ex, ocr, want_ex, want_ocr)


def test_refusals_and_unknown_keys():
    frames, _truth = clip("change")
    src = extractor.ArraySource(list(frames), FPS)
    base = dict(sub_area=AREA, frame_selector="change", interval_image="quantile")
    on = {"streaming": True, "ring_seconds": 30}
    for one_pass in (False, True):
        # the ring is device memory the caller grants: without ring_seconds the streaming key stays the error it was
        for params in ({"streaming": True}, {"streaming": True, "samples": 5, "ring_fn": None, "keep_patches": True}):
            with pytest.raises(ValueError) as e:
                extractor.SubtitleExtractor(src, None, one_pass=one_pass, composite_params=params, **base)
            assert all(w in str(e.value) for w in ("streaming", "quantile", "ring_seconds")), str(e.value)
        ex = extractor.SubtitleExtractor(src, None, one_pass=one_pass, composite_params={
            **on, "quantile": 0.25, "samples": 7, "trim_seconds": 0.1, "ring_fn": None, "keep_patches": True}, **base)
        assert ex.streaming and ex.keep_patches and ex.one_pass == one_pass and ex.clamped_quantiles == 0
        assert ex.composite_params == {"quantile": 0.25, "samples": 7, "trim_seconds": 0.1, "ring_seconds": 30, "ring_fn": None}
        for more, words in ((dict(interval_text="fused"), ("streaming", "fused")), (dict(shard=(0, 2)), ("streaming", "shard")),
                            (dict(interval_frame="sharpest"), ("sharpest", "quantile"))):
            with pytest.raises(ValueError) as e:
                extractor.SubtitleExtractor(src, None, one_pass=one_pass, composite_params=on, **base, **more)
            assert all(w in str(e.value) for w in words), str(e.value)
        for key in ("stream_fn", "rank_fn", "mode", "accumulate_fn", "batch"):
            with pytest.raises(ValueError) as e:
                extractor.SubtitleExtractor(src, None, one_pass=one_pass, composite_params={**on, key: None}, **base)
            assert str(e.value) == ("composite_params={'streaming': True} with interval_image='quantile' takes quantile, samples, trim_seconds, "
                                    f"ring_seconds, ring_fn and keep_patches beside it, not ['{key}']")
        # the ring's keys stay with the quantile: the min / max / mean pictures refuse them in the words they had
        for key in ("ring_fn", "ring_seconds", "samples"):
            with pytest.raises(ValueError) as e:
                extractor.SubtitleExtractor(src, None, one_pass=one_pass, composite_params={"streaming": True, key: None},
                                            **{**base, "interval_image": "min"})
            assert str(e.value) == f"composite_params={{'streaming': True}} takes trim_seconds, stream_fn and keep_patches beside it, not ['{key}']"
    # without the key: one pass refuses the quantile in the words it had, and the ring's keys mean nothing
    with pytest.raises(ValueError) as e:
        extractor.SubtitleExtractor(src, None, one_pass=True, **base)
    assert str(e.value) == ("interval_image='quantile' is not available in one pass (a sequential source, or one_pass=True): it needs a "
                            "second look at frames already gone")
    for key in ("ring_fn", "ring_seconds", "keep_patches"):
        with pytest.raises(ValueError) as e:
            extractor.SubtitleExtractor(src, None, composite_params={key: None}, **base)
        assert "streaming" in str(e.value) and key in str(e.value)
    with pytest.raises(ValueError, match="samples"):
        extractor.SubtitleExtractor(src, None, composite_params={**on, "samples": 64}, **base)._interval_selector()


def test_command_line_streaming_quantile(host_stack, tmp_path, monkeypatch, capsys):  # noqa: F811
    frames, truth = clip("change")
    path, out = str(tmp_path / "clip.y4m"), str(tmp_path / "out.srt")
    ingest.write_y4m(path, [ingest.bgr_to_yuv420(f) for f in frames], FPS)
    src = ingest.Y4mSource(path)
    decoded = list(src.frames())
    _want_ex, want_ocr, want = extract(src, decoded, truth, "change", 8, None, "quantile",
                                       {"rank_fn": interval_rank_ref.NumpyRanker(), "samples": 5, "quantile": 0.25})
    src.close()
    with open(path, "rb") as fp:
        data = fp.read()
    area = f"{AREA.ymin},{AREA.ymax},{AREA.xmin},{AREA.xmax}"

    def main(args, **fns):
        pipe, th = piped(data, 4099)
        monkeypatch.setattr("sys.stdin", type("Stdin", (), {"buffer": pipe})())
        ocr = AreaOcr(decoded, truth, AREA)
        rc = extractor.main(args, ocr=ocr, counter=NumpyCounter(), **fns)
        pipe.close()
        th.join()
        return rc, ocr
    common = ["--area", area, "--selector", "change", "--batch", "8", "-o", out]
    flags = ["--interval-image", "quantile", "--streaming-composite", "--interval-samples", "5", "--quantile", "0.25"]
    for video, more in (("-", []), (path, []), ("-", ["--ring-seconds", "10"])):       # a pipe: one pass; a file: several passes
        fn = interval_ring_ref.NumpyRingRanker()
        rc, ocr = main([video] + flags + more + common, ring_fn=fn)
        assert rc == 0 and ocr.seen == want[1] and open(out).read() == want[3] and fn.calls and want[3].count(" --> ") >= 2
        assert all(np.array_equal(ocr.shown[r], want_ocr.shown[r]) for r in want[1])
        assert fn.ring.cap == int(round((10 if more else 60) * FPS)) + 3 + 0 + 8 + 1
    capsys.readouterr()
    fn = interval_ring_ref.NumpyRingRanker()
    for bad, fns, word in ((["-", "--interval-image", "quantile", "--interval-samples", "5"] + common, {}, "second look"),
                           (["-", "--ring-seconds", "10", "--interval-image", "quantile"] + common, {}, "--ring-seconds"),
                           (["-", "--ring-seconds", "10", "--interval-image", "min", "--streaming-composite"] + common, {}, "--ring-seconds"),
                           (["-"] + flags + ["--ring-seconds", "-1"] + common, {}, "ring_seconds"),
                           (["-"] + flags[:2] + ["--interval-samples", "64"] + common, {}, "samples"),
                           (["-"] + flags[:2] + ["--quantile", "2"] + common, {}, "quantile"),
                           (["-"] + flags + common, {"stream_fn": fn}, "stream_fn"),
                           (["-"] + flags + common, {"composite_fn": fn}, "composite_fn"),
                           (["-"] + flags + ["--interval-frame", "sharpest"] + common, {}, "sharpest")):
        rc, ocr = main(bad, ring_fn=fn, **fns)
        err = capsys.readouterr().err
        assert rc == 2 and err.startswith("extractor: ") and word in err and ocr.seen == [] and not fn.calls, (bad, err)
    with pytest.raises(SystemExit):
        extractor.main(["--help"])
    text = capsys.readouterr().out
    assert "--ring-seconds" in text and "(not in one pass) [middle]" not in " ".join(text.split())
