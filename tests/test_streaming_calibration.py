"""The edge threshold chosen in the selector's own pass, on the host: frame_select.CalibratingChangeSelector against AreaLocator's
calibration pass followed by ChangeFrameSelector, SubtitleExtractor with area_params={"streaming": True} in several passes (E1) and in
one pass over a pipe (E2) against the several-pass run without the key, what one pass keeps while the threshold is open (E3), a clip
without subtitles, every refusal, and the command line.  CPU only: the numpy cells and counters (tests/edge_calibrate_ref.py,
tests/frame_change_ref.py) on the calibration tests' clips of little contrast, and a scripted recogniser."""
import logging

import numpy as np
import pytest

import frame_change_ref as FC
from area_clip import FPS, H, LOCATOR, W, decorated_clip
from edge_calibrate_ref import NumpyCellsMulti, low_contrast, noisy_low_contrast
from frame_change_ref import NumpyCounter
from test_one_pass import LookupOcr, piped, text_box
from vse_amd import area_locator, extractor, frame_select, ingest, synth

THS = area_locator.AUTO_THRESHOLDS
BAND = extractor.SubtitleArea(ymin=300, ymax=H, xmin=0, xmax=W)
BATCH = 8
KEY = "area_params={'streaming': True}"


class NumpyCellsCounts:
    """cells_fn of CalibratingChangeSelector on the host: NumpyCellsMulti's totals, and per threshold the counts of
    frame_change_ref over the same frames; `export` hands a threshold's last mask to a NumpyCounter."""

    def __init__(self):
        self.multi, self.prev, self.frames, self.exported = NumpyCellsMulti(), None, 0, []

    def __call__(self, frames, area, params, reset, flush, thresholds):
        totals = self.multi(frames, area, params, reset, flush, thresholds=thresholds)
        if reset or self.prev is None:
            self.prev = [None] * len(thresholds)
        rows = []
        if frames is not None and len(frames):
            self.frames += len(frames)
            for q, th in enumerate(thresholds):
                c, self.prev[q] = FC.counts(np.asarray(frames), area, th, self.prev[q])
                rows.append(c)
        return totals, np.stack(rows, 1) if rows else np.zeros((0, len(thresholds), 3), np.int32)

    def export(self, area, q, counter):
        self.exported.append(q)
        counter.prev = self.prev[q]


@pytest.fixture(scope="module")
def clip():
    frames, truth = decorated_clip()
    frames.setflags(write=False)
    return frames, truth


@pytest.fixture(scope="module")
def low(clip):
    frames = low_contrast(clip[0])
    frames.setflags(write=False)
    return frames


@pytest.fixture
def host_stack(monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)          # the scripted recogniser takes the list of host frames


# ---- the selector ---------------------------------------------------------------------------------------------------------------------
def two_passes(frames, window, batch=BATCH):
    """The calibration pass over the first `window` frames, then the plain selector at its choice -> (locator, selector)."""
    loc = area_locator.AreaLocator(NumpyCellsMulti(), edge_thresh="auto", search_area=BAND, batch=batch,
                                   probe=None if window is None else (1, window), **LOCATOR)
    loc.run(list(frames), FPS)
    sel = frame_select.ChangeFrameSelector(NumpyCounter(), edge_thresh=128 if loc.edge_thresh is None else loc.edge_thresh, batch=batch)
    sel.run(list(frames), BAND, FPS)
    return loc, sel


@pytest.mark.parametrize("kind", ["low", "noisy"])
@pytest.mark.parametrize("window", [None, 30, 32, 66, 100, 1])
def test_selector_equals_the_calibration_pass_and_the_plain_selector(clip, low, kind, window):
    frames = low if kind == "low" else noisy_low_contrast(clip[0])
    loc, plain = two_passes(frames, window)
    cells, counter = NumpyCellsCounts(), NumpyCounter()
    sel = frame_select.CalibratingChangeSelector(counter, cells, window=window, locator_params=LOCATOR, batch=BATCH)
    seen, yielded = 0, []
    for items, closed in sel.iter_run(list(frames), BAND, FPS):
        seen += len(items)
        decided_at = min(window or len(frames), len(frames))
        if seen < decided_at or (window is None and items):
            assert closed == [] and sel.tracker is None and not sel.decided and len(sel.trackers) == len(THS)
        yielded += closed
    assert sel.decided and sel.tracker is sel.trackers[sel.chosen] and cells.exported == [sel.chosen]
    assert sel.frames_scanned == loc.frames_scanned == min(window or 66, 66) and cells.frames == sel.frames_scanned
    assert np.array_equal(sel.totals, loc.totals) and sel.scores == loc.scores
    assert sel.edge_thresh == (128 if loc.edge_thresh is None else loc.edge_thresh)
    assert sel.intervals == yielded == plain.intervals and np.array_equal(sel.counts, plain.counts)
    # the plain counter ran on the frames behind the window only: once per batch that reaches beyond it
    assert counter.calls == sum(1 for first in range(0, 66, BATCH) if min(first + BATCH, 66) > sel.frames_scanned)
    if window != 1:
        assert sel.edge_thresh == (32 if kind == "low" else 48) and len(sel.intervals) == len(clip[1])


def test_selector_arguments():
    with pytest.raises(ValueError, match="window"):
        frame_select.CalibratingChangeSelector(NumpyCounter(), NumpyCellsCounts(), window=0)
    with pytest.raises(ValueError, match="must contain 128"):
        frame_select.CalibratingChangeSelector(NumpyCounter(), NumpyCellsCounts(), locator_params={"thresholds": (32, 64)})
    with pytest.raises(ValueError, match="automaton"):
        frame_select.CalibratingChangeSelector(NumpyCounter(), NumpyCellsCounts(), locator_params={"automaton": "hold"})
    sel = frame_select.CalibratingChangeSelector(NumpyCounter(), NumpyCellsCounts(), window=5)
    assert sel.run([], BAND, FPS) == [] and sel.edge_thresh is None and not sel.decided


# ---- the extractor --------------------------------------------------------------------------------------------------------------------
class CountingSource(extractor.ArraySource):
    """ArraySource that counts how often the clip is decoded from its start."""
    passes = 0

    def frames(self):
        self.passes += 1
        return super().frames()


def make(source, decoded, truth, key, one_pass=None, cells=None, batch=BATCH, **area_params):
    ocr = LookupOcr(decoded, truth, text_box(BAND))
    own = {"streaming": True, "cells_counts_fn": cells or NumpyCellsCounts()} if key else {"cells_fn": NumpyCellsMulti()}
    ex = extractor.SubtitleExtractor(source, ocr, sub_area=BAND, mode="fast", frame_selector="change", change_counter=NumpyCounter(),
                                     drop_score=0.0, batch=batch, one_pass=one_pass, change_params={"edge_thresh": "auto"},
                                     area_params={**own, **LOCATOR, **area_params})
    return ex, ocr


def results(ex, ocr):
    text = ex.run()
    return ex.edge_thresh, ex.intervals, ocr.seen, ex.raw_lines, text


@pytest.mark.parametrize("kind", ["low", "noisy"])
def test_e1_several_passes_equal_the_run_without_the_key_and_save_a_decode(host_stack, clip, low, kind):
    frames = low if kind == "low" else noisy_low_contrast(clip[0])
    truth = clip[1]
    src = CountingSource(list(frames), FPS)
    want = results(*make(src, frames, truth, key=False))
    passes_without = src.passes
    src = CountingSource(list(frames), FPS)
    ex, ocr = make(src, frames, truth, key=True)
    assert ex.edge_thresh is None and not ex.one_pass
    got = results(ex, ocr)
    assert got == want and got[0] == (32 if kind == "low" else 48)
    assert len(got[1]) == len(truth) and got[4].count(" --> ") == len(truth) and all(t in got[4] for _s, _e, t in truth)
    assert src.passes == passes_without - 1 == 1
    assert ex.frames_calibrated == 66 and ex.edge_scores[THS.index(got[0])] > 0


@pytest.fixture(scope="module")
def y4m(low, tmp_path_factory):
    """The low-contrast clip as a YUV4MPEG2 file -> (its bytes, the frames a reader decodes from them)."""
    path = str(tmp_path_factory.mktemp("calib") / "low.y4m")
    ingest.write_y4m(path, [ingest.bgr_to_yuv420(f) for f in low], FPS)
    src = ingest.Y4mSource(path)
    decoded = list(src.frames())
    src.close()
    with open(path, "rb") as fp:
        return path, fp.read(), decoded


@pytest.mark.parametrize("seconds,window", [(3.0, 30), (3.2, 32), (10.0, 100)])       # inside a batch, at a batch's end, beyond the clip
def test_e2_one_pass_over_a_pipe_equals_several_passes_with_that_probe(host_stack, clip, y4m, seconds, window):
    path, data, decoded = y4m
    truth = clip[1]
    src = ingest.Y4mSource(path)
    want = results(*make(src, decoded, truth, key=False, probe=(1, window)))
    src.close()
    pipe, th = piped(data, 65536)
    stream = ingest.Y4mStream(pipe)
    ex, ocr = make(stream, decoded, truth, key=True, calibrate_seconds=seconds)
    got = results(ex, ocr)
    th.join()
    pipe.close()
    assert ex.one_pass and ex.clamped_intervals == 0 and stream.frame_count == len(decoded)
    assert got == want and got[0] in THS and got[0] < 96
    assert len(got[1]) == len(truth) and got[4].count(" --> ") == len(truth)
    assert ex.frames_calibrated == min(window, len(decoded))
    # a seekable source forced into one pass takes the same road
    ex, ocr = make(extractor.ArraySource(list(decoded), FPS), decoded, truth, key=True, one_pass=True, calibrate_seconds=seconds)
    assert results(ex, ocr)[:4] == want[:4]                      # (the SRT's times: an array source has no timestamps of its own)


@pytest.mark.parametrize("batch", [1, 8])
def test_e3_the_window_keeps_no_more_than_the_candidates_may_want(host_stack, clip, low, batch):
    """While the threshold is open a frame stays for as long as any candidate's rule wants it: per candidate the frames at or behind
    the middle of its open run and the middle frames of the intervals it has closed.  The union is at most the sum over the
    candidates, computed here from the selector's own trackers batch by batch, plus the batch that has just arrived."""
    truth = clip[1]
    sel = frame_select.CalibratingChangeSelector(NumpyCounter(), NumpyCellsCounts(), window=None, locator_params=LOCATOR, batch=batch)
    allowed, bound, union_peak = 0, 0, 0
    for items, _closed in sel.iter_run(list(low), BAND, FPS):
        bound = max(bound, allowed + len(items))
        if items:
            t = sel.trackers[0].fed
            halves = [0 if tr.open_start is None else t - (tr.open_start + t) // 2 + 1 for tr in sel.trackers]
            allowed = sum(halves) + sum(len(p) for p in sel.pending)
            union_peak = max(union_peak, max(halves))
    ex, ocr = make(extractor.ArraySource(list(low), FPS), low, truth, key=True, one_pass=True, batch=batch, calibrate_seconds=100.0)
    got = results(ex, ocr)
    assert len(got[1]) == len(truth) and ex.clamped_intervals == 0
    assert union_peak <= ex.peak_retained <= bound, (union_peak, ex.peak_retained, bound)
    # ... and once the threshold is decided, what only the other thresholds wanted goes: a short window ends below the whole-clip one
    short, ocr = make(extractor.ArraySource(list(low), FPS), low, truth, key=True, one_pass=True, batch=batch, calibrate_seconds=2.0)
    assert results(short, ocr)[1:] == got[1:] or short.edge_thresh != ex.edge_thresh
    assert short.peak_retained <= ex.peak_retained


def test_retain_bytes_stays_the_fallback_in_the_window(host_stack, clip, low, caplog):
    truth = clip[1]
    ex, ocr = make(extractor.ArraySource(list(low), FPS), low, truth, key=True, one_pass=True, calibrate_seconds=100.0)
    ex.retain_bytes = 1
    with caplog.at_level(logging.WARNING, logger="vse_amd.extractor"):
        ex.run()
    want, _ocr = make(extractor.ArraySource(list(low), FPS), low, truth, key=True, one_pass=True, calibrate_seconds=100.0)
    want.run()
    assert [(s, e) for s, e, _r in ex.intervals] == [(s, e) for s, e, _r in want.intervals]      # the times are untouched
    assert ex.clamped_intervals >= 1 and ex.peak_retained <= 2 * BATCH
    assert len([r for r in caplog.records if "retain_bytes" in r.getMessage()]) == 1


def test_a_clip_without_subtitles_warns_once_and_goes_on_at_128(host_stack, caplog):
    frames, truth = synth.make_clip([(None, 20)], 120, W, seed=3)
    band = extractor.SubtitleArea(ymin=60, ymax=120, xmin=0, xmax=W)
    for one_pass in (None, True):
        caplog.clear()
        ocr = LookupOcr(frames, truth, text_box(band))
        ex = extractor.SubtitleExtractor(extractor.ArraySource(list(frames), FPS), ocr, sub_area=band, mode="fast", frame_selector="change",
                                         change_counter=NumpyCounter(), drop_score=0.0, batch=BATCH, one_pass=one_pass,
                                         change_params={"edge_thresh": "auto"},
                                         area_params={"streaming": True, "calibrate_seconds": 1.0, "cells_counts_fn": NumpyCellsCounts(), **LOCATOR})
        with caplog.at_level(logging.WARNING):
            text = ex.run()
        fallbacks = [r for r in caplog.records if "edge_thresh='auto'" in r.getMessage() and "128" in r.getMessage()]
        assert len(fallbacks) == 1 and "in 10 frames" in fallbacks[0].getMessage()
        assert ex.edge_thresh == 128 and ex.intervals == [] and text == "" and ex.frames_calibrated == 10


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def build(one_pass=None, area_params=None, **kw):
    frames = np.zeros((4, 16, 16, 3), np.uint8)
    args = dict(sub_area=BAND, frame_selector="change", change_params={"edge_thresh": "auto"}, one_pass=one_pass,
                area_params={"streaming": True, **(area_params or {})})
    args.update(kw)
    return extractor.SubtitleExtractor(extractor.ArraySource(list(frames), FPS), LookupOcr([], [], None), **args)


@pytest.mark.parametrize("names,kw", [
    (["frame_selector='hold'"], dict(frame_selector="hold")),
    (["automaton='hold'"], dict(area_params={"automaton": "hold"})),
    (["max_hold_seconds"], dict(area_params={"automaton": "change", "max_hold_seconds": 12})),
    (["max_hold_frames"], dict(area_params={"max_hold_frames": 100})),
    (["sub_area='auto'"], dict(sub_area="auto")),
    (["interval_frame='sharpest'"], dict(interval_frame="sharpest")),
    (["composite_params={'streaming': True}"], dict(interval_image="min", composite_params={"streaming": True})),
    (["shard=(0, 2)"], dict(shard=(0, 2))),
    (["probe"], dict(area_params={"probe": (1, 20)})),
    (["sub_area=None"], dict(sub_area=None)),
    (["mode='accurate'"], dict(mode="accurate")),
])
def test_the_key_refuses_what_needs_the_threshold_from_the_first_frame(names, kw):
    with pytest.raises(ValueError) as e:
        build(**kw)
    assert KEY in str(e.value) and "does not combine with" in str(e.value) and all(n in str(e.value) for n in names)


def test_the_key_and_its_window_mean_nothing_alone():
    with pytest.raises(ValueError, match=r"area_params=\{'streaming': True\} .* means\s+nothing without it"):
        build(change_params={"edge_thresh": 64})
    with pytest.raises(ValueError, match=r"area_params=\{'streaming': True\} .* means\s+nothing without it"):
        build(change_params=None)
    for own in ("calibrate_seconds", "cells_counts_fn", "export_fn"):
        with pytest.raises(ValueError, match=rf"area_params: \['{own}'\] belong to area_params=\{{'streaming': True\}} and mean nothing without it"):
            build(area_params={"streaming": False, own: 3.0})
    with pytest.raises(ValueError, match="calibrate_seconds must be positive"):
        build(area_params={"calibrate_seconds": 0})
    with pytest.raises(ValueError, match="in one pass needs calibrate_seconds: the window bounds the frames kept while eight thresholds are undecided"):
        build(one_pass=True)
    build(one_pass=True, area_params={"calibrate_seconds": 5})                        # accepted
    build()                                                                          # several passes: the whole clip decides


def test_without_the_key_the_old_refusals_stay_word_for_word():
    frames = np.zeros((4, 16, 16, 3), np.uint8)
    src = extractor.ArraySource(list(frames), FPS)
    for area_params in (None, {}, {"streaming": False}, {"min_seconds": 0.5}):
        with pytest.raises(ValueError, match=r"edge_thresh='auto' is not available in one pass \(a sequential source, or one_pass=True\): "
                                             "it needs a second look at frames already gone"):
            extractor.SubtitleExtractor(src, LookupOcr([], [], None), sub_area=BAND, frame_selector="change",
                                        change_params={"edge_thresh": "auto"}, one_pass=True, area_params=area_params)
    with pytest.raises(ValueError, match="edge_thresh must be an integer or 'auto'"):
        extractor.SubtitleExtractor(src, LookupOcr([], [], None), sub_area=BAND, frame_selector="change", change_params={"edge_thresh": "best"})


# ---- the command line -----------------------------------------------------------------------------------------------------------------
def test_command_line(host_stack, clip, y4m, monkeypatch, capsys):
    path, data, decoded = y4m
    truth = clip[1]
    area = f"{BAND.ymin},{BAND.ymax},{BAND.xmin},{BAND.xmax}"
    common = ["--area", area, "--selector", "change", "--batch", str(BATCH)]

    def main(args, stdin=True):
        pipe, th = piped(data if stdin else b"", 4099)
        monkeypatch.setattr("sys.stdin", type("Stdin", (), {"buffer": pipe})())
        ocr = LookupOcr(decoded, truth, text_box(BAND))
        rc = extractor.main(args, ocr=ocr, counter=NumpyCounter(), cells_fn=NumpyCellsMulti(), cells_counts_fn=NumpyCellsCounts())
        pipe.close()
        th.join()
        return rc, ocr, capsys.readouterr()
    rc, _ocr, several = main([path] + common + ["--edge-thresh", "auto"], stdin=False)            # two passes, the whole clip decides
    assert rc == 0 and several.out.count(" --> ") == len(truth)
    rc, ocr, out = main(["-"] + common + ["--edge-thresh", "auto", "--streaming-calibration"])   # a pipe: 300 s, beyond this clip
    assert rc == 0 and out.out == several.out and len(ocr.seen) == len(truth)
    rc, _ocr, out = main([path] + common + ["--edge-thresh", "auto", "--streaming-calibration"], stdin=False)     # a file: the whole clip
    assert rc == 0 and out.out == several.out
    src = ingest.Y4mSource(path)
    want = results(*make(src, decoded, truth, key=False, probe=(1, 30)))[4]
    src.close()
    rc, _ocr, out = main(["-"] + common + ["--edge-thresh", "auto", "--streaming-calibration", "--calibrate-seconds", "3"])
    assert rc == 0 and out.out == want
    for bad, word in ((["-"] + common + ["--edge-thresh", "auto", "--calibrate-seconds", "3"], "--calibrate-seconds"),
                      (["-"] + common + ["--streaming-calibration"], "edge_thresh"),
                      (["-"] + common + ["--edge-thresh", "auto", "--streaming-calibration", "--calibrate-seconds", "0"], "calibrate_seconds"),
                      (["-", "--area", area, "--selector", "hold", "--edge-thresh", "auto", "--streaming-calibration"], "frame_selector='hold'"),
                      (["-"] + common + ["--edge-thresh", "auto"], "edge_thresh='auto' is not available in one pass")):
        rc, ocr, out = main(bad)
        assert rc == 2 and out.err.startswith("extractor: ") and word in out.err and ocr.seen == [], bad
    with pytest.raises(SystemExit):
        extractor.main(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--streaming-calibration" in text and "a policy, not a measurement" in text
