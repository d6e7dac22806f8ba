"""The locator and the threshold calibration on bounded runs, on the host: the numpy restatement of vse_frame_cells_hold_bounded
(tests/area_cells_hold_bounded_ref.py) whole and streamed, area_locator.AreaLocator(automaton="hold", max_hold_frames=...) on clips whose
busy background stands still (where the held automaton finds no area, or a wrong one, and no threshold), SubtitleExtractor with
area_params={"automaton": "hold", "max_hold_frames": ...} and a scripted recogniser, the refusals and the command lines.  CPU only."""
import json

import numpy as np
import pytest

import area_cells_ref as R
from area_cells_hold_bounded_ref import NumpyCellsHoldBounded, bounded_cell_counts, clip_totals_hold_bounded
from area_cells_hold_ref import NumpyCellsHold, clip_totals_hold
from frame_hold_bounded_ref import NumpyBoundedHoldCounter, counts as bounded_counts
from test_change_select import stamped
from test_frame_hold import BandOcr
from test_frame_hold_bounded import SCHEDULE, TRUE
from vse_amd import area_locator, extractor, synth

FPS = 25.0
WHOLE = (0, 120, 0, 320)
TEXT_BOX = (90, 110, 20, 300)             # make_moving_clip: one line of height 20, centred, 10 pixels above the bottom edge
P = R.Params(edge_thresh=128, min_edges=16, ratio_num=1, ratio_den=2, min_frames=8, max_frames=500)
# make_moving_clip's background with pan (0, 0): a texture that stands still behind the subtitles
STATIC = {"busier": dict(amp=(120, 120), cells=(8, 3)), "loud": dict(amp=(250, 250), cells=(8, 3))}
_cache = {}


def static_clip(name):
    if name not in _cache:
        frames, truth = synth.make_moving_clip(SCHEDULE, pan=(0, 0), seed=1, **STATIC[name])
        frames.setflags(write=False)
        _cache[name] = frames, truth
    return _cache[name]


def noisy_clip():
    """The "busier" clip with seeded noise on every byte: pixels near the threshold flicker, so there are runs of every short length
    (the synthetic clip alone has none shorter than a subtitle)."""
    if "noisy" not in _cache:
        frames, _ = static_clip("busier")
        noise = np.random.default_rng(7).integers(-24, 25, frames.shape)
        _cache["noisy"] = np.clip(frames.astype(np.int64) + noise, 0, 255).astype(np.uint8)
        _cache["noisy"].setflags(write=False)
    return _cache["noisy"]


def as_tuple(a):
    return None if a is None else (a.ymin, a.ymax, a.xmin, a.xmax)


def contains_text(a):
    return a is not None and a.ymin <= TEXT_BOX[0] and TEXT_BOX[1] <= a.ymax and a.xmin <= TEXT_BOX[2] and TEXT_BOX[3] <= a.xmax


# ---- the reference against itself -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold,max_hold", [(1, 1), (3, 5), (3, 30), (2, 200)])
@pytest.mark.parametrize("batch", (1, 7, 64, 65, 90))
def test_streaming_cells_equal_the_whole_clip(hold, max_hold, batch):
    frames = noisy_clip()
    area = (76, 120, 0, 320)
    p = P._replace(min_frames=max(3, hold))
    whole = clip_totals_hold_bounded(frames, area, p, hold, max_hold)
    cells, fed = NumpyCellsHoldBounded(), 0
    checks = 0
    while fed < len(frames):
        got = cells(frames[fed:fed + batch], area, p, fed == 0, False, hold=hold, max_hold=max_hold)
        fed = min(len(frames), fed + batch)
        if checks < 3 or fed == len(frames):               # (the whole-clip reference is the slow side)
            assert np.array_equal(got, clip_totals_hold_bounded(frames[:fed], area, p, hold, max_hold, flush=False)), fed
            checks += 1
    assert np.array_equal(cells(None, area, p, False, True, hold=hold, max_hold=max_hold), whole)
    assert whole.shape == (6, 5, 4) and whole[..., 2].max() > 0
    # the rows of all calls together are the clip's rows, each exactly once
    assert np.array_equal(np.concatenate(cells.rows[0]), bounded_cell_counts(frames, area, p.edge_thresh, hold, max_hold))


def test_two_thresholds_side_by_side():
    frames, _ = static_clip("busier")
    area = (76, 120, 0, 320)
    both = NumpyCellsHoldBounded()(frames, area, P, True, True, thresholds=(96, 128), hold=3, max_hold=30)
    assert np.array_equal(both[1], clip_totals_hold_bounded(frames, area, P, 3, 30))
    assert np.array_equal(both[0], clip_totals_hold_bounded(frames, area, P._replace(edge_thresh=96), 3, 30))
    assert not np.array_equal(both[0], both[1])


@pytest.mark.parametrize("name", sorted(STATIC))
def test_unbounded_is_the_held_cells(name):
    frames, _ = static_clip(name)
    area = (76, 120, 0, 320)
    for hold in (1, 3, 8):
        for max_hold in (len(frames), 4000):
            assert np.array_equal(clip_totals_hold_bounded(frames, area, P, hold, max_hold), clip_totals_hold(frames, area, P, hold))
    assert not np.array_equal(clip_totals_hold_bounded(frames, area, P, 3, 30), clip_totals_hold(frames, area, P, 3))


@pytest.mark.parametrize("hold,max_hold", [(1, 1), (3, 5), (3, 30), (2, 200)])
def test_cell_rows_sum_to_the_selectors_rows(hold, max_hold):
    frames, _ = static_clip("loud")
    for area in (WHOLE, (76, 120, 3, 290)):
        assert np.array_equal(bounded_cell_counts(frames, area, 128, hold, max_hold).sum((1, 2)),
                              bounded_counts(frames, area, 128, hold, max_hold))


def test_one_cell_by_hand():
    """A 3 x 3 region has one interior pixel, hence one cell: an edge in frames 1-2, 4-6 and 8-12 of fourteen, runs of 2, 3 and 5
    frames.  Runs of 3..4 frames: frames 4-6 alone.  Runs of 2..3: frames 1-2 and 4-6.  Runs of 1..5: all three."""
    edge = np.zeros((3, 3, 3), np.uint8)
    edge[:, 2] = 255
    frames = np.stack([edge if e else np.zeros_like(edge) for e in (1, 1, 0, 1, 1, 1, 0, 1, 1, 1, 1, 1, 0, 0)])
    p = R.Params(edge_thresh=128, min_edges=1, ratio_num=1, ratio_den=2, min_frames=2, max_frames=5)
    area = (0, 3, 0, 3)
    assert bounded_cell_counts(frames, area, 128, 3, 4).reshape(14, 3).tolist() == \
        [[0, 0, 0]] * 3 + [[1, 1, 0], [1, 0, 0], [1, 0, 0], [0, 0, 1]] + [[0, 0, 0]] * 7
    assert clip_totals_hold_bounded(frames, area, p, 3, 4).tolist() == [[[3, 1, 3, 0]]]
    assert clip_totals_hold_bounded(frames, area, p, 2, 3).tolist() == [[[5, 2, 5, 0]]]
    assert clip_totals_hold_bounded(frames, area, p, 1, 5).tolist() == [[[10, 3, 10, 0]]]
    assert clip_totals_hold_bounded(frames, area, p, 4, 4).tolist() == [[[0, 0, 0, 0]]]
    # without a flush the rows of the last max_hold frames are pending: of 14 frames at max_hold 5 the frames 1-9 are counted, the run
    # of frames 8-9 left open; at max_hold 3 the frames 1-11, where the run of five is already known to be too long
    assert clip_totals_hold_bounded(frames, area, p, 1, 5, flush=False).tolist() == [[[5, 2, 7, 0]]]
    assert clip_totals_hold_bounded(frames, area, p, 2, 3, flush=False).tolist() == [[[5, 2, 5, 0]]]
    assert clip_totals_hold_bounded(frames[:0], area, p, 3, 4).tolist() == [[[0, 0, 0, 0]]]
    cells = NumpyCellsHoldBounded()
    assert cells(frames[:9], area, p, True, False, hold=1, max_hold=5).tolist() == [[[2, 1, 3, 0]]]         # frames 1-4, frame 4's run open
    assert cells(frames[9:], area, p, False, True, hold=1, max_hold=5).tolist() == [[[10, 3, 10, 0]]]


# ---- the locator on a busy background that stands still --------------------------------------------------------------------------
def test_held_automaton_finds_nothing_on_the_loud_clip(caplog):
    """Why the option exists: the static edges keep the subtitle's own cells present in every frame (the logo rule scores them 0) and
    dilute every other cell's cut ratio."""
    import logging
    frames, _ = static_clip("loud")
    loc = area_locator.AreaLocator(NumpyCellsHold(), automaton="hold", edge_thresh="auto", hold_frames=3)
    with caplog.at_level(logging.WARNING):
        assert loc.run(list(frames), FPS) is None
    assert loc.scores == [0] * 8 and loc.edge_thresh is None and loc.max_hold is None
    assert any("with the hold automaton in 90 frames" in r.getMessage() for r in caplog.records)


def test_held_automaton_misses_the_text_on_the_busier_clip():
    frames, _ = static_clip("busier")
    loc = area_locator.AreaLocator(NumpyCellsHold(), automaton="hold", edge_thresh="auto", hold_frames=3)
    got = loc.run(list(frames), FPS)
    assert loc.scores == [0, 0, 0, 0, 0, 0, 0, 120] and loc.edge_thresh == 192
    assert as_tuple(got) == (89, 113, 1, 257) and not contains_text(got)          # the text's right end is outside


@pytest.mark.parametrize("name,thresh,area,scores", [
    ("busier", 48, (81, 120, 0, 320), [220, 220, 254, 240, 210, 220, 190, 180]),
    ("loud", 64, (81, 120, 1, 320), [200, 220, 210, 240, 168, 160, 228, 216])])
def test_bounded_runs_find_the_band_and_a_threshold(name, thresh, area, scores):
    frames, _ = static_clip(name)
    cells = NumpyCellsHoldBounded()
    loc = area_locator.AreaLocator(cells, automaton="hold", edge_thresh="auto", hold_frames=3, max_hold_frames=30, batch=32)
    got = loc.run(list(frames), FPS)
    assert contains_text(got) and loc.edge_thresh in area_locator.AUTO_THRESHOLDS
    assert (as_tuple(got), loc.edge_thresh, loc.scores) == (area, thresh, scores)
    assert (loc.hold, loc.max_hold) == (3, 30) and set(cells.holds) == {(3, 30)} and cells.calls == 3 + 1
    assert loc.frames_scanned == 90 and loc.params(FPS) == (0, 16, 1, 2, 8, 500)
    assert loc.totals.shape == (8, 15, 5, 4)
    k = area_locator.AUTO_THRESHOLDS.index(thresh)
    assert np.array_equal(loc.totals[k], clip_totals_hold_bounded(frames, WHOLE, loc.params(FPS)._replace(edge_thresh=thresh), 3, 30))


def test_bounded_runs_at_one_threshold():
    frames, _ = static_clip("loud")
    loc = area_locator.AreaLocator(NumpyCellsHoldBounded(), automaton="hold", edge_thresh=64, hold_frames=3, max_hold_frames=30)
    assert as_tuple(loc.run(list(frames), FPS)) == (81, 120, 1, 320) and loc.totals.shape == (15, 5, 4)


def test_max_hold_comes_from_the_frame_rate_like_the_selectors():
    mk = lambda **kw: area_locator.AreaLocator(NumpyCellsHoldBounded(), automaton="hold", **kw)
    for kw, fps, want in ((dict(max_hold_seconds=12), 25.0, 300), (dict(max_hold_seconds=1.2), 25.0, 30), (dict(max_hold_seconds=15), 24.0, 360),
                          (dict(max_hold_seconds=12, max_hold_frames=40), 25.0, 40)):
        assert mk(**kw).max_hold_for(fps) == want
    assert mk().max_hold_for(25.0) is None and mk().bounded is False
    assert mk(hold_frames=3, max_hold_frames=3).max_hold_for(25.0) == 3


@pytest.mark.parametrize("kw", [dict(automaton="change", max_hold_frames=30), dict(max_hold_seconds=12), dict(automaton="hold", max_hold_frames=0),
                                dict(automaton="hold", max_hold_frames=4001), dict(automaton="hold", hold_frames=5, max_hold_frames=4)])
def test_refused_when_built(kw):
    with pytest.raises(ValueError):
        area_locator.AreaLocator(NumpyCellsHoldBounded(), **kw)


@pytest.mark.parametrize("kw", [dict(max_hold_seconds=0.2), dict(max_hold_seconds=200), dict(max_hold_frames=7)])
def test_refused_once_the_frame_rate_is_known(kw):
    frames, _ = static_clip("busier")
    cells = NumpyCellsHoldBounded()
    with pytest.raises(ValueError, match="max_hold"):               # hold is 8 frames at 25 fps
        area_locator.AreaLocator(cells, automaton="hold", **kw).run(list(frames[:5]), FPS)
    assert cells.calls == 0


def test_warning_names_the_automaton_with_its_bounds(caplog):
    import logging
    frames, _ = static_clip("busier")
    with caplog.at_level(logging.WARNING):
        loc = area_locator.AreaLocator(NumpyCellsHoldBounded(), edge_thresh="auto", automaton="hold", hold_frames=2, max_hold_frames=9)
        assert loc.run(list(frames[:7]), FPS) is None
    assert any("hold (runs of 2..9 frames) automaton" in r.getMessage() and "128" in r.getMessage() for r in caplog.records)


def test_without_the_option_the_held_call_is_unchanged():
    """automaton="hold" alone: cells_fn gets `hold` and no `max_hold`, as before."""
    frames, _ = static_clip("busier")
    seen = []

    def strict(frames, area, params, reset, flush, hold):          # a cells_fn written before the option: unknown keywords are a TypeError
        seen.append(hold)
        return np.zeros(area_locator.cells_dims(area[1] - area[0], area[3] - area[2]) + (4,), np.int32)
    loc = area_locator.AreaLocator(strict, automaton="hold", hold_frames=3)
    assert loc.run(list(frames[:10]), FPS) is None and seen == [3, 3] and loc.max_hold is None


# ---- the extractor --------------------------------------------------------------------------------------------------------------
def run_extractor(frames, truth, sub_area, **kw):
    src = extractor.ArraySource(list(stamped(frames)), FPS)
    ocr = BandOcr(truth, True)
    kw.setdefault("change_counter", NumpyBoundedHoldCounter())
    ex = extractor.SubtitleExtractor(src, ocr, sub_area=sub_area, mode="fast", frame_selector="hold", drop_score=0.0, batch=8, **kw)
    text = ex.run()
    return ex, text


CHANGE = {"hold_frames": 3, "max_hold_frames": 30, "edge_thresh": "auto"}


@pytest.mark.parametrize("name", sorted(STATIC))
def test_extractor_end_to_end(monkeypatch, name):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    frames, truth = static_clip(name)
    cells = NumpyCellsHoldBounded()
    ex, text = run_extractor(frames, truth, "auto", change_params=dict(CHANGE),
                             area_params=dict(cells_fn=cells, automaton="hold", max_hold_frames=30))
    assert contains_text(ex.located_area) and ex.sub_area == ex.located_area
    assert ex.edge_thresh in area_locator.AUTO_THRESHOLDS
    assert set(cells.holds) == {(3, 30)}                           # hold from the selector's change_params, max_hold area_params' own
    spans = [(s, e) for s, e, _r in ex.intervals]
    assert set(TRUE) <= set(spans)
    for (s, e), (_s, _e, line) in zip(TRUE, truth):
        assert line in text
        assert f"{extractor.srt.frame_to_timecode(s, FPS)} --> {extractor.srt.frame_to_timecode(e, FPS)}" in text


def test_extractor_does_not_inherit_the_selectors_max_hold(monkeypatch, caplog):
    """change_params' max_hold_* stay the selector's: runs that set them with automaton="hold" keep the held locator."""
    import logging
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    frames, truth = static_clip("loud")
    cells = NumpyCellsHold()
    with caplog.at_level(logging.WARNING):
        ex, _text = run_extractor(frames, truth, "auto", change_params=dict(CHANGE), area_params=dict(cells_fn=cells, automaton="hold"))
    assert ex.located_area is None and ex.edge_thresh == 128 and set(cells.holds) == {3}


def test_extractor_calibrates_over_a_given_area(monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    frames, truth = static_clip("loud")
    cells = NumpyCellsHoldBounded()
    ex, text = run_extractor(frames, truth, extractor.SubtitleArea(81, 120, 1, 320), change_params=dict(CHANGE),
                             area_params=dict(cells_fn=cells, automaton="hold", max_hold_seconds=1.2))
    assert ex.located_area is None and ex.edge_thresh in area_locator.AUTO_THRESHOLDS and set(cells.holds) == {(3, 30)}
    assert set(TRUE) <= {(s, e) for s, e, _r in ex.intervals}
    assert all(line in text for _s, _e, line in truth)


# ---- command lines ----------------------------------------------------------------------------------------------------------------
def test_locator_cli_takes_the_bound_and_reports_it(tmp_path, capsys):
    frames, _ = static_clip("loud")
    path = tmp_path / "loud.npy"
    np.save(path, frames)
    common = [str(path), "--fps", "25", "--json", "--edge-thresh", "auto"]
    cells = NumpyCellsHoldBounded()
    assert area_locator.main(common + ["--locator-automaton", "hold", "--hold-frames", "3", "--max-hold-frames", "30"], cells_fn=cells) == 0
    got = json.loads(capsys.readouterr().out)
    assert (got["ymin"], got["ymax"], got["xmin"], got["xmax"]) == (81, 120, 1, 320) and got["edge_thresh"] == 64
    assert got["automaton"] == "hold" and got["hold"] == 3 and got["max_hold"] == 30 and set(cells.holds) == {(3, 30)}
    cells = NumpyCellsHoldBounded()
    assert area_locator.main(common + ["--locator-automaton", "hold", "--hold-frames", "3", "--max-hold-seconds", "1.2"], cells_fn=cells) == 0
    assert json.loads(capsys.readouterr().out)["max_hold"] == 30
    assert area_locator.main(common + ["--locator-automaton", "hold", "--hold-frames", "3"], cells_fn=NumpyCellsHold()) == 1
    assert "no subtitle area" in capsys.readouterr().err
    for bad in (["--max-hold-frames", "30"], ["--locator-automaton", "change", "--max-hold-seconds", "12"]):
        assert area_locator.main(common + bad, cells_fn=NumpyCellsHoldBounded()) == 2
        assert "--locator-automaton hold" in capsys.readouterr().err
    assert area_locator.main(common + ["--locator-automaton", "hold", "--max-hold-frames", "5000"], cells_fn=NumpyCellsHoldBounded()) == 2
    assert "max_hold_frames" in capsys.readouterr().err
    assert area_locator.main(common + ["--locator-automaton", "hold", "--max-hold-frames", "4"], cells_fn=NumpyCellsHoldBounded()) == 2
    assert "max_hold" in capsys.readouterr().err


def test_extractor_cli_takes_the_locators_bound(monkeypatch, tmp_path, capsys):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    frames, truth = static_clip("loud")
    path = tmp_path / "loud.npy"
    np.save(path, stamped(frames))
    # at 25 fps --max-hold-seconds 1.2 is 30 frames; the default hold of 0.3 s is 8 frames
    common = [str(path), "--fps", "25", "--selector", "hold", "--area", "auto", "--batch", "8", "--edge-thresh", "auto", "--max-hold-seconds", "1.2"]
    cells = NumpyCellsHoldBounded()
    assert extractor.main(common + ["--locator-automaton", "hold", "--locator-max-hold-seconds", "1.2"], ocr=BandOcr(truth, True),
                          counter=NumpyBoundedHoldCounter(), cells_fn=cells) == 0
    text = capsys.readouterr().out
    assert set(cells.holds) == {(8, 30)} and text.count(" --> ") >= 1
    held = NumpyCellsHold()                                        # the selector's bound alone does not reach the locator
    assert extractor.main(common + ["--locator-automaton", "hold"], ocr=BandOcr(truth, True), counter=NumpyBoundedHoldCounter(),
                          cells_fn=held) == 0
    capsys.readouterr()
    assert set(held.holds) == {8}
    for bad in ([], ["--locator-automaton", "change"]):
        assert extractor.main(common + bad + ["--locator-max-hold-seconds", "1.2"], ocr=BandOcr(truth, True),
                              counter=NumpyBoundedHoldCounter(), cells_fn=NumpyCellsHoldBounded()) == 2
        assert "--locator-automaton hold" in capsys.readouterr().err
