"""The locator and the threshold calibration on held edges, on the host: the numpy restatement of vse_frame_cells_hold
(tests/area_cells_hold_ref.py) whole and streamed, area_locator.AreaLocator(automaton="hold") on a clip whose textured background
moves (where the change automaton finds no area and no threshold), SubtitleExtractor with area_params={"automaton": "hold"} and a
scripted recogniser, and the command lines.  CPU only."""
import json

import numpy as np
import pytest

import area_cells_ref as R
from area_cells_hold_ref import NumpyCellsHold, clip_totals_hold, held_cell_counts
from frame_hold_ref import NumpyHoldCounter, counts as hold_counts
from test_change_select import stamped
from test_frame_hold import BandOcr, MOVING
from vse_amd import area_locator, extractor, synth

FPS = 25.0
WHOLE = (0, 120, 0, 320)
HELD_AREA = (81, 120, 1, 320)             # what the held rule finds: cell rows 10..14 padded by one cell, all columns
TEXT_BOX = (90, 110, 20, 300)             # make_moving_clip: one line of height 20, centred, 10 pixels above the bottom edge
P = R.Params(edge_thresh=128, min_edges=16, ratio_num=1, ratio_den=2, min_frames=8, max_frames=500)
_cache = {}


def busy_clip():
    """synth.make_moving_clip with a texture strong enough that the change automaton sees a cut in every cell at every frame."""
    if "busy" not in _cache:
        frames, truth = synth.make_moving_clip(MOVING, amp=(120, 120))
        frames.setflags(write=False)
        _cache["busy"] = frames, truth
    return _cache["busy"]


def as_tuple(a):
    return None if a is None else (a.ymin, a.ymax, a.xmin, a.xmax)


# ---- the reference against itself -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hold", (1, 2, 3, 8, 32))
def test_streaming_cells_equal_the_whole_clip(hold):
    frames, _ = busy_clip()
    area = (60, 120, 0, 320)
    p = P._replace(min_frames=max(3, hold))
    whole = clip_totals_hold(frames, area, p, hold)
    cells, fed = NumpyCellsHold(), 0
    for n in (1, 2, 3, 64, len(frames) - 70):
        got = cells(frames[fed:fed + n], area, p, fed == 0, False, hold=hold)
        fed += n
        assert np.array_equal(got, clip_totals_hold(frames[:fed], area, p, hold, flush=False)), fed
    assert fed == len(frames)
    assert np.array_equal(cells(None, area, p, False, True, hold=hold), whole)
    assert whole.shape == (8, 5, 4) and whole[..., 2].max() > 0
    both = NumpyCellsHold()(frames, area, p, True, True, thresholds=(96, 128), hold=hold)
    assert np.array_equal(both[1], whole) and not np.array_equal(both[0], both[1])


def test_hold_one_is_the_change_cells():
    frames, _ = busy_clip()
    area = (60, 120, 0, 320)
    p = P._replace(min_frames=3)
    assert np.array_equal(clip_totals_hold(frames, area, p, 1), R.clip_totals(frames, area, p))
    assert np.array_equal(clip_totals_hold(frames, area, p, 1, flush=False), R.clip_totals(frames, area, p, flush=False))
    assert np.array_equal(held_cell_counts(frames, area, 128, 1), R.cell_counts(frames, area, 128)[0])
    for hold in (1, 3, 8):                  # summed over the cells: vse_frame_hold's rows
        assert np.array_equal(held_cell_counts(frames, area, 128, hold).sum((1, 2)), hold_counts(frames, area, 128, hold))


def test_one_cell_by_hand():
    """A 3 x 3 region has one interior pixel, hence one cell: an edge in frames 1-2, 4-6 and 9-10 of ten.  At hold 3 only frames
    4-6 are held: one run of three frames.  At hold 1 and 2 all three runs count, the last one closed by the flush."""
    edge = np.zeros((3, 3, 3), np.uint8)
    edge[:, 2] = 255
    frames = np.stack([edge if e else np.zeros_like(edge) for e in (1, 1, 0, 1, 1, 1, 0, 0, 1, 1)])
    p = R.Params(edge_thresh=128, min_edges=1, ratio_num=1, ratio_den=2, min_frames=2, max_frames=5)
    area = (0, 3, 0, 3)
    assert held_cell_counts(frames, area, 128, 3).reshape(10, 3).tolist() == \
        [[0, 0, 0]] * 3 + [[1, 1, 0], [1, 0, 0], [1, 0, 0], [0, 0, 1]] + [[0, 0, 0]] * 3
    assert clip_totals_hold(frames, area, p, 3).tolist() == [[[3, 1, 3, 0]]]
    assert clip_totals_hold(frames, area, p, 1).tolist() == clip_totals_hold(frames, area, p, 2).tolist() == [[[7, 3, 7, 0]]]
    assert clip_totals_hold(frames, area, p, 1, flush=False).tolist() == [[[5, 2, 7, 0]]]       # the run of frames 9-10 is open
    assert clip_totals_hold(frames, area, p, 2, flush=False).tolist() == [[[5, 2, 6, 0]]]       # frame 10's mask is not complete
    assert clip_totals_hold(frames, area, p._replace(min_frames=3), 3).tolist() == [[[3, 1, 3, 0]]]
    assert clip_totals_hold(frames, area, p, 4).tolist() == [[[0, 0, 0, 0]]]
    assert clip_totals_hold(frames[:0], area, p, 3).tolist() == [[[0, 0, 0, 0]]]


# ---- the locator on a moving background ---------------------------------------------------------------------------------------
def test_change_automaton_finds_no_area_on_a_moving_background():
    """Why automaton="hold" exists."""
    frames, _ = busy_clip()
    loc = area_locator.AreaLocator(R.NumpyCells())
    assert loc.run(list(frames), FPS) is None and loc.frames_scanned == len(frames)
    assert loc.automaton == "change" and loc.hold is None


def test_held_automaton_finds_the_text_band():
    frames, _ = busy_clip()
    cells = NumpyCellsHold()
    loc = area_locator.AreaLocator(cells, automaton="hold", batch=32)
    got = loc.run(list(frames), FPS)
    assert as_tuple(got) == HELD_AREA
    assert got.ymin <= TEXT_BOX[0] and TEXT_BOX[1] <= got.ymax and got.xmin <= TEXT_BOX[2] and TEXT_BOX[3] <= got.xmax
    assert loc.hold == 8 and set(cells.holds) == {8} and cells.calls == 3 + 1
    assert loc.params(FPS) == (128, 16, 1, 2, 8, 500)
    assert np.array_equal(loc.totals, clip_totals_hold(frames, WHOLE, loc.params(FPS), 8))


def test_held_automaton_calibrates_the_threshold():
    frames, _ = busy_clip()
    loc = area_locator.AreaLocator(NumpyCellsHold(), automaton="hold", edge_thresh="auto")
    got = loc.run(list(frames), FPS)
    assert loc.scores == [256, 252, 243, 235, 231, 231, 231, 231]
    assert loc.edge_thresh == 64 and as_tuple(got) == HELD_AREA
    assert loc.totals.shape == (8, 15, 5, 4)


def test_hold_comes_from_the_frame_rate_like_the_selectors():
    for fps, want in ((25.0, 8), (10.0, 3), (1.0, 1), (200.0, 32)):
        loc = area_locator.AreaLocator(NumpyCellsHold(), automaton="hold")
        assert loc.hold_for(fps) == want and loc.params(fps).min_frames >= want
    loc = area_locator.AreaLocator(NumpyCellsHold(), automaton="hold", hold_frames=5, min_seconds=0.1)
    assert loc.hold_for(25.0) == 5 and loc.params(25.0).min_frames == 5
    assert area_locator.AreaLocator(hold_frames=5).hold_for(25.0) is None            # the change automaton has no hold
    for bad in (dict(automaton="held"), dict(automaton="hold", hold_frames=33), dict(hold_frames=0)):
        with pytest.raises(ValueError):
            area_locator.AreaLocator(NumpyCellsHold(), **bad)


def test_warning_names_the_automaton(caplog):
    import logging
    frames, _ = busy_clip()
    with caplog.at_level(logging.WARNING):
        assert area_locator.AreaLocator(NumpyCellsHold(), edge_thresh="auto", automaton="hold", hold_frames=2).run(list(frames[:7]), FPS) is None
    assert any("hold automaton" in r.getMessage() and "128" in r.getMessage() for r in caplog.records)


# ---- the extractor --------------------------------------------------------------------------------------------------------------
def run_extractor(frames, truth, sub_area, **kw):
    src = extractor.ArraySource(list(stamped(frames)), FPS)
    ocr = BandOcr(truth, True)
    kw.setdefault("change_counter", NumpyHoldCounter())
    ex = extractor.SubtitleExtractor(src, ocr, sub_area=sub_area, mode="fast", frame_selector="hold", drop_score=0.0, batch=8, **kw)
    text = ex.run()
    return ex, (text, ex.intervals, ex.raw_lines, ex.short_lines, ocr.seen)


def test_extractor_locates_the_area_on_held_edges(monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    frames, truth = busy_clip()
    cells = NumpyCellsHold()
    auto, got = run_extractor(frames, truth, "auto", area_params=dict(cells_fn=cells, automaton="hold"))
    assert as_tuple(auto.located_area) == HELD_AREA and auto.sub_area == auto.located_area
    assert set(cells.holds) == {8}                                # the selector's default at 25 fps
    given, want = run_extractor(frames, truth, extractor.SubtitleArea(*HELD_AREA))
    assert given.located_area is None
    assert got == want
    text, intervals, _raw, _short, seen = got
    assert intervals == [(s, e, (s + e) // 2) for s, e, _t in truth] and sorted(seen) == [r for _s, _e, r in intervals]
    assert text.count(" --> ") == 4


def test_extractor_calibrates_on_held_edges(monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    frames, truth = busy_clip()
    auto, got = run_extractor(frames, truth, "auto", change_params={"edge_thresh": "auto"},
                              area_params=dict(cells_fn=NumpyCellsHold(), automaton="hold"))
    assert auto.edge_thresh == 64 and as_tuple(auto.located_area) == HELD_AREA
    _given, want = run_extractor(frames, truth, extractor.SubtitleArea(*HELD_AREA), change_params={"edge_thresh": 64})
    # the calibration's threshold reaches the selector: the run is the run with 64 passed by hand.  (What the hold selector makes of
    # this clip at 64 is its own matter: texture edges held inside the band bridge the two back-to-back text changes.)
    assert got == want and len(got[1]) >= 2
    # over a drawn box: calibrate_edge_thresh
    cells = NumpyCellsHold()
    boxed, _ = run_extractor(frames, truth, extractor.SubtitleArea(*HELD_AREA), change_params={"edge_thresh": "auto", "hold_frames": 3},
                             area_params=dict(cells_fn=cells, automaton="hold"))
    assert boxed.edge_thresh in area_locator.AUTO_THRESHOLDS and set(cells.holds) == {3}


def test_extractor_hands_the_selectors_hold_to_the_locator(monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    frames, truth = busy_clip()
    cells = NumpyCellsHold()
    ex, got = run_extractor(frames, truth, "auto", change_params={"hold_frames": 3}, area_params=dict(cells_fn=cells, automaton="hold"))
    assert set(cells.holds) == {3} and as_tuple(ex.located_area) == HELD_AREA
    assert got[1] == [(s, e, (s + e) // 2) for s, e, _t in truth]
    cells = NumpyCellsHold()                                      # area_params' own wins
    run_extractor(frames, truth, "auto", change_params={"hold_frames": 3}, area_params=dict(cells_fn=cells, automaton="hold", hold_frames=5))
    assert set(cells.holds) == {5}
    cells = NumpyCellsHold()
    run_extractor(frames, truth, "auto", change_params={"hold_seconds": 0.2}, area_params=dict(cells_fn=cells, automaton="hold"))
    assert set(cells.holds) == {5}
    cells = NumpyCellsHold()                                      # ... whichever of the two it sets
    run_extractor(frames, truth, "auto", change_params={"hold_frames": 3}, area_params=dict(cells_fn=cells, automaton="hold", hold_seconds=0.16))
    assert set(cells.holds) == {4}


def test_without_the_option_cells_fn_gets_no_new_keyword(monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    frames, truth = busy_clip()
    inner, calls = R.NumpyCells(), []

    def strict(frames, area, params, reset, flush):               # a cells_fn written before the option: unknown keywords are a TypeError
        calls.append(params)
        return inner(frames, area, params, reset, flush)
    ex, got = run_extractor(frames, truth, "auto", change_params={"hold_frames": 3}, area_params=dict(cells_fn=strict))
    assert ex.located_area is None and len(calls) == (len(frames) + 7) // 8 + 1       # the change automaton: no area on this clip
    assert calls[0].min_frames == 8                                # min_seconds alone: the selector's hold does not reach it
    assert got[1] is None


# ---- command lines ----------------------------------------------------------------------------------------------------------------
def test_locator_cli_takes_the_automaton_and_reports_it(tmp_path, capsys):
    frames, _ = busy_clip()
    path = tmp_path / "busy.npy"
    np.save(path, frames)
    common = [str(path), "--fps", "25", "--json"]
    cells = NumpyCellsHold()
    assert area_locator.main(common + ["--locator-automaton", "hold"], cells_fn=cells) == 0
    got = json.loads(capsys.readouterr().out)
    assert (got["ymin"], got["ymax"], got["xmin"], got["xmax"]) == HELD_AREA
    assert got["automaton"] == "hold" and got["hold"] == 8 and got["edge_thresh"] == 128 and set(cells.holds) == {8}
    assert area_locator.main(common + ["--locator-automaton", "hold", "--hold-frames", "3", "--edge-thresh", "auto"], cells_fn=NumpyCellsHold()) == 0
    got = json.loads(capsys.readouterr().out)
    assert got["automaton"] == "hold" and got["hold"] == 3 and got["edge_thresh"] in area_locator.AUTO_THRESHOLDS
    assert area_locator.main(common + ["--locator-automaton", "hold", "--hold-seconds", "0.2"], cells_fn=NumpyCellsHold()) == 0
    assert json.loads(capsys.readouterr().out)["hold"] == 5
    assert area_locator.main(common, cells_fn=R.NumpyCells()) == 1                    # the default is the change automaton
    assert "no subtitle area" in capsys.readouterr().err
    quiet = tmp_path / "quiet.npy"
    np.save(quiet, synth.make_clip([(None, 5), ("the quick brown fox", 12), (None, 5)], 120, 320, seed=1)[0])
    assert area_locator.main([str(quiet), "--fps", "10", "--json"], cells_fn=R.NumpyCells()) == 0
    got = json.loads(capsys.readouterr().out)
    assert got["automaton"] == "change" and got["hold"] is None
    assert area_locator.main(common + ["--locator-automaton", "hold", "--hold-frames", "40"], cells_fn=NumpyCellsHold()) == 2
    assert "hold_frames" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        area_locator.main(common + ["--locator-automaton", "held"], cells_fn=NumpyCellsHold())


def test_extractor_cli_takes_the_automaton(monkeypatch, tmp_path, capsys):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    frames, truth = busy_clip()
    path = tmp_path / "busy.npy"
    np.save(path, stamped(frames))
    common = [str(path), "--fps", "25", "--selector", "hold", "--area", "auto", "--batch", "8"]
    cells = NumpyCellsHold()
    assert extractor.main(common + ["--locator-automaton", "hold"], ocr=BandOcr(truth, True), counter=NumpyHoldCounter(), cells_fn=cells) == 0
    text = capsys.readouterr().out
    assert text.count(" --> ") == 4 and set(cells.holds) == {8}
    _ex, want = run_extractor(frames, truth, extractor.SubtitleArea(*HELD_AREA))
    assert text == want[0]
    # the default stays the change automaton, which finds no area here: the run without an area
    assert extractor.main(common, ocr=BandOcr(truth, True), counter=NumpyHoldCounter(), cells_fn=R.NumpyCells()) == 0
    assert capsys.readouterr().out != text
    with pytest.raises(SystemExit):
        extractor.main(common + ["--locator-automaton", "held"], ocr=BandOcr(truth, True))
