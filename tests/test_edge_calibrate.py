"""Edge threshold per clip on the host: pick_edge_thresh's rule on hand-made score tables, AreaLocator(edge_thresh="auto") fed by the
numpy cells (tests/edge_calibrate_ref.py over tests/area_cells_ref.py) on the locator's clip at normal and at little contrast,
SubtitleExtractor with change_params' edge_thresh="auto" and scripted OCR, and both command lines.  CPU only."""
import logging

import numpy as np
import pytest

import area_cells_ref as R
from area_clip import FPS, H, LOCATOR, W, as_tuple, decorated_clip, text_boxes
from edge_calibrate_ref import NumpyCellsMulti, low_contrast, noisy_low_contrast
from frame_change_ref import NumpyCounter
from frame_hold_ref import NumpyHoldCounter
from vse_amd import area_locator, extractor, frame_select, ingest, synth

THS = area_locator.AUTO_THRESHOLDS
LOWER = extractor.SubtitleArea(ymin=240, ymax=H, xmin=0, xmax=W)            # the lower third, where the numpy cells take a second or two


# ---- pick_edge_thresh on hand-made tables ------------------------------------------------------------------------------------------
def table(scores, gy=3, gx=2):
    """totals [nt,gy,gx,4] whose best grid row sums to scores[k]: the score split over the two cells of row 1, half of it in row 0."""
    t = np.zeros((len(scores), gy, gx, 4), np.int32)
    for k, s in enumerate(scores):
        t[k, 1, 0, 0], t[k, 1, 1, 0] = s - s // 3, s // 3
        t[k, 0, 0, 0] = s // 2
        t[k, ..., 2] = 40
    return t


def pick(scores, ths=THS, **kw):
    t = table(scores)
    assert area_locator.edge_thresh_scores(t, 100) == list(scores)
    return area_locator.pick_edge_thresh(t, ths, 100, **kw)


def test_pick_plateau_in_the_middle():
    assert pick([0, 10, 190, 200, 185, 180, 20, 0]) == 3                 # indices 2..5: element (4 - 1) // 2 of the run
    assert pick([0, 10, 190, 200, 185, 179, 20, 0]) == 3                 # 179 < 0.9 * 200: indices 2..4, the middle one
    assert pick([0, 10, 190, 200, 185, 180, 20, 0], plateau_frac=0.95) == 2       # indices 2..3
    assert pick([0, 10, 190, 200, 185, 180, 20, 0], plateau_frac=0.05) == 3       # indices 1..6


def test_pick_plateau_at_either_end():
    assert pick([200, 199, 195, 196, 0, 0, 0, 0]) == 1                   # the low-contrast clip's table: 32
    assert pick([0, 0, 0, 0, 0, 190, 200, 195]) == 6
    assert pick([0, 145, 200, 200, 199, 195, 193, 192]) == 4             # the unmodified clip's: 96
    assert pick([0, 199, 196, 193, 0, 0, 0, 0]) == 2                     # the noisy low-contrast clip's: 48
    assert pick([200] * 8) == 3                                          # everything works: 64, the lower of the two middle ones


def test_pick_single_winner_and_all_zero():
    assert pick([0, 0, 7, 0, 0, 0, 0, 0]) == 2
    assert pick([0] * 7 + [1]) == 7
    assert pick([5], ths=(128,)) == 0
    assert pick([0] * 8) is None
    assert pick([0], ths=(128,)) is None


def test_pick_two_plateaus_takes_the_arg_maxs():
    assert pick([190, 195, 0, 0, 0, 200, 198, 0]) == 5                   # 5..6, although 0..1 also pass 0.9 * 200
    assert pick([200, 195, 0, 0, 0, 199, 198, 198]) == 0                 # 0..1
    # equal maxima: the one nearest 128 (index 5) decides which plateau
    assert pick([200, 200, 0, 0, 0, 200, 0, 0]) == 5
    assert pick([200, 200, 0, 200, 0, 0, 0, 200]) == 3                   # 64 and 192 are equally near: the lower one


def test_pick_leaves_out_logo_cells():
    t = table([100, 100, 100])
    t[1, 2, :, 0], t[1, 2, :, 2] = 500, 95                               # a row of cells present in 95 of 100 frames at threshold 1
    assert area_locator.edge_thresh_scores(t, 100) == [100, 100, 100]
    assert area_locator.edge_thresh_scores(t, 100, static_frac=0.96) == [100, 1000, 100]
    assert area_locator.pick_edge_thresh(t, (32, 64, 128), 100) == 1
    assert area_locator.pick_edge_thresh(t, (32, 64, 128), 100, static_frac=0.96) == 1
    t[0, 2, :, 0], t[0, 2, :, 2] = 500, 94                               # at threshold 0 the same row is no logo: it wins alone
    assert area_locator.pick_edge_thresh(t, (32, 64, 128), 100) == 0
    with pytest.raises(ValueError):
        area_locator.pick_edge_thresh(t, (32, 64), 100)
    with pytest.raises(ValueError):
        area_locator.AreaLocator(edge_thresh="auto", thresholds=(64, 32))
    with pytest.raises(ValueError):
        area_locator.AreaLocator(edge_thresh="auto", thresholds=range(1, 10))


# ---- the clips -----------------------------------------------------------------------------------------------------------------------
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


@pytest.fixture(scope="module")
def low_auto(low):
    """AreaLocator(edge_thresh="auto") over the whole low-contrast clip, run once."""
    cells = NumpyCellsMulti()
    loc = area_locator.AreaLocator(cells, edge_thresh="auto", **LOCATOR)
    return loc, loc.run(list(low), FPS), cells


def judge(intervals, truth):
    """One interval per true subtitle, starts at most 2 frames late (the faded one), ends equal."""
    assert len(intervals) == len(truth)
    for (s, e, rep), (ts, te, _text) in zip(intervals, truth):
        assert 0 <= s - ts <= 2 and e == te and s <= rep <= e


def contains_the_text(area):
    for y0, y1, x0, x1 in text_boxes():
        assert area.ymin <= y0 and y1 <= area.ymax and area.xmin <= x0 and x1 <= area.xmax


def test_the_constant_finds_nothing_at_little_contrast(low):
    """Pins the problem: at 128 the locator finds no area and the change selector no interval."""
    assert area_locator.AreaLocator(R.NumpyCells(), **LOCATOR).run(list(low), FPS) is None
    band = extractor.SubtitleArea(ymin=321, ymax=353, xmin=129, xmax=513)
    assert frame_select.ChangeFrameSelector(NumpyCounter(), batch=16).run(list(low), band) == []


def test_auto_finds_the_band_at_little_contrast(low, low_auto, clip):
    loc, area, cells = low_auto
    assert area is not None and loc.edge_thresh is not None and loc.edge_thresh < 96 and loc.edge_thresh in THS
    contains_the_text(area)
    assert loc.totals.shape == (8, 45, 10, 4) and loc.frames_scanned == 66 and cells.calls == 2 + 1          # one pass and the flush
    assert loc.scores == area_locator.edge_thresh_scores(loc.totals, 66)
    assert [s > 0 for s in loc.scores] == [True] * 4 + [False] * 4 and loc.edge_thresh == 32
    k = THS.index(loc.edge_thresh)
    assert as_tuple(area) == R.locate(loc.totals[k], 66, (0, H, 0, W), (H, W))
    # every slice is the single-threshold pass at that threshold
    p = area_locator.AreaLocator(**LOCATOR).params(FPS)
    for j in (1, 5):
        assert np.array_equal(loc.totals[j], R.clip_totals(low, (0, H, 0, W), p._replace(edge_thresh=THS[j])))
    judge(frame_select.ChangeFrameSelector(NumpyCounter(), edge_thresh=loc.edge_thresh, batch=16).run(list(low), area), clip[1])


def test_auto_on_the_noisy_low_contrast_clip(clip):
    frames, truth = clip
    noisy = noisy_low_contrast(frames)
    loc = area_locator.AreaLocator(NumpyCellsMulti(), edge_thresh="auto", search_area=LOWER, **LOCATOR)
    area = loc.run(list(noisy), FPS)
    assert loc.edge_thresh == 48 and loc.scores[0] == 0 and loc.scores[4:] == [0] * 4
    contains_the_text(area)
    judge(frame_select.ChangeFrameSelector(NumpyCounter(), edge_thresh=48, batch=16).run(list(noisy), area), truth)


def test_auto_on_the_unmodified_clip_equals_128(clip):
    """The same area, and the same intervals by the judgement above.  Frame for frame they are equal but for one start: the subtitle
    that fades in (true start 38) starts at 39 at the chosen 96 and at 40 at 128, the lower threshold seeing the fade a frame sooner;
    so the starts at 96 are held between the true ones and those at 128, and everything else equal."""
    frames, truth = clip
    auto = area_locator.AreaLocator(NumpyCellsMulti(), edge_thresh="auto", search_area=LOWER, **LOCATOR)
    fixed = area_locator.AreaLocator(R.NumpyCells(), search_area=LOWER, **LOCATOR)
    area = auto.run(list(frames), FPS)
    assert auto.edge_thresh == 96 and auto.scores[0] == 0 and min(auto.scores[2:]) >= 0.9 * max(auto.scores)
    assert as_tuple(area) == as_tuple(fixed.run(list(frames), FPS)) and fixed.edge_thresh == 128
    assert np.array_equal(auto.totals[THS.index(128)], fixed.totals)
    at_96 = frame_select.ChangeFrameSelector(NumpyCounter(), edge_thresh=96, batch=16).run(list(frames), area)
    at_128 = frame_select.ChangeFrameSelector(NumpyCounter(), batch=16).run(list(frames), area)
    judge(at_96, truth)
    judge(at_128, truth)
    assert [e for _s, e, _r in at_96] == [e for _s, e, _r in at_128]
    assert all(ts <= a <= b for (a, _e, _r), (b, _e2, _r2), (ts, _te, _t) in zip(at_96, at_128, truth))
    assert [a == b for (a, _e, _r), (b, _e2, _r2) in zip(at_96, at_128)] == [True, True, False, True]        # the faded one: 39, 40


# ---- the extractor -------------------------------------------------------------------------------------------------------------------
class ScriptedOcr:
    """Recognises the frame number stamped into pixel (0, 0) as the truth text of that frame, in a box inside the text rows."""

    def __init__(self, truth):
        self.truth, self.seen = truth, []
        self.predict_batch = lambda frames: [self.predict(np.asarray(f)) for f in frames]

    def predict(self, img):
        no = int(img[0, 0, 0]) | (int(img[0, 0, 1]) << 8)
        self.seen.append(no)
        for s, e, text in self.truth:
            if s <= no <= e:
                return [[[240, 330], [400, 330], [400, 346], [240, 346]]], [(text, 0.95)]
        return [], []


def stamped(frames):
    frames = frames.copy()
    for i in range(len(frames)):
        frames[i, 0, 0, 0], frames[i, 0, 0, 1] = (i + 1) & 255, (i + 1) >> 8
    return frames


def make_extractor(frames, truth, sub_area, cells, selector="change", **kw):
    src = extractor.ArraySource(list(stamped(frames)), FPS)
    return extractor.SubtitleExtractor(src, ScriptedOcr(truth), sub_area=sub_area, mode="fast", frame_selector=selector,
                                       change_counter=NumpyCounter() if selector == "change" else NumpyHoldCounter(), drop_score=0.0, batch=8, change_params={"edge_thresh": "auto"},
                                       area_params=dict(cells_fn=cells, **LOCATOR), **kw)


def test_extractor_auto_area_and_auto_threshold(low, low_auto, clip, monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    truth = clip[1]
    cells = NumpyCellsMulti()
    ex = make_extractor(low, truth, "auto", cells)
    assert ex.edge_thresh is None
    text = ex.run()
    loc, area, _cells = low_auto
    assert ex.edge_thresh == loc.edge_thresh == 32 and as_tuple(ex.located_area) == as_tuple(area)
    assert cells.calls == (66 + 7) // 8 + 1                                # ONE locator pass yields the area and the threshold
    judge(ex.intervals, truth)
    assert text.count(" --> ") == len(truth) and all(t in text for _s, _e, t in truth)
    # the same run at the constant: no area, no intervals, the fps sampler
    src = extractor.ArraySource(list(stamped(low)), FPS)
    fixed = extractor.SubtitleExtractor(src, ScriptedOcr(truth), sub_area="auto", mode="fast", frame_selector="change",
                                        change_counter=NumpyCounter(), drop_score=0.0, batch=8,
                                        area_params=dict(cells_fn=R.NumpyCells(), **LOCATOR))
    fixed.run()
    assert fixed.located_area is None and fixed.intervals is None and fixed.edge_thresh == 128


@pytest.mark.parametrize("selector", ["change", "hold"])
def test_extractor_given_area_scans_only_its_rows(low, low_auto, clip, monkeypatch, selector):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    truth = clip[1]
    band = low_auto[1]
    cells = NumpyCellsMulti()
    ex = make_extractor(low, truth, band, cells, selector=selector)
    ex.run()
    assert ex.edge_thresh == 32 and ex.located_area is None and ex.sub_area == band
    assert cells.rows and set(cells.rows) == {band.ymax - band.ymin} and cells.calls == (66 + 7) // 8 + 1
    assert len(ex.intervals) == len(truth)
    if selector == "change":
        judge(ex.intervals, truth)
        want = frame_select.ChangeFrameSelector(NumpyCounter(), edge_thresh=32, batch=8).run(list(low), band)
        assert ex.intervals == want


def test_extractor_without_subtitles_warns_and_uses_128(monkeypatch, caplog):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    frames, truth = synth.make_clip([(None, 20)], 120, W, seed=3)
    band = extractor.SubtitleArea(ymin=60, ymax=120, xmin=0, xmax=W)
    for sub_area in (band, "auto"):
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            ex = make_extractor(frames, truth, sub_area, NumpyCellsMulti())
            ex.run()
        fallbacks = [r for r in caplog.records if "edge_thresh='auto'" in r.getMessage() and "128" in r.getMessage()]
        assert len(fallbacks) == 1 and ex.edge_thresh == 128
        assert ex.intervals == ([] if sub_area is band else None)


def test_one_pass_refuses_auto(clip):
    frames, truth = clip
    src = extractor.ArraySource(list(frames[:4]), FPS)
    with pytest.raises(ValueError, match=r"edge_thresh='auto' is not available in one pass \(a sequential source, or one_pass=True\): "
                                         "it needs a second look at frames already gone"):
        extractor.SubtitleExtractor(src, ScriptedOcr(truth), sub_area=LOWER, frame_selector="change", change_params={"edge_thresh": "auto"},
                                    one_pass=True)
    extractor.SubtitleExtractor(src, ScriptedOcr(truth), sub_area=LOWER, frame_selector="change", change_params={"edge_thresh": 64},
                                one_pass=True)
    with pytest.raises(ValueError, match="edge_thresh"):
        extractor.SubtitleExtractor(src, ScriptedOcr(truth), sub_area=LOWER, frame_selector="change", change_params={"edge_thresh": "best"})


# ---- command lines -------------------------------------------------------------------------------------------------------------------
def test_locator_cli_edge_thresh(low, tmp_path, capsys):
    import json
    path = tmp_path / "low.npy"
    np.save(path, low[:, 240:])                                            # the lower third as a clip of its own
    want = area_locator.AreaLocator(NumpyCellsMulti(), edge_thresh="auto").run(list(low[:, 240:]), FPS)
    assert area_locator.main([str(path), "--fps", "10", "--edge-thresh", "auto"], cells_fn=NumpyCellsMulti()) == 0
    assert capsys.readouterr().out.split() == [str(v) for v in as_tuple(want)] + ["32"]
    assert area_locator.main([str(path), "--fps", "10", "--edge-thresh", "auto", "--json"], cells_fn=NumpyCellsMulti()) == 0
    got = json.loads(capsys.readouterr().out)
    assert got["edge_thresh"] == 32 and list(got["scores"]) == [str(t) for t in THS] and got["scores"]["128"] == 0 < got["scores"]["32"]
    assert got["cells"] == [15, 10] and (got["ymin"], got["ymax"]) == (want.ymin, want.ymax)
    # an integer: four numbers, as before; the default is 128
    assert area_locator.main([str(path), "--fps", "10", "--edge-thresh", "48"], cells_fn=NumpyCellsMulti()) == 0
    at_48 = area_locator.AreaLocator(R.NumpyCells(), edge_thresh=48).run(list(low[:, 240:]), FPS)
    assert capsys.readouterr().out.split() == [str(v) for v in as_tuple(at_48)]
    assert area_locator.main([str(path), "--fps", "10", "--edge-thresh", "48", "--json"], cells_fn=NumpyCellsMulti()) == 0
    got = json.loads(capsys.readouterr().out)
    assert got["edge_thresh"] == 48 and got["scores"] is None
    assert area_locator.main([str(path), "--fps", "10"], cells_fn=NumpyCellsMulti()) == 1
    capsys.readouterr()
    for bad in ("best", "0", "256", "-3", "12.5"):
        assert area_locator.main([str(path), "--fps", "10", f"--edge-thresh={bad}"], cells_fn=NumpyCellsMulti()) == 2
        assert "--edge-thresh" in capsys.readouterr().err


def test_extractor_cli_edge_thresh(low, low_auto, clip, tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    truth = clip[1]
    band = low_auto[1]
    path = tmp_path / "low.npy"
    np.save(path, stamped(low))
    common = [str(path), "--fps", "10", "--selector", "change", "--area", f"{band.ymin},{band.ymax},{band.xmin},{band.xmax}"]

    def run(*more):
        rc = extractor.main(common + list(more), ocr=ScriptedOcr(truth), counter=NumpyCounter(), cells_fn=NumpyCellsMulti())
        return rc, capsys.readouterr()
    rc, out = run("--edge-thresh", "auto")
    assert rc == 0 and out.out.count(" --> ") == len(truth)
    rc, at_32 = run("--edge-thresh", "32")
    assert rc == 0 and at_32.out == out.out
    rc, at_128 = run()
    assert rc == 0 and at_128.out.count(" --> ") == 0                      # the default stays 128: nothing found
    for bad in ("best", "0", "256"):
        rc, out = run("--edge-thresh", bad)
        assert rc == 2 and "--edge-thresh" in out.err
    # one pass refuses it, with the other options' wording
    y4m = tmp_path / "low.y4m"
    ingest.write_y4m(y4m, [ingest.bgr_to_yuv420(f) for f in low[:4]], FPS)
    with open(y4m, "rb") as fp:
        monkeypatch.setattr("sys.stdin", type("Stdin", (), {"buffer": fp})())
        rc = extractor.main(["-", "--selector", "change", "--area", "300,360,0,640", "--edge-thresh", "auto"], ocr=ScriptedOcr(truth),
                            counter=NumpyCounter(), cells_fn=NumpyCellsMulti())
    assert rc == 2 and "edge_thresh='auto' is not available in one pass" in capsys.readouterr().err
