"""Subtitle-area locator on the host: locate_area's rule on hand-made maps, the per-cell automaton against
frame_select.change_intervals, AreaLocator fed by the numpy restatement (tests/area_cells_ref.py) on a synth.make_clip clip with a
logo and a flickering pattern, SubtitleExtractor(sub_area="auto") with scripted OCR, and the command line.  CPU only."""
import logging
from fractions import Fraction

import numpy as np
import pytest

import area_cells_ref as R
from area_clip import BARS, FPS, H, LOCATOR, LOGO, W, as_tuple, decorated_clip, text_boxes
from frame_change_ref import NumpyCounter
from vse_amd import area_locator, extractor, frame_select, synth


@pytest.fixture(scope="module")
def clip():
    frames, truth = decorated_clip()
    frames.setflags(write=False)
    return frames, truth


# ---- locate_area on hand-made maps ----------------------------------------------------------------------------------------------
FRAME = (100, 700)               # whole-frame region: 13 x 11 cells
GY, GX = 13, 11


def totals_map(covered, present=None):
    t = np.zeros((GY, GX, 4), np.int32)
    for (j, i), c in covered.items():
        t[j, i, 0] = c
        t[j, i, 1] = 1
    for (j, i), p in (present or {}).items():
        t[j, i, 2] = p
    return t


def locate(t, scanned=100, region=(0, 100, 0, 700), frame=FRAME, **kw):
    got = as_tuple(area_locator.locate_area(t, scanned, region, frame, **kw))
    assert got == R.locate(t, scanned, region, frame, **kw)
    return got


def test_dims_match_the_reference():
    for h, w in [(3, 3), (10, 66), (11, 67), (100, 700), (360, 640), (1080, 1920)]:
        assert area_locator.cells_dims(h, w) == R.dims(h, w)
    assert R.dims(*FRAME) == (GY, GX)


def test_all_zero_map_gives_none():
    assert locate(totals_map({})) is None
    assert locate(totals_map({}, {(3, 3): 50})) is None


def test_one_cell_padding():
    # cell (5, 4): rows 41:49, columns 257:321, padded by one cell of 8 x 64
    assert locate(totals_map({(5, 4): 30})) == (33, 57, 193, 385)
    assert locate(totals_map({(5, 4): 30}), pad_cells=0) == (41, 49, 257, 321)
    assert locate(totals_map({(5, 4): 30}), pad_cells=2) == (25, 65, 129, 449)


def test_tie_goes_to_the_lower_band():
    assert locate(totals_map({(2, 4): 30, (9, 4): 30}), pad_cells=0) == (73, 81, 257, 321)
    assert locate(totals_map({(2, 4): 31, (9, 4): 30}), pad_cells=0) == (17, 25, 257, 321)


def test_row_frac_both_sides():
    base = {(6, 4): 40}
    assert locate(totals_map({**base, (5, 4): 10, (7, 4): 9}), pad_cells=0) == (41, 57, 257, 321)          # 10 = 0.25 * 40: in; 9: out
    assert locate(totals_map({**base, (5, 4): 9, (7, 4): 10}), pad_cells=0) == (49, 65, 257, 321)
    assert locate(totals_map({**base, (5, 4): 10, (4, 4): 10, (3, 4): 9, (1, 4): 40 - 1}), pad_cells=0) == (33, 57, 257, 321)
    assert locate(totals_map({**base, (5, 4): 20, (7, 4): 19}), pad_cells=0, row_frac=0.5) == (41, 57, 257, 321)


def test_col_frac_both_sides():
    row = {(6, 2): 5, (6, 3): 100, (6, 5): 0, (6, 6): 4, (6, 8): 5, (6, 9): 4}
    assert locate(totals_map(row), pad_cells=0) == (49, 57, 129, 577)               # 5 = 0.05 * 100: columns 2..8; the gap stays inside
    assert locate(totals_map({**row, (6, 2): 4}), pad_cells=0) == (49, 57, 193, 577)
    assert locate(totals_map(row), pad_cells=0, col_frac=0.5) == (49, 57, 193, 257)
    # the column score is summed over the band's rows only
    assert locate(totals_map({**row, (6, 2): 4, (1, 2): 50}), pad_cells=0) == (49, 57, 193, 577)


def test_static_cells_drop_at_exactly_static_frac():
    cov = {(1, 1): 90, (6, 4): 30}
    assert locate(totals_map(cov, {(1, 1): 74}), scanned=100, static_frac=0.75, pad_cells=0) == (9, 17, 65, 129)
    assert locate(totals_map(cov, {(1, 1): 75}), scanned=100, static_frac=0.75, pad_cells=0) == (49, 57, 257, 321)      # exactly: dropped
    assert locate(totals_map(cov, {(1, 1): 75, (6, 4): 80}), scanned=100, static_frac=0.75) is None


def test_clamps_at_all_four_borders():
    assert locate(totals_map({(0, 0): 30})) == (0, 17, 0, 129)
    # the last cells are cut off at the interior's end (row 99, column 699) before the padding
    assert locate(totals_map({(GY - 1, GX - 1): 30})) == (89, 100, 577, 700)
    assert locate(totals_map({(GY - 1, GX - 1): 30}), pad_cells=0) == (97, 99, 641, 699)


def test_region_inside_a_larger_frame():
    t = np.zeros((2, 2, 4), np.int32)              # region rows 200:212 (10 interior rows), columns 300:400 (98 interior columns)
    t[1, 1, 0] = 7
    assert locate(t, region=(200, 212, 300, 400), frame=(360, 640)) == (201, 219, 301, 463)
    assert locate(t, region=(200, 212, 300, 400), frame=(215, 420)) == (201, 215, 301, 420)
    with pytest.raises(ValueError):
        area_locator.locate_area(t, 10, (0, 100, 0, 700), FRAME)


# ---- the automaton against change_intervals -------------------------------------------------------------------------------------
def covered_by_intervals(series, p):
    iv = frame_select.change_intervals(np.asarray(series, np.int32).reshape(-1, 3), p.min_edges, p.ratio_num / p.ratio_den, p.min_frames)
    return sum(e - s + 1 for s, e, _r in iv if e - s + 1 <= p.max_frames), sum(1 for s, e, _r in iv if e - s + 1 <= p.max_frames)


def random_series(rng, n):
    """A cell's (e, a, v) series from random masks of 40 pixels that mostly hold, sometimes change a little, half or wholly."""
    out = []
    prev = np.zeros(40, bool)
    cur = rng.random(40) < 0.5
    for _ in range(n):
        kind = rng.integers(0, 10)
        if kind == 0:
            cur = np.zeros(40, bool)
        elif kind == 1:
            cur = rng.random(40) < 0.5
        elif kind == 2:
            cur = cur.copy()
            flip = rng.choice(40, rng.integers(1, 20), replace=False)
            cur[flip] = ~cur[flip]
        out.append((int(cur.sum()), int((cur & ~prev).sum()), int((prev & ~cur).sum())))
        prev = cur
    return out


@pytest.mark.parametrize("ratio", [Fraction(1, 2), Fraction(2, 5), Fraction(1, 3), Fraction(333, 1024)])
def test_automaton_matches_change_intervals_on_random_series(ratio):
    rng = np.random.default_rng(ratio.denominator)
    p = R.Params(0, 6, ratio.numerator, ratio.denominator, 3, 9)
    at_equality = 0
    for _ in range(40):
        s = random_series(rng, 120)
        covered, runs, present, cuts = R.series_totals(s, p)
        assert (covered, runs) == covered_by_intervals(s, p)
        assert present == sum(e >= p.min_edges for e, _a, _v in s)
        at_equality += sum((a + v) * ratio.denominator == ratio.numerator * (s[t - 1][0] + a) and a + v > 0
                           for t, (e, a, v) in enumerate(s) if t)
    assert at_equality > 0 or ratio.denominator == 1024             # the small fractions meet exact equality


def test_automaton_ratio_cut_at_exact_equality():
    p = R.Params(0, 10, 1, 2, 2, 100)
    hold = [(100, 100, 0), (100, 0, 0)]
    assert R.series_totals(hold + [(100, 0, 50), (100, 0, 0)], p) == [4, 2, 4, 1]          # 50 / 100 = 1 / 2: a cut
    assert R.series_totals(hold + [(100, 0, 49), (100, 0, 0)], p) == [4, 1, 4, 0]
    assert R.series_totals(hold + [(100, 25, 25), (100, 0, 0)], p._replace(ratio_num=2, ratio_den=5)) == [4, 2, 4, 1]      # 50 / 125
    assert R.series_totals(hold + [(100, 25, 25), (100, 0, 0)], p._replace(ratio_num=410, ratio_den=1024)) == [4, 1, 4, 0]
    for s, q in [(hold + [(100, 0, 50), (100, 0, 0)], p), (hold + [(100, 25, 25), (100, 0, 0)], p._replace(ratio_num=2, ratio_den=5))]:
        assert R.series_totals(s, q)[:2] == list(covered_by_intervals(s, q))


def test_automaton_run_lengths_at_the_bounds():
    p = R.Params(0, 10, 1, 2, 4, 7)

    def runs_of(*lengths):
        s = []
        for n in lengths:
            s += [(50, 50, 0)] + [(50, 0, 0)] * (n - 1) + [(0, 0, 50)]
        return s
    assert R.series_totals(runs_of(3), p) == [0, 0, 3, 0]
    assert R.series_totals(runs_of(4), p) == [4, 1, 4, 0]
    assert R.series_totals(runs_of(7), p) == [7, 1, 7, 0]
    assert R.series_totals(runs_of(8), p) == [0, 0, 8, 0]
    s = runs_of(3, 4, 7, 8)
    assert R.series_totals(s, p) == [11, 2, 22, 0]
    assert R.series_totals(s, p)[:2] == list(covered_by_intervals(s, p))
    # an open run counts only when flushed
    assert R.series_totals(runs_of(5)[:-1], p, flush=False) == [0, 0, 5, 0]
    assert R.series_totals(runs_of(5)[:-1], p, flush=True) == [5, 1, 5, 0]


# ---- AreaLocator on the numpy cells ----------------------------------------------------------------------------------------------
def test_locator_finds_the_text_band(clip):
    frames, _truth = clip
    loc = area_locator.AreaLocator(R.NumpyCells(), **LOCATOR)
    area = loc.run(list(frames), FPS)
    assert loc.params(FPS)[4:] == (5, 40) and loc.frames_scanned == len(frames) == 66
    assert as_tuple(area) == R.locate(loc.totals, 66, (0, H, 0, W), (H, W))
    boxes = np.array(text_boxes())
    ty0, ty1, tx0, tx1 = boxes[:, 0].min(), boxes[:, 1].max(), boxes[:, 2].min(), boxes[:, 3].max()
    assert ty0 == 328 and ty1 in (348, 349)                          # a line of 20 or 21 rows
    for y0, y1, x0, x1 in boxes:
        assert area.ymin <= y0 and y1 <= area.ymax and area.xmin <= x0 and x1 <= area.xmax
    # at most two cells beyond the union of the text boxes on any side (a cell's own coarseness plus the padding cell)
    assert ty0 - area.ymin <= 16 and area.ymax - ty1 <= 16
    assert tx0 - area.xmin <= 128 and area.xmax - tx1 <= 128
    assert area.ymin >= LOGO[1] and area.ymin > BARS[1]              # the logo's and the flicker's rows lie outside
    rows = np.where(loc.totals[..., 2] >= 0.95 * 66, 0, loc.totals[..., 0]).sum(1)
    logo_rows, bar_rows, text_rows = rows[0:5], rows[21:24], rows[41:43]
    # the flicker's chance runs of 5 frames stay far below the row_frac share of the text rows that would let them compete
    assert logo_rows.max() == 0 and 0 < bar_rows.max() < 0.25 * text_rows.min() and text_rows.min() >= 150
    assert loc.totals[1:4, 0, 2].min() == 66                         # the logo is there in every frame


@pytest.mark.parametrize("batch", [1, 7, 64])
def test_locator_batches_give_one_calls_totals(clip, batch):
    frames, _truth = clip
    whole = R.clip_totals(frames, (0, H, 0, W), area_locator.AreaLocator(**LOCATOR).params(FPS))
    cells = R.NumpyCells()
    loc = area_locator.AreaLocator(cells, batch=batch, **LOCATOR)
    loc.run(iter(frames), FPS)
    assert np.array_equal(loc.totals, whole)
    assert cells.calls == (66 + batch - 1) // batch + 1               # every frame once, then the flush


def test_locator_probe_and_search_area(clip):
    frames, _truth = clip
    p = area_locator.AreaLocator(**LOCATOR).params(FPS)
    loc = area_locator.AreaLocator(R.NumpyCells(), probe=(7, 26), **LOCATOR)
    loc.run(list(frames), FPS)
    assert loc.frames_scanned == 26 and np.array_equal(loc.totals, R.clip_totals(frames[6:32], (0, H, 0, W), p))
    band = extractor.SubtitleArea(ymin=180, ymax=H, xmin=30, xmax=W + 50)
    loc = area_locator.AreaLocator(R.NumpyCells(), search_area=band, **LOCATOR)
    area = loc.run(list(frames), FPS)
    assert np.array_equal(loc.totals, R.clip_totals(frames[:, 180:], (0, 180, 30, W), p))
    assert as_tuple(area) == R.locate(loc.totals, 66, (180, H, 30, W), (H, W))
    assert area.ymin <= 328 and area.ymax >= 348
    assert area_locator.AreaLocator(R.NumpyCells()).run([], FPS) is None
    with pytest.raises(ValueError):
        area_locator.AreaLocator(R.NumpyCells(), search_area=extractor.SubtitleArea(0, 2, 0, W)).run(list(frames[:2]), FPS)


def test_locator_parameters():
    loc = area_locator.AreaLocator(change_ratio=0.4, min_seconds=0.3, max_seconds=20)
    assert loc.params(25.0) == (128, 16, 2, 5, 8, 500)
    assert loc.params(3.0)[4:] == (2, 60)
    assert area_locator.AreaLocator(change_ratio=1 / 3).params(25.0)[2:4] == (1, 3)
    assert area_locator.AreaLocator(change_ratio=0.333).params(25.0)[2:4] == (333, 1000)
    with pytest.raises(ValueError):
        area_locator.AreaLocator(change_ratio=0.0)


# ---- the extractor -----------------------------------------------------------------------------------------------------------------
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


def run_extractor(frames, truth, sub_area, **kw):
    src = extractor.ArraySource(list(stamped(frames)), FPS)
    ocr = ScriptedOcr(truth)
    ex = extractor.SubtitleExtractor(src, ocr, sub_area=sub_area, mode="fast", frame_selector="change", change_counter=NumpyCounter(),
                                     drop_score=0.0, batch=8, **kw)
    text = ex.run()
    return ex, (text, ex.intervals, ex.raw_lines, ex.short_lines, ocr.seen)


def test_extractor_auto_area_equals_the_area_passed(clip, monkeypatch):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    frames, truth = clip
    cells = R.NumpyCells()
    auto, got = run_extractor(frames, truth, "auto", area_params=dict(cells_fn=cells, **LOCATOR))
    assert auto.located_area is not None and auto.sub_area == auto.located_area
    assert as_tuple(auto.located_area) == as_tuple(area_locator.AreaLocator(R.NumpyCells(), **LOCATOR).run(list(frames), FPS))
    assert cells.calls == (66 + 7) // 8 + 1                       # the extractor's batch size, one pass
    given, want = run_extractor(frames, truth, auto.located_area)
    assert given.located_area is None
    assert got == want
    text, intervals, _raw, _short, seen = got
    assert len(intervals) == len(truth) and len(seen) == len(truth) and text.count(" --> ") >= 3


def test_extractor_auto_area_without_text_is_the_run_without_area(monkeypatch, caplog):
    monkeypatch.setattr(extractor, "_stack", lambda frames: frames)
    frames, truth = synth.make_clip([(None, 30)], H, W, seed=3)
    with caplog.at_level(logging.WARNING):
        auto, got = run_extractor(frames, truth, "auto", area_params=dict(cells_fn=R.NumpyCells(), **LOCATOR))
    assert auto.located_area is None and auto.sub_area is None
    assert any("no subtitle area" in r.getMessage() for r in caplog.records)
    _none, want = run_extractor(frames, truth, None)
    assert got == want and got[1] is None                        # no intervals: the fps sampler ran


# ---- command line ----------------------------------------------------------------------------------------------------------------
def test_cli_prints_the_area_or_exits_1(clip, tmp_path, capsys):
    frames, _truth = clip
    path = tmp_path / "clip.npy"
    np.save(path, frames)
    assert area_locator.main([str(path), "--fps", "10"], cells_fn=R.NumpyCells()) == 0
    line = capsys.readouterr().out.strip()
    want = area_locator.AreaLocator(R.NumpyCells()).run(list(frames), 10.0)
    assert line == f"{want.ymin} {want.ymax} {want.xmin} {want.xmax}"
    assert want.ymin <= 328 and want.ymax >= 348 and want.ymin >= LOGO[1]
    bare = tmp_path / "bare.npy"
    np.save(bare, synth.make_clip([(None, 12)], H, W, seed=3)[0])
    assert area_locator.main([str(bare), "--fps", "10"], cells_fn=R.NumpyCells()) == 1
    captured = capsys.readouterr()
    assert "no subtitle area found in 12 frames" in captured.err and captured.out == ""
    assert area_locator.main([str(path), "--fps", "10", "--json", "--probe", "7", "40"], cells_fn=R.NumpyCells()) == 0
    assert '"frames_scanned": 40' in capsys.readouterr().out
    assert area_locator.main([str(path)], cells_fn=R.NumpyCells()) == 2                  # a .npy stack carries no frame rate
