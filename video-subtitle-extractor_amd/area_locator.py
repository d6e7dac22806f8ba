"""Find the subtitle area of a clip on the GPU, so that the frame-accurate paths need no hand-drawn box.

In the reference a person draws the area in the GUI (config.subtitleSelectionAreas, backend/config.py:49) and SubtitleExtractor.run
needs it to take either frame-accurate path (backend/main.py:137-147).  The reference has no algorithm for this; this module plays
that role with its own, fully specified rule.  A subtitle is strong luma edges that hold still for between a fraction of a second
and a few seconds and then change all at once; a station logo never changes; scene edges change all the time.  The device looks at
every frame once (vse_frame_cells, csrc/frame_change.hip): the edge mask of frame_select's change selector, counted per cell of 8
x 64 interior pixels, with change_intervals' automaton run per cell, and hands back four integers per cell for the whole clip:
  covered  frames inside runs (stretches of present frames without a cut) of min_frames..max_frames frames,
  runs     how many such runs, present: frames with at least min_edges edge pixels, cuts: how many ratio cuts.
`locate_area` turns those integers into a rectangle on the host.

The defaults are a judgement, not a measurement on real footage (there is none to measure on): how well the rule finds the band
of a real film, with hard-coded logos, tickers or busy static scenery, is unmeasured.
  edge_thresh 128, change_ratio 0.5   the change selector's own;
  min_edges 16                        of a cell's 512 pixels: a stroke or two;
  min_seconds 0.3, max_seconds 20     shorter is flicker, longer is a logo or a caption burnt into the scene;
  row_frac 0.25, col_frac 0.05        a second text line counts when it is shown a quarter as long as the main one; the columns
                                      reach out to where text is shown a twentieth as long as in the busiest column;
  static_frac 0.95                    a cell present in 95 % of the scanned frames is a logo (clips shorter than max_seconds);
  pad_cells 1                         the rectangle is as coarse as the cells are, and the OCR filter wants the whole box inside.

Edge threshold per clip (edge_thresh="auto").  128 describes white text with a black outline; yellow text, a soft shadow, no outline
over a bright scene or a washed-out transfer put the text's gradient below it, and then no cell ever holds an edge: no area, no
intervals, an empty SRT.  The locator's own statistic tells working thresholds from failing ones (too high: nothing is an edge; too
low: the noise becomes edges that change every frame, and every frame is a cut), so the device evaluates several thresholds in the
same single pass (vse_frame_cells_multi: the bytes are read and the gradient computed once) and `pick_edge_thresh` takes the middle
of the plateau of thresholds whose best grid row scores at least plateau_frac of the best one:
  thresholds 24 32 48 64 96 128 160 192   about half an octave apart around the constant;
  plateau_frac 0.9                        a judgement like the defaults above, not a measurement.
With search_area set to a known subtitle area this is the calibration for a film whose box the user drew.
That calibration also runs inside the change selector's own pass, without a pass of its own (frame_select.CalibratingChangeSelector,
vse_frame_cells_counts; SubtitleExtractor's area_params={"streaming": True}): the cells of search_area tile the interior of the
selector's area and their mask is the selector's, so the kernel that keeps these totals also hands back the selector's counts at every
threshold, and `edge_thresh_scores` / `pick_edge_thresh` below decide on the same integers after the window's last frame.
The locator itself runs inside the change selector's pass as well (frame_select.LocatingChangeSelector; SubtitleExtractor's
area_params={"streaming_locate": True} with sub_area="auto"), which is what a pipe needs.  There the identity above fails by one pixel:
`locate_area` returns ymin = y0 + 1 + 8 (j0 - pad) and xmin = x0 + 1 + 64 (i0 - pad), so the interior of the located rectangle starts one
row and one column off the whole-frame cell grid (unless the clamp to 0 hits) and ends one short of it, and no sum of the cells' counts
is vse_frame_change's count on it.  A pixel's edge mask, however, depends on its four neighbours and the threshold only, so the cells'
kernel keeps its mask words, one bit per pixel and threshold (vse_frame_cells_masks), these totals decide as they always do after the
window's last frame, and vse_frame_masks_replay counts the located rectangle out of the kept words.
Known limits: the locator and the calibration run the CHANGE automaton unless `automaton="hold"`.  On a moving textured background
every frame is a cut in every cell at every threshold, nothing scores, no area is found and "auto" falls back to 128 with a warning.
How the rule behaves on real footage is unmeasured: there are no real clips here.

Held edges (automaton="hold"), for the footage of frame_select.HoldFrameSelector: the same cells, automaton, thresholds and rule, but
each cell counts the HELD mask of its frames (edge pixels that stay edges for `hold` frames; vse_frame_cells_hold), so the edges of a
texture that moves behind the subtitle drop out before the automaton sees them.  `hold` is HoldFrameSelector's: hold_frames, else
max(1, min(32, round(hold_seconds * fps))), and a run counts from max(min_frames, hold) frames on.  Known limit: texture that keeps
an edge on a pixel for `hold` frames is held too.  At low thresholds fine, fast texture does that: on synth.make_moving_clip(amp=(120,
120), cells=(8, 3)) with hold 8 the threshold 64 locates a wrong band and only the thresholds from 96 up the true one (EXPERIMENTS.md).
Real footage is unmeasured here as well.

Bounded runs (automaton="hold" with max_hold_seconds / max_hold_frames), for the footage of HoldFrameSelector(max_hold_seconds=...): a busy
background that STANDS STILL behind the subtitle (an interview, a news desk, shelves, a logo in the band).  On held masks its edges are
present in every frame, so the subtitle's own cells fall to the logo rule and score 0, and elsewhere they dilute every cell's cut ratio.
Here each cell counts the BOUNDED mask of its frames (edge pixels whose run is hold .. max_hold frames long; vse_frame_cells_hold_bounded):
the static edges drop out before the automaton sees them.  max_hold is HoldFrameSelector's: max_hold_frames, else round(max_hold_seconds *
fps), hold .. 4000.  Both None (the default): the held path above, call for call.  Known limits: a gap between two subtitles shorter than
max_hold lets the background runs under the text count (the text cuts them to a length in range), so the cells stay present through the
gap; a subtitle shown for longer than max_hold vanishes; a row is final only max_hold frames later, which the device keeps per cell (55 MB
for whole-frame 1080p at max_hold 360 and eight thresholds); 12-15 s is a guess.  Nothing is measured on real footage.

    python -m vse_amd.area_locator VIDEO [--fps F --size WxH --layout i420|nv12] [--probe START COUNT] [--edge-thresh auto|N]
                                         [--locator-automaton change|hold [--hold-seconds S | --hold-frames N]
                                          [--max-hold-seconds S | --max-hold-frames N]] [--json]

prints `ymin ymax xmin xmax` (and the chosen threshold as a fifth number when `--edge-thresh auto` was asked); VIDEO is what
ingest.open_source reads.
"""
import argparse
import itertools
import json
import logging
import sys
from fractions import Fraction

import numpy as np

from . import staging
from .engine import FRAME_HOLD_BOUNDED_MAX, CellParams, DeviceState
from .frame_select import band_batches

CELL_H, CELL_W = 8, 64          # interior pixels of a cell (the tile of csrc/frame_change.hip)
AUTO_THRESHOLDS = (24, 32, 48, 64, 96, 128, 160, 192)      # what edge_thresh="auto" chooses from
DEFAULT_EDGE_THRESH = 128       # the selectors' constant, and what "auto" falls back to when no threshold scores


def cells_dims(area_h, area_w):
    """(gy, gx) of a region of area_h x area_w pixels: vse_frame_cells_dims."""
    return (area_h - 2 + CELL_H - 1) // CELL_H, (area_w - 2 + CELL_W - 1) // CELL_W


def _covered(totals, frames_scanned, static_frac):
    """int64 [..., gy, gx, 4] -> covered per cell after the logo rule: a cell present in static_frac of the frames counts 0."""
    return np.where(totals[..., 2] >= static_frac * frames_scanned, 0, totals[..., 0])


def edge_thresh_scores(totals, frames_scanned, static_frac=0.95):
    """totals: int [nt,gy,gx,4] -> [nt] ints: per threshold the largest grid-row sum of covered after the logo rule, which is
    locate_area's `best` on that threshold's totals."""
    totals = np.asarray(totals, np.int64)
    if totals.ndim != 4 or totals.shape[3] != 4:
        raise ValueError(f"edge_thresh_scores: totals of shape {totals.shape}, not [nt, gy, gx, 4]")
    return [int(v) for v in _covered(totals, frames_scanned, static_frac).sum(2).max(1)]


def pick_edge_thresh(totals, thresholds, frames_scanned, static_frac=0.95, plateau_frac=0.9):
    """totals: int [nt,gy,gx,4] of vse_frame_cells_multi at the ascending `thresholds` -> the index of the threshold to use, or None
    when no threshold scores.  A pure function of integers: score[k] = edge_thresh_scores; the working set is the maximal contiguous
    run of k around the arg-max (ties: the threshold nearest 128, then the lower one) with score[k] >= plateau_frac * max(score);
    the result is that run's element (len - 1) // 2, the middle of the plateau, so that the choice has margin on both sides."""
    thresholds = [int(v) for v in thresholds]
    scores = edge_thresh_scores(totals, frames_scanned, static_frac)
    if len(scores) != len(thresholds):
        raise ValueError(f"pick_edge_thresh: totals for {len(scores)} thresholds, {len(thresholds)} given")
    best = max(scores)
    if best <= 0:
        return None
    k0 = k1 = min((k for k in range(len(scores)) if scores[k] == best), key=lambda k: (abs(thresholds[k] - DEFAULT_EDGE_THRESH), k))
    while k0 > 0 and scores[k0 - 1] >= plateau_frac * best:
        k0 -= 1
    while k1 < len(scores) - 1 and scores[k1 + 1] >= plateau_frac * best:
        k1 += 1
    return k0 + (k1 - k0) // 2


def locate_area(totals, frames_scanned, region, frame_hw, row_frac=0.25, col_frac=0.05, static_frac=0.95, pad_cells=1):
    """totals: int [gy,gx,4] covered / runs / present / cuts per cell of `region` = (y0, y1, x0, x1) in the pixels of a frame of
    frame_hw = (height, width) -> extractor.SubtitleArea, or None when no cell holds a qualifying run.  A pure function of integers:
      covered of a cell with present >= static_frac * frames_scanned counts as 0 (a logo);
      row_score = covered summed over a grid row; the band starts at the arg-max row (ties: the lowest row in the picture) and grows
      up and down while the neighbouring row scores >= row_frac * the maximum;
      within those rows a column's score is its covered sum; the band keeps the first to the last column scoring >= col_frac * the best;
      interior row 8 j is region row 1 + 8 j (columns: 64 i, 1 + 64 i); the rectangle is padded by pad_cells cells on every side
      and clamped to the frame.
    Only the strongest band is returned: a second band elsewhere in the picture (subtitles at the top as well, or two languages far
    apart) is ignored."""
    from .extractor import SubtitleArea
    totals = np.asarray(totals, np.int64)
    y0, y1, x0, x1 = (int(v) for v in region)
    gy, gx = cells_dims(y1 - y0, x1 - x0)
    if totals.shape != (gy, gx, 4):
        raise ValueError(f"locate_area: totals of shape {totals.shape} for a region of {gy} x {gx} cells")
    covered = _covered(totals, frames_scanned, static_frac)
    row_score = covered.sum(1)
    best = int(row_score.max())
    if best <= 0:
        return None
    j0 = j1 = int(np.flatnonzero(row_score == best)[-1])
    while j0 > 0 and row_score[j0 - 1] >= row_frac * best:
        j0 -= 1
    while j1 < gy - 1 and row_score[j1 + 1] >= row_frac * best:
        j1 += 1
    col_score = covered[j0:j1 + 1].sum(0)
    keep = np.flatnonzero(col_score >= col_frac * int(col_score.max()))
    i0, i1 = int(keep[0]), int(keep[-1])
    h, w = (int(v) for v in frame_hw)
    ymin = y0 + 1 + CELL_H * (j0 - pad_cells)
    ymax = min(y0 + 1 + CELL_H * (j1 + 1), y1 - 1) + CELL_H * pad_cells
    xmin = x0 + 1 + CELL_W * (i0 - pad_cells)
    xmax = min(x0 + 1 + CELL_W * (i1 + 1), x1 - 1) + CELL_W * pad_cells
    return SubtitleArea(ymin=max(0, ymin), ymax=min(h, ymax), xmin=max(0, xmin), xmax=min(w, xmax))


class EngineCells(DeviceState):
    """cells_fn of AreaLocator on the GPU (Context.frame_cells; with `thresholds`, Context.frame_cells_multi; with `hold`,
    Context.frame_cells_hold at `thresholds` or at params.edge_thresh alone; with `max_hold` as well, Context.frame_cells_hold_bounded):
    keeps the device state of the last region (and threshold count, and hold or max_hold) between calls, and with a hold the number of
    frames fed since the last reset."""

    def __init__(self, ctx):
        super().__init__(ctx)
        self.fed = 0

    def __call__(self, frames, area, params, reset, flush, thresholds=None, hold=None, max_hold=None):
        t = self.ctx.torch
        y0, y1, x0, x1 = area
        frames = t.empty((0, y1, x1, 3), dtype=t.uint8, device=self.ctx.tdev) if frames is None else self._device(frames)
        if max_hold is not None:
            if hold is None:
                raise ValueError("EngineCells: max_hold needs a hold")
            ths = (params.edge_thresh,) if thresholds is None else tuple(thresholds)
            if self._fresh((y1 - y0, x1 - x0, len(ths), "max_hold", int(max_hold)),
                           lambda h, w, nt, _, mh: self.ctx.frame_cells_hold_bounded_state(h, w, nt, mh)) or reset:
                self.fed = 0
            totals = self.ctx.frame_cells_hold_bounded(frames, area, ths, hold, max_hold, params, self._state, self.fed, flush)
            self.fed += len(frames)
            return totals[0] if thresholds is None else totals
        if hold is not None:
            ths = (params.edge_thresh,) if thresholds is None else tuple(thresholds)
            if self._fresh((y1 - y0, x1 - x0, len(ths), int(hold)), self.ctx.frame_cells_hold_state) or reset:
                self.fed = 0
            totals = self.ctx.frame_cells_hold(frames, area, ths, hold, params, self._state, self.fed, flush)
            self.fed += len(frames)
            return totals[0] if thresholds is None else totals
        if thresholds is None:
            reset = self._fresh((y1 - y0, x1 - x0), self.ctx.frame_cells_state) or reset
            return self.ctx.frame_cells(frames, area, params, self._state, reset, flush)
        reset = self._fresh((y1 - y0, x1 - x0, len(thresholds)), self.ctx.frame_cells_multi_state) or reset
        return self.ctx.frame_cells_multi(frames, area, thresholds, params, self._state, reset, flush)


class AreaLocator:
    """Frames in, subtitle area out (see the module text for the rule and what the defaults rest on).

    cells_fn(frames uint8 [n,h,w,3] | None, area (y0, y1, x0, x1) in their pixels, engine.CellParams, reset, flush) -> int [gy,gx,4]
    totals since the last reset; it carries each cell's last mask and open run to the next call (reset on the first batch of a clip),
    and frames None with flush closes the open runs.  Default: EngineCells on the shim's device.
    probe = (first_frame, count): scan only `count` frames from the 1-based frame number first_frame on (default: the whole clip);
    search_area (.ymin .ymax .xmin .xmax): scan only this part of the picture; locate_kwargs: locate_area's fractions and padding.
    edge_thresh="auto": the same single pass evaluates all `thresholds` (1..8, ascending, each 1..255): cells_fn is then called with
    thresholds=that tuple as well, ignores params.edge_thresh and returns int [nt,gy,gx,4]; run() keeps `totals` of all thresholds,
    `scores` (edge_thresh_scores) and `edge_thresh` (the threshold pick_edge_thresh chose, None when none scores: one warning, and
    the callers fall back to 128) and locates the area on the chosen threshold's totals.  plateau_frac: pick_edge_thresh's.
    automaton="hold" (default "change"; see the module text): cells_fn is called with hold=`hold` as a further keyword (and params'
    min_frames at least `hold`) and counts held masks; `hold` is kept on the object: hold_frames, or max(1, min(32, round(hold_seconds
    * fps))) when that is None.  With "change" cells_fn gets no such keyword.
    max_hold_seconds / max_hold_frames (with automaton="hold" only; both None: the call above, keyword for keyword): cells_fn gets
    max_hold=`max_hold` as well and counts bounded masks; `max_hold` is kept on the object: max_hold_frames, or round(max_hold_seconds *
    fps) when that is None (HoldFrameSelector's rule); below `hold` or above 4000 is a ValueError.
    key_fn(frames, area) -> frames of the same shape (frame_select.ColourKey.apply, EngineKey): when given, every staged batch goes
    through it and cells_fn counts on its result, so the cells see the colour key's gradient (coloured subtitles).  None: cells_fn
    receives the staged data itself."""

    def __init__(self, cells_fn=None, edge_thresh=128, min_edges=16, change_ratio=0.5, min_seconds=0.3, max_seconds=20.0, batch=64,
                 probe=None, search_area=None, thresholds=AUTO_THRESHOLDS, plateau_frac=0.9, automaton="change", hold_seconds=0.3,
                 hold_frames=None, max_hold_seconds=None, max_hold_frames=None, key_fn=None, **locate_kwargs):
        if automaton not in ("change", "hold"):
            raise ValueError(f"AreaLocator: automaton must be 'change' or 'hold', not {automaton!r}")
        if hold_frames is not None and not 1 <= int(hold_frames) <= 32:
            raise ValueError(f"AreaLocator: hold_frames must be 1..32, not {hold_frames}")
        self.bounded = max_hold_seconds is not None or max_hold_frames is not None
        if self.bounded and automaton != "hold":
            raise ValueError("AreaLocator: max_hold_seconds / max_hold_frames need automaton='hold'")
        if max_hold_frames is not None and not 1 <= int(max_hold_frames) <= FRAME_HOLD_BOUNDED_MAX:
            raise ValueError(f"AreaLocator: max_hold_frames must be 1..{FRAME_HOLD_BOUNDED_MAX}, not {max_hold_frames}")
        if hold_frames is not None and max_hold_frames is not None and int(max_hold_frames) < int(hold_frames):
            raise ValueError(f"AreaLocator: max_hold_frames {max_hold_frames} is below hold_frames {hold_frames}")
        self.automaton, self.hold_seconds, self.hold_frames, self.hold = automaton, hold_seconds, hold_frames, None
        self.max_hold_seconds, self.max_hold_frames, self.max_hold = max_hold_seconds, max_hold_frames, None
        self.cells_fn, self.key_fn = cells_fn, key_fn
        self.auto = isinstance(edge_thresh, str) and edge_thresh == "auto"
        self.thresholds = tuple(int(v) for v in thresholds)
        if self.auto and not (1 <= len(self.thresholds) <= 8 and all(1 <= v <= 255 for v in self.thresholds)
                              and all(a < b for a, b in zip(self.thresholds, self.thresholds[1:]))):
            raise ValueError(f"AreaLocator: thresholds {thresholds} are not 1..8 ascending values in 1..255")
        self.edge_thresh, self.min_edges = None if self.auto else int(edge_thresh), int(min_edges)
        self.plateau_frac, self.scores = plateau_frac, None
        self.ratio = Fraction(change_ratio).limit_denominator(1024)
        if self.ratio <= 0:
            raise ValueError(f"AreaLocator: change_ratio {change_ratio} is not at least 1 / 1024")
        self.min_seconds, self.max_seconds = min_seconds, max_seconds
        self.batch, self.probe, self.search_area, self.locate_kwargs = int(batch), probe, search_area, locate_kwargs
        self.totals = None
        self.frames_scanned = 0
        self.area = None

    def hold_for(self, fps):
        """The hold in frames at this frame rate (HoldFrameSelector's rule), None with the change automaton."""
        if self.automaton != "hold":
            return None
        return int(self.hold_frames) if self.hold_frames is not None else max(1, min(32, int(round(self.hold_seconds * fps))))

    def max_hold_for(self, fps):
        """The longest run that counts, in frames at this frame rate (HoldFrameSelector's rule), None when runs are not bounded."""
        if not self.bounded:
            return None
        hold = self.hold_for(fps)
        max_hold = int(self.max_hold_frames if self.max_hold_frames is not None else round(self.max_hold_seconds * fps))
        if not hold <= max_hold <= FRAME_HOLD_BOUNDED_MAX:
            raise ValueError(f"AreaLocator: max_hold must be hold ({hold}) .. {FRAME_HOLD_BOUNDED_MAX} frames, not {max_hold}")
        return max_hold

    def describe_automaton(self):
        """How the warnings name the automaton: `change`, `hold`, or `hold` with its bounds."""
        return self.automaton if self.max_hold is None else f"{self.automaton} (runs of {self.hold}..{self.max_hold} frames)"

    def params(self, fps):
        min_frames = max(2, round(self.min_seconds * fps), self.hold_for(fps) or 0)
        return CellParams(0 if self.auto else self.edge_thresh, self.min_edges, self.ratio.numerator, self.ratio.denominator, min_frames,
                          max(min_frames, round(self.max_seconds * fps)))

    def run(self, frames, fps, uploader=None):
        """frames: iterable of uint8 BGR frames (or ingest.Yuv420Frame with an uploader) in decode order -> extractor.SubtitleArea or
        None; `totals` (host int32 [gy,gx,4]; [nt,gy,gx,4] with edge_thresh="auto") and `frames_scanned` are kept on the object.  Whole
        frames, or the rows of search_area alone, are batched by frame_select.band_batches and staged by staging.staged_batches.  The
        device keeps the totals: one read-back of a few KB after the last batch."""
        if self.cells_fn is None:
            from . import shim
            self.cells_fn = EngineCells(shim._context())
        it = iter(frames)
        if self.probe is not None:
            first_frame, count = (int(v) for v in self.probe)
            if first_frame < 1 or count < 1:
                raise ValueError(f"AreaLocator: probe {self.probe} is not (first frame >= 1, count >= 1)")
            it = itertools.islice(it, first_frame - 1, first_frame - 1 + count)
        self.totals, self.frames_scanned, self.area, self.scores = None, 0, None, None
        if self.auto:
            self.edge_thresh = None
        bands = band_batches(it, self.search_area, self.batch, "AreaLocator")
        area = bands.area
        if area is None:
            return None
        params = self.params(fps)
        self.hold, self.max_hold = self.hold_for(fps), self.max_hold_for(fps)
        kw = {**({"thresholds": self.thresholds} if self.auto else {}), **({"hold": self.hold} if self.hold is not None else {}),
              **({"max_hold": self.max_hold} if self.max_hold is not None else {})}
        cells = self.cells_fn if not kw else (lambda *a: self.cells_fn(*a, **kw))
        for items, data in staging.staged_batches(bands, uploader):
            cells(data if self.key_fn is None else self.key_fn(data, area), area, params, not self.frames_scanned, False)
            self.frames_scanned += len(items)
        totals = cells(None, area, params, False, True)
        self.totals = np.asarray(totals.cpu() if hasattr(totals, "cpu") else totals).astype(np.int32)
        chosen = self.totals
        if self.auto:
            static_frac = self.locate_kwargs.get("static_frac", 0.95)
            self.scores = edge_thresh_scores(self.totals, self.frames_scanned, static_frac)
            k = pick_edge_thresh(self.totals, self.thresholds, self.frames_scanned, static_frac, self.plateau_frac)
            if k is None:
                logging.getLogger(__name__).warning("edge_thresh='auto': none of the thresholds %s scores with the %s automaton in %d "
                                                    "frames; falling back to %d", self.thresholds, self.describe_automaton(), self.frames_scanned,
                                                    DEFAULT_EDGE_THRESH)
                return None
            self.edge_thresh, chosen = self.thresholds[k], self.totals[k]
        self.area = locate_area(chosen, self.frames_scanned, bands.geometry, bands.frame_hw, **self.locate_kwargs)
        return self.area


def parse_edge_thresh(text):
    """`auto` or an integer 1..255 (the command lines' --edge-thresh)."""
    if text == "auto":
        return "auto"
    if not (text.isdigit() and 1 <= int(text) <= 255):
        raise ValueError(f"--edge-thresh takes auto or an integer 1..255, not {text!r}")
    return int(text)


def main(argv=None, cells_fn=None, key_fn=None):
    """cells_fn: see AreaLocator (None: the GPU, frames staged through an uploader, YUV 4:2:0 converted on the device); key_fn: given the
    frame_select.ColourKey of `--text-colour`, what takes the key (None: frame_select.EngineKey on the GPU)."""
    p = argparse.ArgumentParser(prog="python -m vse_amd.area_locator", description="Find a video's subtitle area on the GPU and print "
                                "it as `ymin ymax xmin xmax` (what SubtitleExtractor takes as sub_area).")
    p.add_argument("video", help="uncompressed BGR24 or Motion-JPEG AVI, a .npy frame stack, .y4m, or headerless .yuv / .i420 / .nv12")
    p.add_argument("--fps", type=float, default=None, help="frame rate, for files that carry none (.npy, headerless YUV)")
    p.add_argument("--size", default=None, metavar="WxH", help="frame size of a headerless YUV 4:2:0 file")
    p.add_argument("--layout", default=None, choices=("i420", "nv12"), help="plane layout of a headerless YUV 4:2:0 file [by extension]")
    p.add_argument("--matrix", default="bt601", choices=("bt601", "bt709", "bt2020"), help="YUV -> BGR matrix [bt601]; bt2020 needs "
                   "--wide-yuv or --pix-fmt")
    p.add_argument("--wide-yuv", action="store_true", help="Y4M: also accept 9 to 16 bits, 4:2:2, 4:4:4, grey and full range")
    p.add_argument("--range", default="auto", choices=("auto", "limited", "full"), help="--wide-yuv / --pix-fmt: the colour range [auto]")
    p.add_argument("--pix-fmt", default=None, metavar="NAME", help="pixel format of a headerless YUV file by FFmpeg's name (yuv420p10le, "
                   "p010le ...) [by extension]")
    p.add_argument("--deinterlace", default=None, choices=("adaptive", "interpolate", "match"), help="interlaced YUV (Y4M with It / Ib, or a "
                   "headerless file with --pix-fmt and --field-order): deinterlace on the GPU as the extractor does; match is for film "
                   "carried in interlaced video (3:2 pulldown, shifted fields); turns --wide-yuv on [none]")
    p.add_argument("--field-order", default="auto", choices=("auto", "tff", "bff"), help="--deinterlace: which field comes first [auto: the "
                   "Y4M header's]")
    p.add_argument("--deinterlace-thresh", type=int, default=10, metavar="N", help="--deinterlace adaptive: a sample that changed by more "
                   "than N 8-bit levels since the previous frame has moved, 0..255 [10]")
    from .extractor import add_colour_arguments, add_match_arguments, add_square_arguments, colour_arguments, match_arguments, square_arguments
    add_match_arguments(p)
    add_square_arguments(p)
    add_colour_arguments(p)
    p.add_argument("--transfer", default=None, choices=("pq", "hlg"), help="HDR video (needs --wide-yuv or --pix-fmt): undo PQ or HLG and "
                   "tone-map to SDR on the GPU [none]")
    p.add_argument("--white-nits", type=float, default=None, metavar="N", help="--transfer: the luminance that becomes SDR white [203]")
    p.add_argument("--peak-nits", type=float, default=None, metavar="N", help="--transfer: the luminance the roll-off brings down to SDR "
                   "white [1000]")
    p.add_argument("--tone-curve", default=None, choices=("knee", "clip"), help="--transfer: roll highlights off, or clip at SDR white [knee]")
    p.add_argument("--probe", type=int, nargs=2, default=None, metavar=("START", "COUNT"),
                   help="scan COUNT frames from the 1-based frame number START on [the whole clip]")
    p.add_argument("--edge-thresh", default=str(DEFAULT_EDGE_THRESH), metavar="auto|N", help="luma gradient that makes an edge pixel, or "
                   "`auto` to choose it for this clip in the same pass (printed as a fifth number) [128]")
    p.add_argument("--locator-automaton", default="change", choices=("change", "hold"), help="what the cells count: every edge pixel, or "
                   "with `hold` only edges that hold still, for a textured background that moves behind the subtitles [change]")
    p.add_argument("--hold-seconds", type=float, default=0.3, help="with --locator-automaton hold: how long an edge must hold still [0.3]")
    p.add_argument("--hold-frames", type=int, default=None, help="... the same in frames, 1..32 [from --hold-seconds and the frame rate]")
    p.add_argument("--max-hold-seconds", type=float, default=None, help="with --locator-automaton hold: count only edges that hold still "
                   "for at most this long, for a busy background that stands still behind the subtitles [no bound]")
    p.add_argument("--max-hold-frames", type=int, default=None, help="... the same in frames, up to 4000 [from --max-hold-seconds and the "
                   "frame rate]")
    p.add_argument("--json", action="store_true", help="print a JSON object instead (area, frames scanned, grid size, edge threshold, "
                   "the automaton, its hold and max_hold in frames, and with `auto` the score of every threshold tried)")
    args = p.parse_args(argv)
    if (args.max_hold_seconds is not None or args.max_hold_frames is not None) and args.locator_automaton != "hold":
        print("area_locator: --max-hold-seconds / --max-hold-frames need --locator-automaton hold", file=sys.stderr)
        return 2
    from . import ingest
    try:
        size = None
        if args.size is not None:
            w, sep, h = args.size.lower().partition("x")
            if not (sep and w.isdigit() and h.isdigit()):
                raise ValueError(f"--size takes WIDTHxHEIGHT, not {args.size!r}")
            size = (int(w), int(h))
        from .extractor import tone_arguments
        colour = colour_arguments(args)
        if colour is not None:
            from .frame_select import EngineKey
            colour = EngineKey(None, colour) if key_fn is None else key_fn(colour)
        if args.deinterlace is None and (args.field_order != "auto" or args.deinterlace_thresh != 10):
            raise ValueError("--field-order and --deinterlace-thresh belong to --deinterlace adaptive | interpolate | match")
        fields = {} if args.deinterlace is None else dict(deinterlace=args.deinterlace, field_order=args.field_order,
                                                          deinterlace_thresh=args.deinterlace_thresh)
        source = ingest.open_source(args.video, fps=args.fps, size=size, layout=args.layout, matrix=args.matrix,
                                    wide=args.wide_yuv or args.deinterlace is not None, range=args.range, pix_fmt=args.pix_fmt,
                                    **fields, **match_arguments(args), **tone_arguments(args), **square_arguments(args))
        loc = AreaLocator(cells_fn, probe=args.probe, edge_thresh=parse_edge_thresh(args.edge_thresh), automaton=args.locator_automaton,
                          hold_seconds=args.hold_seconds, hold_frames=args.hold_frames, max_hold_seconds=args.max_hold_seconds,
                          max_hold_frames=args.max_hold_frames, key_fn=colour)
        if cells_fn is None:
            from . import staging
            up = staging.default_uploader()
            area = loc.run(source.raw_frames() if up is not None and hasattr(source, "raw_frames") else source.frames(), source.fps, up)
        else:
            area = loc.run(source.frames(), source.fps)
    except (OSError, ValueError) as e:
        print(f"area_locator: {e}", file=sys.stderr)
        return 2
    if area is None:
        print(f"area_locator: no subtitle area found in {loc.frames_scanned} frames of {args.video}", file=sys.stderr)
        return 1
    if args.json:
        print(json.dumps({"ymin": area.ymin, "ymax": area.ymax, "xmin": area.xmin, "xmax": area.xmax,
                          "frames_scanned": loc.frames_scanned, "cells": list(loc.totals.shape[-3:-1]), "edge_thresh": loc.edge_thresh,
                          "scores": dict(zip(map(str, loc.thresholds), loc.scores)) if loc.auto else None,
                          "automaton": loc.automaton, "hold": loc.hold, "max_hold": loc.max_hold}))
    elif loc.auto:
        print(area.ymin, area.ymax, area.xmin, area.xmax, loc.edge_thresh)
    else:
        print(area.ymin, area.ymax, area.xmin, area.xmax)
    return 0


if __name__ == "__main__":
    sys.exit(main())
