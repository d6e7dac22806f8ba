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

    python -m vse_amd.area_locator VIDEO [--fps F --size WxH --layout i420|nv12] [--probe START COUNT] [--json]

prints `ymin ymax xmin xmax`; VIDEO is what ingest.open_source reads.
"""
import argparse
import itertools
import json
import sys
from fractions import Fraction

import numpy as np

from .engine import CellParams

CELL_H, CELL_W = 8, 64          # interior pixels of a cell (the tile of csrc/frame_change.hip)


def cells_dims(area_h, area_w):
    """(gy, gx) of a region of area_h x area_w pixels: vse_frame_cells_dims."""
    return (area_h - 2 + CELL_H - 1) // CELL_H, (area_w - 2 + CELL_W - 1) // CELL_W


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
    covered = np.where(totals[..., 2] >= static_frac * frames_scanned, 0, totals[..., 0])
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


class EngineCells:
    """cells_fn of AreaLocator on the GPU (Context.frame_cells): keeps the device state of the last region between calls."""

    def __init__(self, ctx):
        self.ctx = ctx
        self._state = None
        self._key = None

    def __call__(self, frames, area, params, reset, flush):
        t = self.ctx.torch
        y0, y1, x0, x1 = area
        if frames is None:
            frames = t.empty((0, y1, x1, 3), dtype=t.uint8, device=self.ctx.tdev)
        elif not t.is_tensor(frames):
            frames = t.from_numpy(np.ascontiguousarray(frames)).to(self.ctx.tdev)
        if self._key != (y1 - y0, x1 - x0):
            self._key = (y1 - y0, x1 - x0)
            self._state = self.ctx.frame_cells_state(*self._key)
            reset = True
        return self.ctx.frame_cells(frames, area, params, self._state, reset, flush)


class AreaLocator:
    """Frames in, subtitle area out (see the module text for the rule and what the defaults rest on).

    cells_fn(frames uint8 [n,h,w,3] | None, area (y0, y1, x0, x1) in their pixels, engine.CellParams, reset, flush) -> int [gy,gx,4]
    totals since the last reset; it carries each cell's last mask and open run to the next call (reset on the first batch of a clip),
    and frames None with flush closes the open runs.  Default: EngineCells on the shim's device.
    probe = (first_frame, count): scan only `count` frames from the 1-based frame number first_frame on (default: the whole clip);
    search_area (.ymin .ymax .xmin .xmax): scan only this part of the picture; locate_kwargs: locate_area's fractions and padding."""

    def __init__(self, cells_fn=None, edge_thresh=128, min_edges=16, change_ratio=0.5, min_seconds=0.3, max_seconds=20.0, batch=64,
                 probe=None, search_area=None, **locate_kwargs):
        self.cells_fn = cells_fn
        self.edge_thresh, self.min_edges = int(edge_thresh), int(min_edges)
        self.ratio = Fraction(change_ratio).limit_denominator(1024)
        if self.ratio <= 0:
            raise ValueError(f"AreaLocator: change_ratio {change_ratio} is not at least 1 / 1024")
        self.min_seconds, self.max_seconds = min_seconds, max_seconds
        self.batch, self.probe, self.search_area, self.locate_kwargs = int(batch), probe, search_area, locate_kwargs
        self.totals = None
        self.frames_scanned = 0
        self.area = None

    def params(self, fps):
        min_frames = max(2, round(self.min_seconds * fps))
        return CellParams(self.edge_thresh, self.min_edges, self.ratio.numerator, self.ratio.denominator, min_frames,
                          max(min_frames, round(self.max_seconds * fps)))

    def run(self, frames, fps, uploader=None):
        """frames: iterable of uint8 BGR frames (or ingest.Yuv420Frame with an uploader) in decode order -> extractor.SubtitleArea or
        None; `totals` (host int32 [gy,gx,4]) and `frames_scanned` are kept on the object.  Staged like ChangeFrameSelector.run:
        whole frames, or the rows of search_area alone; with an uploader (staging.Uploader) through pinned memory on its producer
        thread.  The device keeps the totals: one read-back of a few KB after the last batch."""
        if self.cells_fn is None:
            from . import shim
            self.cells_fn = EngineCells(shim._context())
        it = iter(frames)
        if self.probe is not None:
            first_frame, count = (int(v) for v in self.probe)
            if first_frame < 1 or count < 1:
                raise ValueError(f"AreaLocator: probe {self.probe} is not (first frame >= 1, count >= 1)")
            it = itertools.islice(it, first_frame - 1, first_frame - 1 + count)
        self.totals, self.frames_scanned, self.area = None, 0, None
        first = next(it, None)
        if first is None:
            return None
        h, w = first.shape[:2]
        y0, y1, x0, x1 = 0, h, 0, w
        if self.search_area is not None:
            s = self.search_area
            y0, y1, x0, x1 = max(0, int(s.ymin)), min(h, int(s.ymax)), max(0, int(s.xmin)), min(w, int(s.xmax))
        if y1 - y0 < 3 or x1 - x0 < 3:
            raise ValueError(f"AreaLocator: the region [{y0}, {y1}) x [{x0}, {x1}) of a {h} x {w} frame is smaller than 3 x 3 pixels")
        area = (0, y1 - y0, x0, x1)
        params = self.params(fps)

        def batches():
            buf = [(None, first[y0:y1])]
            for f in it:
                if len(buf) == self.batch:
                    yield buf
                    buf = []
                buf.append((None, f[y0:y1]))
            if buf:
                yield buf

        if uploader is not None:
            from . import staging
            for k, (items, staged) in enumerate(staging.prefetch(batches(), uploader)):
                self.cells_fn(staged.tensor(), area, params, k == 0, False)
                self.frames_scanned += len(items)
        else:
            for k, items in enumerate(batches()):
                self.cells_fn(np.stack([f for _, f in items]), area, params, k == 0, False)
                self.frames_scanned += len(items)
        totals = self.cells_fn(None, area, params, False, True)
        self.totals = np.asarray(totals.cpu() if hasattr(totals, "cpu") else totals).astype(np.int32)
        self.area = locate_area(self.totals, self.frames_scanned, (y0, y1, x0, x1), (h, w), **self.locate_kwargs)
        return self.area


def main(argv=None, cells_fn=None):
    """cells_fn: see AreaLocator (None: the GPU, frames staged through an uploader, YUV 4:2:0 converted on the device)."""
    p = argparse.ArgumentParser(prog="python -m vse_amd.area_locator", description="Find a video's subtitle area on the GPU and print "
                                "it as `ymin ymax xmin xmax` (what SubtitleExtractor takes as sub_area).")
    p.add_argument("video", help="uncompressed BGR24 or Motion-JPEG AVI, a .npy frame stack, .y4m, or headerless .yuv / .i420 / .nv12")
    p.add_argument("--fps", type=float, default=None, help="frame rate, for files that carry none (.npy, headerless YUV)")
    p.add_argument("--size", default=None, metavar="WxH", help="frame size of a headerless YUV 4:2:0 file")
    p.add_argument("--layout", default=None, choices=("i420", "nv12"), help="plane layout of a headerless YUV 4:2:0 file [by extension]")
    p.add_argument("--probe", type=int, nargs=2, default=None, metavar=("START", "COUNT"),
                   help="scan COUNT frames from the 1-based frame number START on [the whole clip]")
    p.add_argument("--json", action="store_true", help="print a JSON object instead (area, frames scanned, grid size)")
    args = p.parse_args(argv)
    from . import ingest
    try:
        size = None
        if args.size is not None:
            w, sep, h = args.size.lower().partition("x")
            if not (sep and w.isdigit() and h.isdigit()):
                raise ValueError(f"--size takes WIDTHxHEIGHT, not {args.size!r}")
            size = (int(w), int(h))
        source = ingest.open_source(args.video, fps=args.fps, size=size, layout=args.layout)
        loc = AreaLocator(cells_fn, probe=args.probe)
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
                          "frames_scanned": loc.frames_scanned, "cells": list(loc.totals.shape[:2])}))
    else:
        print(area.ymin, area.ymax, area.xmin, area.xmax)
    return 0


if __name__ == "__main__":
    sys.exit(main())
