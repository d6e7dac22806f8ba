"""numpy / plain-Python restatement of the subtitle-area locator (include/vse_hip.h vse_frame_cells and
vse_amd.area_locator.locate_area), written from the specification and independent of the product code: the device kernel must agree
with it integer for integer, and the CPU tests drive the host side with it."""
from collections import namedtuple

import numpy as np

from frame_change_ref import edge_mask

Params = namedtuple("Params", "edge_thresh min_edges ratio_num ratio_den min_frames max_frames")      # the field order of engine.CellParams


def dims(area_h, area_w):
    return -(-(area_h - 2) // 8), -(-(area_w - 2) // 64)


def cell_sums(mask):
    """bool [n, ih, iw] -> int64 [n, gy, gx]: the mask summed over cells of 8 x 64 (the last ones cut off)."""
    n, ih, iw = mask.shape
    gy, gx = -(-ih // 8), -(-iw // 64)
    pad = np.zeros((n, gy * 8, gx * 64), np.int64)
    pad[:, :ih, :iw] = mask
    return pad.reshape(n, gy, 8, gx, 64).sum((2, 4))


def cell_counts(frames, area, edge_thresh, prev=None):
    """uint8 BGR [n,H,W,3], area (y0, y1, x0, x1) -> (int32 [n,gy,gx,3] edges / appeared / vanished per frame and cell, the last
    frame's mask).  prev: the mask of the frame before the first (None = empty)."""
    e = edge_mask(frames, area, edge_thresh)
    p = np.concatenate([np.zeros_like(e[:1]) if prev is None else prev[None], e[:-1]])
    return np.stack([cell_sums(e), cell_sums(e & ~p), cell_sums(p & ~e)], -1).astype(np.int32), e[-1]


class Automaton:
    """One cell: (e, a, v) per frame in, (covered, runs, present, cuts) out; `prev_e` and `run` are what a batch hands to the next."""

    def __init__(self, p):
        self.p = p
        self.prev_e = self.run = 0
        self.covered = self.runs = self.present = self.cuts = 0

    def close(self):
        if self.p.min_frames <= self.run <= self.p.max_frames:
            self.covered += self.run
            self.runs += 1
        self.run = 0

    def feed(self, e, a, v):
        e, a, v = int(e), int(a), int(v)
        if e < self.p.min_edges:
            self.close()
        else:
            self.present += 1
            union = self.prev_e + a
            if self.run and union > 0 and (a + v) * self.p.ratio_den >= self.p.ratio_num * union:
                self.cuts += 1
                self.close()
            self.run += 1
        self.prev_e = e

    def totals(self):
        return [self.covered, self.runs, self.present, self.cuts]


def series_totals(series, p, flush=True):
    """[(e, a, v)] of one cell -> [covered, runs, present, cuts]."""
    m = Automaton(p)
    for e, a, v in series:
        m.feed(e, a, v)
    if flush:
        m.close()
    return m.totals()


class NumpyCells:
    """cells_fn of area_locator.AreaLocator on the host: carries the last mask and every cell's automaton from one call to the next."""

    def __init__(self):
        self.prev = self.cells = None
        self.calls = 0

    def __call__(self, frames, area, params, reset, flush):
        self.calls += 1
        p = Params(*params)
        gy, gx = dims(area[1] - area[0], area[3] - area[2])
        if reset or self.cells is None:
            self.prev, self.cells = None, [[Automaton(p) for _ in range(gx)] for _ in range(gy)]
        if frames is not None and len(frames):
            c, self.prev = cell_counts(np.asarray(frames), area, p.edge_thresh, self.prev)
            for t in range(len(c)):
                for j in range(gy):
                    for i in range(gx):
                        self.cells[j][i].feed(*c[t, j, i])
        if flush:
            for row in self.cells:
                for m in row:
                    m.close()
        return np.array([[m.totals() for m in row] for row in self.cells], np.int32).reshape(gy, gx, 4)


def clip_totals(frames, area, params, flush=True):
    """One call over a whole clip -> int32 [gy,gx,4]."""
    return NumpyCells()(frames, area, params, True, flush)


def locate(totals, frames_scanned, region, frame_hw, row_frac=0.25, col_frac=0.05, static_frac=0.95, pad_cells=1):
    """The rule of area_locator.locate_area -> (ymin, ymax, xmin, xmax) or None."""
    y0, y1, x0, x1 = region
    t = np.asarray(totals).astype(np.int64)
    gy, gx = t.shape[:2]
    cov = [[0 if t[j, i, 2] >= static_frac * frames_scanned else int(t[j, i, 0]) for i in range(gx)] for j in range(gy)]
    rows = [sum(r) for r in cov]
    best = max(rows)
    if best == 0:
        return None
    top = bot = max(j for j in range(gy) if rows[j] == best)           # ties: the lowest row in the picture
    while top > 0 and rows[top - 1] >= row_frac * best:
        top -= 1
    while bot + 1 < gy and rows[bot + 1] >= row_frac * best:
        bot += 1
    cols = [sum(cov[j][i] for j in range(top, bot + 1)) for i in range(gx)]
    good = [i for i in range(gx) if cols[i] >= col_frac * max(cols)]
    left, right = good[0], good[-1]
    # cell rows top..bot are region rows 1 + 8 top .. 1 + 8 (bot + 1), the last cell cut off at the interior's end
    ymin, ymax = y0 + 1 + 8 * top, y0 + min(1 + 8 * (bot + 1), y1 - y0 - 1)
    xmin, xmax = x0 + 1 + 64 * left, x0 + min(1 + 64 * (right + 1), x1 - x0 - 1)
    h, w = frame_hw
    return (max(0, ymin - 8 * pad_cells), min(h, ymax + 8 * pad_cells), max(0, xmin - 64 * pad_cells), min(w, xmax + 64 * pad_cells))
