"""numpy / plain-Python restatement of the locator's cells on bounded runs (include/vse_hip.h vse_frame_cells_hold_bounded), written from
the specification as the composition of two references: tests/area_cells_ref.py's cell automaton fed with the per-cell counts of
tests/frame_hold_bounded_ref.py's bounded masks.  The device kernel must agree with it integer for integer, and the CPU tests drive the
host side with it."""
import numpy as np

from area_cells_hold_ref import _rows
from area_cells_ref import Automaton, Params, dims
from frame_change_ref import edge_mask
from frame_hold_bounded_ref import bounded_masks, emitted


def bounded_cell_counts(frames, area, thresh, hold, max_hold):
    """A whole clip, uint8 BGR [T,H,W,3], area (y0, y1, x0, x1) -> int32 [T,gy,gx,3]: e, a, v of the bounded masks per frame and cell
    (runs cut off at both ends of the clip: what a call with fed = 0 and flush counts)."""
    y0, y1, x0, x1 = area
    if not len(frames):
        return np.zeros((0,) + dims(y1 - y0, x1 - x0) + (3,), np.int32)
    return _rows(bounded_masks(edge_mask(np.asarray(frames), area, thresh), hold, max_hold))


def totals_of(counts, params, flush=True):
    """int [T,gy,gx,3] rows in frame order -> int32 [gy,gx,4]: every cell's automaton over them, the last run closed with flush."""
    p = Params(*params)
    gy, gx = counts.shape[1:3]
    out = np.zeros((gy, gx, 4), np.int32)
    for j in range(gy):
        for i in range(gx):
            m = Automaton(p)
            for e, a, v in counts[:, j, i]:
                m.feed(e, a, v)
            if flush:
                m.close()
            out[j, i] = m.totals()
    return out


def clip_totals_hold_bounded(frames, area, params, hold, max_hold, flush=True):
    """One call over a whole clip at params.edge_thresh -> int32 [gy,gx,4].  Without flush: the frames whose row is final (1 .. T -
    max_hold; a run that reaches from one of them to the last frame fed is too long whatever follows), the last run left open."""
    c = bounded_cell_counts(frames, area, Params(*params).edge_thresh, hold, max_hold)
    if not flush:
        # the runs that reach the last frame fed are still open: only those longer than max_hold are decided, and they are out.  A
        # clip cut off there counts the shorter ones, but none of them covers a frame up to T - max_hold.
        c = c[:max(0, len(c) - max_hold)]
    return totals_of(c, params, flush)


class _Stream:
    """One threshold of NumpyCellsHoldBounded: the edge masks a pending row's run can still reach (NumpyBoundedHoldCounter's window),
    the last bounded mask counted, and every cell's automaton."""

    def __init__(self, p, gy, gx):
        self.first, self.masks, self.prev = 1, None, None
        self.cells = [[Automaton(p) for _ in range(gx)] for _ in range(gy)]
        self.rows = []                  # per call: the rows it completed, int32 [rows,gy,gx,3]

    def feed(self, new, fed, hold, max_hold, flush):
        self.masks = new if self.masks is None else np.concatenate([self.masks, new])
        assert self.first + len(self.masks) == fed + len(new) + 1, "frames of a clip arrive in order"
        lo, hi = emitted(fed, len(new), max_hold, flush)
        c = np.zeros((0, len(self.cells), len(self.cells[0]), 3), np.int32)
        if hi > lo:
            held = bounded_masks(self.masks, hold, max_hold)[lo + 1 - self.first:hi + 1 - self.first]
            c = _rows(held, self.prev)
            self.prev = held[-1]
            for t in range(len(c)):
                for j, row in enumerate(self.cells):
                    for i, m in enumerate(row):
                        m.feed(*c[t, j, i])
        self.rows.append(c)
        keep = max(self.first, hi + 1 - max_hold)
        self.masks, self.first = self.masks[keep - self.first:], keep
        if flush:
            for row in self.cells:
                for m in row:
                    m.close()

    def totals(self):
        return [[m.totals() for m in row] for row in self.cells]


class NumpyCellsHoldBounded:
    """cells_fn of area_locator.AreaLocator(automaton="hold", max_hold_*=...) on the host, streaming, with the device's lag: a call
    counts the frames whose row max_hold further frames (or the flush) have made final.  thresholds None: one threshold,
    params.edge_thresh, and totals [gy,gx,4]; else [nt,gy,gx,4].  `rows[k]`: per call the rows threshold k completed."""

    def __init__(self):
        self.streams = None
        self.fed = self.calls = 0
        self.holds = []                 # (hold, max_hold) of every call

    def __call__(self, frames, area, params, reset, flush, thresholds=None, hold=1, max_hold=None):
        assert max_hold is not None, "NumpyCellsHoldBounded is the cells_fn of a locator with max_hold_*"
        self.calls += 1
        self.holds.append((hold, max_hold))
        p = Params(*params)
        y0, y1, x0, x1 = area
        gy, gx = dims(y1 - y0, x1 - x0)
        ths = (p.edge_thresh,) if thresholds is None else tuple(thresholds)
        if reset or self.streams is None:
            self.streams, self.fed = [_Stream(p, gy, gx) for _ in ths], 0
        n = 0 if frames is None else len(frames)
        for th, s in zip(ths, self.streams):
            new = edge_mask(np.asarray(frames), area, th) if n else np.zeros((0, y1 - y0 - 2, x1 - x0 - 2), bool)
            s.feed(new, self.fed, hold, max_hold, flush)
        self.fed += n
        out = np.array([s.totals() for s in self.streams], np.int32).reshape(len(ths), gy, gx, 4)
        return out[0] if thresholds is None else out

    @property
    def rows(self):
        return [s.rows for s in self.streams]
