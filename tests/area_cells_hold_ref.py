"""numpy / plain-Python restatement of the locator's cells on held edges (include/vse_hip.h vse_frame_cells_hold), written from the
specification as the composition of two references: tests/area_cells_ref.py's cell automaton fed with the per-cell counts of
tests/frame_hold_ref.py's held masks.  The device kernel must agree with it integer for integer, and the CPU tests drive the host
side with it."""
import numpy as np

from area_cells_ref import Automaton, Params, cell_sums, dims
from frame_change_ref import edge_mask
from frame_hold_ref import emitted, held_masks


def _rows(held, prev=None):
    """held masks bool [T,ih,iw] of consecutive frames -> int32 [T,gy,gx,3]: |H_u|, |H_u minus H_{u-1}|, |H_{u-1} minus H_u| per cell;
    prev: the mask before the first (None = empty)."""
    p = np.concatenate([np.zeros_like(held[:1]) if prev is None else prev[None], held[:-1]])
    return np.stack([cell_sums(held), cell_sums(held & ~p), cell_sums(p & ~held)], -1).astype(np.int32)


def held_cell_counts(frames, area, thresh, hold):
    """A whole clip, uint8 BGR [T,H,W,3], area (y0, y1, x0, x1) -> int32 [T,gy,gx,3]: e, a, v of the held masks per frame and cell (runs
    cut off at both ends of the clip: what a call with fed = 0 and flush counts)."""
    y0, y1, x0, x1 = area
    if not len(frames):
        return np.zeros((0,) + dims(y1 - y0, x1 - x0) + (3,), np.int32)
    return _rows(held_masks(edge_mask(np.asarray(frames), area, thresh), hold))


def clip_totals_hold(frames, area, params, hold, flush=True):
    """One call over a whole clip at params.edge_thresh -> int32 [gy,gx,4].  Without flush: the frames whose held mask is complete
    (1 .. T - hold + 1; a run that reaches the last frame fed is long enough for them whatever follows), the last run left open."""
    p = Params(*params)
    gy, gx = dims(area[1] - area[0], area[3] - area[2])
    c = held_cell_counts(frames, area, p.edge_thresh, hold)
    if not flush:
        c = c[:max(0, len(c) - hold + 1)]
    out = np.zeros((gy, gx, 4), np.int32)
    for j in range(gy):
        for i in range(gx):
            m = Automaton(p)
            for e, a, v in c[:, j, i]:
                m.feed(e, a, v)
            if flush:
                m.close()
            out[j, i] = m.totals()
    return out


class _Stream:
    """One threshold of NumpyCellsHold: the edge masks a later frame's run can still reach back to (frame_hold_ref.NumpyHoldCounter's
    idea), the last held mask counted, and every cell's automaton."""

    def __init__(self, p, gy, gx):
        self.first, self.masks, self.prev = 1, None, None
        self.cells = [[Automaton(p) for _ in range(gx)] for _ in range(gy)]

    def feed(self, new, fed, hold, flush):
        self.masks = new if self.masks is None else np.concatenate([self.masks, new])
        assert self.first + len(self.masks) == fed + len(new) + 1, "frames of a clip arrive in order"
        lo, hi = emitted(fed, len(new), hold, flush)
        held = held_masks(self.masks, hold)[lo + 1 - self.first:hi + 1 - self.first]
        if len(held):
            c = _rows(held, self.prev)
            self.prev = held[-1]
            for t in range(len(c)):
                for j, row in enumerate(self.cells):
                    for i, m in enumerate(row):
                        m.feed(*c[t, j, i])
        keep = max(self.first, hi + 1 - (hold - 1))
        self.masks, self.first = self.masks[keep - self.first:], keep
        if flush:
            for row in self.cells:
                for m in row:
                    m.close()

    def totals(self):
        return [[m.totals() for m in row] for row in self.cells]


class NumpyCellsHold:
    """cells_fn of area_locator.AreaLocator(automaton="hold") on the host, streaming, with the device's lag: a call counts the frames
    whose held mask it completes.  thresholds None: one threshold, params.edge_thresh, and totals [gy,gx,4]; else [nt,gy,gx,4]."""

    def __init__(self):
        self.streams = None
        self.fed = self.calls = 0
        self.holds = []                 # the hold of every call

    def __call__(self, frames, area, params, reset, flush, thresholds=None, hold=1):
        self.calls += 1
        self.holds.append(hold)
        p = Params(*params)
        y0, y1, x0, x1 = area
        gy, gx = dims(y1 - y0, x1 - x0)
        ths = (p.edge_thresh,) if thresholds is None else tuple(thresholds)
        if reset or self.streams is None:
            self.streams, self.fed = [_Stream(p, gy, gx) for _ in ths], 0
        n = 0 if frames is None else len(frames)
        for th, s in zip(ths, self.streams):
            new = edge_mask(np.asarray(frames), area, th) if n else np.zeros((0, y1 - y0 - 2, x1 - x0 - 2), bool)
            s.feed(new, self.fed, hold, flush)
        self.fed += n
        out = np.array([s.totals() for s in self.streams], np.int32).reshape(len(ths), gy, gx, 4)
        return out[0] if thresholds is None else out
