"""numpy restatement of the held locator's kept masks (include/vse_hip.h vse_frame_cells_hold_masks, vse_frame_masks_replay_hold): the
rows of a rectangle out of a mask buffer are frame_masks_ref.unpack -> frame_hold_ref.held_masks -> frame_hold_ref.rows_of, and the host
callables of frame_select.LocatingHoldSelector stand beside frame_masks_ref.NumpyCellsMasks and frame_hold_ref.NumpyHoldCounter.  The
device must agree with all of it integer for integer."""
import numpy as np

from area_cells_hold_ref import NumpyCellsHold
from frame_hold_ref import emitted, held_masks, rows_of
from frame_masks_ref import CELL_H, dims, mask_words, unpack


def rect_masks(words, area_h, area_w, q, f0, f1, rect):
    """Slots [f0, f1) of a mask buffer (uint64 [cap, nt, gy, gx, 8]) at threshold index q -> bool [f1 - f0, ih, iw], the edge masks of
    the interior of rect = (ry0, ry1, rx0, rx1) in region coordinates: its pixel (iy, ix) is region-interior pixel (ry0 + iy, rx0 + ix)."""
    ry0, ry1, rx0, rx1 = rect
    assert 0 <= ry0 and ry1 <= area_h and 0 <= rx0 and rx1 <= area_w and ry1 - ry0 >= 3 and rx1 - rx0 >= 3
    assert 0 <= f0 <= f1 <= len(words)
    if f1 == f0:
        return np.zeros((0, ry1 - ry0 - 2, rx1 - rx0 - 2), bool)
    return unpack(words[f0:f1, q:q + 1], area_h, area_w)[:, 0, ry0:ry1 - 2, rx0:rx1 - 2]


def replay_hold(words, area_h, area_w, q, f0, f1, rect, hold, flush=True):
    """The slots [f0, f1) as a whole clip (fed = 0) -> int32 [rows, 3]: vse_frame_hold's rows of those frames on the rectangle, all
    f1 - f0 of them with flush, the first f1 - f0 - hold + 1 without."""
    m = rect_masks(words, area_h, area_w, q, f0, f1, rect)
    lo, hi = emitted(0, len(m), hold, flush)
    held = held_masks(m, hold)[lo:hi]
    return rows_of(held) if len(held) else np.zeros((0, 3), np.int32)


class NumpyCellsHoldMasks:
    """cells_fn of frame_select.LocatingHoldSelector on the host: NumpyCellsHold's totals, and the EDGE mask words of every frame fed kept
    in a buffer of `cap` slots; `replay` walks a rectangle through them and leaves a NumpyHoldCounter where vse_frame_hold would stand
    after those frames.  `frames`: frames fed since the last reset; `replayed`: the (q, rect, hold, flush) of every replay."""

    def __init__(self):
        self.cells, self.words, self.frames, self.replayed = NumpyCellsHold(), None, 0, []

    def __call__(self, frames, area, params, reset, flush, thresholds, cap, hold):
        totals = self.cells(frames, area, params, reset, flush, thresholds=thresholds, hold=hold)
        y0, y1, x0, x1 = area
        shape = (cap, len(thresholds)) + dims(y1 - y0, x1 - x0) + (CELL_H,)
        if reset or self.words is None or self.words.shape != shape:
            self.words, self.frames = np.full(shape, 0xA5A5A5A5A5A5A5A5, np.uint64), 0
        if frames is not None and len(frames):
            n = len(frames)
            assert self.frames + n <= cap, "no wrap"
            self.words[self.frames:self.frames + n] = mask_words(np.asarray(frames), area, thresholds)
            self.frames += n
        return totals

    def replay(self, area, q, rect, counter, hold, flush):
        y0, y1, x0, x1 = area
        self.replayed.append((q, tuple(rect), hold, flush))
        m = rect_masks(self.words, y1 - y0, x1 - x0, q, 0, self.frames, rect)
        lo, hi = emitted(0, len(m), hold, flush)
        held = held_masks(m, hold)[lo:hi]
        # what NumpyHoldCounter keeps after a call with these frames: the edge masks a later run can reach back to, the last mask counted
        keep = max(1, hi + 1 - (hold - 1))
        counter.first, counter.masks, counter.prev = keep, m[keep - 1:], held[-1] if len(held) else None
        return rows_of(held) if len(held) else np.zeros((0, 3), np.int32)
