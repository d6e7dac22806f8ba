"""numpy restatement of the bounded locator's kept masks (include/vse_hip.h vse_frame_cells_hold_bounded_masks,
vse_frame_masks_replay_hold_bounded): the rows of a rectangle out of a mask buffer are frame_masks_ref's words ->
frame_hold_bounded_ref.bounded_masks -> frame_hold_ref.rows_of, and the host callables of frame_select.LocatingBoundedHoldSelector stand
beside frame_masks_hold_ref.NumpyCellsHoldMasks and frame_hold_bounded_ref.NumpyBoundedHoldCounter.  The device must agree with all of it
integer for integer."""
import numpy as np

from area_cells_hold_bounded_ref import NumpyCellsHoldBounded
from frame_hold_bounded_ref import bounded_masks, emitted
from frame_hold_ref import rows_of
from frame_masks_hold_ref import rect_masks
from frame_masks_ref import CELL_H, dims, mask_words


def run_lengths(e, max_hold):
    """bool [T,h,w] edge masks of consecutive frames -> int32 [h,w]: every pixel's run of edge frames that ends with the last frame,
    saturating at max_hold + 1 as the device's uint16 does (what vse_frame_hold_bounded's state keeps per pixel)."""
    e = np.asarray(e, bool)
    run = np.zeros(e.shape[1:], np.int32)
    for m in e:
        run = np.where(m, np.minimum(run + 1, max_hold + 1), 0)
    return run


def replay_hold_bounded(words, area_h, area_w, q, f0, f1, rect, hold, max_hold, flush=True):
    """The slots [f0, f1) as a whole clip (fed = 0) -> (int32 [rows, 3], int32 [ih, iw]): vse_frame_hold_bounded's rows of those frames
    on the rectangle, all f1 - f0 of them with flush, the first max(0, f1 - f0 - max_hold) without; and the run lengths it leaves."""
    m = rect_masks(words, area_h, area_w, q, f0, f1, rect)
    lo, hi = emitted(0, len(m), max_hold, flush)
    held = bounded_masks(m, hold, max_hold)[lo:hi] if len(m) else m
    return (rows_of(held) if len(held) else np.zeros((0, 3), np.int32)), run_lengths(m, max_hold)


class NumpyCellsHoldBoundedMasks:
    """cells_fn of frame_select.LocatingBoundedHoldSelector on the host: NumpyCellsHoldBounded's totals, and the EDGE mask words of
    every frame fed kept in a buffer of `cap` slots; `replay` walks a rectangle through them and leaves a NumpyBoundedHoldCounter where
    vse_frame_hold_bounded would stand after those frames.  `frames`: frames fed since the last reset; `replayed`: the (q, rect, hold,
    max_hold, flush) of every replay."""

    def __init__(self):
        self.cells, self.words, self.frames, self.replayed = NumpyCellsHoldBounded(), None, 0, []

    def __call__(self, frames, area, params, reset, flush, thresholds, cap, hold, max_hold):
        totals = self.cells(frames, area, params, reset, flush, thresholds=thresholds, hold=hold, max_hold=max_hold)
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

    def replay(self, area, q, rect, counter, hold, max_hold, flush):
        y0, y1, x0, x1 = area
        self.replayed.append((q, tuple(rect), hold, max_hold, flush))
        m = rect_masks(self.words, y1 - y0, x1 - x0, q, 0, self.frames, rect)
        lo, hi = emitted(0, len(m), max_hold, flush)
        held = bounded_masks(m, hold, max_hold)[lo:hi]
        # what NumpyBoundedHoldCounter keeps after a call with these frames: the edge masks a pending row's run can still reach, and
        # the last mask counted
        keep = max(1, hi + 1 - max_hold)
        counter.first, counter.masks, counter.prev = keep, m[keep - 1:], held[-1] if len(held) else None
        return rows_of(held) if len(held) else np.zeros((0, 3), np.int32)
