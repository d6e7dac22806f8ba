"""numpy restatement of the locator's kept masks (include/vse_hip.h vse_frame_cells_masks, vse_frame_masks_replay): the mask buffer built
from frame_change_ref's mask and laid out as the header says, the replay of a rectangle out of such a buffer, and the host callables
of frame_select.LocatingChangeSelector beside edge_calibrate_ref.NumpyCellsMulti and frame_change_ref.NumpyCounter.  The device must
agree with all of it bit for bit."""
import numpy as np

import frame_change_ref as FC
from edge_calibrate_ref import NumpyCellsMulti

CELL_H, CELL_W = 8, 64


def dims(area_h, area_w):
    return (area_h - 2 + CELL_H - 1) // CELL_H, (area_w - 2 + CELL_W - 1) // CELL_W


def pack_rows(mask):
    """bool [..., rows, cols] -> uint64 [..., rows, ceil(cols / 64)]: bit b of word w is column 64 w + b; zero beyond the columns."""
    mask = np.asarray(mask, bool)
    wpr = (mask.shape[-1] + 63) // 64
    padded = np.zeros(mask.shape[:-1] + (wpr * 64,), bool)
    padded[..., :mask.shape[-1]] = mask
    bits = padded.reshape(mask.shape[:-1] + (wpr, 64)).astype(np.uint64)
    return (bits << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)


def mask_words(frames, area, thresholds):
    """uint8 BGR [n,H,W,3], region (y0, y1, x0, x1), thresholds -> uint64 [n, nt, gy, gx, 8], the slots vse_frame_cells_masks writes for
    these frames: word [f, q, cy, cx, k], bit b = region-interior pixel (8 cy + k, 64 cx + b) is an edge pixel of frame f at
    thresholds[q]; zero beyond the interior, in rows and in columns."""
    y0, y1, x0, x1 = area
    gy, gx = dims(y1 - y0, x1 - x0)
    n = len(frames)
    out = np.zeros((n, len(thresholds), gy * CELL_H, gx), np.uint64)
    for q, th in enumerate(thresholds):
        if n:
            out[:, q, :y1 - y0 - 2] = pack_rows(FC.edge_mask(frames, area, th))
    return np.ascontiguousarray(out.reshape(n, len(thresholds), gy, CELL_H, gx).transpose(0, 1, 2, 4, 3))


def unpack(words, area_h, area_w):
    """uint64 [n, nt, gy, gx, 8] -> bool [n, nt, area_h - 2, area_w - 2], the region-interior masks, pixel by pixel."""
    n, nt, gy, gx, _ = words.shape
    rows = words.transpose(0, 1, 2, 4, 3).reshape(n, nt, gy * CELL_H, gx)
    bits = (rows[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return bits.reshape(n, nt, gy * CELL_H, gx * 64)[:, :, :area_h - 2, :area_w - 2].astype(bool)


def replay(words, area_h, area_w, q, f0, f1, rect, reset=True):
    """The slots [f0, f1) of a mask buffer (uint64 [cap, nt, gy, gx, 8]) at threshold index q on rect = (ry0, ry1, rx0, rx1) in region
    coordinates -> (int32 [f1 - f0, 3] edges / appeared / vanished, the last slot's mask of the rectangle's interior as bool, the same as
    the words vse_frame_change keeps, uint64 [ih * wpr]).  Rectangle-interior pixel (iy, ix) is region-interior pixel (ry0 + iy, rx0 +
    ix); the mask before slot f0 is empty with reset, slot f0 - 1's without."""
    ry0, ry1, rx0, rx1 = rect
    assert 0 <= ry0 and ry1 <= area_h and 0 <= rx0 and rx1 <= area_w and ry1 - ry0 >= 3 and rx1 - rx0 >= 3
    assert 0 <= f0 < f1 <= len(words) and (reset or f0 >= 1)
    first = f0 if reset else f0 - 1
    m = unpack(words[first:f1, q:q + 1], area_h, area_w)[:, 0, ry0:ry1 - 2, rx0:rx1 - 2]
    e = m if reset else m[1:]
    p = np.concatenate([np.zeros_like(m[:1]), m[:-1]]) if reset else m[:-1]
    counts = np.stack([e.sum((1, 2)), (e & ~p).sum((1, 2)), (p & ~e).sum((1, 2))], 1).astype(np.int32)
    return counts, e[-1], pack_rows(e[-1]).reshape(-1)


class NumpyCellsMasks:
    """cells_fn of frame_select.LocatingChangeSelector on the host: NumpyCellsMulti's totals, and the mask words of every frame fed kept in
    a buffer of `cap` slots; `replay` counts a rectangle out of them and hands the last mask to a NumpyCounter.  `frames`: frames fed
    since the last reset; `replayed`: the (q, rect) of every replay."""

    def __init__(self):
        self.multi, self.words, self.frames, self.replayed = NumpyCellsMulti(), None, 0, []

    def __call__(self, frames, area, params, reset, flush, thresholds, cap):
        totals = self.multi(frames, area, params, reset, flush, thresholds=thresholds)
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

    def replay(self, area, q, rect, counter):
        y0, y1, x0, x1 = area
        self.replayed.append((q, tuple(rect)))
        counts, counter.prev, _words = replay(self.words, y1 - y0, x1 - x0, q, 0, self.frames, rect, True)
        return counts
