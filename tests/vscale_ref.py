"""The vertical scale of include/vse_hip.h vse_yuv_vscale restated in numpy, independently of the product's code: int64 arithmetic, an
explicit floor division by 2**14 instead of int32 and a shift, the table builder of tests/resample_ref.py (row by row in Python floats)
over the heights, and the band rule written out by search.  A format is the tuple of tests/yuv_format_ref.py.  A table is (top[Q],
coef[Q][K]); for a plane of ph stored rows of which the band holds rows [b0, b1):

    acc = sum over k of coef[y][k] * S[clamp(clamp(top[y] + k, 0, ph - 1), b0, b1 - 1)][x]
    out = clip(0, 2**depth - 1, floor((acc + 8192) / 2**14))

S the stored word, or with msb = 1 the word >> (16 - depth), the result then << (16 - depth).  With the whole plane (b0 = 0, b1 = ph) the
second clamp does nothing.  A semi-planar UV plane is a plane of 2 cw samples per row.
"""
import numpy as np

import yuv_format_ref as R
from resample_ref import FILTERS, identity, random_table, table, taps_needed, weight  # noqa: F401

TAPS = (2, 4, 6, 8, 10, 12, 14, 16)


def chroma_height(h, fmt):
    return (h + fmt[1]) >> fmt[1]


def chroma_rows(y0, y1, fmt):
    """The chroma rows that go with luma rows [y0, y1)."""
    return y0 >> fmt[1], ((y1 - 1) >> fmt[1]) + 1


def tables(h_in, h_out, fmt, name):
    return table(h_in, h_out, name), (table(chroma_height(h_in, fmt), chroma_height(h_out, fmt), name) if fmt[2] else None)


class Stats:
    """What the calls through plane() exercised: output values at both ends of the range, taps (of a weight other than zero) clamped at the
    picture's top and bottom, and such taps moved by the band clamp."""

    def __init__(self):
        self.low = self.high = self.above = self.below = self.band = 0


def plane(src, top, coef, fmt, r0, r1, ph, b0=0, b1=None, stats=None):
    """src: rows [b0, b1) of a stored plane of ph rows (stored words) -> rows [r0, r1) of the output plane, same dtype."""
    depth, msb = fmt[3], fmt[4]
    shift, maxv = (16 - depth if msb else 0), (1 << depth) - 1
    b1 = ph if b1 is None else b1
    src = np.asarray(src)
    assert src.shape[0] == b1 - b0 and 0 <= b0 < b1 <= ph
    s = src.astype(np.int64) >> shift
    out = np.zeros((r1 - r0, s.shape[1]), np.int64)
    for y in range(r0, r1):
        acc = np.zeros(s.shape[1], np.int64)
        for k in range(np.asarray(coef).shape[1]):
            want = int(top[y]) + k
            row = min(max(want, 0), ph - 1)
            held = min(max(row, b0), b1 - 1)
            if stats is not None:
                used = int(coef[y][k]) != 0                              # (a tap of weight zero may point anywhere)
                stats.above, stats.below = stats.above + (used and want < 0), stats.below + (used and want > ph - 1)
                stats.band += used and held != row
            acc += int(coef[y][k]) * s[held - b0]
            assert np.abs(acc).max(initial=0) < 2 ** 31 - 8192
        out[y - r0] = np.clip(np.floor_divide(acc + 8192, 2 ** 14), 0, maxv)
    if stats is not None:
        stats.low, stats.high = stats.low + int((out == 0).sum()), stats.high + int((out == maxv).sum())
    return (out << shift).astype(src.dtype)


def picture(planes, fmt, luma, chroma, h_in, y0, y1, s0=0, s1=None, stats=None):
    """planes: the planes of the packed band of stored luma rows [s0, s1) of a picture of h_in rows -> the planes of the packed band of
    output rows [y0, y1); luma, chroma: (top, coef), chroma None for grey."""
    s1 = h_in if s1 is None else s1
    cb, co = chroma_rows(s0, s1, fmt), chroma_rows(y0, y1, fmt)
    out = [plane(planes[0], *luma, fmt, y0, y1, h_in, s0, s1, stats)]
    for p in planes[1:]:
        out.append(plane(p, *chroma, fmt, co[0], co[1], chroma_height(h_in, fmt), cb[0], cb[1], stats))
    return tuple(out)


def needed(top, coef, ph, r0, r1):
    """The stored rows that output rows [r0, r1) read with a coefficient other than zero."""
    return {min(max(int(top[y]) + k, 0), ph - 1) for y in range(r0, r1) for k in range(np.asarray(coef).shape[1]) if int(coef[y][k]) != 0}


def source_rows(luma, chroma, fmt, h_in, y0, y1):
    """The band rule, by search: the smallest band of stored luma rows [s0, s1) whose luma rows, and whose chroma rows s0 >> sub_y ..
    ((s1 - 1) >> sub_y) + 1, hold everything that output rows [y0, y1) need in every plane; (0, 1) where nothing is needed."""
    sy = fmt[1]
    need_y = needed(*luma, h_in, y0, y1)
    need_c = needed(*chroma, chroma_height(h_in, fmt), *chroma_rows(y0, y1, fmt)) if chroma is not None else set()
    if not need_y and not need_c:
        return 0, 1
    s0 = max(s for s in range(h_in) if all(r >= s for r in need_y) and all(r >= s >> sy for r in need_c))
    s1 = min(s for s in range(s0 + 1, h_in + 1) if all(r < s for r in need_y) and all(r <= (s - 1) >> sy for r in need_c))
    return s0, s1


def covers(luma, chroma, fmt, h_in, y0, y1, s0, s1):
    """Whether the band [s0, s1) holds what output rows [y0, y1) need in every plane."""
    c0, c1 = chroma_rows(s0, s1, fmt)
    return all(s0 <= r < s1 for r in needed(*luma, h_in, y0, y1)) and (chroma is None or all(
        c0 <= r < c1 for r in needed(*chroma, chroma_height(h_in, fmt), *chroma_rows(y0, y1, fmt))))


class Tables:
    """What Context.yuv_vscale takes in an ingest.VScale's place: fixed tables for one call, hashable by identity."""

    def __init__(self, h_in, h_out, luma, chroma):
        self.in_height, self.out_height, self._tables = h_in, h_out, (luma, chroma)

    def tables(self, fmt):
        return tuple(None if t is None else (np.asarray(t[0], np.int32), np.asarray(t[1], np.int16)) for t in self._tables)

    def packed(self, fmt):
        return tuple(None if t is None else t[0].astype("<i4").tobytes() + t[1].astype("<i2").tobytes() for t in self.tables(fmt))


def pack(planes, fmt):
    return R.pack(planes, fmt)
