"""The horizontal resample of include/vse_hip.h vse_yuv_resample restated in numpy, independently of the product's code: int64 arithmetic,
an explicit floor division by 2**14 instead of int32 and a shift, and a table builder of its own, column by column in Python floats.
A format is the tuple of tests/yuv_format_ref.py.  A table is (left[P], coef[P][K]); for a plane of pw stored columns:

    acc = sum over k of coef[x][k] * S[clamp(left[x] + k, 0, pw - 1)]
    out = clip(0, 2**depth - 1, floor((acc + 8192) / 2**14))

S the stored word, or with msb = 1 the word >> (16 - depth), the result then << (16 - depth).  A semi-planar UV plane is a plane of cw
columns of two components that share the chroma table.
"""
import math

import numpy as np

import yuv_format_ref as R

FILTERS = ("bicubic", "bilinear", "lanczos")
SUPPORT = {"bicubic": 2.0, "bilinear": 1.0, "lanczos": 3.0}
# (stored columns, sample aspect ratio, columns shown): the eight ratios of DVD, HDV and DVCPRO HD material
DISPLAY = [(720, (32, 27), 854), (720, (16, 11), 1048), (720, (8, 9), 640), (720, (16, 15), 768), (1440, (4, 3), 1920), (1280, (3, 2), 1920),
           (960, (4, 3), 1280), (704, (10, 11), 640)]


def display_width(w, num, den):
    """The nearest even number to w * num / den."""
    return 2 * ((w * num + den) // (2 * den))


def weight(name, t):
    a = abs(t)
    if name == "bilinear":
        return max(1.0 - a, 0.0)
    if name == "bicubic":                 # Keys' cubic with a = -1/2 (Catmull-Rom; Mitchell-Netravali B = 0, C = 1/2)
        if a < 1.0:
            return 1.5 * a ** 3 - 2.5 * a ** 2 + 1.0
        return -0.5 * a ** 3 + 2.5 * a ** 2 - 4.0 * a + 2.0 if a < 2.0 else 0.0
    if a >= 3.0:
        return 0.0
    return 1.0 if a == 0.0 else math.sin(math.pi * a) / (math.pi * a) * math.sin(math.pi * a / 3.0) / (math.pi * a / 3.0)


def taps_needed(pw_in, pw_out, name):
    k = math.ceil(2.0 * SUPPORT[name] * max(1.0, pw_in / pw_out))
    return k + k % 2


def table(pw_in, pw_out, name):
    """-> (left int64[pw_out], coef int64[pw_out, K]); every row sums to 16384."""
    stretch = max(1.0, pw_in / pw_out)
    k = taps_needed(pw_in, pw_out, name)
    left, coef = np.zeros(pw_out, np.int64), np.zeros((pw_out, k), np.int64)
    for x in range(pw_out):
        c = (x + 0.5) * pw_in / pw_out - 0.5
        left[x] = math.floor(c - SUPPORT[name] * stretch) + 1
        w = [weight(name, (left[x] + j - c) / stretch) for j in range(k)]
        total = sum(w)
        q = [int(np.rint(v / total * 16384.0)) for v in w]
        q[max(range(k), key=lambda j: w[j])] += 16384 - sum(q)          # (the first of equal largest taps)
        coef[x] = q
    return left, coef


def identity(p):
    coef = np.zeros((p, 2), np.int64)
    coef[:, 0] = 16384
    return np.arange(p, dtype=np.int64), coef


def dense(left, coef, pw):
    """The table as a matrix [P, pw]: the clamped taps added up."""
    m = np.zeros((len(left), pw), np.int64)
    for x in range(len(left)):
        for j in range(coef.shape[1]):
            m[x, min(max(int(left[x]) + j, 0), pw - 1)] += int(coef[x, j])
    return m


def rows(plane, left, coef, fmt, comps=1):
    """Rows [r, pw * comps] of stored words -> [r, P * comps] of the same dtype."""
    depth, msb = fmt[3], fmt[4]
    shift = 16 - depth if msb else 0
    plane = np.asarray(plane)
    s = plane.astype(np.int64) >> shift
    pw = s.shape[1] // comps
    left, coef = np.asarray(left, np.int64), np.asarray(coef, np.int64)
    out = np.zeros((s.shape[0], len(left) * comps), np.int64)
    for e in range(comps):
        comp = s[:, e::comps]
        acc = np.zeros((s.shape[0], len(left)), np.int64)
        for j in range(coef.shape[1]):
            acc += comp[:, np.clip(left + j, 0, pw - 1)] * coef[:, j][None, :]
        assert np.abs(acc).max(initial=0) < 2 ** 31 - 8192
        out[:, e::comps] = np.clip(np.floor_divide(acc + 8192, 2 ** 14), 0, (1 << depth) - 1) << shift
    return out.astype(plane.dtype)


def picture(planes, fmt, luma, chroma):
    """The planes of a picture (or of a band of its rows) -> the resampled planes; luma, chroma: (left, coef), chroma None for grey."""
    return tuple(rows(p, *(chroma if k else luma), fmt, comps=2 if k and fmt[2] == 2 else 1) for k, p in enumerate(planes))


def chroma_width(w, fmt):
    return (w + fmt[0]) >> fmt[0]


def tables(w_in, w_out, fmt, name):
    return table(w_in, w_out, name), (table(chroma_width(w_in, fmt), chroma_width(w_out, fmt), name) if fmt[2] else None)


def random_table(rng, pw, p, k, wild=True):
    """A table no filter would produce: left from below 0 to past the right edge, int16 coefficients of any sign whose absolute values
    sum to at most 32767 per row, some rows summing high and some low so that both ends clip."""
    left = rng.integers(-k - 2, pw + 2, size=p).astype(np.int64)
    mag = rng.integers(0, 32768, size=(p, k)).astype(np.int64)
    scale = rng.integers(1, 32768, size=p).astype(np.float64) / np.maximum(mag.sum(axis=1), 1)
    mag = np.floor(mag * np.minimum(scale, 1.0)[:, None]).astype(np.int64)
    sign = np.where(rng.random((p, k)) < (0.35 if wild else 0.0), -1, 1)
    kind = rng.integers(0, 3, size=p)                      # 1: all positive (clips high), 2: all negative (clips at 0)
    sign = np.where(kind[:, None] == 1, 1, np.where(kind[:, None] == 2, -1, sign))
    coef = mag * sign
    assert np.abs(coef).sum(axis=1).max() <= 32767
    return left, coef


class Tables:
    """What Context.yuv_resample takes in an ingest.Resample's place: fixed tables for one call, hashable by identity."""

    def __init__(self, w_in, w_out, luma, chroma):
        self.in_width, self.out_width, self._tables = w_in, w_out, (luma, chroma)

    def tables(self, fmt):
        return tuple(None if t is None else (np.asarray(t[0], np.int32), np.asarray(t[1], np.int16)) for t in self._tables)

    def packed(self, fmt):
        return tuple(None if t is None else t[0].astype("<i4").tobytes() + t[1].astype("<i2").tobytes() for t in self.tables(fmt))


def pack(planes, fmt):
    return R.pack(planes, fmt)
