"""The deinterlacing rule of include/vse_hip.h vse_yuv_deinterlace restated independently of the product's code: int64 and plain loops
over rows, one plane at a time.  A format is the tuple of tests/yuv_format_ref.py, (sub_x, sub_y, chroma, depth, msb, matrix, full_range);
planes hold stored words (uint8, or uint16 above 8 bits): (Y,), (Y, U, V) or (Y, UV).

    out[y] = C[y]                                   for y & 1 == keep, and for every y when R == 1
    for y & 1 != keep:
      moved[x] = no previous picture, or mode == interpolate,
                 or |C[r][x] - P[r][x]| > T for any r in {y - 1, y, y + 1} inside [0, R)
      a = C[y - 1] if y >= 1 else C[y + 1];   b = C[y + 1] if y + 1 < R else C[y - 1]
      out[y][x] = moved[x] ? (a[x] + b[x] + 1) >> 1 : C[y][x]
    T = thresh << (depth - 8), and << (16 - depth) more for msb formats
"""
import numpy as np

ADAPTIVE, INTERPOLATE = 0, 1


def threshold(fmt, thresh):
    depth, msb = fmt[3], fmt[4]
    t = thresh << (depth - 8)
    return t << (16 - depth) if msb else t


def plane(cur, prev, keep, mode, t):
    """One plane -> (deinterlaced plane, moved [R, W] bool: where a row of the other field was interpolated; False on kept rows)."""
    c = np.asarray(cur).astype(np.int64)
    p = None if prev is None else np.asarray(prev).astype(np.int64)
    rows = c.shape[0]
    out = c.copy()
    took = np.zeros(c.shape, bool)
    for y in range(rows):
        if (y & 1) == keep or rows == 1:
            continue
        if p is None or mode == INTERPOLATE:
            moved = np.ones(c.shape[1], bool)
        else:
            moved = np.zeros(c.shape[1], bool)
            for r in (y - 1, y, y + 1):
                if 0 <= r < rows:
                    moved |= np.abs(c[r] - p[r]) > t
        a = c[y - 1] if y >= 1 else c[y + 1]
        b = c[y + 1] if y + 1 < rows else c[y - 1]
        out[y] = np.where(moved, (a + b + 1) // 2, c[y])
        took[y] = moved
    return out.astype(np.asarray(cur).dtype), took


def picture(planes, prev, fmt, keep=0, mode=ADAPTIVE, thresh=10):
    """Every plane of a picture -> the progressive picture's planes."""
    t = threshold(fmt, thresh)
    return tuple(plane(c, None if prev is None else prev[k], keep, mode, t)[0] for k, c in enumerate(planes))


def shares(planes, prev, fmt, keep=0, mode=ADAPTIVE, thresh=10):
    """-> (interpolated, woven) sample counts over the rows of the other field of every plane."""
    t = threshold(fmt, thresh)
    inter = total = 0
    for k, c in enumerate(planes):
        rows = np.asarray(c).shape[0]
        if rows == 1:
            continue
        took = plane(c, None if prev is None else prev[k], keep, mode, t)[1]
        other = took[1 - keep::2]
        inter += int(other.sum())
        total += other.size
    return inter, total - inter


def near_threshold_prev(rng, planes, fmt, thresh=10):
    """A previous picture P = C + d, d drawn from {0, +-(T - 1), +-T, +-(T + 1), large} at weights 30 / 25 / 25 / 10 / 10 %, kept inside the
    words' range (a sample that cannot move by d one way moves the other way)."""
    t = threshold(fmt, thresh)
    top = 255 if fmt[3] == 8 else 65535
    out = []
    for c in planes:
        c64 = np.asarray(c).astype(np.int64)
        mag = rng.choice([0, t - 1, t, t + 1, max(4 * t, top // 3)], size=c64.shape, p=[0.30, 0.25, 0.25, 0.10, 0.10])
        sign = rng.choice([-1, 1], size=c64.shape)
        p = c64 + sign * mag
        flip = (p < 0) | (p > top)
        p = np.where(flip, c64 - sign * mag, p)
        p = np.clip(p, 0, top)
        out.append(p.astype(np.asarray(c).dtype))
    return tuple(out)
