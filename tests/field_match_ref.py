"""The field-matching rule of include/vse_hip.h vse_yuv_field_match restated independently of the product's code: int64 and plain loops
over rows.  A format is the tuple of tests/yuv_format_ref.py, (sub_x, sub_y, chroma, depth, msb, matrix, full_range); planes hold stored
words (uint8, or uint16 above 8 bits): (Y,), (Y, U, V) or (Y, UV).  C the picture, P the previous one, R luma rows, w columns:

    candidates  c: every row from C;  p1: rows of parity keep from C, the others from P;  p2: rows of parity keep from P, the others from C
                (every plane, row by row of that plane)
    count(W)    over luma, rows 1 <= y <= R - 2, every column: d1 = W[y] - W[y - 1], d2 = W[y] - W[y + 1];
                combed iff (d1 > T and d2 > T) or (d1 < -T and d2 < -T);  R < 3: 0
    T           comb_thresh << (depth - 8), and << (16 - depth) more for msb formats
    choice      the smallest count, ties to c, then p1, then p2; without P only c
    fallback    comb_limit >= 0 (not None) and best * 1000 > comb_limit * w * (R - 2): choice 3, the picture of tests/deinterlace_ref.py in
                mode adaptive with the same keep and `thresh`
"""
import numpy as np

import deinterlace_ref as D

C, P1, P2, ADAPTIVE = 0, 1, 2, 3


def candidate(planes, prev, keep, choice):
    """The planes of candidate `choice` (0..2), row by row."""
    out = []
    for k, c in enumerate(planes):
        c = np.asarray(c)
        w = c.copy()
        for y in range(c.shape[0]):
            first = (y & 1) == keep
            from_prev = (choice == P1 and not first) or (choice == P2 and first)
            if from_prev:
                w[y] = np.asarray(prev[k])[y]
        out.append(w)
    return tuple(out)


def comb_count(luma, t):
    w = np.asarray(luma).astype(np.int64)
    rows = w.shape[0]
    count = 0
    for y in range(1, rows - 1):
        d1, d2 = w[y] - w[y - 1], w[y] - w[y + 1]
        count += int((((d1 > t) & (d2 > t)) | ((d1 < -t) & (d2 < -t))).sum())
    return count


def stats(planes, prev, fmt, keep=0, comb_thresh=10, comb_limit=20):
    """-> (count c, count p1, count p2, choice 0..3)"""
    t = D.threshold(fmt, comb_thresh)
    rows, width = np.asarray(planes[0]).shape
    counts = [comb_count(planes[0], t), 0, 0]
    if prev is not None:
        for k in (P1, P2):
            counts[k] = comb_count(candidate(planes[:1], prev[:1], keep, k)[0], t)
    best, choice = counts[0], C
    if prev is not None:
        for k in (P1, P2):
            if counts[k] < best:
                best, choice = counts[k], k
    if comb_limit is not None and comb_limit >= 0 and best * 1000 > comb_limit * width * (rows - 2):
        choice = ADAPTIVE
    return counts[0], counts[1], counts[2], choice


def picture(planes, prev, fmt, keep=0, comb_thresh=10, comb_limit=20, thresh=10):
    """-> (the matched picture's planes, stats)"""
    st = stats(planes, prev, fmt, keep, comb_thresh, comb_limit)
    if st[3] == ADAPTIVE:
        return D.picture(planes, prev, fmt, keep, D.ADAPTIVE, thresh), st
    return candidate(planes, prev, keep, st[3]), st


# ---- pictures for the tests -----------------------------------------------------------------------------------------------------------
def smooth_planes(rng, like, fmt, k, comb_thresh=10):
    """Picture number k (0..4) of a film of vertically smooth pictures with the shapes and dtypes of the plane tuple `like`: level
    (30 + 40 k) 8-bit levels plus noise of 0..T/2 words, T the comb threshold in words: neighbouring rows lie within T/2 of each other
    and two pictures differ by more than 2 T everywhere (40 levels - T/2 > 2 T at comb_thresh 10), so a weave of fields of two pictures
    combs in every sample and a weave of one picture's fields in none."""
    assert 0 <= k <= 4 and comb_thresh <= 10
    t = D.threshold(fmt, comb_thresh)
    level = (30 + 40 * k) * D.threshold(fmt, 1)
    return tuple((level + rng.integers(0, t // 2 + 1, size=np.asarray(p).shape)).astype(np.asarray(p).dtype) for p in like)
