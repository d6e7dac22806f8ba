"""The conversion of include/vse_hip.h vse_yuv_to_bgr_tonemap restated in numpy, independently of the product's code: int64 arithmetic and
explicit floor divisions instead of int32 and shifts.  Formats, stored words, factors, planes and chroma sampling are those of
tests/yuv_format_ref.py (R below).  With its c = max(Y - yoff, 0) * KY_s (full range: yoff = 0), u, v and K_s:

    E_B = clip(0, 4095, floor((c + BU_s u + 2**15) / 2**16)),  E_G likewise with GU_s u + GV_s v,  E_R with RV_s v
    L_k = A[E_k]                                                              A: 4096 entries of 0..65535
    P_r = clip(0, 65535, floor((M[r][0] L_R + M[r][1] L_G + M[r][2] L_B + 2**13) / 2**14))      rows and columns of M: R, G, B
    out_r = T[P_r if P_r < 4096 else 3840 + floor(P_r / 16)]                  T: 7936 entries of 0..255

and the bytes are B, G, R.  The tables are arguments: nothing here knows what they mean.
"""
import numpy as np

import yuv_format_ref as R

A_LEN, T_LEN = 4096, 7936
TABLE_BYTES = 2 * A_LEN + T_LEN


def codes(y, u, v, fmt):
    """Arrays of stored Y, U, V words of one shape -> the 12-bit codes (E_B, E_G, E_R), int64."""
    sums = R.sums(R.values(y, fmt), R.values(u, fmt), R.values(v, fmt), fmt)                  # each carries + 2**19
    return tuple(np.clip(np.floor_divide(s - 2 ** 19 + 2 ** 15, 2 ** 16), 0, A_LEN - 1) for s in sums)


def t_index(p):
    p = np.asarray(p, np.int64)
    return np.where(p < 4096, p, 3840 + np.floor_divide(p, 16))


def light_to_bytes(lr, lg, lb, table_t, gamut):
    """Linear light of one shape (int64) -> uint8 [..., 3] BGR and the three indices into T (B, G, R)."""
    m = np.asarray(gamut, np.int64).reshape(3, 3)
    idx = []
    for r in (2, 1, 0):                                                               # B, G, R
        p = np.clip(np.floor_divide(m[r, 0] * lr + m[r, 1] * lg + m[r, 2] * lb + 2 ** 13, 2 ** 14), 0, 65535)
        idx.append(t_index(p))
    return np.stack([np.asarray(table_t)[i] for i in idx], axis=-1).astype(np.uint8), idx


def pixels(y, u, v, fmt, table_a, table_t, gamut, trace=None):
    """Arrays of stored Y, U, V words of one shape -> uint8 [..., 3] BGR.  trace: a dict that receives the codes ("E") and the indices
    into T ("T") that were read, for tests that must know what a picture exercises."""
    eb, eg, er = codes(y, u, v, fmt)
    a = np.asarray(table_a).astype(np.int64)
    out, idx = light_to_bytes(a[er], a[eg], a[eb], table_t, gamut)
    if trace is not None:
        trace["E"] = np.unique(np.concatenate([e.reshape(-1) for e in (eb, eg, er)]))
        trace["T"] = np.unique(np.concatenate([i.reshape(-1) for i in idx]))
    return out


def convert(planes, fmt, table_a, table_t, gamut, rows=None, parity=0, trace=None):
    """uint8 BGR [r1 - r0, w, 3] of luma rows [r0, r1) (default: all) of the planes, as yuv_format_ref.convert."""
    y, u, v = R.split_chroma(planes, fmt)
    h, w = y.shape
    r0, r1 = (0, h) if rows is None else rows
    if r1 <= r0:
        return np.zeros((0, w, 3), np.uint8)
    if u is None:
        z = np.zeros((r1 - r0, w), np.int64)
        return pixels(y[r0:r1], z, z, fmt, table_a, table_t, gamut, trace)
    cr, cc = (np.arange(r0, r1) + parity) >> fmt[1], np.arange(w) >> fmt[0]
    return pixels(y[r0:r1], u[cr][:, cc], v[cr][:, cc], fmt, table_a, table_t, gamut, trace)


def gamut_ok(gamut):
    m = np.asarray(gamut, np.int64).reshape(3, 3)
    return all(row[row > 0].sum() <= 32767 and row[row < 0].sum() >= -32768 for row in m)


def random_tables(rng):
    """Tables without any structure (not monotone: an indexing slip cannot hide) and a gamut whose rows reach both bounds' neighbourhood."""
    table_a = rng.integers(0, 65536, size=A_LEN).astype(np.uint16)
    table_t = rng.integers(0, 256, size=T_LEN).astype(np.uint8)
    gamut = np.zeros((3, 3), np.int32)
    for r in range(3):
        sign = rng.permutation([1, 1, -1] if rng.integers(0, 2) else [1, -1, -1])
        pos, neg = int(rng.integers(20000, 32768)), int(rng.integers(20000, 32769))
        for s, total in ((1, pos), (-1, neg)):
            where = np.nonzero(sign == s)[0]
            cut = int(rng.integers(0, total + 1)) if len(where) == 2 else total
            parts = [cut, total - cut] if len(where) == 2 else [total]
            for k, part in zip(where, parts):
                gamut[r, k] = s * part
    assert gamut_ok(gamut)
    return table_a, table_t, gamut


def pack_table(table_a, table_t):
    """-> the 16 128 bytes the device takes: A little-endian, then T."""
    a, t = np.asarray(table_a), np.asarray(table_t)
    assert a.shape == (A_LEN,) and t.shape == (T_LEN,)
    return np.concatenate([a.astype("<u2").view(np.uint8), t.astype(np.uint8)])
