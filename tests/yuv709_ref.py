"""The BT.709 conversion of include/vse_hip.h (vse_yuv_to_bgr_matrix, matrix 1) restated in numpy, independently of the product's code:
int64 arithmetic and an explicit floor division by 2**20 instead of int32 and a shift.  Limited range, nearest chroma; everything but
the four chroma factors is tests/yuv_ref.py's BT.601 (whose plane helpers are used here).

    c = max(Y - 16, 0) * 1220542, u = U - 128, v = V - 128
    B = clip8(floor((c + 2215014 u               + 2**19) / 2**20))
    G = clip8(floor((c -  223607 u -  558796 v   + 2**19) / 2**20))
    R = clip8(floor((c               + 1879825 v + 2**19) / 2**20))

The factors are round(k * 2**20) of 2 (1 - Kb) 255/224, 2 Kb (1 - Kb) / Kg 255/224, 2 Kr (1 - Kr) / Kg 255/224 and 2 (1 - Kr) 255/224
with Kr = 0.2126, Kb = 0.0722, Kg = 1 - Kr - Kb (factors() recomputes them).
"""
import numpy as np

import yuv_ref

BU, GU, GV, RV = 2215014, -223607, -558796, 1879825

# (Y, U, V) -> [B, G, R]: black, white, and the four corners of (U, V) at Y = 16 and Y = 235, worked out by hand from the integers above
# (the luma factor 1220542 is 1.164 * 2**20, not 255/219: the R of (235, x, 0) is 25 where the real-number matrix rounds to 26)
ANCHORS = [((16, 128, 128), [0, 0, 0]), ((235, 128, 128), [255, 255, 255]),
           ((16, 0, 0), [0, 96, 0]), ((16, 0, 255), [0, 0, 228]), ((16, 255, 0), [255, 41, 0]), ((16, 255, 255), [255, 0, 228]),
           ((235, 0, 0), [0, 255, 25]), ((235, 0, 255), [0, 215, 255]), ((235, 255, 0), [255, 255, 25]), ((235, 255, 255), [255, 160, 255])]


def factors():
    kr, kb = 0.2126, 0.0722
    kg = 1.0 - kr - kb
    s = 255.0 / 224.0 * 2 ** 20
    return (round(2 * (1 - kb) * s), -round(2 * kb * (1 - kb) / kg * s), -round(2 * kr * (1 - kr) / kg * s), round(2 * (1 - kr) * s))


def pixels(y, u, v):
    """Arrays of Y, U, V samples of one shape -> uint8 [..., 3] BGR."""
    y, u, v = (np.asarray(a).astype(np.int64) for a in (y, u, v))
    c = np.maximum(y - 16, 0) * 1220542
    u, v = u - 128, v - 128
    half, one = 2 ** 19, 2 ** 20
    chans = [np.floor_divide(c + BU * u + half, one), np.floor_divide(c + GU * u + GV * v + half, one), np.floor_divide(c + RV * v + half, one)]
    return np.stack([np.minimum(np.maximum(ch, 0), 255) for ch in chans], axis=-1).astype(np.uint8)


def convert(planes, layout, rows=None, parity=0):
    """uint8 BGR [r1 - r0, w, 3] of luma rows [r0, r1) (default: all) of the planes (yuv_ref.convert with this file's pixels)."""
    y, u, v = yuv_ref.split_chroma(planes, layout)
    h, w = y.shape
    r0, r1 = (0, h) if rows is None else rows
    if r1 <= r0:
        return np.zeros((0, w, 3), np.uint8)
    cr, cc = (np.arange(r0, r1) + parity) // 2, np.arange(w) // 2
    return pixels(y[r0:r1], u[cr][:, cc], v[cr][:, cc])
