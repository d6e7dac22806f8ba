"""The YUV 4:2:0 -> BGR conversion of include/vse_hip.h (vse_yuv420_to_bgr) restated in numpy, independently of the product's code:
int64 arithmetic and an explicit floor division by 2**20 instead of int32 and a shift.  BT.601 limited range, nearest chroma.

    c = max(Y - 16, 0) * 1220542, u = U - 128, v = V - 128
    B = clip8(floor((c + 2116026 u               + 2**19) / 2**20))
    G = clip8(floor((c -  409993 u -  852492 v   + 2**19) / 2**20))
    R = clip8(floor((c               + 1673527 v + 2**19) / 2**20))

Planes: layout "i420" = (Y [h,w], U [ch,cw], V [ch,cw]), "nv12" = (Y [h,w], UV [ch,2 cw]) with U at the even bytes.  Output row r of
the row range [r0, r1) takes its chroma from row (r + parity) >> 1 of the chroma planes given, column x >> 1.
"""
import numpy as np

# (Y, U, V) -> [B, G, R]: the anchor values of the specification
ANCHORS = [((235, 128, 128), [255, 255, 255]), ((16, 128, 128), [0, 0, 0]), ((81, 90, 240), [0, 0, 254]), ((145, 54, 34), [1, 255, 0]),
           ((41, 240, 110), [255, 0, 0]), ((0, 0, 0), [0, 154, 0]), ((255, 255, 255), [255, 125, 255]), ((255, 0, 0), [20, 255, 74]),
           ((128, 255, 0), [255, 185, 0]), ((1, 2, 3), [0, 151, 0])]


def pixels(y, u, v):
    """Arrays of Y, U, V samples of one shape -> uint8 [..., 3] BGR."""
    y, u, v = (np.asarray(a).astype(np.int64) for a in (y, u, v))
    c = np.maximum(y - 16, 0) * 1220542
    u, v = u - 128, v - 128
    half, one = 2 ** 19, 2 ** 20
    chans = [np.floor_divide(c + 2116026 * u + half, one), np.floor_divide(c - 409993 * u - 852492 * v + half, one),
             np.floor_divide(c + 1673527 * v + half, one)]
    return np.stack([np.minimum(np.maximum(ch, 0), 255) for ch in chans], axis=-1).astype(np.uint8)


def split_chroma(planes, layout):
    """-> (Y, U, V) as separate 2-D planes."""
    if layout == "i420":
        y, u, v = planes
        return np.asarray(y), np.asarray(u), np.asarray(v)
    assert layout == "nv12", layout
    y, uv = planes
    uv = np.asarray(uv)
    return np.asarray(y), uv[:, 0::2], uv[:, 1::2]


def convert(planes, layout, rows=None, parity=0):
    """uint8 BGR [r1 - r0, w, 3] of luma rows [r0, r1) (default: all) of the planes."""
    y, u, v = split_chroma(planes, layout)
    h, w = y.shape
    r0, r1 = (0, h) if rows is None else rows
    rr = np.arange(r0, r1)
    cr = (rr + parity) // 2
    cc = np.arange(w) // 2
    if r1 <= r0:
        return np.zeros((0, w, 3), np.uint8)
    return pixels(y[r0:r1], u[cr][:, cc], v[cr][:, cc])


def packed_bytes(h, w, parity=0):
    return h * w + 2 * ((w + 1) // 2) * ((h + parity + 1) // 2)


def unpack(packed, h, w, layout, parity=0):
    """A packed (sub-)frame (h luma rows, then (h + parity + 1) >> 1 chroma rows per plane) -> planes for convert()."""
    packed = np.asarray(packed, np.uint8).reshape(-1)
    ch, cw = (h + parity + 1) // 2, (w + 1) // 2
    assert packed.size >= packed_bytes(h, w, parity)
    y = packed[:h * w].reshape(h, w)
    if layout == "i420":
        return y, packed[h * w:h * w + ch * cw].reshape(ch, cw), packed[h * w + ch * cw:h * w + 2 * ch * cw].reshape(ch, cw)
    return y, packed[h * w:h * w + 2 * ch * cw].reshape(ch, 2 * cw)


def pack(planes, layout):
    """Planes -> the packed bytes (1-D uint8)."""
    return np.concatenate([np.ascontiguousarray(p, np.uint8).reshape(-1) for p in planes])


def random_planes(rng, h, w, layout, parity=0, mid=False):
    """Random planes of an h x w (sub-)frame: uniform bytes (about 40 % of the channels clip), or mid-range ones that almost never do."""
    ch, cw = (h + parity + 1) // 2, (w + 1) // 2
    ylo, yhi, clo, chi = (60, 201, 100, 157) if mid else (0, 256, 0, 256)
    y = rng.integers(ylo, yhi, size=(h, w), dtype=np.uint8)
    if layout == "i420":
        return y, rng.integers(clo, chi, size=(ch, cw), dtype=np.uint8), rng.integers(clo, chi, size=(ch, cw), dtype=np.uint8)
    return y, rng.integers(clo, chi, size=(ch, 2 * cw), dtype=np.uint8)
