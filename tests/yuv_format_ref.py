"""The conversion of include/vse_hip.h vse_yuv_to_bgr_format restated in numpy, independently of the product's code: int64 arithmetic and
an explicit floor division by 2**20 instead of int32 and a shift.  A format is the tuple (sub_x, sub_y, chroma, depth, msb, matrix,
full_range) of integers (matrix 0 bt601, 1 bt709, 2 bt2020).  With s = depth - 8:

    sample  = word                      (depth 8, or msb 0: a word above 2**depth - 1 counts as 2**depth - 1)
            = word >> (16 - depth)      (msb 1)
    limited: c = max(Y - (16 << s), 0) * KY_s        full: c = Y * (2**20 >> s)
    u = U - (128 << s), v = V - (128 << s)           (grey: u = v = 0)
    B = clip8(floor((c + BU_s u + 2**19) / 2**20)), G = clip8(floor((c + GU_s u + GV_s v + 2**19) / 2**20)), R = clip8(floor((c + RV_s v + 2**19) / 2**20))
    K_s = sign(K_0) * ((|K_0| + ((1 << s) >> 1)) >> s)

Planes hold samples (uint8, or uint16 above 8 bits): (Y,), (Y, U, V) or (Y, UV) with U at the even samples.  Output row r of the row range
takes its chroma from row (r + parity) >> sub_y of the chroma planes given, column x >> sub_x.
"""
import numpy as np

MATRICES = ("bt601", "bt709", "bt2020")
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}
KY_LIMITED = 1220542
# limited range: BT.601 and BT.709 as tests/yuv_ref.py and tests/yuv709_ref.py have them; the rest by literals() below
LIMITED = {"bt601": (2116026, -409993, -852492, 1673527), "bt709": (2215014, -223607, -558796, 1879825),
           "bt2020": (2245811, -196426, -682019, 1760217)}
FULL = {"bt601": (1858077, -360853, -748826, 1470104), "bt709": (1945738, -196424, -490864, 1651297),
        "bt2020": (1972791, -172546, -599107, 1546230)}


def literals(matrix, full_range):
    """(BU, GU, GV, RV)_0 from the formulas, in float64: round(k * 2**20) of 2 (1 - Kb), -2 Kb (1 - Kb) / Kg, -2 Kr (1 - Kr) / Kg,
    2 (1 - Kr), times 255/224 for limited range."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    s = 2.0 ** 20 * (1.0 if full_range else 255.0 / 224.0)
    return (round(2 * (1 - kb) * s), -round(2 * kb * (1 - kb) / kg * s), -round(2 * kr * (1 - kr) / kg * s), round(2 * (1 - kr) * s))


def scaled(k0, s):
    m = (abs(k0) + ((1 << s) >> 1)) >> s
    return -m if k0 < 0 else m


def factors(fmt):
    """-> (yoff, coff, KY_s, BU_s, GU_s, GV_s, RV_s) as Python integers."""
    _sx, _sy, _chroma, depth, _msb, matrix, full = fmt
    s = depth - 8
    name = MATRICES[matrix]
    k0 = ((1 << 20,) + FULL[name]) if full else ((KY_LIMITED,) + LIMITED[name])
    return (0 if full else 16 << s, 128 << s) + tuple(scaled(k, s) for k in k0)


def values(words, fmt):
    """Stored words -> sample values, int64."""
    depth, msb = fmt[3], fmt[4]
    w = np.asarray(words).astype(np.int64)
    return w >> (16 - depth) if msb else np.minimum(w, (1 << depth) - 1)


def sums(y, u, v, fmt):
    """Sample VALUES of one shape -> the three sums before the division (B, G, R), in the integer type of the inputs' promotion with
    `dtype` int64 (the int32 test calls sums32)."""
    yoff, coff, ky, bu, gu, gv, rv = factors(fmt)
    y, u, v = (np.asarray(a).astype(np.int64) for a in (y, u, v))
    c = np.maximum(y - yoff, 0) * ky
    u, v = (u - coff, v - coff) if fmt[2] else (u * 0, v * 0)
    half = 2 ** 19
    return c + bu * u + half, c + gu * u + gv * v + half, c + rv * v + half


def sums32(y, u, v, fmt):
    """sums() with every operation in int32 (numpy wraps silently on overflow, which is what the comparison is for)."""
    yoff, coff, ky, bu, gu, gv, rv = (np.int32(k) for k in factors(fmt))
    y, u, v = (np.asarray(a).astype(np.int32) for a in (y, u, v))
    with np.errstate(over="ignore"):
        c = np.maximum(y - yoff, np.int32(0)) * ky
        u, v = (u - coff, v - coff) if fmt[2] else (u * np.int32(0), v * np.int32(0))
        half = np.int32(2 ** 19)
        return c + bu * u + half, c + gu * u + gv * v + half, c + rv * v + half


def pixels(y, u, v, fmt):
    """Arrays of stored Y, U, V words of one shape -> uint8 [..., 3] BGR."""
    chans = [np.floor_divide(t, 2 ** 20) for t in sums(values(y, fmt), values(u, fmt), values(v, fmt), fmt)]
    return np.stack([np.minimum(np.maximum(ch, 0), 255) for ch in chans], axis=-1).astype(np.uint8)


def float_pixels(y, u, v, fmt):
    """The real-number conversion of sample VALUES, float64, rounded to nearest and clipped -> uint8 [..., 3] BGR."""
    _sx, _sy, chroma, depth, _msb, matrix, full = fmt
    kr, kb = KR_KB[MATRICES[matrix]]
    kg = 1.0 - kr - kb
    s = float(1 << (depth - 8))
    y, u, v = (np.asarray(a, np.float64) for a in (y, u, v))
    if full:
        yy, cs = y / s, 1.0 / s
    else:
        yy, cs = np.maximum(y - 16 * s, 0) * (255.0 / 219.0) / s, 255.0 / 224.0 / s
    u, v = ((u - 128 * s) * cs, (v - 128 * s) * cs) if chroma else (u * 0, v * 0)
    b = yy + 2 * (1 - kb) * u
    g = yy - 2 * kb * (1 - kb) / kg * u - 2 * kr * (1 - kr) / kg * v
    r = yy + 2 * (1 - kr) * v
    return np.stack([np.clip(np.floor(ch + 0.5), 0, 255) for ch in (b, g, r)], axis=-1).astype(np.uint8)


def sample_dtype(fmt):
    return np.uint8 if fmt[3] == 8 else np.dtype("<u2")


def chroma_dims(h, w, fmt, parity=0):
    """Chroma rows and columns of a packed (sub-)frame of h x w pixels that starts at row parity `parity`."""
    return ((h - 1 + parity) >> fmt[1]) + 1, (w + fmt[0]) >> fmt[0]


def plane_shapes(h, w, fmt, parity=0):
    ch, cw = chroma_dims(h, w, fmt, parity)
    return [(h, w)] + ([], [(ch, cw)] * 2, [(ch, 2 * cw)])[fmt[2]]


def packed_bytes(h, w, fmt, parity=0):
    return np.dtype(sample_dtype(fmt)).itemsize * sum(r * c for r, c in plane_shapes(h, w, fmt, parity))


def split_chroma(planes, fmt):
    """-> (Y, U, V) as separate 2-D planes (grey: U = V = None)."""
    if fmt[2] == 0:
        return np.asarray(planes[0]), None, None
    if fmt[2] == 1:
        return tuple(np.asarray(p) for p in planes)
    uv = np.asarray(planes[1])
    return np.asarray(planes[0]), uv[:, 0::2], uv[:, 1::2]


def convert(planes, fmt, rows=None, parity=0):
    """uint8 BGR [r1 - r0, w, 3] of luma rows [r0, r1) (default: all) of the planes."""
    y, u, v = split_chroma(planes, fmt)
    h, w = y.shape
    r0, r1 = (0, h) if rows is None else rows
    if r1 <= r0:
        return np.zeros((0, w, 3), np.uint8)
    if u is None:
        z = np.zeros((r1 - r0, w), np.int64)
        return pixels(y[r0:r1], z, z, fmt)
    cr, cc = (np.arange(r0, r1) + parity) >> fmt[1], np.arange(w) >> fmt[0]
    return pixels(y[r0:r1], u[cr][:, cc], v[cr][:, cc], fmt)


def pack(planes, fmt):
    """Planes -> the packed bytes (1-D uint8), samples little-endian."""
    return np.concatenate([np.ascontiguousarray(p, sample_dtype(fmt)).reshape(-1).view(np.uint8) for p in planes])


def unpack(packed, h, w, fmt, parity=0):
    """A packed (sub-)frame -> planes for convert()."""
    packed = np.ascontiguousarray(packed, np.uint8).reshape(-1)
    assert packed.size >= packed_bytes(h, w, fmt, parity)
    ss, pos, planes = np.dtype(sample_dtype(fmt)).itemsize, 0, []
    for r, c in plane_shapes(h, w, fmt, parity):
        planes.append(packed[pos:pos + r * c * ss].view(sample_dtype(fmt)).reshape(r, c))
        pos += r * c * ss
    return tuple(planes)


def sub_frame(planes, fmt, y0, y1):
    """The planes of the packed sub-frame of luma rows [y0, y1) of a whole picture's planes, and its row parity: luma rows y0..y1, chroma
    rows y0 >> sub_y .. ((y1 - 1) >> sub_y) + 1."""
    c0, c1 = y0 >> fmt[1], ((y1 - 1) >> fmt[1]) + 1
    return (planes[0][y0:y1],) + tuple(p[c0:c1] for p in planes[1:]), y0 & fmt[1]


def random_planes(rng, h, w, fmt, parity=0, wild=False):
    """Random planes of an h x w (sub-)frame: stored words of the format (values 0 .. 2**depth - 1, shifted up for msb formats, whose low
    bits are random too; wild: any 16-bit word for the low-bit 2-byte formats, so that some exceed 2**depth - 1)."""
    depth, msb = fmt[3], fmt[4]
    out = []
    for shp in plane_shapes(h, w, fmt, parity):
        if depth == 8:
            out.append(rng.integers(0, 256, size=shp, dtype=np.uint8))
        elif msb or wild:
            out.append(rng.integers(0, 65536, size=shp).astype("<u2"))
        else:
            out.append(rng.integers(0, 1 << depth, size=shp).astype("<u2"))
    return tuple(out)
