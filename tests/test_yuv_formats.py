"""The wider YUV ingest on the host: the integers of vse_yuv_to_bgr_format (tests/yuv_format_ref.py restates them in int64) against their
float64 formulas, against the 8-bit references at depth 8 and against int32; ingest.YuvFormat / YuvFrame / the Y4M parser with wide=True /
YuvSource / Y4mStream; the command lines with a scripted recogniser.  CPU only."""
import itertools

import numpy as np
import pytest

import area_cells_ref
import yuv709_ref
import yuv_format_ref as R
import yuv_ref
from frame_change_ref import NumpyCounter
from test_one_pass import AREA, FPS, LookupOcr, clip, host_stack, piped, run, text_box  # noqa: F401  (host_stack is a fixture)
from vse_amd import area_locator, extractor, ingest

SUBS = [(0, 0), (1, 0), (1, 1)]
DEPTHS = (8, 10, 12, 16)


def all_formats(depths=DEPTHS, matrices=(0, 1, 2), ranges=(0, 1)):
    """Every valid (sub_x, sub_y, chroma, depth, msb, matrix, full_range) at the depths given."""
    out = []
    for depth, matrix, full in itertools.product(depths, matrices, ranges):
        for msb in ((0,) if depth == 8 else (0, 1)):
            out.append((0, 0, 0, depth, msb, matrix, full))
            out += [(sx, sy, 1, depth, msb, matrix, full) for sx, sy in SUBS]
            out.append((1, 1, 2, depth, msb, matrix, full))
    return out


def product_format(fmt):
    return ingest.YuvFormat(*fmt[:5], R.MATRICES[fmt[5]], fmt[6])


def ident(fmt):
    return "-".join(str(v) for v in fmt)


# ---- the integers ----------------------------------------------------------------------------------------------------------------
def test_literals_equal_their_formulas():
    for m in R.MATRICES:
        assert R.literals(m, 1) == R.FULL[m], m
    assert R.literals("bt2020", 0) == R.LIMITED["bt2020"]
    assert R.literals("bt709", 0) == R.LIMITED["bt709"] == yuv709_ref.factors() == ingest.YUV_MATRICES["bt709"]
    assert R.LIMITED["bt601"] == ingest.YUV_MATRICES["bt601"]               # (cv2's numbers, kept)
    # the product's table is the reference's
    for full, m in itertools.product((0, 1), R.MATRICES):
        assert ingest.YUV_K0[full, m] == ((1 << 20,) + R.FULL[m] if full else (R.KY_LIMITED,) + R.LIMITED[m])
    # K_s: rounded to nearest, sign kept; full range's luma factor is 2**20 >> s at every depth
    assert [R.scaled(k, 2) for k in (1220542, -409993, 7, -7, 6, -6)] == [305136, -102498, 2, -2, 2, -2]
    for depth in range(8, 17):
        assert R.factors((1, 1, 1, depth, 0, 0, 1))[2] == (1 << 20) >> (depth - 8)
        assert product_format((1, 1, 1, depth, 0, 2, 0)).factors()[2:] == R.factors((1, 1, 1, depth, 0, 2, 0))


def test_depth_8_is_the_8_bit_references_on_every_triple():
    """s = 0, limited: tests/yuv_ref.py (BT.601) and tests/yuv709_ref.py (BT.709) bit for bit, on their anchors and on all 2**24 triples."""
    for ref, matrix in ((yuv_ref, 0), (yuv709_ref, 1)):
        fmt = (1, 1, 1, 8, 0, matrix, 0)
        for (y, u, v), bgr in ref.ANCHORS:
            assert R.pixels(y, u, v, fmt).tolist() == bgr
        uu, vv = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
        for y0 in range(0, 256, 16):
            y = np.arange(y0, y0 + 16)[:, None, None]
            assert np.array_equal(R.pixels(y + 0 * uu, uu + 0 * y, vv + 0 * y, fmt), ref.pixels(y + 0 * uu, uu + 0 * y, vv + 0 * y)), (matrix, y0)


@pytest.mark.parametrize("depth", range(8, 17))
def test_int32_holds_the_sums(depth):
    """The extreme sample values of the depth, every matrix and range: the int32 sums are the int64 sums and stay inside the bound that
    csrc/yuv.hip states (600 545 152); every operand fits 24 signed bits."""
    maxv, s = (1 << depth) - 1, depth - 8
    ends = sorted({0, 1, (16 << s) - 1, 16 << s, (128 << s) - 1, 128 << s, (128 << s) + 1, maxv - 1, maxv})
    y, u, v = (a.reshape(-1) for a in np.meshgrid(ends, ends, ends, indexing="ij"))
    for matrix, full, chroma in itertools.product((0, 1, 2), (0, 1), (0, 1)):
        fmt = (0, 0, chroma, depth, 0, matrix, full)
        wide, narrow = R.sums(y, u, v, fmt), R.sums32(y, u, v, fmt)
        for a, b in zip(wide, narrow):
            assert np.array_equal(a, b.astype(np.int64)) and np.abs(a).max() <= 600545152, fmt
        assert all(abs(k) < 1 << 23 for k in R.factors(fmt)[2:])


# ---- the product's host conversion --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", all_formats(), ids=ident)
def test_host_to_bgr_equals_reference(fmt):
    rng = np.random.default_rng(hash(fmt) & 0xffff)
    pf = product_format(fmt)
    for (h, w), wild in (((5, 7), False), ((6, 8), True), ((1, 1), False)):
        planes = R.random_planes(rng, h, w, fmt, wild=wild)
        assert [p.shape for p in planes] == pf.plane_shapes(h, w) == R.plane_shapes(h, w, fmt)
        assert pf.frame_bytes(h, w) == R.packed_bytes(h, w, fmt)
        got = ingest.YuvFrame(planes, h, w, pf).to_bgr()
        assert got.dtype == np.uint8 and np.array_equal(got, R.convert(planes, fmt)), (h, w, wild)


def exhaustive_10_bit(matrix, full):
    """4:4:4 10-bit planes [1024, 2048]: the left half holds every (Y, U) with a seeded random V, the right half every (Y, V) with a
    seeded random U, so B is checked over all of its inputs on the left and R on the right."""
    rng = np.random.default_rng(7 + matrix + 3 * full)
    a, b = np.meshgrid(np.arange(1024), np.arange(1024), indexing="ij")
    rnd = rng.integers(0, 1024, size=(1024, 1024))
    y = np.concatenate([a, a], axis=1).astype("<u2")
    u = np.concatenate([b, rnd], axis=1).astype("<u2")
    v = np.concatenate([rnd, b], axis=1).astype("<u2")
    return (y, u, v), (0, 0, 1, 10, 0, matrix, full)


def extremes_and_random(depth, rng, count=1 << 16):
    """Sample VALUES for G: every combination of the extreme values of the depth, then `count` seeded random triples."""
    maxv, s = (1 << depth) - 1, depth - 8
    ends = [0, 16 << s, (128 << s) - 1, 128 << s, 235 << s, 240 << s, maxv]
    e = np.array(list(itertools.product(ends, ends, ends)))
    r = rng.integers(0, maxv + 1, size=(count, 3))
    return np.concatenate([e, r]).T


@pytest.mark.parametrize("matrix,full", list(itertools.product((0, 1, 2), (0, 1))))
def test_every_10_bit_luma_chroma_pair(matrix, full):
    planes, fmt = exhaustive_10_bit(matrix, full)
    got = ingest.YuvFrame(planes, 1024, 2048, product_format(fmt)).to_bgr()
    want = R.convert(planes, fmt)
    assert np.array_equal(got[:, :1024, 0], want[:, :1024, 0]) and np.array_equal(got[:, 1024:, 2], want[:, 1024:, 2])
    assert np.array_equal(got, want)
    # G: the extremes and a seeded random set
    y, u, v = extremes_and_random(10, np.random.default_rng(11))
    row = tuple(a.astype("<u2").reshape(1, -1) for a in (y, u, v))
    assert np.array_equal(ingest.YuvFrame(row, 1, y.size, product_format(fmt)).to_bgr(), R.convert(row, fmt))


@pytest.mark.parametrize("depth", DEPTHS)
def test_integers_stay_within_one_level_of_the_real_numbers(depth):
    """Against the float64 matrix rounded to nearest: at most one level apart on every (Y, U) and (Y, V) pair (depth 8 and 10; a 2**20
    seeded sample of them above) and on G's extremes and random set.  The share of pixels that differ is printed (EXPERIMENTS.md)."""
    rng = np.random.default_rng(depth)
    maxv = (1 << depth) - 1
    for matrix, full in itertools.product((0, 1, 2), (0, 1)):
        fmt = (0, 0, 1, depth, 0, matrix, full)
        if depth <= 10:
            a, b = (g.reshape(-1) for g in np.meshgrid(np.arange(maxv + 1), np.arange(maxv + 1), indexing="ij"))
        else:
            a, b = rng.integers(0, maxv + 1, size=(2, 1 << 20))
        other = rng.integers(0, maxv + 1, size=a.size)
        ey, eu, ev = extremes_and_random(depth, rng)
        y, u, v = np.concatenate([a, a, ey]), np.concatenate([b, other, eu]), np.concatenate([other, b, ev])
        ints = R.pixels(y, u, v, fmt).astype(np.int64)       # (low-bit words that are values: values() leaves them)
        real = R.float_pixels(y, u, v, fmt).astype(np.int64)
        diff = np.abs(ints - real)
        share = float(np.mean(diff > 0))
        print(f"depth {depth} {R.MATRICES[matrix]} {'full' if full else 'limited'}: {share:.4%} of the channel values differ by one level")
        assert diff.max() <= 1, (fmt, int(diff.max()))


# ---- frames: slices and packing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [(0, 0, 0, 10, 0, 0, 0), (0, 0, 1, 8, 0, 1, 0), (1, 0, 1, 10, 0, 1, 1), (1, 1, 1, 10, 0, 2, 0), (1, 1, 2, 10, 1, 1, 0),
                                 (1, 1, 2, 8, 0, 0, 1), (1, 1, 1, 8, 0, 0, 0)], ids=ident)
def test_row_slices_and_packing(fmt):
    h, w = 9, 7
    rng = np.random.default_rng(5)
    pf = product_format(fmt)
    planes = R.random_planes(rng, h, w, fmt)
    frame = ingest.YuvFrame(planes, h, w, pf)
    whole = R.convert(planes, fmt)
    assert frame.shape == (h, w, 3) and frame.row_parity == 0 and frame.packed_bytes == R.packed_bytes(h, w, fmt)
    for y0, y1 in ((0, 9), (1, 9), (3, 4), (3, 8), (4, 9), (5, 6), (2, 2)):
        part = frame[y0:y1]
        assert part.shape == (y1 - y0, w, 3) and part.row_parity == (y0 & fmt[1]) and np.array_equal(part.to_bgr(), whole[y0:y1])
        if y1 == y0:
            continue
        sub, parity = R.sub_frame(planes, fmt, y0, y1)
        want = R.pack(sub, fmt)
        assert part.packed_bytes == want.size == R.packed_bytes(y1 - y0, w, fmt, parity)
        dst = np.full(want.size + 5, 0xA5, np.uint8)
        assert part.pack_into(dst) == want.size and np.array_equal(dst[:want.size], want) and np.all(dst[want.size:] == 0xA5)
        assert np.array_equal(R.convert(R.unpack(dst, y1 - y0, w, fmt, parity), fmt, parity=parity), whole[y0:y1])
    inner = frame[2:8][1:3]
    assert (inner.y0, inner.y1) == (3, 5) and np.array_equal(inner.to_bgr(), whole[3:5])
    for bad in (0, (slice(None), 0), slice(None, None, 2)):
        with pytest.raises(TypeError):
            frame[bad]
    with pytest.raises(ValueError):
        ingest.YuvFrame(planes[:-1] + (planes[-1][:, :-1],), h, w, pf)
    if fmt[3] > 8:
        with pytest.raises(ValueError):
            ingest.YuvFrame(tuple(p.astype(np.uint8) for p in planes), h, w, pf)


# ---- names -----------------------------------------------------------------------------------------------------------------------------
PIX_FMTS = {"yuv420p": (1, 1, 1, 8, 0, 0), "yuvj420p": (1, 1, 1, 8, 0, 1), "nv12": (1, 1, 2, 8, 0, 0), "yuv422p": (1, 0, 1, 8, 0, 0),
            "yuv444p": (0, 0, 1, 8, 0, 0), "gray": (0, 0, 0, 8, 0, 0), "yuv420p10le": (1, 1, 1, 10, 0, 0), "yuv422p10le": (1, 0, 1, 10, 0, 0),
            "yuv444p10le": (0, 0, 1, 10, 0, 0), "yuv420p12le": (1, 1, 1, 12, 0, 0), "p010le": (1, 1, 2, 10, 1, 0), "p016le": (1, 1, 2, 16, 1, 0),
            "gray10le": (0, 0, 0, 10, 0, 0), "yuvj444p": (0, 0, 1, 8, 0, 1), "yuv420p9le": (1, 1, 1, 9, 0, 0), "yuv444p16le": (0, 0, 1, 16, 0, 0),
            "p012le": (1, 1, 2, 12, 1, 0), "i420": (1, 1, 1, 8, 0, 0), "gray16le": (0, 0, 0, 16, 0, 0), "yuv422p14le": (1, 0, 1, 14, 0, 0)}


def test_pix_fmt_names():
    for name, (sx, sy, chroma, depth, msb, full) in PIX_FMTS.items():
        assert ingest.YuvFormat.from_pix_fmt(name) == ingest.YuvFormat(sx, sy, chroma, depth, msb, "bt601", full), name
    f = ingest.YuvFormat.from_pix_fmt("yuv420p10le", matrix="bt2020", range="full")
    assert (f.matrix, f.full_range, f.sample_bytes, f.sample_dtype) == ("bt2020", 1, 2, np.dtype("<u2"))
    assert ingest.YuvFormat.from_pix_fmt("yuvj420p", range="limited").full_range == 0
    for bad in ("yuv420p10be", "p010be", "gray12be"):
        with pytest.raises(ValueError, match="big-endian"):
            ingest.YuvFormat.from_pix_fmt(bad)
    for bad in ("yuyv422", "uyvy422", "y210le", "yuv411p", "yuv410p", "yuva420p", "yuv420p11le", "yuvj420p10le", "nv21", "rgb24", "yuv420p8le"):
        with pytest.raises(ValueError, match=bad):
            ingest.YuvFormat.from_pix_fmt(bad)
    with pytest.raises(ValueError, match="range"):
        ingest.YuvFormat.from_pix_fmt("yuv420p", range="tv")
    for bad in (dict(sub_x=0, sub_y=1), dict(chroma=3), dict(depth=7), dict(depth=17), dict(depth=8, msb=1), dict(chroma=0), dict(chroma=2, sub_y=0),
                dict(matrix="bt470")):
        with pytest.raises(ValueError):
            ingest.YuvFormat(**bad)


# ---- the Y4M header --------------------------------------------------------------------------------------------------------------------
ACCEPTED = {"C420": (1, 1, 1, 8), "C420jpeg": (1, 1, 1, 8), "C420mpeg2": (1, 1, 1, 8), "C420paldv": (1, 1, 1, 8), "C422": (1, 0, 1, 8),
            "C444": (0, 0, 1, 8), "Cmono": (0, 0, 0, 8)}
for _sub, (_sx, _sy) in (("420", (1, 1)), ("422", (1, 0)), ("444", (0, 0))):
    for _d in (9, 10, 12, 14, 16):
        ACCEPTED[f"C{_sub}p{_d}"] = (_sx, _sy, 1, _d)
for _d in (9, 10, 12, 14, 16):
    ACCEPTED[f"Cmono{_d}"] = (0, 0, 0, _d)
REFUSED = ["It", "Ib", "Im", "C411", "C444alpha", "C420p11", "C420p8", "C410", "Cmono11", "C420jpegp10", "XCOLORRANGE=WIDE", "Q7", "C"]


def header_both_ways(tmp_path, tokens, **kw):
    """Y4mSource(path, wide=True) and Y4mStream(pipe, wide=True) over one header -> the two sources (or the two ValueErrors)."""
    data = b"YUV4MPEG2 W4 H2 F25:1 " + tokens.encode() + b"\n"
    path = str(tmp_path / "clip.y4m")
    with open(path, "wb") as fp:
        fp.write(data)
    out = []
    for make in (lambda: ingest.Y4mSource(path, wide=True, **kw), None):
        fp = th = None
        try:
            if make is None:
                fp, th = piped(data, 3)
                out.append(ingest.Y4mStream(fp, name=path, wide=True, **kw))
            else:
                out.append(make())
        except ValueError as e:
            out.append(e)
        finally:
            if fp is not None:
                fp.close()
                th.join()
    return out


@pytest.mark.parametrize("token", sorted(ACCEPTED))
def test_wide_parser_accepts(tmp_path, token):
    sx, sy, chroma, depth = ACCEPTED[token]
    for rng_tok, range_kw, full in (("", "auto", 0), ("XCOLORRANGE=FULL", "auto", 1), ("XCOLORRANGE=LIMITED", "auto", 0), ("XCOLORRANGE=FULL", "limited", 0),
                                    ("", "full", 1)):
        src, st = header_both_ways(tmp_path, f"Ip A1:1 {token} XYSCSS=FOO {rng_tok}", range=range_kw, matrix="bt709")
        want = ingest.YuvFormat(sx, sy, chroma, depth, 0, "bt709", full)
        assert src.fmt == st.fmt == want and (src.width, src.height, src.fps) == (st.width, st.height, st.fps) == (4, 2, 25.0)
        src.close()
    # without a C token: 4:2:0
    src, st = header_both_ways(tmp_path, "")
    assert src.fmt == st.fmt == ingest.YuvFormat()
    src.close()


@pytest.mark.parametrize("token", REFUSED)
def test_wide_parser_refuses_naming_the_token(tmp_path, token):
    of_file, of_stream = header_both_ways(tmp_path, token)
    assert isinstance(of_file, ValueError) and isinstance(of_stream, ValueError)
    assert token in str(of_file) and str(of_file) == str(of_stream)                      # one parser, one message


def test_wide_is_opt_in(tmp_path):
    """Without wide=True the readers refuse what they refused, in the words they used; bt2020 needs wide as well."""
    for token in ("C420p10", "C422", "XCOLORRANGE=FULL"):
        path = str(tmp_path / "clip.y4m")
        with open(path, "wb") as fp:
            fp.write(b"YUV4MPEG2 W2 H2 F25:1 " + token.encode() + b"\n")
        with pytest.raises(ValueError) as e:
            ingest.open_source(path)
        assert token in str(e.value) and "is not supported" in str(e.value)
        assert ingest.open_source(path, wide=True).fmt is not None
    with pytest.raises(ValueError, match="bt2020"):
        ingest.open_source(path, matrix="bt2020")
    assert ingest.open_source(path, matrix="bt2020", wide=True).fmt.matrix == "bt2020"
    with pytest.raises(ValueError, match="bt470"):
        ingest.open_source(path, matrix="bt470", wide=True)


# ---- sources ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [1, 7, 4099])
@pytest.mark.parametrize("fmt", [(1, 1, 1, 10, 0, 1, 0), (0, 0, 1, 12, 0, 2, 1), (1, 0, 1, 8, 0, 0, 1), (0, 0, 0, 10, 0, 0, 0)], ids=ident)
def test_wide_stream_over_a_pipe_equals_the_file_source(tmp_path, fmt, chunk):
    h, w = 5, 7
    rng = np.random.default_rng(chunk)
    pf = product_format(fmt)
    frames = [R.random_planes(rng, h, w, fmt) for _ in range(4)]
    path = str(tmp_path / "clip.y4m")
    ingest.write_yuv(path, frames, pf, fps=FPS, y4m=True)
    with open(path, "rb") as fp:
        data = fp.read()
    kw = dict(wide=True, matrix=pf.matrix)
    src = ingest.open_source(path, **kw)
    assert isinstance(src, ingest.Y4mSource) and src.fmt == pf and src.frame_count == 4 and (src.width, src.height) == (w, h)
    fp, th = piped(data, chunk)
    st = ingest.Y4mStream(fp, **kw)
    assert st.fmt == pf and st.frame_count is None and not hasattr(st, "read")
    got = list(st.raw_frames())
    th.join()
    fp.close()
    assert st.frame_count == len(got) == 4
    for no, raw in enumerate(got, 1):
        assert isinstance(raw, ingest.YuvFrame) and raw.fmt == pf and raw.shape == (h, w, 3)
        assert all(np.array_equal(a, b) for a, b in zip(raw.planes, src.read_raw(no).planes))
        assert all(np.array_equal(a, b) for a, b in zip(raw.planes, frames[no - 1]))
        assert np.array_equal(raw.to_bgr(), src.read(no)) and np.array_equal(src.read(no), R.convert(frames[no - 1], fmt))
    assert src.read(5) is None and src.read_raw(0) is None
    # a stream that ends inside its last frame drops it, as the file does
    fp, th = piped(data[:-3], chunk)
    assert len(list(ingest.Y4mStream(fp, **kw).frames())) == 3
    th.join()
    fp.close()
    src.close()


@pytest.mark.parametrize("name,ext,fmt", [("p010le", ".p010", (1, 1, 2, 10, 1, 0, 0)), ("yuv422p10le", ".yuv", (1, 0, 1, 10, 0, 0, 0)),
                                          ("yuvj420p", ".bin", (1, 1, 1, 8, 0, 0, 1)), ("gray", ".raw", (0, 0, 0, 8, 0, 0, 0))])
def test_headerless_source(tmp_path, name, ext, fmt):
    h, w = 6, 10
    rng = np.random.default_rng(3)
    frames = [R.random_planes(rng, h, w, fmt) for _ in range(3)]
    path = str(tmp_path / ("clip" + ext))
    ingest.write_yuv(path, frames, product_format(fmt))
    with open(path, "ab") as fp:
        fp.write(b"\0" * 11)                                  # a partial last frame
    src = ingest.open_source(path, pix_fmt=None if ext == ".p010" else name, size=(w, h), fps=FPS)
    assert isinstance(src, ingest.YuvSource) and src.fmt == product_format(fmt) and src.frame_count == 3 and src.fps == FPS
    for no, (raw, bgr) in enumerate(zip(src.raw_frames(), src.frames()), 1):
        assert np.array_equal(bgr, R.convert(frames[no - 1], fmt)) and np.array_equal(raw.to_bgr(), bgr) and np.array_equal(src.read(no), bgr)
        assert raw.planes[0].dtype == R.sample_dtype(fmt)
    assert src.pos_msec(1) == 1000.0 / FPS and src.pos_msec(3) is None
    src.close()
    for kw in (dict(size=(w, h)), dict(fps=FPS)):
        with pytest.raises(ValueError):
            ingest.open_source(path, pix_fmt=name, **kw)
    with pytest.raises(ValueError, match="yuyv422"):
        ingest.open_source(path, pix_fmt="yuyv422", size=(w, h), fps=FPS)


def test_retention_counts_the_real_bytes():
    fmt = ingest.YuvFormat.from_pix_fmt("yuv420p10le")
    planes = R.random_planes(np.random.default_rng(1), 6, 8, tuple(fmt[:5]) + (0, 0))
    assert extractor._frame_nbytes(ingest.YuvFrame(planes, 6, 8, fmt)) == 6 * 8 * 3 == fmt.frame_bytes(6, 8)


# ---- the command lines ---------------------------------------------------------------------------------------------------------------
def wide_clip(tmp_path, kind):
    """The change clip as a 10-bit 4:2:0 Y4M (samples << 2) or as an 8-bit Y4M tagged full range -> (path, its frames converted on the
    host, truth)."""
    frames, truth = clip("change")
    yuv = [ingest.bgr_to_yuv420(f) for f in frames]
    path = str(tmp_path / f"{kind}.y4m")
    if kind == "ten":
        fmt = ingest.YuvFormat(depth=10)
        ingest.write_yuv(path, [tuple(p.astype("<u2") << 2 for p in f) for f in yuv], fmt, fps=FPS, y4m=True)
    else:
        fmt = ingest.YuvFormat(full_range=1)
        ingest.write_yuv(path, yuv, fmt, fps=FPS, y4m=True)
    src = ingest.Y4mSource(path, wide=True)
    assert src.fmt == fmt and src.frame_count == len(frames)
    decoded = list(src.frames())
    src.close()
    return path, decoded, truth


def bgr_source(decoded):
    """The converted frames as a BGR source with the time stamps of a constant frame rate, as the YUV sources give them."""
    arr = extractor.ArraySource(decoded, FPS)
    arr.pos_msec = lambda k: None if not 0 <= k < len(decoded) else k * 1000.0 / FPS
    return arr


@pytest.mark.parametrize("kind", ["ten", "full"])
def test_extractor_command_line_takes_wide_yuv(host_stack, tmp_path, monkeypatch, capsys, kind):
    path, decoded, truth = wide_clip(tmp_path, kind)
    _, want = run(bgr_source(decoded), decoded, truth, "change", 8, None)
    assert want[3].count(" --> ") == len(truth)
    area = f"{AREA.ymin},{AREA.ymax},{AREA.xmin},{AREA.xmax}"
    common = ["--area", area, "--selector", "change", "--batch", "8"]
    out = str(tmp_path / "out.srt")
    ocr = LookupOcr(decoded, truth, text_box(AREA))
    assert extractor.main([path, "--wide-yuv", "-o", out] + common, ocr=ocr, counter=NumpyCounter()) == 0
    assert open(out).read() == want[3] and ocr.seen == want[1]
    # the same bytes on standard input, in one pass
    with open(path, "rb") as fp:
        data = fp.read()
    pipe, th = piped(data, 4099)
    monkeypatch.setattr("sys.stdin", type("Stdin", (), {"buffer": pipe})())
    ocr = LookupOcr(decoded, truth, text_box(AREA))
    assert extractor.main(["-", "--wide-yuv"] + common, ocr=ocr, counter=NumpyCounter()) == 0
    pipe.close()
    th.join()
    assert capsys.readouterr().out == want[3]
    # without --wide-yuv: refused by the parser, in its words
    ocr = LookupOcr(decoded, truth, text_box(AREA))
    assert extractor.main([path] + common, ocr=ocr, counter=NumpyCounter()) == 2 and ocr.seen == []
    err = capsys.readouterr().err
    assert err.startswith("extractor: ") and ("C420p10" if kind == "ten" else "XCOLORRANGE=FULL") in err
    assert extractor.main([path, "--matrix", "bt2020"] + common, ocr=ocr, counter=NumpyCounter()) == 2
    assert "extractor: " in capsys.readouterr().err
    if kind == "full":          # --range overrides the header: limited gives the 8-bit reader's frames, hence not `decoded`
        src = ingest.open_source(path, wide=True, range="limited")
        assert np.array_equal(src.read(5), ingest.Yuv420Frame(src.read_raw(5).planes, *decoded[0].shape[:2]).to_bgr())
        src.close()


def test_extractor_command_line_takes_a_pix_fmt(host_stack, tmp_path, capsys):
    frames, truth = clip("change")
    fmt = ingest.YuvFormat.from_pix_fmt("p010le")
    path = str(tmp_path / "clip.p010")
    yuv = [ingest.bgr_to_yuv420(f) for f in frames]
    ingest.write_yuv(path, [(y.astype("<u2") << 8, np.stack([u, v], axis=2).reshape(u.shape[0], -1).astype("<u2") << 8) for y, u, v in yuv], fmt)
    src = ingest.open_source(path, size=(frames[0].shape[1], frames[0].shape[0]), fps=FPS)
    decoded = list(src.frames())
    src.close()
    _, want = run(bgr_source(decoded), decoded, truth, "change", 8, None)
    area = f"{AREA.ymin},{AREA.ymax},{AREA.xmin},{AREA.xmax}"
    common = ["--area", area, "--selector", "change", "--batch", "8", "--size", "640x360", "--fps", str(FPS)]
    for more in ([], ["--pix-fmt", "p010le"]):
        ocr = LookupOcr(decoded, truth, text_box(AREA))
        assert extractor.main([path] + more + common, ocr=ocr, counter=NumpyCounter()) == 0
        assert capsys.readouterr().out == want[3] and want[3].count(" --> ") == len(truth)
    ocr = LookupOcr(decoded, truth, text_box(AREA))
    assert extractor.main([path, "--pix-fmt", "y210le"] + common, ocr=ocr, counter=NumpyCounter()) == 2
    assert "y210le" in capsys.readouterr().err


def test_locator_command_line_takes_wide_yuv(tmp_path, capsys):
    path, decoded, _ = wide_clip(tmp_path, "ten")
    want = area_locator.AreaLocator(area_cells_ref.NumpyCells()).run(decoded, FPS)
    assert area_locator.main([path, "--wide-yuv"], cells_fn=area_cells_ref.NumpyCells()) == (0 if want is not None else 1)
    got = capsys.readouterr().out.split()
    if want is not None:
        assert got == [str(v) for v in (want.ymin, want.ymax, want.xmin, want.xmax)]
    assert area_locator.main([path], cells_fn=area_cells_ref.NumpyCells()) == 2
    assert "C420p10" in capsys.readouterr().err


# ---- the clip of the GPU's end-to-end run ----------------------------------------------------------------------------------------------
E2E_AREA = extractor.SubtitleArea(ymin=int(0.75 * 360) + 1, ymax=360, xmin=0, xmax=640)


def e2e_clips(tmp_path):
    """One synthetic clip as 8-bit 4:2:0 Y4M and as 10-bit 4:2:0 Y4M with the same samples << 2 -> (path, path, truth)."""
    from vse_amd import synth
    frames, truth = synth.make_clip([(None, 2), ("the quick brown fox", 7), ("seven wizards quietly box", 6), (None, 2), ("near frozen lakes", 4)],
                                    360, 640, seed=6)
    yuv = [ingest.bgr_to_yuv420(f) for f in frames]
    path8, path10 = str(tmp_path / "clip8.y4m"), str(tmp_path / "clip10.y4m")
    ingest.write_y4m(path8, yuv, FPS)
    ingest.write_yuv(path10, [tuple(p.astype("<u2") << 2 for p in f) for f in yuv], ingest.YuvFormat(depth=10), fps=FPS, y4m=True)
    return path8, path10, truth


def test_10_bit_clip_keeps_its_intervals(host_stack, tmp_path):
    """The premise of tests/test_gpu_yuv_formats.py's end-to-end run, with the numpy counter: the 10-bit clip's converted bytes differ from
    the 8-bit clip's by at most one level, and the change selector finds the same intervals (the clip's truth) and middle frames on both."""
    path8, path10, truth = e2e_clips(tmp_path)
    a, b = ingest.Y4mSource(path8), ingest.Y4mSource(path10, wide=True)
    got = []
    for src in (a, b):
        decoded = list(src.frames())
        got.append((decoded, run(src, decoded, truth, "change", 8, None, sub_area=E2E_AREA)[1]))
    diff = np.abs(np.stack(got[0][0]).astype(np.int16) - np.stack(got[1][0]))
    assert diff.max() <= 1
    assert got[0][1][0] == got[1][1][0] and got[0][1][1] == got[1][1][1]
    assert [(s, e) for s, e, _r in got[0][1][0]] == [(s, e) for s, e, _t in truth]
    a.close()
    b.close()
