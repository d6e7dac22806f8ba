"""YUV 4:2:0 ingest on the host: the conversion formula (tests/yuv_ref.py), ingest.Yuv420Frame (host conversion, row slices, packing
for vse_yuv420_to_bgr), the Y4M and headerless sources with their writers, open_source's dispatch and the extractor's host route.
CPU only: the size function comes from the cross-compiled library without a device."""
import ctypes

import numpy as np
import pytest

import yuv_ref
from vse_amd import extractor, ingest

LAYOUTS = ("i420", "nv12")


def make_frame(rng, h, w, layout, mid=False):
    return ingest.Yuv420Frame(yuv_ref.random_planes(rng, h, w, layout, mid=mid), h, w, layout)


def yuv_triples(rng, n, h, w):
    """n random (Y, U, V) plane triples (what the writers take)."""
    return [yuv_ref.random_planes(rng, h, w, "i420") for _ in range(n)]


def bgr_of(triple):
    return yuv_ref.convert(triple, "i420")


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree_on_the_yuv_entry_points(built_lib):
    """tests/test_abi.py reads function names without digits; the two entry points here carry one: header = library = engine's list."""
    import os
    import re
    from vse_amd import engine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "vse_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(vse_[a-z0-9_]+)\s*\(", src))
    numbered = sorted(n for n in declared if re.search(r"[0-9]", n))
    assert numbered == sorted(engine.EXPORTS_NUMBERED) == ["vse_yuv420_frame_bytes", "vse_yuv420_to_bgr"]
    assert declared == set(engine.EXPORTS) | set(engine.EXPORTS_NUMBERED)
    lib = ctypes.CDLL(built_lib)
    assert all(hasattr(lib, n) for n in numbered)
    assert engine.load_library().vse_yuv420_frame_bytes(2, 2, 0) == 6


# ---- the formula -----------------------------------------------------------------------------------------------------------------
def test_reference_gives_the_anchor_values():
    for (y, u, v), bgr in yuv_ref.ANCHORS:
        assert yuv_ref.pixels(y, u, v).tolist() == bgr, (y, u, v)
        assert yuv_ref.convert((np.array([[y]], np.uint8), np.array([[u]], np.uint8), np.array([[v]], np.uint8)), "i420").tolist() == [[bgr]]
        assert yuv_ref.convert((np.array([[y]], np.uint8), np.array([[u, v]], np.uint8)), "nv12").tolist() == [[bgr]]
        assert ingest.Yuv420Frame((np.array([[y]], np.uint8), np.array([[u, v]], np.uint8)), 1, 1, "nv12").to_bgr().tolist() == [[bgr]]


def test_reference_sums_fit_int32():
    """The largest magnitude of the three sums over the whole input domain is the specification's 560 969 128."""
    y, u, v = (np.array(a, np.int64) for a in np.meshgrid([0, 16, 255], [0, 255], [0, 255], indexing="ij"))
    c = np.maximum(y - 16, 0) * 1220542 + 2 ** 19
    sums = np.stack([c + 2116026 * (u - 128), c - 409993 * (u - 128) - 852492 * (v - 128), c + 1673527 * (v - 128)])
    assert np.abs(sums).max() == 560969128 < 2 ** 31


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("hw", [(1, 1), (2, 2), (3, 5), (5, 1), (16, 64), (17, 70)])
def test_host_conversion_equals_reference(hw, layout):
    h, w = hw
    rng = np.random.default_rng(100 * h + w)
    for mid in (False, True):
        f = make_frame(rng, h, w, layout, mid)
        got = f.to_bgr()
        assert got.dtype == np.uint8 and got.shape == f.shape == (h, w, 3)
        assert np.array_equal(got, yuv_ref.convert(f.planes, layout))


# ---- row slices and packing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_row_slices(layout):
    f = make_frame(np.random.default_rng(3), 7, 10, layout)
    full = f.to_bgr()
    for y0 in range(8):
        for y1 in range(8):
            s = f[y0:y1]
            assert s.shape == full[y0:y1].shape == (max(y1 - y0, 0), 10, 3)
            assert np.array_equal(s.to_bgr(), full[y0:y1]), (y0, y1)
    # Python slice rules: open ends, negative and out-of-range bounds; a slice of a slice composes
    for sl in (slice(None), slice(3, None), slice(None, 3), slice(-3, None), slice(1, -1), slice(2, 100), slice(-100, 4), slice(5, 2)):
        assert np.array_equal(f[sl].to_bgr(), full[sl]), sl
    assert np.array_equal(f[1:6][2:4].to_bgr(), full[1:6][2:4])
    assert np.array_equal(f[3:][1:][:-1].to_bgr(), full[3:][1:][:-1])
    assert f[1:6][2:4].row_parity == 1 and (f[1:6][2:4].y0, f[1:6][2:4].y1) == (3, 5)
    for bad in (0, -1, (slice(0, 2), slice(0, 2)), slice(0, 6, 2), slice(None, None, -1), Ellipsis, [0, 1], np.arange(2)):
        with pytest.raises(TypeError):
            f[bad]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_packing(built_lib, layout):
    lib = ctypes.CDLL(built_lib)
    lib.vse_yuv420_frame_bytes.restype = ctypes.c_size_t
    lib.vse_yuv420_frame_bytes.argtypes = [ctypes.c_int] * 3
    h, w = 7, 10
    f = make_frame(np.random.default_rng(4), h, w, layout)
    full = yuv_ref.convert(f.planes, layout)
    for y0 in range(h):
        for y1 in range(y0 + 1, h + 1):
            s = f[y0:y1]
            want = lib.vse_yuv420_frame_bytes(y1 - y0, w, y0 & 1)
            assert s.packed_bytes == want == yuv_ref.packed_bytes(y1 - y0, w, y0 & 1), (y0, y1)
            buf = np.full(want + 7, 0xA5, np.uint8)
            assert s.pack_into(buf) == want and np.all(buf[want:] == 0xA5)
            planes = yuv_ref.unpack(buf[:want], y1 - y0, w, layout, y0 & 1)
            assert np.array_equal(yuv_ref.convert(planes, layout, parity=y0 & 1), full[y0:y1]), (y0, y1)
    # what the call refuses has no size
    for args in [(0, 4, 0), (4, 0, 0), (-1, 4, 0), (4, 4, 2), (4, 4, -1), (1 << 16, 1 << 15, 0)]:
        assert lib.vse_yuv420_frame_bytes(*args) == 0, args
    assert lib.vse_yuv420_frame_bytes(1080, 1920, 0) == 1080 * 1920 * 3 // 2 and lib.vse_yuv420_frame_bytes(1, 1, 1) == 3


def test_frame_checks_its_planes():
    y, u, v = yuv_ref.random_planes(np.random.default_rng(5), 4, 6, "i420")
    with pytest.raises(ValueError):
        ingest.Yuv420Frame((y, u[:1], v), 4, 6, "i420")
    with pytest.raises(ValueError):
        ingest.Yuv420Frame((y, u, v), 4, 6, "nv12")
    with pytest.raises(ValueError):
        ingest.Yuv420Frame((y, u, v), 4, 6, "yv12")
    with pytest.raises(ValueError):
        ingest.Yuv420Frame((y, u, v), 4, 6, "i420", 2, 5)


# ---- Y4M -----------------------------------------------------------------------------------------------------------------------
def test_y4m_round_trip(tmp_path):
    rng = np.random.default_rng(6)
    for h, w, fps in [(6, 8, 25.0), (5, 7, 30000 / 1001)]:
        clip = yuv_triples(rng, 4, h, w)
        path = str(tmp_path / f"clip{h}.y4m")
        ingest.write_y4m(path, clip, fps)
        src = ingest.Y4mSource(path)
        assert (src.frame_count, src.width, src.height, src.layout) == (4, w, h, "i420") and abs(src.fps - fps) < 1e-9
        assert src.read(0) is None and src.read(5) is None and src.read_raw(0) is None and src.read_raw(5) is None
        for no, tr in enumerate(clip, 1):
            raw = src.read_raw(no)
            assert isinstance(raw, ingest.Yuv420Frame) and raw.shape == (h, w, 3)
            assert all(np.array_equal(a, b) for a, b in zip(raw.planes, tr))
            assert np.array_equal(src.read(no), bgr_of(tr))
        assert all(np.array_equal(a, bgr_of(tr)) for a, tr in zip(src.frames(), clip))
        assert [r.planes[0].tobytes() for r in src.raw_frames()] == [tr[0].tobytes() for tr in clip]
        assert src.pos_msec(0) == 0.0 and src.pos_msec(3) == pytest.approx(3000.0 / fps) and src.pos_msec(4) is None and src.pos_msec(-1) is None
        src.close()


def y4m_bytes(header, clip, frame_header=b"FRAME\n"):
    return header + b"".join(frame_header + b"".join(p.tobytes() for p in tr) for tr in clip)


def test_y4m_hand_written_header(tmp_path):
    clip = yuv_triples(np.random.default_rng(7), 3, 4, 6)
    path = str(tmp_path / "hand.y4m")
    with open(path, "wb") as fp:
        fp.write(y4m_bytes(b"YUV4MPEG2 W6 H4 F30000:1001 Ip A128:117 C420mpeg2 XYSCSS=420MPEG2 XCOLORRANGE=LIMITED\n", clip, b"FRAME Ip XFOO=1\n"))
    src = ingest.Y4mSource(path)
    assert src.frame_count == 3 and (src.width, src.height) == (6, 4) and src.fps == pytest.approx(30000 / 1001)
    assert all(np.array_equal(src.read(k + 1), bgr_of(clip[k])) for k in range(3))
    assert src.pos_msec(2) == pytest.approx(2 * 1001 / 30.0)
    # no I, no C, no A: accepted; `I?` too
    for head in (b"YUV4MPEG2 W6 H4 F25:1\n", b"YUV4MPEG2 H4 W6 I? F25:1 C420paldv\n", b"YUV4MPEG2 W6 H4 F25:1 C420jpeg\n", b"YUV4MPEG2 W6 H4 F25:1 C420\n"):
        with open(path, "wb") as fp:
            fp.write(y4m_bytes(head, clip))
        src = ingest.Y4mSource(path)
        assert src.frame_count == 3 and src.fps == 25.0 and np.array_equal(src.read(3), bgr_of(clip[2]))


def test_y4m_truncated_last_frame_is_dropped(tmp_path):
    clip = yuv_triples(np.random.default_rng(8), 3, 4, 6)
    data = y4m_bytes(b"YUV4MPEG2 W6 H4 F25:1\n", clip)
    per = 6 + 4 * 6 * 3 // 2
    path = str(tmp_path / "cut.y4m")
    # cut inside the payload, right behind / inside / in front of the frame header, inside the frame before, nowhere
    for cut, frames in [(1, 2), (per - 7, 2), (per - 6, 2), (per - 5, 2), (per - 3, 2), (per, 2), (per + 2, 1), (0, 3)]:
        with open(path, "wb") as fp:
            fp.write(data[:len(data) - cut])
        src = ingest.Y4mSource(path)
        assert src.frame_count == frames, cut
        assert np.array_equal(src.read(frames), bgr_of(clip[frames - 1])) and src.read(frames + 1) is None


def test_y4m_frame_rate(tmp_path):
    clip = yuv_triples(np.random.default_rng(9), 1, 2, 2)
    path = str(tmp_path / "rate.y4m")
    for head in (b"YUV4MPEG2 W2 H2 F0:0\n", b"YUV4MPEG2 W2 H2\n"):
        with open(path, "wb") as fp:
            fp.write(y4m_bytes(head, clip))
        with pytest.raises(ValueError, match="fps"):
            ingest.Y4mSource(path)
        with pytest.raises(ValueError, match="fps"):
            ingest.open_source(path)
        assert ingest.Y4mSource(path, fps=12.5).fps == 12.5 and ingest.open_source(path, fps=12.5).pos_msec(0) == 0.0


@pytest.mark.parametrize("token", ["C422", "C420p10", "It", "XCOLORRANGE=FULL", "C444", "Cmono", "C420p16", "Ib", "Im"])
def test_y4m_refuses_what_it_cannot_convert(tmp_path, token):
    path = str(tmp_path / "bad.y4m")
    with open(path, "wb") as fp:
        fp.write(y4m_bytes(b"YUV4MPEG2 W2 H2 F25:1 " + token.encode() + b"\n", yuv_triples(np.random.default_rng(10), 1, 2, 2)))
    with pytest.raises(ValueError) as e:
        ingest.Y4mSource(path)
    assert token in str(e.value)


def test_y4m_garbage_between_frames_names_the_offset(tmp_path):
    clip = yuv_triples(np.random.default_rng(11), 2, 4, 6)
    head = b"YUV4MPEG2 W6 H4 F25:1\n"
    one = y4m_bytes(b"", clip[:1])
    path = str(tmp_path / "garbage.y4m")
    for junk in (b"junkjunkjunk", b"FRAMEX\n" + b"\0" * 40, b"RIFF"):
        with open(path, "wb") as fp:
            fp.write(head + one + junk + y4m_bytes(b"", clip[1:]))
        with pytest.raises(ValueError) as e:
            ingest.Y4mSource(path)
        assert f"offset {len(head) + len(one)} " in str(e.value), (junk, str(e.value))
    with open(path, "wb") as fp:
        fp.write(b"RIFF....AVI ")
    with pytest.raises(ValueError):
        ingest.Y4mSource(path)


# ---- headerless files and dispatch -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("hw", [(6, 8), (5, 7)])
def test_raw_source_round_trip(tmp_path, layout, hw):
    h, w = hw
    clip = yuv_triples(np.random.default_rng(12), 3, h, w)
    path = str(tmp_path / ("clip." + ("yuv" if layout == "i420" else "nv12")))
    ingest.write_yuv420(path, clip, layout)
    with open(path, "ab") as fp:
        fp.write(b"\x01" * (h * w))                        # a partial fourth frame
    src = ingest.Yuv420Source(path, w, h, 24.0, layout)
    assert (src.frame_count, src.fps, src.layout) == (3, 24.0, layout)
    assert src.read(0) is None and src.read(4) is None and src.pos_msec(3) is None and src.pos_msec(2) == pytest.approx(2000 / 24.0)
    for no, tr in enumerate(clip, 1):
        raw = src.read_raw(no)
        assert raw.layout == layout and raw.shape == (h, w, 3)
        assert all(np.array_equal(a, b) for a, b in zip(yuv_ref.split_chroma(raw.planes, layout), tr))
        assert np.array_equal(src.read(no), bgr_of(tr)) and np.array_equal(raw[1:].to_bgr(), bgr_of(tr)[1:])
    assert len(list(src.frames())) == len(list(src.raw_frames())) == 3
    src.close()


def test_open_source_dispatch(tmp_path):
    clip = yuv_triples(np.random.default_rng(13), 2, 4, 6)
    y4m = str(tmp_path / "a.y4m")
    ingest.write_y4m(y4m, clip, 25)
    s = ingest.open_source(y4m)
    assert isinstance(s, ingest.Y4mSource) and s.frame_count == 2 and s.fps == 25.0
    for ext, layout in [(".yuv", "i420"), (".i420", "i420"), (".nv12", "nv12")]:
        path = str(tmp_path / ("b" + ext))
        ingest.write_yuv420(path, clip, layout)
        s = ingest.open_source(path, fps=30, size=(6, 4))
        assert isinstance(s, ingest.Yuv420Source) and (s.layout, s.width, s.height, s.frame_count, s.fps) == (layout, 6, 4, 2, 30.0)
        assert np.array_equal(s.read(2), bgr_of(clip[1]))
        with pytest.raises(ValueError, match="size"):
            ingest.open_source(path, fps=30)
        with pytest.raises(ValueError, match="fps"):
            ingest.open_source(path, size=(6, 4))
    # the sources there were: unchanged
    frames = [np.full((4, 6, 3), k, np.uint8) for k in range(3)]
    avi, npy = str(tmp_path / "c.avi"), str(tmp_path / "d.npy")
    ingest.write_avi_bgr24(avi, frames, 10)
    np.save(npy, np.stack(frames))
    assert isinstance(ingest.open_source(avi), ingest.AviBgr24Source) and isinstance(ingest.open_source(npy, fps=10), ingest.NpySource)
    with pytest.raises(ValueError, match="fps"):
        ingest.open_source(npy)


def test_bgr_to_yuv420_makes_plausible_planes():
    """Only a test-input generator: grey stays grey, the primaries land near their BT.601 codes, odd sizes give (h + 1) >> 1 chroma rows."""
    grey = np.full((5, 7, 3), 128, np.uint8)
    y, u, v = ingest.bgr_to_yuv420(grey)
    assert y.shape == (5, 7) and u.shape == v.shape == (3, 4) and y.dtype == u.dtype == np.uint8
    assert np.all(y == 126) and np.all(u == 128) and np.all(v == 128)
    back = ingest.Yuv420Frame((y, u, v), 5, 7).to_bgr().astype(int)
    assert np.abs(back - 128).max() <= 1
    red = np.zeros((2, 2, 3), np.uint8)
    red[..., 2] = 255
    assert [int(p[0, 0]) for p in ingest.bgr_to_yuv420(red)] == [81, 90, 240]


# ---- the extractor's host route ---------------------------------------------------------------------------------------------------
def test_run_ocr_tasks_reads_bgr_without_an_uploader(tmp_path):
    """No uploader: run_ocr_tasks reads BGR ndarrays (to_bgr) from a Y4mSource, cropped to the lower half of an odd half (H = 6 -> 3)."""
    clip = yuv_triples(np.random.default_rng(14), 5, 6, 8)
    path = str(tmp_path / "e.y4m")
    ingest.write_y4m(path, clip, 10)
    src = ingest.Y4mSource(path)
    seen = []

    class Ocr:
        def predict(self, frame):
            assert isinstance(frame, np.ndarray) and frame.dtype == np.uint8
            seen.append(np.array(frame))
            return [], []

    tasks = extractor.fps_tasks(src.frame_count, src.fps, 10, extractor.LOWER_PART)
    assert len(tasks) == 5 and extractor.run_ocr_tasks(src, tasks, Ocr(), batch=2) == []
    assert len(seen) == 5
    for no, (got, tr) in enumerate(zip(seen, clip), 1):
        assert got.shape == (3, 8, 3) and np.array_equal(got, bgr_of(tr)[3:])
        assert np.array_equal(got, src.read_raw(no).to_bgr()[3:]) and np.array_equal(got, src.read_raw(no)[3:].to_bgr())
