"""vse_yuv_to_bgr_format on the MI355X: every comparison is byte equality with the numpy restatement (tests/yuv_format_ref.py).  Every
format on the shapes of the 16-byte kernel and of the general one, views / offsets / strides / parities, the exhaustive 10-bit planes, the
8-bit 4:2:0 route against vse_yuv_to_bgr_matrix, what the call must refuse and must not write, staging.Uploader over ingest.YuvFrames,
and SubtitleExtractor in one pass over a 10-bit Y4M stream against the 8-bit clip."""
import ctypes as C
import itertools

import numpy as np
import pytest

import yuv_format_ref as R
from test_yuv_formats import exhaustive_10_bit, ident, product_format

pytestmark = pytest.mark.gpu

FILL = 0xA5
FAST_SHAPES = [(2, 16), (6, 48)]                                  # 16-byte aligned bases and strides: the 16-byte kernel where the format has one
GENERAL_SHAPES = [(1, 1), (2, 2), (3, 5), (5, 17), (6, 34)]


def layouts(depths=(8, 10, 12, 16)):
    """(sub_x, sub_y, chroma, depth, msb): every load pattern."""
    out = []
    for depth in depths:
        for msb in ((0,) if depth == 8 else (0, 1)):
            out += [(0, 0, 0, depth, msb), (0, 0, 1, depth, msb), (1, 0, 1, depth, msb), (1, 1, 1, depth, msb), (1, 1, 2, depth, msb)]
    return out


def convert(ctx, packed, n, h, w, fmt, parity=0, out=None):
    """packed: host uint8, 1-D (frames back to back) or [n, stride] -> host uint8 [n,h,w,3] from the device."""
    import torch
    dev = torch.from_numpy(np.ascontiguousarray(packed)).to(ctx.tdev)
    return ctx.yuv_to_bgr(dev, n, h, w, product_format(fmt), parity, out=out).cpu().numpy()


# ---- every format ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", layouts(), ids=ident)
def test_every_format_bit_for_bit(ctx, layout):
    """The three matrices and both ranges of one load pattern on the fast-path shapes and the general-path shapes (row parity 1 where
    the format has one); 2-byte low-bit formats also with words above 2**depth - 1."""
    rng = np.random.default_rng(sum(layout))
    for matrix, full in itertools.product((0, 1, 2), (0, 1)):
        fmt = layout + (matrix, full)
        for h, w in FAST_SHAPES + GENERAL_SHAPES:
            for parity in range(fmt[1] + 1):
                planes = R.random_planes(rng, h, w, fmt, parity, wild=bool((h + matrix) & 1))
                packed = R.pack(planes, fmt)
                assert packed.size == R.packed_bytes(h, w, fmt, parity) == ctx.lib.vse_yuv_frame_bytes(h, w, *fmt[:4], parity)
                got = convert(ctx, packed, 1, h, w, fmt, parity)
                assert got.shape == (1, h, w, 3) and np.array_equal(got[0], R.convert(planes, fmt, parity=parity)), (fmt, h, w, parity)


VIEW_FORMATS = [(1, 1, 1, 10, 0, 1, 0), (1, 1, 2, 10, 1, 2, 0), (1, 0, 1, 8, 0, 0, 1), (0, 0, 1, 12, 0, 1, 1), (0, 0, 0, 10, 0, 0, 0), (1, 1, 2, 8, 0, 2, 1)]


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("fmt", VIEW_FORMATS, ids=ident)
def test_views_offsets_and_strides(ctx, fmt, n):
    """A padded output pitch at a byte offset inside a tensor filled with 0xA5, a source base offset by 0 to 3 samples, padded frame
    strides (16-aligned and not): the payload equals the reference and every other byte is still 0xA5."""
    import torch
    ss = 1 if fmt[3] == 8 else 2
    rng = np.random.default_rng(n)
    for (h, w), parity in (((6, 48), 0), ((5, 17), fmt[1])):
        frame = R.packed_bytes(h, w, fmt, parity)
        planes = [R.random_planes(rng, h, w, fmt, parity) for _ in range(n)]
        want = np.stack([R.convert(p, fmt, parity=parity) for p in planes])
        for soff, spad, pitch, doff in ((0, 0, 3 * w, 0), (0, 32, ((3 * w + 15) // 16 + 1) * 16, 16), (1, 6, 3 * w + 5, 1), (2, 2, 3 * w, 4), (3, 34, 3 * w + 16, 3)):
            sstride = frame + spad * ss
            host = np.full(soff * ss + n * sstride, FILL, np.uint8)
            for f in range(n):
                a = soff * ss + f * sstride
                host[a:a + frame] = R.pack(planes[f], fmt)
            src = torch.from_numpy(host).to(ctx.tdev)[soff * ss:].as_strided((n, sstride), (sstride, 1))
            fstride = h * pitch + 32
            big = torch.full((doff + n * fstride + 64,), FILL, dtype=torch.uint8, device=ctx.tdev)
            view = big.as_strided((n, h, w, 3), (fstride, pitch, 3, 1), doff)
            assert ctx.yuv_to_bgr(src, n, h, w, product_format(fmt), parity, out=view) is view
            got = big.cpu().numpy()
            mask = np.zeros(got.size, bool)
            for f in range(n):
                for r in range(h):
                    a = doff + f * fstride + r * pitch
                    mask[a:a + 3 * w] = True
                    assert np.array_equal(got[a:a + 3 * w], want[f, r].reshape(-1)), (h, w, soff, pitch, doff, f, r)
            assert np.all(got[~mask] == FILL), (h, w, soff, pitch, doff)


# ---- the arithmetic over its 10-bit domain ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix,full", [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)])
def test_every_10_bit_pair_444(ctx, matrix, full):
    """4:4:4 10-bit, the general kernel: every (Y, U) for B on the left 1024 x 1024, every (Y, V) for R on the right."""
    planes, fmt = exhaustive_10_bit(matrix, full)
    got = convert(ctx, R.pack(planes, fmt), 1, 1024, 2048, fmt)[0]
    assert np.array_equal(got, R.convert(planes, fmt))


@pytest.mark.parametrize("chroma,msb,matrix,full", [(1, 0, 1, 0), (2, 1, 2, 0), (1, 0, 0, 1), (2, 1, 1, 1)])
def test_every_10_bit_pair_420_fast(ctx, chroma, msb, matrix, full):
    """4:2:0 10-bit on the 16-byte kernel, planar (low bits) and P010 (high bits, random low bits): chroma sample (i, j) holds U = j and
    V = (i + j) % 1024 under luma i, so every (Y, U) and every (Y, V) occurs."""
    fmt = (1, 1, chroma, 10, msb, matrix, full)
    i, j = np.meshgrid(np.arange(1024), np.arange(1024), indexing="ij")
    y = np.repeat(np.repeat(i, 2, 0), 2, 1)
    u, v = j, (i + j) % 1024
    assert np.unique(i * 1024 + u).size == np.unique(i * 1024 + v).size == 1 << 20
    if msb:
        rng = np.random.default_rng(chroma)
        y, u, v = ((a << 6) | rng.integers(0, 64, size=a.shape) for a in (y, u, v))
    planes = (y.astype("<u2"), u.astype("<u2"), v.astype("<u2")) if chroma == 1 else \
        (y.astype("<u2"), np.stack([u, v], axis=2).reshape(1024, 2048).astype("<u2"))
    got = convert(ctx, R.pack(planes, fmt), 1, 2048, 2048, fmt)[0]
    want = np.concatenate([R.convert(planes, fmt, rows=(r, r + 256)) for r in range(0, 2048, 256)])
    assert np.array_equal(got, want)


# ---- 8-bit 4:2:0 keeps its kernels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chroma", [1, 2])
@pytest.mark.parametrize("matrix", [0, 1])
def test_8_bit_420_equals_the_matrix_entry(ctx, chroma, matrix):
    import torch
    layout = ("i420", "nv12")[chroma - 1]
    fmt = (1, 1, chroma, 8, 0, matrix, 0)
    rng = np.random.default_rng(chroma + 2 * matrix)
    for (h, w), parity in (((16, 64), 0), ((7, 10), 0), ((7, 10), 1)):
        packed = torch.from_numpy(np.stack([R.pack(R.random_planes(rng, h, w, fmt, parity), fmt) for _ in range(2)])).to(ctx.tdev)
        old = ctx.yuv420_to_bgr(packed, 2, h, w, layout, parity, matrix=matrix)
        new = ctx.yuv_to_bgr(packed, 2, h, w, product_format(fmt), parity)
        assert torch.equal(old, new)
        assert np.array_equal(new.cpu().numpy(), np.stack([R.convert(R.unpack(p, h, w, fmt, parity), fmt, parity=parity) for p in packed.cpu().numpy()]))


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx):
    import torch
    lib = ctx.lib
    h, w, n = 8, 16, 2
    ok = dict(n=n, h=h, w=w, sub_x=1, sub_y=1, chroma=1, depth=10, msb=0, matrix=1, full=0, parity=0, sstride=None, pitch=3 * w, dstride=h * w * 3, off=0)
    frame = R.packed_bytes(h, w, (1, 1, 1, 10, 0, 1, 0))
    src = torch.zeros(4 * frame + 16, dtype=torch.uint8, device=ctx.tdev)
    out = torch.full((4 * h * w * 3,), FILL, dtype=torch.uint8, device=ctx.tdev)

    def call(a):
        return lib.vse_yuv_to_bgr_format(ctx.handle, C.c_void_p(src.data_ptr() + a["off"]), a["n"], a["h"], a["w"], a["sub_x"], a["sub_y"], a["chroma"],
                                         a["depth"], a["msb"], a["matrix"], a["full"], a["parity"], frame if a["sstride"] is None else a["sstride"],
                                         C.c_void_p(out.data_ptr()), a["pitch"], a["dstride"], ctx.stream())
    bad = [dict(h=0), dict(w=0), dict(n=0), dict(h=-1), dict(sub_x=0, sub_y=1), dict(sub_x=2), dict(sub_y=-1), dict(chroma=3), dict(chroma=-1),
           dict(chroma=0), dict(chroma=2, sub_y=0), dict(depth=7), dict(depth=17), dict(depth=8, msb=1), dict(msb=2), dict(msb=-1), dict(matrix=3),
           dict(matrix=-1), dict(full=2), dict(full=-1), dict(parity=2), dict(parity=-1), dict(sub_y=0, parity=1), dict(pitch=3 * w - 1),
           dict(sstride=frame - 2), dict(sstride=frame + 1), dict(off=1), dict(dstride=h * w * 3 - 1),
           dict(pitch=3 * w + 4, dstride=(h - 1) * (3 * w + 4) + 3 * w - 1), dict(h=1 << 16, w=1 << 15)]
    for change in bad:
        assert call(dict(ok, **change)) == -1, change
        msg = lib.vse_last_error().decode()
        assert "vse_yuv_to_bgr_format" in msg and f"depth {dict(ok, **change)['depth']} " in msg, change
        assert lib.vse_yuv_frame_bytes(0, w, 1, 1, 1, 10, 0) == 0
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    # the accepted call next to them does write: all-zero words are (Y, U, V) = (0, 0, 0)
    assert call(ok) == 0
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    want = R.pixels(0, 0, 0, (1, 1, 1, 10, 0, 1, 0)).tolist()
    assert np.all(host[:n * h * w * 3].reshape(-1, 3) == want) and np.all(host[n * h * w * 3:] == FILL)


# ---- staging ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [(1, 1, 1, 10, 0, 1, 0), (1, 0, 1, 8, 0, 0, 0), (1, 0, 1, 10, 0, 2, 1), (1, 1, 2, 10, 1, 1, 0)], ids=ident)
def test_uploader_stages_yuv_frames(ctx, fmt):
    from vse_amd import ingest, staging
    h, w = 46, 70
    rng = np.random.default_rng(41)
    pf = product_format(fmt)
    frames = [ingest.YuvFrame(R.random_planes(rng, h, w, fmt), h, w, pf) for _ in range(6)]
    up = staging.Uploader(ctx.tdev, depth=2, ctx=ctx)
    try:
        for rows in (slice(None), slice(23, None), slice(None, 23), slice(11, 40)):
            first, second = [f[rows] for f in frames[:3]], [f[rows] for f in frames[3:]]
            a, b = up.stage(first), up.stage(second)                  # two batches in flight through two slabs
            c = up.stage(first[::-1])                                 # the first slab again
            for staged, batch in ((a, first), (b, second), (c, first[::-1])):
                got = staged.tensor()
                want = np.stack([f.to_bgr() for f in batch])
                assert tuple(got.shape) == want.shape and np.array_equal(got.cpu().numpy(), want), rows
                assert np.array_equal(want, np.stack([R.convert(f.planes, fmt, rows=(f.y0, f.y1)) for f in batch]))
        with pytest.raises(ValueError):
            up.stage([frames[0][10:20], frames[1][10:22]])
        if fmt[1]:
            with pytest.raises(ValueError):
                up.stage([frames[0][10:20], frames[1][11:21]])             # one shape, two row parities
        other = product_format(fmt[:5] + ((fmt[5] + 1) % 3, fmt[6]))
        with pytest.raises(ValueError):
            up.stage([frames[0], ingest.YuvFrame(frames[1].planes, h, w, other)])
    finally:
        up.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_one_pass_over_a_10_bit_stream_equals_the_8_bit_clip(ctx, tmp_path):
    """A synthetic clip as 8-bit 4:2:0 Y4M and as 10-bit 4:2:0 Y4M (the same samples << 2), each read once as a stream by SubtitleExtractor
    with the change selector: the same intervals and the same frames recognised.  (The converted bytes may differ by one level at rounding
    ties; tests/test_yuv_formats.py::test_10_bit_clip_keeps_its_intervals holds on the CPU that this clip's intervals do not depend on it.)"""
    import torch
    from oracle import net_ref, pipeline_ref as P
    from test_yuv_formats import E2E_AREA, e2e_clips
    from vse_amd import extractor, frame_select, ingest, pipeline, shim, staging
    pipe = pipeline.OcrPipeline(ctx, net_ref.get_weights("V3_ch_det_fast"), net_ref.get_weights("V4_en_rec_fast"), P.en_charset(),
                                rec_mode="reference")

    class EngineOcr:
        def predict(self, frame):
            b, r = pipe.ocr(torch.from_numpy(np.ascontiguousarray(frame)).cuda()[None])[0]
            return shim.OcrRecogniser.arrange(b, r)

        def predict_batch(self, frames):
            assert torch.is_tensor(frames) and frames.dtype == torch.uint8
            return [shim.OcrRecogniser.arrange(b, r) for b, r in pipe.ocr(frames)]

    path8, path10, truth = e2e_clips(tmp_path)
    up = staging.Uploader(ctx.tdev, ctx=ctx)
    runs = []
    try:
        for path, wide in ((path8, False), (path10, True)):
            with open(path, "rb") as fp:
                src = ingest.Y4mStream(fp, wide=wide)
                assert (src.fmt is not None and src.fmt.depth == 10) == wide
                ex = extractor.SubtitleExtractor(src, EngineOcr(), sub_area=E2E_AREA, mode="auto", drop_score=0.0, batch=8, uploader=up,
                                                 frame_selector="change", change_counter=frame_select.EngineCounter(ctx))
                assert ex.one_pass
                ex.run()
                runs.append(ex.intervals)
    finally:
        up.close()
    assert runs[0] == runs[1] and [(s, e) for s, e, _r in runs[0]] == [(s, e) for s, e, _t in truth]
