"""vse_yuv420_to_bgr on the MI355X: every comparison is byte equality with the numpy restatement (tests/yuv_ref.py).  The whole input
domain on the 16-byte kernel, the odd shapes / parities / pitches / byte offsets of the general one, what the call must refuse and
must not write, staging.Uploader over ingest.Yuv420Frames, and SubtitleExtractor over a Y4M file against the same pixels as BGR."""
import ctypes as C

import numpy as np
import pytest

import yuv_ref

pytestmark = pytest.mark.gpu

LAYOUTS = ("i420", "nv12")
FILL = 0xA5


def convert(ctx, packed, n, h, w, layout, parity=0, out=None):
    """packed: host uint8, 1-D (frames back to back) or [n, stride] -> host uint8 [n,h,w,3] from the device."""
    import torch
    dev = torch.from_numpy(np.ascontiguousarray(packed)).to(ctx.tdev)
    got = ctx.yuv420_to_bgr(dev, n, h, w, layout, parity, out=out)
    return got.cpu().numpy()


def reference_in_row_chunks(planes, layout, rows=64):
    """yuv_ref.convert of a large frame, 64 rows at a time (its int64 temporaries, 8 bytes per sample, then stay in the host's cache)."""
    h = planes[0].shape[0]
    return np.concatenate([yuv_ref.convert(planes, layout, rows=(r, min(r + rows, h))) for r in range(0, h, rows)])


# ---- the arithmetic over its whole domain ---------------------------------------------------------------------------------------
def all_luma_around(pairs_u, pairs_v, ch, cw):
    """Chroma planes [ch, cw] in which chroma sample i holds pair i // 64, and the luma plane [2 ch, 2 cw] whose four samples around
    chroma sample i are 4 (i % 64) + (0, 1, 2, 3): every pair meets every Y exactly once."""
    i = np.arange(ch * cw).reshape(ch, cw)
    u, v = pairs_u[i // 64].astype(np.uint8), pairs_v[i // 64].astype(np.uint8)
    y = np.empty((2 * ch, 2 * cw), np.uint8)
    for dy in (0, 1):
        for dx in (0, 1):
            y[dy::2, dx::2] = 4 * (i % 64) + 2 * dy + dx
    return y, u, v


def test_every_input_value_i420(ctx):
    pairs = np.arange(65536)
    y, u, v = all_luma_around(pairs >> 8, pairs & 255, 2048, 2048)
    code = (y.astype(np.int64) << 16) | (np.repeat(np.repeat(u, 2, 0), 2, 1).astype(np.int64) << 8) | np.repeat(np.repeat(v, 2, 0), 2, 1)
    assert np.array_equal(np.bincount(code.reshape(-1), minlength=1 << 24), np.ones(1 << 24, np.int64))      # each (Y, U, V) exactly once
    got = convert(ctx, yuv_ref.pack((y, u, v), "i420"), 1, 4096, 4096, "i420")[0]
    assert np.array_equal(got, reference_in_row_chunks((y, u, v), "i420"))


def test_every_luma_value_nv12(ctx):
    rng = np.random.default_rng(21)
    pairs = rng.choice(65536, size=256 * 2048 // 64, replace=False)
    y, u, v = all_luma_around(pairs >> 8, pairs & 255, 256, 2048)
    planes = (y, np.stack([u, v], axis=2).reshape(256, 4096))
    got = convert(ctx, yuv_ref.pack(planes, "nv12"), 1, 512, 4096, "nv12")[0]
    assert np.array_equal(got, reference_in_row_chunks(planes, "nv12"))


# ---- shapes ------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (2, 2), (3, 5), (5, 1), (2, 16), (2, 32), (16, 64), (17, 64), (16, 72), (6, 1040), (9, 2050)]


@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("hw", SHAPES)
def test_shapes(ctx, hw, layout, parity):
    h, w = hw
    rng = np.random.default_rng(1000 * h + w + parity)
    for mid in (False, True):
        planes = yuv_ref.random_planes(rng, h, w, layout, parity, mid)
        want = yuv_ref.convert(planes, layout, parity=parity)
        if h * w >= 64:                        # the premise of the two fills: uniform bytes clip about 40 % of the channels, mid-range ones almost none
            clipped = np.mean((want == 0) | (want == 255))
            assert clipped < 0.02 if mid else clipped > 0.25, clipped
        packed = yuv_ref.pack(planes, layout)
        assert packed.size == ctx.lib.vse_yuv420_frame_bytes(h, w, parity)
        got = convert(ctx, packed, 1, h, w, layout, parity)
        assert got.shape == (1, h, w, 3) and np.array_equal(got[0], want), (hw, layout, parity, mid)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("hw,pad", [((16, 64), 32), ((16, 64), 33), ((9, 50), 16), ((9, 50), 7)])
def test_batches_with_a_padded_frame_stride(ctx, hw, pad, layout):
    """n = 3, packed frame stride larger than the frame: 16-aligned (the 16-byte kernel where the shape allows) and odd."""
    h, w = hw
    rng = np.random.default_rng(pad)
    frame = yuv_ref.packed_bytes(h, w)
    packed = np.full((3, frame + pad), FILL, np.uint8)
    want = []
    for f in range(3):
        planes = yuv_ref.random_planes(rng, h, w, layout)
        packed[f, :frame] = yuv_ref.pack(planes, layout)
        want.append(yuv_ref.convert(planes, layout))
    assert np.array_equal(convert(ctx, packed, 3, h, w, layout), np.stack(want))


# ---- destination and source views ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("hw", [(16, 64), (7, 10)])
def test_destination_views_keep_their_padding(ctx, hw, layout):
    """Padded pitches (a multiple of 16, and 3 w + 5) at base byte offsets 0, 1, 4, 16 inside a tensor pre-filled with 0xA5: the payload
    equals the reference and every other byte is still 0xA5."""
    import torch
    h, w = hw
    n = 2
    rng = np.random.default_rng(31)
    planes = [yuv_ref.random_planes(rng, h, w, layout) for _ in range(n)]
    want = np.stack([yuv_ref.convert(p, layout) for p in planes])
    packed = torch.from_numpy(np.concatenate([yuv_ref.pack(p, layout) for p in planes])).to(ctx.tdev)
    for pitch in (((3 * w + 15) // 16 + 1) * 16, 3 * w + 5):
        for off in (0, 1, 4, 16):
            fstride = h * pitch + 32
            big = torch.full((off + n * fstride + 64,), FILL, dtype=torch.uint8, device=ctx.tdev)
            view = big.as_strided((n, h, w, 3), (fstride, pitch, 3, 1), off)
            assert ctx.yuv420_to_bgr(packed, n, h, w, layout, out=view) is view
            host = big.cpu().numpy()
            mask = np.zeros(host.size, bool)
            for f in range(n):
                for r in range(h):
                    a = off + f * fstride + r * pitch
                    mask[a:a + 3 * w] = True
                    assert np.array_equal(host[a:a + 3 * w], want[f, r].reshape(-1)), (pitch, off, f, r)
            assert np.all(host[~mask] == FILL), (pitch, off)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("hw", [(16, 64), (7, 10)])
def test_source_byte_offsets(ctx, hw, layout):
    import torch
    h, w = hw
    n = 2
    rng = np.random.default_rng(32)
    planes = [yuv_ref.random_planes(rng, h, w, layout) for _ in range(n)]
    want = np.stack([yuv_ref.convert(p, layout) for p in planes])
    host = np.concatenate([yuv_ref.pack(p, layout) for p in planes])
    for off in (0, 1, 8):
        big = torch.zeros(off + host.size, dtype=torch.uint8, device=ctx.tdev)
        big[off:] = torch.from_numpy(host).to(ctx.tdev)
        out = torch.full((n, h, w, 3), FILL, dtype=torch.uint8, device=ctx.tdev)
        ctx.yuv420_to_bgr(big[off:], n, h, w, layout, out=out)
        assert np.array_equal(out.cpu().numpy(), want), off


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx):
    import torch
    lib = ctx.lib
    h, w, n = 8, 16, 2
    frame = yuv_ref.packed_bytes(h, w)
    src = torch.zeros(4 * frame, dtype=torch.uint8, device=ctx.tdev)
    out = torch.full((4 * h * w * 3,), FILL, dtype=torch.uint8, device=ctx.tdev)
    ok = dict(n=n, h=h, w=w, layout=0, parity=0, sstride=frame, pitch=3 * w, dstride=h * w * 3)
    bad = [dict(h=0), dict(w=0), dict(n=0), dict(h=-1), dict(layout=2), dict(layout=-1), dict(parity=2), dict(parity=-1), dict(pitch=3 * w - 1),
           dict(sstride=frame - 1), dict(dstride=h * w * 3 - 1), dict(pitch=3 * w + 4, dstride=(h - 1) * (3 * w + 4) + 3 * w - 1)]
    for change in bad:
        a = dict(ok, **change)
        rc = lib.vse_yuv420_to_bgr(ctx.handle, C.c_void_p(src.data_ptr()), a["n"], a["h"], a["w"], a["layout"], a["parity"], a["sstride"],
                                   C.c_void_p(out.data_ptr()), a["pitch"], a["dstride"], ctx.stream())
        assert rc == -1, change
        assert "vse_yuv420_to_bgr" in lib.vse_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    # the accepted call next to them does write
    rc = lib.vse_yuv420_to_bgr(ctx.handle, C.c_void_p(src.data_ptr()), n, h, w, 0, 0, frame, C.c_void_p(out.data_ptr()), 3 * w, h * w * 3, ctx.stream())
    assert rc == 0
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    assert np.all(host[:n * h * w * 3].reshape(-1, 3) == [0, 154, 0]) and np.all(host[n * h * w * 3:] == FILL)      # (Y, U, V) = (0, 0, 0)


# ---- staging ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_uploader_stages_yuv_frames(ctx, layout):
    from vse_amd import ingest, staging
    h, w = 46, 70
    rng = np.random.default_rng(41)
    frames = [ingest.Yuv420Frame(yuv_ref.random_planes(rng, h, w, layout), h, w, layout) for _ in range(10)]
    up = staging.Uploader(ctx.tdev, depth=2, ctx=ctx)
    try:
        for rows in (slice(None), slice(23, None), slice(None, 23), slice(11, 40)):
            first, second = [f[rows] for f in frames[:5]], [f[rows] for f in frames[5:]]
            a, b = up.stage(first), up.stage(second)                  # two batches in flight through two slabs
            c = up.stage(first[::-1])                                 # the first slab again
            for staged, batch in ((a, first), (b, second), (c, first[::-1])):
                got = staged.tensor()
                want = np.stack([yuv_ref.convert(f.planes, layout, rows=(f.y0, f.y1)) for f in batch])
                assert got.dtype.is_floating_point is False and tuple(got.shape) == want.shape
                assert np.array_equal(got.cpu().numpy(), want), rows
                assert np.array_equal(want, np.stack([f.to_bgr() for f in batch]))
        with pytest.raises(ValueError):
            up.stage([frames[0][10:20], frames[1][11:21]])             # one shape, two row parities
        with pytest.raises(ValueError):
            up.stage([frames[0][10:20], frames[1][10:22]])
        other = "nv12" if layout == "i420" else "i420"
        with pytest.raises(ValueError):
            up.stage([frames[0], ingest.Yuv420Frame(yuv_ref.random_planes(rng, h, w, other), h, w, other)])
        # BGR batches take the path they took
        bgr = [f.to_bgr() for f in frames[:3]]
        assert np.array_equal(up.stage(bgr).tensor().cpu().numpy(), np.stack(bgr))
    finally:
        up.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_extractor_over_y4m_equals_the_same_pixels_as_bgr(ctx, tmp_path):
    """A synthetic clip written as Y4M: SubtitleExtractor with an Uploader over the Y4mSource (planes uploaded, converted on the device)
    and over an ArraySource of that file's read() frames (the same pixels, converted on the host) gives the same tasks, intervals,
    raw.txt lines and SRT — in fps mode with the lower-half crop and with the subtitle-change selector on a sub-area of odd first row."""
    import torch
    from oracle import net_ref, pipeline_ref as P
    from vse_amd import extractor, frame_select, ingest, pipeline, shim, staging, synth
    pipe = pipeline.OcrPipeline(ctx, net_ref.get_weights("V3_ch_det_fast"), net_ref.get_weights("V4_en_rec_fast"), P.en_charset(),
                                rec_mode="reference")

    class EngineOcr:
        def predict(self, frame):
            b, r = pipe.ocr(torch.from_numpy(np.ascontiguousarray(frame)).cuda()[None])[0]
            return shim.OcrRecogniser.arrange(b, r)

        def predict_batch(self, frames):
            assert torch.is_tensor(frames) and frames.dtype == torch.uint8
            return [shim.OcrRecogniser.arrange(b, r) for b, r in pipe.ocr(frames)]

    h, w = 360, 640
    frames, truth = synth.make_clip([(None, 2), ("the quick brown fox", 7), ("seven wizards quietly box", 6), (None, 2), ("near frozen lakes", 4)],
                                    h, w, seed=6)
    path = str(tmp_path / "clip.y4m")
    ingest.write_y4m(path, [ingest.bgr_to_yuv420(f) for f in frames], 12)
    y4m = ingest.Y4mSource(path)
    assert y4m.frame_count == len(frames) == 21
    arr = extractor.ArraySource([y4m.read(no) for no in range(1, y4m.frame_count + 1)], y4m.fps)
    arr.pos_msec = y4m.pos_msec              # the file's time stamps for both, so the SRTs can be compared as well
    raw_reads = []
    read_raw, raw_frames = y4m.read_raw, y4m.raw_frames
    y4m.read_raw = lambda no: (raw_reads.append(no), read_raw(no))[1]
    y4m.raw_frames = lambda: (raw_reads.append("all"), raw_frames())[1]
    area = extractor.SubtitleArea(ymin=int(0.75 * h) + 1, ymax=h, xmin=0, xmax=w)
    modes = [dict(sub_area=None, mode="fast", extract_frequency=12, default_subtitle_area=extractor.LOWER_PART),
             dict(sub_area=area, mode="auto", frame_selector="change", change_counter=frame_select.EngineCounter(ctx))]
    up = staging.Uploader(ctx.tdev, ctx=ctx)
    try:
        for kw in modes:
            runs = []
            for src in (y4m, arr):
                del raw_reads[:]
                ex = extractor.SubtitleExtractor(src, EngineOcr(), drop_score=0.0, batch=8, uploader=up, **kw)
                tasks = ex.select_tasks()
                text = ex.run()
                runs.append((tasks, ex.intervals, ex.raw_lines, text))
                if src is y4m:
                    assert any(isinstance(no, int) for no in raw_reads) and (("all" in raw_reads) == ("frame_selector" in kw))
            assert runs[0] == runs[1]
            if "frame_selector" in kw:
                assert len(runs[0][1]) == len(runs[0][0]) == len(truth)                 # one interval and one task per subtitle of the clip
            else:
                assert len(runs[0][0]) == 21 and len(runs[0][2]) >= 1 and runs[0][3].count(" --> ") >= 1      # the run did see subtitles
    finally:
        up.close()
        y4m.close()
