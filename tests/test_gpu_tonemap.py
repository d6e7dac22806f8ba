"""vse_yuv_to_bgr_tonemap on the MI355X: every comparison is byte equality with the numpy restatement (tests/tonemap_ref.py).  Every format
family with random tables and a random gamut on the shapes of both kernels, strides / pitches / parities / a misaligned base, a picture
that reads every entry of A and both halves of T, real ToneMaps through Context.yuv_to_bgr, two tables back to back, what the call must
refuse and must not write, staging.Uploader over tone-mapped and interlaced frames, and SubtitleExtractor in one pass over a 10-bit PQ
stream against the SDR clip."""
import ctypes as C

import numpy as np
import pytest

import tonemap_ref as TM
import yuv_format_ref as R
from test_tonemap import Tables, tone_formats
from test_yuv_formats import ident, product_format

pytestmark = pytest.mark.gpu

FILL = 0xA5
SHAPES = [(11, 37), (8, 64)]                                      # (h, w): odd, no multiple of any tile; the 16-byte kernel's where the format has one


def convert(ctx, packed, n, h, w, fmt, tone, parity=0, out=None):
    import torch
    dev = torch.from_numpy(np.ascontiguousarray(packed)).to(ctx.tdev)
    return ctx.yuv_to_bgr(dev, n, h, w, product_format(fmt), parity, out=out, tone=tone).cpu().numpy()


@pytest.mark.parametrize("fmt", tone_formats(), ids=ident)
def test_every_format_bit_for_bit(ctx, fmt):
    rng = np.random.default_rng(sum(fmt) + 1)
    tone = Tables(rng)
    for h, w in SHAPES:
        for parity in range(fmt[1] + 1):
            planes = R.random_planes(rng, h, w, fmt, parity, wild=bool(parity))
            got = convert(ctx, R.pack(planes, fmt), 1, h, w, fmt, tone, parity)
            assert got.shape == (1, h, w, 3) and np.array_equal(got[0], TM.convert(planes, fmt, *tone.tables(), parity=parity)), (h, w, parity)


VIEW_FORMATS = [(1, 1, 1, 10, 0, 2, 0), (1, 1, 2, 10, 1, 2, 0), (1, 0, 1, 8, 0, 0, 1), (0, 0, 1, 12, 0, 1, 1), (0, 0, 0, 10, 0, 0, 0), (1, 1, 2, 8, 0, 1, 0)]


@pytest.mark.parametrize("fmt", VIEW_FORMATS, ids=ident)
def test_views_offsets_and_strides(ctx, fmt):
    """n = 3 behind padded frame strides and a padded pitch at a byte offset inside a tensor filled with 0xA5, the source base offset by 0 or
    1 sample: aligned 64 x 8 takes the 16-byte kernel (2-byte 4:2:0), every other case the general one.  The payload equals the reference
    and every other byte is still 0xA5."""
    import torch
    n, ss = 3, 1 if fmt[3] == 8 else 2
    rng = np.random.default_rng(fmt[3])
    tone = Tables(rng)
    for (h, w), parity in (((8, 64), 0), ((11, 37), fmt[1])):
        frame = R.packed_bytes(h, w, fmt, parity)
        planes = [R.random_planes(rng, h, w, fmt, parity) for _ in range(n)]
        want = np.stack([TM.convert(p, fmt, *tone.tables(), parity=parity) for p in planes])
        for soff, spad, pitch, doff in ((0, 0, 3 * w, 0), (0, 32, ((3 * w + 15) // 16 + 1) * 16, 16), (1, 7, 3 * w + 5, 1)):
            sstride = frame + spad * ss
            host = np.full(soff * ss + n * sstride, FILL, np.uint8)
            for f in range(n):
                a = soff * ss + f * sstride
                host[a:a + frame] = R.pack(planes[f], fmt)
            src = torch.from_numpy(host).to(ctx.tdev)[soff * ss:].as_strided((n, sstride), (sstride, 1))
            fstride = h * pitch + 32
            big = torch.full((doff + n * fstride + 64,), FILL, dtype=torch.uint8, device=ctx.tdev)
            view = big.as_strided((n, h, w, 3), (fstride, pitch, 3, 1), doff)
            assert ctx.yuv_to_bgr(src, n, h, w, product_format(fmt), parity, out=view, tone=tone) is view
            got = big.cpu().numpy()
            mask = np.zeros(got.size, bool)
            for f in range(n):
                for r in range(h):
                    a = doff + f * fstride + r * pitch
                    mask[a:a + 3 * w] = True
                    assert np.array_equal(got[a:a + 3 * w], want[f, r].reshape(-1)), (h, w, soff, pitch, doff, f, r)
            assert np.all(got[~mask] == FILL), (h, w, soff, pitch, doff)


@pytest.mark.parametrize("chroma,msb", [(1, 0), (2, 1)])
def test_many_frames_and_items_per_block(ctx, chroma, msb):
    """More work than one launch has blocks for, so that blocks stride items and frames after staging once: 40 frames of 96 x 256 on the
    16-byte kernel, and the same pictures one sample off their alignment on the general kernel."""
    import torch
    fmt = (1, 1, chroma, 10, msb, 2, 0)
    n, h, w = 40, 96, 256
    rng = np.random.default_rng(chroma)
    tone = Tables(rng)
    frame = R.packed_bytes(h, w, fmt)
    planes = [R.random_planes(rng, h, w, fmt) for _ in range(n)]
    want = np.stack([TM.convert(p, fmt, *tone.tables()) for p in planes])
    host = np.zeros(2 + n * frame, np.uint8)
    for f in range(n):
        host[2 + f * frame:2 + (f + 1) * frame] = R.pack(planes[f], fmt)
    dev = torch.from_numpy(host).to(ctx.tdev)
    aligned = dev[2:].clone()
    assert aligned.data_ptr() % 16 == 0 and dev[2:].data_ptr() % 16 == 2
    for src in (aligned, dev[2:]):
        assert np.array_equal(ctx.yuv_to_bgr(src, n, h, w, product_format(fmt), tone=tone).cpu().numpy(), want)


def coverage_picture():
    """A 4:4:4 10-bit limited-range BT.2020 picture, one row per (U, V) pair and every Y along it, with tables under which the picture
    reads T at 4095, 4096 and 7935 -> (fmt, planes, tone)."""
    fmt = (0, 0, 1, 10, 0, 2, 0)
    pairs = [(512 + k, 512 - k) for k in range(-8, 9)]
    y = np.tile(np.arange(1024), (len(pairs), 1))
    u = np.array([p[0] for p in pairs])[:, None] + 0 * y
    v = np.array([p[1] for p in pairs])[:, None] + 0 * y
    table_a = np.arange(4096, dtype=np.int64) * 16                       # L from 0 to 65520
    table_a[4095] = 65535                                                # P = 65535: T's last entry, 7935
    table_a[256] = 4095                                                  # P = 4095, the last entry of T's exact part
    table_a[257] = 4096                                                  # P = 4096, the first of the coarse part
    table_a = table_a.astype(np.uint16)
    table_t = np.random.default_rng(9).integers(0, 256, size=TM.T_LEN).astype(np.uint8)
    gamut = np.eye(3, dtype=np.int32) * 16384                            # P = L
    tone = type("Coverage", (), {"tables": lambda self: (table_a, table_t, gamut), "packed": lambda self: TM.pack_table(table_a, table_t).tobytes()})()
    return fmt, tuple(p.astype("<u2") for p in (y, u, v)), tone


def test_every_code_and_both_halves_of_t(ctx):
    """Coverage by construction, asserted on the reference side: every E of 0..4095 occurs, T is read at 4095, 4096 and 7935, and both
    branches of its index are taken."""
    fmt, planes, tone = coverage_picture()
    trace = {}
    want = TM.convert(planes, fmt, *tone.tables(), trace=trace)
    assert np.array_equal(trace["E"], np.arange(4096))
    assert {4095, 4096, 7935} <= set(trace["T"].tolist()) and trace["T"].min() < 4095 and 4096 < trace["T"].max()
    h, w = planes[0].shape
    assert np.array_equal(convert(ctx, R.pack(planes, fmt), 1, h, w, fmt, tone)[0], want)


@pytest.mark.parametrize("transfer", ["pq", "hlg"])
@pytest.mark.parametrize("curve", ["knee", "clip"])
def test_real_tone_maps_equal_the_host_route(ctx, transfer, curve):
    from vse_amd import ingest
    tone = ingest.ToneMap(transfer, curve=curve)
    rng = np.random.default_rng(len(transfer) + len(curve))
    for fmt, (h, w) in (((1, 1, 2, 10, 1, 2, 0), (16, 64)), ((1, 1, 1, 10, 0, 2, 0), (9, 21)), ((0, 0, 1, 12, 0, 2, 1), (5, 33))):
        planes = R.random_planes(rng, h, w, fmt)
        frame = ingest.YuvFrame(planes, h, w, product_format(fmt), tone=tone)
        got = convert(ctx, R.pack(planes, fmt), 1, h, w, fmt, tone)[0]
        assert np.array_equal(got, frame.to_bgr()) and np.array_equal(got, TM.convert(planes, fmt, *tone.tables()))
    table, gamut = ctx.tone_table(tone)
    assert ctx.tone_table(ingest.ToneMap(transfer, curve=curve))[0] is table and table.data_ptr() % 16 == 0             # uploaded once
    assert table.cpu().numpy().tobytes() == tone.packed() and list(gamut) == tone.tables()[2].reshape(-1).tolist()


def test_two_tables_back_to_back(ctx):
    """Two launches with different tables on one stream, no synchronisation between them: each gives its own bytes."""
    import torch
    fmt = (1, 1, 1, 10, 0, 2, 0)
    h, w = 32, 128
    rng = np.random.default_rng(12)
    one, two = Tables(rng), Tables(rng)
    planes = R.random_planes(rng, h, w, fmt)
    dev = torch.from_numpy(R.pack(planes, fmt)).to(ctx.tdev)
    ctx.tone_table(one), ctx.tone_table(two)
    torch.cuda.synchronize()
    a = ctx.yuv_to_bgr(dev, 1, h, w, product_format(fmt), tone=one)
    b = ctx.yuv_to_bgr(dev, 1, h, w, product_format(fmt), tone=two)
    c = ctx.yuv_to_bgr(dev, 1, h, w, product_format(fmt), tone=one)
    plain = ctx.yuv_to_bgr(dev, 1, h, w, product_format(fmt))
    assert np.array_equal(a.cpu().numpy()[0], TM.convert(planes, fmt, *one.tables()))
    assert np.array_equal(b.cpu().numpy()[0], TM.convert(planes, fmt, *two.tables()))
    assert torch.equal(a, c) and not torch.equal(a, b)
    assert np.array_equal(plain.cpu().numpy()[0], R.convert(planes, fmt))


def test_refusals_launch_nothing(ctx):
    import torch
    lib = ctx.lib
    assert lib.vse_yuv_tonemap_table_bytes() == TM.TABLE_BYTES == 16128
    h, w, n = 8, 16, 2
    fmt = (1, 1, 1, 10, 0, 1, 0)
    ok = dict(n=n, h=h, w=w, sub_x=1, sub_y=1, chroma=1, depth=10, msb=0, matrix=1, full=0, parity=0, sstride=None, pitch=3 * w, dstride=h * w * 3, off=0,
              table=0, gamut=[16384, 0, 0, 0, 16384, 0, 0, 0, 16384])
    frame = R.packed_bytes(h, w, fmt)
    src = torch.zeros(4 * frame + 16, dtype=torch.uint8, device=ctx.tdev)
    out = torch.full((4 * h * w * 3,), FILL, dtype=torch.uint8, device=ctx.tdev)
    rng = np.random.default_rng(4)
    table_a, table_t, _ = TM.random_tables(rng)
    table = torch.from_numpy(np.concatenate([TM.pack_table(table_a, table_t), np.zeros(16, np.uint8)])).to(ctx.tdev)
    assert table.data_ptr() % 16 == 0

    def call(a):
        gamut = None if a["gamut"] is None else (C.c_int32 * 9)(*a["gamut"])
        tab = None if a["table"] is None else C.c_void_p(table.data_ptr() + a["table"])
        return lib.vse_yuv_to_bgr_tonemap(ctx.handle, C.c_void_p(src.data_ptr() + a["off"]), a["n"], a["h"], a["w"], a["sub_x"], a["sub_y"], a["chroma"],
                                          a["depth"], a["msb"], a["matrix"], a["full"], a["parity"], frame if a["sstride"] is None else a["sstride"],
                                          C.c_void_p(out.data_ptr()), a["pitch"], a["dstride"], tab, gamut, ctx.stream())
    # everything vse_yuv_to_bgr_format refuses (tests/test_gpu_yuv_formats.py's list) ...
    bad = [dict(h=0), dict(w=0), dict(n=0), dict(h=-1), dict(sub_x=0, sub_y=1), dict(sub_x=2), dict(sub_y=-1), dict(chroma=3), dict(chroma=-1),
           dict(chroma=0), dict(chroma=2, sub_y=0), dict(depth=7), dict(depth=17), dict(depth=8, msb=1), dict(msb=2), dict(msb=-1), dict(matrix=3),
           dict(matrix=-1), dict(full=2), dict(full=-1), dict(parity=2), dict(parity=-1), dict(sub_y=0, parity=1), dict(pitch=3 * w - 1),
           dict(sstride=frame - 2), dict(sstride=frame + 1), dict(off=1), dict(dstride=h * w * 3 - 1),
           dict(pitch=3 * w + 4, dstride=(h - 1) * (3 * w + 4) + 3 * w - 1), dict(h=1 << 16, w=1 << 15)]
    # ... and what is its own: the table and the gamut
    bad += [dict(table=None), dict(table=1), dict(table=8), dict(gamut=None), dict(gamut=[32767, 1, 0, 0, 16384, 0, 0, 0, 16384]),
            dict(gamut=[16384, 0, 0, -32768, 32767, -1, 0, 0, 16384]), dict(gamut=[16384, 0, 0, 0, 16384, 0, 20000, 12768, 0]),
            dict(gamut=[2 ** 31 - 1, 2 ** 31 - 1, 0, 0, 16384, 0, 0, 0, 16384])]
    for change in bad:
        assert call(dict(ok, **change)) == -1, change
        msg = lib.vse_last_error().decode()
        assert "vse_yuv_to_bgr_tonemap" in msg and f"depth {dict(ok, **change)['depth']} " in msg and "gamut" in msg, change
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    # the bounds themselves are accepted, and the accepted call does write: all-zero words are (Y, U, V) = (0, 0, 0)
    edge = [32767, 0, -32768, 16384, 16383, -16384, -16384, -16384, 32767]
    assert call(dict(ok, gamut=edge)) == 0
    torch.cuda.synchronize()
    host = out.cpu().numpy()
    want = TM.pixels(0, 0, 0, fmt, table_a, table_t, edge).tolist()
    assert np.all(host[:n * h * w * 3].reshape(-1, 3) == want) and np.all(host[n * h * w * 3:] == FILL)


def test_uploader_stages_tone_mapped_frames(ctx):
    from vse_amd import ingest, staging
    h, w = 46, 70
    rng = np.random.default_rng(44)
    tone, other = ingest.ToneMap("pq"), ingest.ToneMap("pq", curve="clip")
    up = staging.Uploader(ctx.tdev, depth=2, ctx=ctx)
    try:
        for fmt in ((1, 1, 1, 10, 0, 2, 0), (1, 1, 2, 10, 1, 2, 0)):
            pf = product_format(fmt)
            frames = [ingest.YuvFrame(R.random_planes(rng, h, w, fmt), h, w, pf, tone=tone) for _ in range(5)]
            for rows in (slice(None), slice(23, None), slice(11, 40)):
                first, second = [f[rows] for f in frames[:3]], [f[rows] for f in frames[3:]]
                a, b = up.stage(first), up.stage(second)
                for staged, batch in ((a, first), (b, second)):
                    want = np.stack([TM.convert(f.planes, fmt, *tone.tables(), rows=(f.y0, f.y1)) for f in batch])
                    assert np.array_equal(staged.tensor().cpu().numpy(), want), rows
                    assert np.array_equal(want, np.stack([f.to_bgr() for f in batch]))
            with pytest.raises(ValueError, match="tone"):
                up.stage([frames[0], ingest.YuvFrame(frames[1].planes, h, w, pf, tone=other)])
            with pytest.raises(ValueError, match="tone"):
                up.stage([frames[0], ingest.YuvFrame(frames[1].planes, h, w, pf)])
        # interlaced + tone: deinterlaced on the device, then tone-mapped, equal to the numpy path
        fmt = (1, 1, 1, 10, 0, 2, 0)
        pf = product_format(fmt)
        pics = [R.random_planes(rng, h, w, fmt) for _ in range(4)]
        woven = [ingest.InterlacedYuvFrame(p, h, w, pf, pics[k - 1] if k else None, "tff", "adaptive", 10, tone=tone) for k, p in enumerate(pics)]
        for rows in (slice(None), slice(11, 40)):
            batch = [f[rows] for f in woven]
            got = up.stage(batch).tensor().cpu().numpy()
            assert np.array_equal(got, np.stack([f.to_bgr() for f in batch]))
            assert np.array_equal(got, np.stack([TM.convert(f.deinterlaced_planes(), fmt, *tone.tables())[f.y0:f.y1] for f in batch]))
        with pytest.raises(ValueError, match="tone"):
            up.stage([woven[1], ingest.InterlacedYuvFrame(pics[2], h, w, pf, pics[1], "tff", "adaptive", 10)])
    finally:
        up.close()


def test_one_pass_over_a_pq_stream_gives_the_sdr_clips_intervals(ctx, tmp_path):
    """A synthetic clip graded as 10-bit 4:2:0 PQ BT.2020, piped as Y4M and read once by SubtitleExtractor with transfer="pq" (tone-mapped
    on the device through the Uploader), against the SDR clip itself: the same intervals, which are the clip's truth."""
    import torch
    from oracle import net_ref, pipeline_ref as P
    from test_one_pass import FPS, piped
    from test_yuv_formats import E2E_AREA
    from vse_amd import extractor, frame_select, ingest, pipeline, shim, staging, synth
    pipe = pipeline.OcrPipeline(ctx, net_ref.get_weights("V3_ch_det_fast"), net_ref.get_weights("V4_en_rec_fast"), P.en_charset(),
                                rec_mode="reference")

    class EngineOcr:
        def predict(self, frame):
            b, r = pipe.ocr(torch.from_numpy(np.ascontiguousarray(frame)).cuda()[None])[0]
            return shim.OcrRecogniser.arrange(b, r)

        def predict_batch(self, frames):
            dev = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames)).to(ctx.tdev)
            return [shim.OcrRecogniser.arrange(b, r) for b, r in pipe.ocr(dev)]

    frames, truth = synth.make_clip([(None, 2), ("the quick brown fox", 7), ("seven wizards quietly box", 6), (None, 2), ("near frozen lakes", 4)],
                                    360, 640, seed=6)
    path = str(tmp_path / "pq.y4m")
    ingest.write_yuv(path, synth.hdr_grade(frames, depth=10, sub=(1, 1)), ingest.YuvFormat(depth=10), fps=FPS, y4m=True)
    with open(path, "rb") as fp:
        data = fp.read()
    up = staging.Uploader(ctx.tdev, ctx=ctx)
    runs = []
    try:
        fp, th = piped(data, 1 << 16)
        sources = (ingest.Y4mStream(fp, wide=True, matrix="bt2020", transfer="pq"), extractor.ArraySource(list(frames), FPS))
        assert sources[0].tone == ingest.ToneMap("pq")
        for src in sources:
            ex = extractor.SubtitleExtractor(src, EngineOcr(), sub_area=E2E_AREA, mode="auto", drop_score=0.0, batch=8, uploader=up,
                                             frame_selector="change", change_counter=frame_select.EngineCounter(ctx), one_pass=True)
            ex.run()
            runs.append([(s, e) for s, e, _r in ex.intervals])
        th.join()
        fp.close()
    finally:
        up.close()
    assert runs[0] == runs[1] == [(s, e) for s, e, _t in truth]
