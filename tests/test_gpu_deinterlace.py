"""vse_yuv_deinterlace on the MI355X: every comparison is byte equality with the int64 restatement of the rule (tests/deinterlace_ref.py),
inside buffers filled with 0xA5 so that a byte written outside a picture shows.  The 16-byte kernel's shapes and the general kernel's, for
1- and 2-byte samples and every plane layout; chained, NULL, pair-strided, padded and byte-offset calls; what the call must refuse;
staging.Uploader over ingest.InterlacedYuvFrames; and SubtitleExtractor over an interlaced Y4M, staged against the host route."""
import ctypes as C
import hashlib
import itertools

import numpy as np
import pytest

import deinterlace_ref as D
import yuv_format_ref as R
from test_yuv_formats import ident, product_format

pytestmark = pytest.mark.gpu

FILL = 0xA5
FAST_SHAPES = [(4, 32), (10, 64)]                    # 16-byte aligned row bytes of every plane of the 1-byte 4:2:0 and wider formats
FAST_SHAPES_2 = [(4, 16), (6, 48)]                   # ... of the 2-byte formats
GENERAL_SHAPES = [(1, 1), (2, 2), (3, 5), (5, 17), (7, 34)]
FORMATS = [(1, 1, 1, 8, 0, 0, 0), (1, 1, 2, 8, 0, 1, 0), (1, 0, 1, 8, 0, 0, 0), (0, 0, 0, 8, 0, 0, 0), (1, 1, 1, 10, 0, 1, 0), (1, 1, 2, 10, 1, 2, 0),
           (0, 0, 1, 16, 0, 0, 0), (1, 0, 1, 12, 1, 1, 0)]
# (name, n, layout, stride padding in samples, base offset in samples)
VARIANTS = [("chained", 1, "chain", 0, 0), ("chained", 3, "chain", 0, 0), ("null", 3, "null", 0, 0), ("pairs", 3, "pairs", 0, 0),
            ("padded 16", 3, "chain", 16, 0), ("padded odd", 3, "pairs", 3, 0), ("base + 1", 3, "chain", 0, 1), ("base + 2", 1, "pairs", 5, 2)]


def run_variant(ctx, rng, fmt, h, w, variant, keep, mode, thresh=10):
    """One call on pictures laid out as `variant` says -> the interpolated / woven sample counts of the reference."""
    import torch
    _name, n, layout, pad, off = variant
    ss = 1 if fmt[3] == 8 else 2
    frame = R.packed_bytes(h, w, fmt)
    stride = frame + pad * ss
    # the pictures: chain P C0 C1 ...: each the previous one + d; pairs P0 C0 P1 C1 ...; null C0 C1 ...
    if layout == "chain":
        pics = [R.random_planes(rng, h, w, fmt)]
        for _ in range(n):
            pics.append(D.near_threshold_prev(rng, pics[-1], fmt, thresh))
        cur, prev, slots, step, first = pics[1:], pics[:-1], pics, 1, 1
    elif layout == "pairs":
        cur = [R.random_planes(rng, h, w, fmt) for _ in range(n)]
        prev = [D.near_threshold_prev(rng, c, fmt, thresh) for c in cur]
        slots, step, first = [p for pair in zip(prev, cur) for p in pair], 2, 1
    else:
        cur = [R.random_planes(rng, h, w, fmt) for _ in range(n)]
        prev, slots, step, first = [None] * n, cur, 1, 0
    base = off * ss
    host = np.full(base + (len(slots) + 1) * stride, FILL, np.uint8)
    for k, p in enumerate(slots):
        host[base + k * stride:base + k * stride + frame] = R.pack(p, fmt)
    src = torch.from_numpy(host).to(ctx.tdev)
    packed = src[base + first * stride:].as_strided((n, step * stride), (step * stride, 1))
    ostride = frame + (pad + (16 if pad % 16 == 0 else 1)) * ss                     # its own padding: 16-byte aligned where the input's is
    obase = 16 + base
    big = torch.full((obase + (n + 1) * ostride,), FILL, dtype=torch.uint8, device=ctx.tdev)
    out = big[obase:].as_strided((n, ostride), (ostride, 1))
    got = ctx.yuv_deinterlace(packed, n, h, w, product_format(fmt), prev=None if layout == "null" else src[base + (first - 1) * stride:],
                              prev_stride=step * stride, keep=keep, mode=mode, thresh=thresh, out=out)
    assert got is out
    want = np.full(big.numel(), FILL, np.uint8)
    inter = woven = 0
    for f in range(n):
        want[obase + f * ostride:obase + f * ostride + frame] = R.pack(D.picture(cur[f], prev[f], fmt, keep, mode, thresh), fmt)
        a, b = D.shares(cur[f], prev[f], fmt, keep, mode, thresh)
        inter, woven = inter + a, woven + b
    assert np.array_equal(big.cpu().numpy(), want), (fmt, h, w, variant, keep, mode)
    assert np.array_equal(src.cpu().numpy(), host)                                   # the inputs are read only
    return inter, woven


@pytest.mark.parametrize("fmt", FORMATS, ids=ident)
def test_bit_for_bit_with_sentinels(ctx, fmt):
    rng = np.random.default_rng(sum(fmt) + 1)
    ss = 1 if fmt[3] == 8 else 2
    combos = [(0, 0), (1, 0), (1, 1), (0, 1)]
    for (h, w), variant in itertools.product(FAST_SHAPES + FAST_SHAPES_2 + GENERAL_SHAPES, VARIANTS):
        if variant[0] == "base + 1" and ss == 2:
            continue                                                 # 2-byte samples at an odd base are refused (test_refusals_launch_nothing)
        for keep, mode in (combos if variant[1] == 3 and variant[2] == "chain" and variant[3] == 0 else combos[:2]):
            inter, woven = run_variant(ctx, rng, fmt, h, w, variant, keep, mode)
            if mode == 0 and variant[2] != "null" and h * w >= 64:
                # both branches are exercised: by the reference, each takes 25 to 75 % of the other field's samples
                assert 0.25 <= inter / (inter + woven) <= 0.75, (fmt, h, w, variant, inter, woven)
            elif (mode == 1 or variant[2] == "null") and h > 1:
                assert woven == 0 and inter > 0                      # no picture is compared: everything is interpolated


def test_small_planes_and_a_base_two_bytes_in(ctx):
    """Two frames each: 10-bit semi-planar high-bit words, 5 x 8, from a base 2 bytes into the buffer (one sample: the planes' offsets
    keep that shift); grey, one plane, 3 x 5 and a single row."""
    rng = np.random.default_rng(58)
    for fmt, h, w, variant in (((1, 1, 2, 10, 1, 2, 0), 5, 8, ("base + 2 bytes", 2, "chain", 0, 1)), ((0, 0, 0, 8, 0, 0, 0), 3, 5, ("chained", 2, "chain", 0, 0)),
                               ((0, 0, 0, 8, 0, 0, 0), 1, 5, ("chained", 2, "chain", 0, 0))):
        for keep, mode in ((0, 0), (1, 0), (1, 1)):
            run_variant(ctx, rng, fmt, h, w, variant, keep, mode)


def test_random_words_and_every_threshold_edge(ctx):
    """Unrelated random pictures (nearly everything moved), identical ones (nothing moved), and thresholds 0 and 255."""
    import torch
    rng = np.random.default_rng(77)
    for fmt, (h, w) in (((1, 1, 1, 8, 0, 0, 0), (10, 64)), ((1, 1, 2, 16, 1, 0, 0), (6, 48)), ((0, 0, 1, 8, 0, 0, 0), (7, 34)), ((1, 0, 1, 10, 0, 0, 0), (5, 17))):
        frame = R.packed_bytes(h, w, fmt)
        cur = R.random_planes(rng, h, w, fmt)
        for prev, thresh in ((R.random_planes(rng, h, w, fmt), 10), (cur, 0), (D.near_threshold_prev(rng, cur, fmt, 255), 255),
                             (D.near_threshold_prev(rng, cur, fmt, 1), 0), (R.random_planes(rng, h, w, fmt), 255)):
            both = torch.from_numpy(np.concatenate([R.pack(prev, fmt), R.pack(cur, fmt)])).to(ctx.tdev)
            for keep in (0, 1):
                got = ctx.yuv_deinterlace(both[frame:], 1, h, w, product_format(fmt), prev=both, keep=keep, thresh=thresh)
                assert np.array_equal(got.cpu().numpy()[0, :frame], R.pack(D.picture(cur, prev, fmt, keep, 0, thresh), fmt)), (fmt, thresh, keep)


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx):
    import torch
    lib = ctx.lib
    h, w, n = 8, 16, 2
    fmt = (1, 1, 1, 10, 0, 1, 0)
    frame = R.packed_bytes(h, w, fmt)
    ok = dict(n=n, h=h, w=w, sub_x=1, sub_y=1, chroma=1, depth=10, msb=0, keep=0, mode=0, thresh=10, sstride=frame, pstride=frame, ostride=frame,
              soff=frame, poff=0, ooff=0, prev=True, out=None)
    src = torch.zeros(4 * frame + 16, dtype=torch.uint8, device=ctx.tdev)
    out = torch.full((4 * frame,), FILL, dtype=torch.uint8, device=ctx.tdev)

    def call(a):
        d_out = out.data_ptr() + a["ooff"] if a["out"] is None else src.data_ptr() + a["out"]
        return lib.vse_yuv_deinterlace(ctx.handle, C.c_void_p(src.data_ptr() + a["soff"]), C.c_void_p(src.data_ptr() + a["poff"]) if a["prev"] else None,
                                       a["n"], a["h"], a["w"], a["sub_x"], a["sub_y"], a["chroma"], a["depth"], a["msb"], a["keep"], a["mode"],
                                       a["thresh"], a["sstride"], a["pstride"], C.c_void_p(d_out), a["ostride"], ctx.stream())
    bad = [dict(h=0), dict(w=0), dict(n=0), dict(h=-1), dict(n=-1), dict(sub_x=0, sub_y=1), dict(sub_x=2), dict(sub_y=-1), dict(chroma=3), dict(chroma=-1),
           dict(chroma=0), dict(chroma=2, sub_y=0), dict(depth=7), dict(depth=17), dict(depth=8, msb=1), dict(msb=2), dict(msb=-1), dict(keep=2),
           dict(keep=-1), dict(mode=2), dict(mode=-1), dict(thresh=-1), dict(thresh=256), dict(sstride=frame - 2), dict(pstride=frame - 2),
           dict(ostride=frame - 2), dict(sstride=frame + 1), dict(pstride=frame + 1), dict(ostride=frame + 1), dict(soff=frame + 1), dict(poff=1),
           dict(ooff=1), dict(out=frame), dict(out=0), dict(h=1 << 16, w=1 << 15)]
    for change in bad:
        assert call(dict(ok, **change)) == -1, change
        msg = lib.vse_last_error().decode()
        assert "vse_yuv_deinterlace" in msg and f"depth {dict(ok, **change)['depth']} " in msg, change
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((src == 0).all())
    # the accepted calls next to them do write: all-zero pictures stay all zero, and only the packed bytes are written
    for more in (dict(), dict(prev=False, pstride=0), dict(mode=1, pstride=frame + 16)):
        out.fill_(FILL)
        assert call(dict(ok, **more)) == 0, more
        torch.cuda.synchronize()
        host = out.cpu().numpy()
        assert np.all(host[:n * frame] == 0) and np.all(host[n * frame:] == FILL)


# ---- staging ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [(1, 1, 1, 8, 0, 0, 0), (1, 1, 1, 10, 0, 1, 0), (1, 0, 1, 8, 0, 0, 1), (1, 1, 2, 10, 1, 1, 0)], ids=ident)
def test_uploader_stages_interlaced_frames(ctx, fmt):
    from vse_amd import ingest, staging
    h, w = 46, 70
    rng = np.random.default_rng(43)
    pf = product_format(fmt)
    pics = [R.random_planes(rng, h, w, fmt)]
    for _ in range(6):
        pics.append(D.near_threshold_prev(rng, pics[-1], fmt))
    frames = [ingest.InterlacedYuvFrame(p, h, w, pf, pics[k - 1] if k else None, "bff" if fmt[2] == 2 else "tff") for k, p in enumerate(pics)]
    keep = frames[0].keep
    whole = [R.convert(D.picture(f.planes, f.prev, fmt, keep), fmt) for f in frames]              # the reference, once
    for f, ref in zip(frames, whole):
        assert np.array_equal(f.to_bgr(), ref)
    index = {id(f.planes): k for k, f in enumerate(frames)}
    up = staging.Uploader(ctx.tdev, depth=2, ctx=ctx)
    try:
        for rows in (slice(None), slice(23, None), slice(None, 23), slice(11, 40), slice(12, 13)):
            chain, second = [f[rows] for f in frames[1:4]], [f[rows] for f in frames[4:]]
            headed = [f[rows] for f in frames[:3]]                    # its first frame has no previous picture
            a, b = up.stage(chain), up.stage(second)                  # two batches in flight through two slabs
            c = up.stage(chain[::-1])                                 # the first slab again; no frame follows its predecessor
            d = up.stage(headed)
            mixed = [chain[0], chain[2], second[0], chain[0]]         # two pairs, a chained frame, a pair
            e = up.stage(mixed)
            for staged, batch in ((a, chain), (b, second), (c, chain[::-1]), (d, headed), (e, mixed)):
                got = staged.tensor()
                want = np.stack([whole[index[id(f.planes)]][f.y0:f.y1] for f in batch])
                assert tuple(got.shape) == want.shape and got.is_contiguous() and np.array_equal(got.cpu().numpy(), want), rows
            assert np.array_equal(mixed[1].to_bgr(), whole[3][mixed[1].y0:mixed[1].y1])          # ... which is what to_bgr() gives
        inter = [ingest.InterlacedYuvFrame(p, h, w, pf, pics[k], mode="interpolate")[11:40] for k, p in enumerate(pics[1:4])]
        assert np.array_equal(up.stage(inter).tensor().cpu().numpy(), np.stack([R.convert(D.picture(f.planes, None, fmt, 0), fmt)[11:40] for f in inter]))
        for other in (frames[2][10:22], frames[2][11:21], ingest.InterlacedYuvFrame(pics[2], h, w, pf, pics[1], "tff" if keep else "bff")[10:20],
                      ingest.InterlacedYuvFrame(pics[2], h, w, pf, pics[1], frames[0].field_order, "interpolate")[10:20],
                      ingest.InterlacedYuvFrame(pics[2], h, w, pf, pics[1], frames[0].field_order, thresh=11)[10:20],
                      ingest.YuvFrame(pics[2], h, w, pf)[10:20]):
            with pytest.raises(ValueError):
                up.stage([frames[1][10:20], other])
    finally:
        up.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_extractor_over_an_interlaced_stream_equals_the_host_route(ctx, tmp_path):
    """tests/test_deinterlace.py's clip (subtitles that switch between the fields of a frame) as an It Y4M: once as a stream through the
    Uploader (deinterlaced and converted on the device), once through the file source without one (on the host); the change selector on
    the engine both times.  Equal intervals and recognised frames, and the intervals of the numpy counter on the reference's frames."""
    import torch
    from frame_change_ref import NumpyCounter
    from oracle import net_ref, pipeline_ref as P
    from test_deinterlace import CHANGE_AREA, FMT420, interlaced_clip
    from test_one_pass import piped
    from vse_amd import extractor, frame_select, ingest, pipeline, shim, staging
    pipe = pipeline.OcrPipeline(ctx, net_ref.get_weights("V3_ch_det_fast"), net_ref.get_weights("V4_en_rec_fast"), P.en_charset(),
                                rec_mode="reference")
    clip = interlaced_clip()
    ref = [R.convert(D.picture(f, clip["woven"][k - 1] if k else None, FMT420), FMT420) for k, f in enumerate(clip["woven"])]
    nos = {hashlib.sha1(f.tobytes()).digest(): no for no, f in enumerate(ref, 1)}

    class EngineOcr:
        def __init__(self):
            self.seen = []

        def predict_batch(self, frames):
            dev = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames)).to(ctx.tdev)
            self.seen += [nos[hashlib.sha1(f.tobytes()).digest()] for f in dev.cpu().numpy()]
            return [shim.OcrRecogniser.arrange(b, r) for b, r in pipe.ocr(dev)]

        def predict(self, frame):
            return self.predict_batch(np.ascontiguousarray(frame)[None])[0]

    path = str(tmp_path / "fields.y4m")
    ingest.write_yuv(path, clip["woven"], product_format(FMT420), fps=12, y4m=True, interlace="t")
    with open(path, "rb") as fp:
        data = fp.read()
    up = staging.Uploader(ctx.tdev, ctx=ctx)
    runs = []
    try:
        for staged in (True, False):
            fp, th = piped(data, 1 << 16) if staged else (None, None)
            src = ingest.Y4mStream(fp, wide=True, deinterlace="adaptive") if staged else ingest.Y4mSource(path, wide=True, deinterlace="adaptive")
            assert src.field_order == "tff"
            ocr = EngineOcr()
            ex = extractor.SubtitleExtractor(src, ocr, sub_area=CHANGE_AREA, mode="auto", drop_score=0.0, batch=8, uploader=up if staged else None,
                                             frame_selector="change", change_counter=frame_select.EngineCounter(ctx))
            assert ex.one_pass == staged
            ex.run()
            runs.append(([(s, e) for s, e, _r in ex.intervals], ocr.seen))
            if staged:
                th.join()
                fp.close()
            else:
                src.close()
    finally:
        up.close()
    want = [(s, e) for s, e, _r in frame_select.ChangeFrameSelector(NumpyCounter(), batch=8).run(list(ref), CHANGE_AREA)]
    assert runs[0] == runs[1] and runs[0][0] == want and len(want) == len(clip["truth"])
    assert runs[0][1] == [(s + e) // 2 for s, e in want]
