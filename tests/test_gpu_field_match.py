"""vse_yuv_field_match on the MI355X: every comparison is byte equality with the int64 restatement of the rule (tests/field_match_ref.py),
pictures and stats inside buffers filled with 0xA5 so that a byte written outside them shows.  The shapes, formats and layouts of
tests/test_gpu_deinterlace.py, plus 720-byte luma rows over 360-byte chroma rows; telecined smooth pictures for the choices 0 to 2 and
unrelated ones for the fallback; the threshold's edges; what the call must refuse; staging.Uploader over frames of mode "match"; and
SubtitleExtractor over a telecined Y4M stream, staged against the host route."""
import ctypes as C
import hashlib
import itertools

import numpy as np
import pytest

import deinterlace_ref as D
import field_match_ref as M
import yuv_format_ref as R
from test_gpu_deinterlace import FAST_SHAPES, FAST_SHAPES_2, FILL, FORMATS, GENERAL_SHAPES, VARIANTS
from test_yuv_formats import ident, product_format
from vse_amd import synth

pytestmark = pytest.mark.gpu

DVD_SHAPE = (6, 720)                    # 8-bit 4:2:0: luma rows take 16-byte moves, the 360-byte chroma rows cannot
FILL32 = int(np.array([FILL] * 4, np.uint8).view(np.int32)[0])
ORDERS = ("tff", "bff")


def build_case(rng, fmt, h, w, variant, keep, kind, comb_thresh=10, comb_limit=20, thresh=10):
    """The pictures of one call laid out as `variant` says, and what the reference makes of them.  kind "film": smooth pictures dealt in
    one of the pulldown phases; "video": unrelated random words around the deinterlacer's threshold (everything combs)."""
    _name, n, layout, pad, off = variant
    like = R.random_planes(rng, h, w, fmt)
    if kind == "film":
        film = [M.smooth_planes(rng, like, fmt, k, comb_thresh) for k in range(5)]
        woven, _ = synth.telecine(film, "32" if (h + n + keep) & 1 else "32b", ORDERS[keep])
        if layout == "chain":
            cur, prev = woven[1:n + 1], woven[:n]
            slots = woven[:n + 1]
        elif layout == "pairs":
            at = [1 + (2 * f + 1) % 4 for f in range(n)]
            cur, prev = [woven[k] for k in at], [woven[k - 1] for k in at]
            slots = [p for pair in zip(prev, cur) for p in pair]
        else:
            cur, prev, slots = woven[:n], [None] * n, woven[:n]
    elif layout == "chain":
        slots = [like]
        for _ in range(n):
            slots.append(D.near_threshold_prev(rng, slots[-1], fmt, thresh))
        cur, prev = slots[1:], slots[:-1]
    elif layout == "pairs":
        cur = [R.random_planes(rng, h, w, fmt) for _ in range(n)]
        prev = [D.near_threshold_prev(rng, c, fmt, thresh) for c in cur]
        slots = [p for pair in zip(prev, cur) for p in pair]
    else:
        cur = [R.random_planes(rng, h, w, fmt) for _ in range(n)]
        prev, slots = [None] * n, cur
    want = [M.picture(c, p, fmt, keep, comb_thresh, None if comb_limit is not None and comb_limit < 0 else comb_limit, thresh) for c, p in zip(cur, prev)]
    return dict(fmt=fmt, h=h, w=w, variant=variant, keep=keep, kind=kind, comb_thresh=comb_thresh, comb_limit=comb_limit, thresh=thresh, slots=slots,
                want=want)


def run_case(ctx, case):
    """One call -> pictures and stats byte for byte the reference's inside their filled buffers, the inputs unchanged."""
    import torch
    fmt, h, w = case["fmt"], case["h"], case["w"]
    _name, n, layout, pad, off = case["variant"]
    slots = case["slots"]
    ss = 1 if fmt[3] == 8 else 2
    frame = R.packed_bytes(h, w, fmt)
    stride = frame + pad * ss
    step, first = (2, 1) if layout == "pairs" else (1, 1) if layout == "chain" else (1, 0)
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
    sbig = torch.full((4 * (n + 2),), FILL32, dtype=torch.int32, device=ctx.tdev)
    stats = sbig[4:4 + 4 * n].view(n, 4)
    got, got_stats = ctx.yuv_field_match(packed, n, h, w, product_format(fmt), prev=None if layout == "null" else src[base + (first - 1) * stride:],
                                         prev_stride=step * stride, keep=case["keep"], comb_thresh=case["comb_thresh"], comb_limit=case["comb_limit"],
                                         thresh=case["thresh"], out=out, stats=stats)
    assert got is out and got_stats is stats
    want = np.full(big.numel(), FILL, np.uint8)
    want_stats = np.full(sbig.numel(), FILL32, np.int32)
    for f, (planes, st) in enumerate(case["want"]):
        want[obase + f * ostride:obase + f * ostride + frame] = R.pack(planes, fmt)
        want_stats[4 + 4 * f:8 + 4 * f] = st
    what = (fmt, h, w, case["variant"], case["keep"], case["kind"], case["comb_thresh"], case["comb_limit"])
    assert np.array_equal(sbig.cpu().numpy(), want_stats), (what, sbig.cpu().numpy().tolist(), want_stats.tolist())
    assert np.array_equal(big.cpu().numpy(), want), what
    assert np.array_equal(src.cpu().numpy(), host), what                            # the inputs are read only


def shapes_of(fmt):
    return FAST_SHAPES + FAST_SHAPES_2 + GENERAL_SHAPES + ([DVD_SHAPE] if fmt[:4] == (1, 1, 1, 8) else [])


def bit_for_bit_cases(fmt):
    rng = np.random.default_rng(sum(fmt) + 21)
    ss = 1 if fmt[3] == 8 else 2
    cases = []
    for k, ((h, w), variant) in enumerate(itertools.product(shapes_of(fmt), VARIANTS)):
        if variant[0] == "base + 1" and ss == 2:
            continue                                                 # 2-byte samples at an odd base are refused (test_refusals_launch_nothing)
        cases += [build_case(rng, fmt, h, w, variant, keep, "film") for keep in (0, 1)]
        cases.append(build_case(rng, fmt, h, w, variant, k & 1, "video"))
    return cases


@pytest.mark.parametrize("fmt", FORMATS, ids=ident)
def test_bit_for_bit_with_sentinels(ctx, fmt):
    cases = bit_for_bit_cases(fmt)
    # by the reference alone every choice occurs, with and without a previous picture where it can, before anything is compared
    seen = {(st[3], c["variant"][2] != "null") for c in cases for _p, st in c["want"]}
    assert seen >= {(0, True), (1, True), (2, True), (3, True), (0, False), (3, False)}, seen
    for case in cases:
        run_case(ctx, case)


@pytest.mark.parametrize("fmt,h,w", [((1, 1, 1, 8, 0, 0, 0), 40, 1024), ((1, 1, 1, 10, 0, 1, 0), 36, 520), ((1, 1, 2, 8, 0, 1, 0), 70, 1030)], ids=["8", "10", "odd"])
def test_counts_add_up_over_blocks(ctx, fmt, h, w):
    """More than one block and more than one wave per frame in the 16-byte kernels (320 and 325 luma items of 256 per block) and in the
    general ones (a 64 x 4 block spans 256 columns and 32 rows): the per-wave sums meet in the frame's stats through atomics."""
    rng = np.random.default_rng(h + w)
    cases = [build_case(rng, fmt, h, w, VARIANTS[1], keep, kind) for keep, kind in ((0, "film"), (1, "film"), (0, "video"))]
    assert {st[3] for c in cases for _p, st in c["want"]} == {0, 1, 2, 3}
    for case in cases:
        run_case(ctx, case)


def test_one_call_makes_both_weave_launches(ctx):
    """8-bit 4:2:0 planar, 6 x 48, two frames: the 48-byte luma rows take the 16-byte weave, the 24-byte chroma rows the quads."""
    rng = np.random.default_rng(648)
    for keep, kind in ((0, "film"), (1, "film"), (0, "video")):
        run_case(ctx, build_case(rng, (1, 1, 1, 8, 0, 0, 0), 6, 48, ("chained", 2, "chain", 0, 0), keep, kind))


def test_threshold_edges_and_limits(ctx):
    """Rows that alternate between b and b + d with d = T in some columns and T + 1 in others, at comb_thresh 0 and 255 (at 8 bits T + 1 =
    256 does not exist: nothing combs), under comb_limit 0 (one combed sample falls back), 1000 (nothing can) and < 0 (never)."""
    rng = np.random.default_rng(88)
    chain3, pairs3 = VARIANTS[1], VARIANTS[3]
    choices = set()
    for fmt, (h, w) in (((1, 1, 1, 8, 0, 0, 0), (10, 64)), ((1, 1, 2, 16, 1, 0, 0), (6, 48)), ((0, 0, 1, 10, 0, 0, 0), (7, 34)), ((1, 0, 1, 10, 1, 0, 0), (5, 17))):
        top = 255 if fmt[3] == 8 else 65535
        for comb_thresh, comb_limit in itertools.product((0, 255), (0, 1000, -1)):
            t = D.threshold(fmt, comb_thresh)
            case = build_case(rng, fmt, h, w, pairs3 if comb_limit else chain3, comb_thresh & 1, "video", comb_thresh, comb_limit)
            for planes in case["slots"]:
                luma = planes[0]
                d = np.minimum(t + rng.integers(0, 2, size=luma.shape[1]), top)
                luma[0::2] = 0
                luma[1::2] = d[None, :].astype(luma.dtype)
            case["slots"][-1][0][1::2] = 0                           # the last picture is flat: a weave with it combs where d > T alone
            cur = case["slots"][1::2] if comb_limit else case["slots"][1:]
            prev = case["slots"][0::2] if comb_limit else case["slots"][:-1]
            case["want"] = [M.picture(c, p, fmt, case["keep"], comb_thresh, None if comb_limit < 0 else comb_limit) for c, p in zip(cur, prev)]
            # by hand: every tested row of the first picture combs in the columns with d = T + 1, and in no other
            assert case["want"][0][1][0] == (h - 2) * int((cur[0][0][1].astype(np.int64) > t).sum())
            choices |= {(comb_limit, st[3]) for _p, st in case["want"]}
            run_case(ctx, case)
    assert {c for lim, c in choices if lim == 1000} <= {0, 1, 2} >= {c for lim, c in choices if lim == -1} and (0, 3) in choices and (0, 0) in choices


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx):
    import torch
    lib = ctx.lib
    h, w, n = 8, 16, 2
    fmt = (1, 1, 1, 10, 0, 1, 0)
    frame = R.packed_bytes(h, w, fmt)
    ok = dict(n=n, h=h, w=w, sub_x=1, sub_y=1, chroma=1, depth=10, msb=0, keep=0, comb_thresh=10, comb_limit=20, thresh=10, sstride=frame, pstride=frame,
              ostride=frame, soff=frame, poff=0, ooff=0, prev=True, out=None, stats=0)
    src = torch.zeros(4 * frame + 16, dtype=torch.uint8, device=ctx.tdev)
    out = torch.full((4 * frame,), FILL, dtype=torch.uint8, device=ctx.tdev)
    stats = torch.full((16,), FILL32, dtype=torch.int32, device=ctx.tdev)

    def call(a):
        d_out = out.data_ptr() + a["ooff"] if a["out"] is None else src.data_ptr() + a["out"]
        d_stats = None if a["stats"] is None else a["stats"] if a["stats"] > 4096 else stats.data_ptr() + a["stats"]
        return lib.vse_yuv_field_match(ctx.handle, C.c_void_p(src.data_ptr() + a["soff"]), C.c_void_p(src.data_ptr() + a["poff"]) if a["prev"] else None,
                                       a["n"], a["h"], a["w"], a["sub_x"], a["sub_y"], a["chroma"], a["depth"], a["msb"], a["keep"], a["comb_thresh"],
                                       a["comb_limit"], a["thresh"], a["sstride"], a["pstride"], C.c_void_p(d_out), a["ostride"],
                                       C.c_void_p(d_stats) if d_stats is not None else None, ctx.stream())
    # everything vse_yuv_deinterlace refuses (it has no mode) ...
    bad = [dict(h=0), dict(w=0), dict(n=0), dict(h=-1), dict(n=-1), dict(sub_x=0, sub_y=1), dict(sub_x=2), dict(sub_y=-1), dict(chroma=3), dict(chroma=-1),
           dict(chroma=0), dict(chroma=2, sub_y=0), dict(depth=7), dict(depth=17), dict(depth=8, msb=1), dict(msb=2), dict(msb=-1), dict(keep=2),
           dict(keep=-1), dict(thresh=-1), dict(thresh=256), dict(sstride=frame - 2), dict(pstride=frame - 2),
           dict(ostride=frame - 2), dict(sstride=frame + 1), dict(pstride=frame + 1), dict(ostride=frame + 1), dict(soff=frame + 1), dict(poff=1),
           dict(ooff=1), dict(out=frame), dict(out=0), dict(h=1 << 16, w=1 << 15)]
    # ... and its own: the stats missing, unaligned or inside the pictures, the comb threshold and limit out of range
    bad += [dict(stats=None), dict(stats=1), dict(stats=2), dict(stats=src.data_ptr() + frame), dict(stats=src.data_ptr() + 8),
            dict(stats=src.data_ptr() + 3 * frame - 4), dict(stats=out.data_ptr() + 2 * frame - 16), dict(stats=out.data_ptr()),
            dict(comb_thresh=-1), dict(comb_thresh=256), dict(comb_limit=1001)]
    for change in bad:
        assert call(dict(ok, **change)) == -1, change
        msg = lib.vse_last_error().decode()
        assert "vse_yuv_field_match" in msg and f"depth {dict(ok, **change)['depth']} " in msg, change
    torch.cuda.synchronize()
    assert bool((out == FILL).all()) and bool((src == 0).all()) and bool((stats == FILL32).all())
    # the accepted calls next to them do write: all-zero pictures stay all zero (every count 0, choice c), only the packed bytes and the
    # 16 n bytes of the stats are written; the stats may lie right behind the pictures
    for more in (dict(), dict(prev=False, pstride=0), dict(comb_limit=-7, pstride=frame + 16), dict(comb_limit=0, comb_thresh=0, stats=16),
                 dict(stats=out.data_ptr() + 2 * frame), dict(comb_limit=1000, comb_thresh=255)):
        out.fill_(FILL)
        stats.fill_(FILL32)
        assert call(dict(ok, **more)) == 0, more
        torch.cuda.synchronize()
        host = out.cpu().numpy()
        if more.get("stats", 0) > 4096:
            assert np.all(host[:n * frame + 16 * n] == 0) and np.all(host[n * frame + 16 * n:] == FILL) and bool((stats == FILL32).all())
            continue
        assert np.all(host[:n * frame] == 0) and np.all(host[n * frame:] == FILL)
        at = more.get("stats", 0) // 4
        st = stats.cpu().numpy()
        assert np.all(st[at:at + 4 * n] == 0) and np.all(st[:at] == FILL32) and np.all(st[at + 4 * n:] == FILL32)


# ---- staging ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [(1, 1, 1, 8, 0, 0, 0), (1, 1, 2, 10, 1, 1, 0)], ids=ident)
def test_uploader_stages_matched_frames(ctx, fmt):
    """A telecined film of smooth pictures followed by unrelated pictures (the fallback): batches that mix NULL, chained and pair slots,
    the whole picture and bands, against the host route (which tests/test_field_match.py holds to the reference)."""
    from vse_amd import ingest, staging
    h, w = 46, 70
    rng = np.random.default_rng(47)
    pf = product_format(fmt)
    like = R.random_planes(rng, h, w, fmt)
    pics, _ = synth.telecine([M.smooth_planes(rng, like, fmt, k) for k in range(5)], "32b", "bff" if fmt[2] == 2 else "tff")
    pics = pics[:5] + [R.random_planes(rng, h, w, fmt) for _ in range(2)]
    order = "bff" if fmt[2] == 2 else "tff"
    frames = [ingest.InterlacedYuvFrame(p, h, w, pf, pics[k - 1] if k else None, order, "match") for k, p in enumerate(pics)]
    assert [f.match_stats()[3] for f in frames] == [0, 0, 2, 2, 0, 3, 3]
    for f in frames[1:]:
        want, st = M.picture(f.planes, f.prev, fmt, f.keep)
        assert f.match_stats() == st and np.array_equal(f.to_bgr(), R.convert(want, fmt))
    up = staging.Uploader(ctx.tdev, depth=2, ctx=ctx)
    try:
        for rows in (slice(None), slice(23, None), slice(11, 40), slice(12, 13)):
            chain, second = [f[rows] for f in frames[1:4]], [f[rows] for f in frames[4:]]
            headed = [f[rows] for f in frames[:3]]                    # its first frame has no previous picture
            a, b = up.stage(chain), up.stage(second)                  # two batches in flight through two slabs
            c = up.stage(chain[::-1])                                 # no frame follows its predecessor: pairs
            d = up.stage(headed)
            mixed = [headed[0], chain[0], chain[2], second[1], second[2], chain[0]]      # NULL, chained, a pair, a pair, chained, a pair
            e = up.stage(mixed)
            for staged, batch in ((a, chain), (b, second), (c, chain[::-1]), (d, headed), (e, mixed)):
                got = staged.tensor()
                want = np.stack([f.to_bgr() for f in batch])
                assert tuple(got.shape) == want.shape and got.is_contiguous() and np.array_equal(got.cpu().numpy(), want), rows
        for other in (ingest.InterlacedYuvFrame(pics[2], h, w, pf, pics[1], order, "match", comb_thresh=11)[10:20],
                      ingest.InterlacedYuvFrame(pics[2], h, w, pf, pics[1], order, "match", comb_limit=None)[10:20],
                      ingest.InterlacedYuvFrame(pics[2], h, w, pf, pics[1], order, "adaptive")[10:20]):
            with pytest.raises(ValueError):
                up.stage([frames[1][10:20], other])
    finally:
        up.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_extractor_over_a_telecined_stream_equals_the_host_route(ctx, tmp_path):
    """tests/test_field_match.py's film in the pulldown phase whose second field runs ahead, as an It Y4M: once as a stream through the
    Uploader in one pass (matched and converted on the device), once through the file source without one (on the host); the change
    selector on the engine both times.  Equal recognised frames, and the film's own intervals."""
    import torch
    from oracle import net_ref, pipeline_ref as P
    from test_change_select import AREA as CHANGE_AREA
    from test_deinterlace import FMT420
    from test_field_match import FILM_32B, film_clip, matched_frames
    from test_one_pass import piped
    from vse_amd import extractor, frame_select, ingest, pipeline, shim, staging
    pipe = pipeline.OcrPipeline(ctx, net_ref.get_weights("V3_ch_det_fast"), net_ref.get_weights("V4_en_rec_fast"), P.en_charset(),
                                rec_mode="reference")
    woven, _pairs = synth.telecine(film_clip()["yuv"], "32b")
    ref = [f.to_bgr() for f in matched_frames(woven)]
    nos = {hashlib.sha1(f.tobytes()).digest(): no for no, f in enumerate(ref, 1)}          # (a repeated picture: its later number)

    class EngineOcr:
        def __init__(self):
            self.seen = []

        def predict_batch(self, frames):
            dev = frames if torch.is_tensor(frames) else torch.from_numpy(np.ascontiguousarray(frames)).to(ctx.tdev)
            self.seen += [nos[hashlib.sha1(f.tobytes()).digest()] for f in dev.cpu().numpy()]
            return [shim.OcrRecogniser.arrange(b, r) for b, r in pipe.ocr(dev)]

        def predict(self, frame):
            return self.predict_batch(np.ascontiguousarray(frame)[None])[0]

    path = str(tmp_path / "film.y4m")
    ingest.write_yuv(path, woven, product_format(FMT420), fps=12, y4m=True, interlace="t")
    with open(path, "rb") as fp:
        data = fp.read()
    up = staging.Uploader(ctx.tdev, ctx=ctx)
    runs = []
    try:
        for staged in (True, False):
            fp, th = piped(data, 1 << 16) if staged else (None, None)
            src = ingest.Y4mStream(fp, wide=True, deinterlace="match") if staged else ingest.Y4mSource(path, wide=True, deinterlace="match")
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
    assert runs[0] == runs[1] and runs[0][0] == FILM_32B and len(runs[0][1]) == len(FILM_32B)
