"""Field matching on the host (deinterlace="match": film carried in interlaced video): ingest.InterlacedYuvFrame against the int64
restatement of the rule (tests/field_match_ref.py), the rule by hand, recovery of the film's pictures from synth.telecine in every pattern
and field order, the interval table of the second pulldown phase, the fallback on true field-rate video, what the sources and headers
accept and refuse, one pass against several, and the command lines.  CPU only."""
import itertools

import numpy as np
import pytest

import field_match_ref as M
import yuv_format_ref as R
from frame_change_ref import NumpyCounter
from test_change_select import AREA as CHANGE_AREA, SCHEDULE
from test_deinterlace import FMT420, FORMATS, HEIGHTS, ORDERS, deinterlaced_bgr, equal_planes, interlaced_clip, pictures, y4m_file
from test_one_pass import FPS, LookupOcr, host_stack, piped, run, text_box  # noqa: F401  (host_stack is a fixture)
from test_yuv_formats import ident, product_format
from vse_amd import area_locator, extractor, frame_select, ingest, synth

PATTERNS = ("32", "32b", "shift")
# the issue's table for the phase in which the second field runs ahead: the film's own intervals and what mode adaptive makes of them
FILM_32B = [(5, 13), (14, 20), (26, 31), (32, 39), (42, 48), (55, 63)]
ADAPTIVE_32B = [(4, 12), (13, 20), (26, 31), (32, 38), (42, 47), (54, 62)]


def frame(cur, prev, fmt, keep=0, **kw):
    h, w = np.asarray(cur[0]).shape
    return ingest.InterlacedYuvFrame(cur, h, w, product_format(fmt), prev, ORDERS[keep], "match", **kw)


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS, ids=ident)
def test_matched_planes_and_stats_equal_the_reference(fmt):
    """Random words around the deinterlacer's threshold (everything combs: the fallback, or with comb_limit None a choice among three
    large counts) and a telecined film of smooth pictures (choices 0, 1 and 2)."""
    rng = np.random.default_rng(sum(fmt) + 11)
    seen = set()
    for h, w in itertools.product(HEIGHTS, (1, 6, 23)):
        cur, prev = pictures(rng, h, w, fmt)
        film = [M.smooth_planes(rng, cur, fmt, k) for k in range(4)]
        cases = [(cur, prev, {}), (cur, prev, dict(comb_limit=None)), (cur, None, {}), (cur, None, dict(comb_limit=None)),
                 (cur, prev, dict(comb_thresh=0, comb_limit=1000, thresh=3))]
        for keep in (0, 1):
            woven, _ = synth.telecine(film, "32b" if (h + w) & 1 else "32", ORDERS[keep])
            for cur_k, prev_k, kw in cases + [(woven[k], woven[k - 1], {}) for k in range(1, 5)]:
                f = frame(cur_k, prev_k, fmt, keep, **kw)
                want, st = M.picture(cur_k, prev_k, fmt, keep, kw.get("comb_thresh", 10), kw.get("comb_limit", 20), kw.get("thresh", 10))
                assert f.match_stats() == st, (h, w, keep, kw)
                assert equal_planes(f.deinterlaced_planes(), want), (h, w, keep, kw, st)
                assert np.array_equal(f.to_bgr(), R.convert(want, fmt)), (h, w, keep, kw, st)
                if h >= 3:
                    seen.add(st[3])
    assert seen == {0, 1, 2, 3}, seen


@pytest.mark.parametrize("fmt,t", [((0, 0, 0, 8, 0, 0, 0), 10), ((0, 0, 0, 10, 0, 0, 0), 40), ((0, 0, 0, 10, 1, 0, 0), 2560)], ids=["8", "10", "10msb"])
def test_threshold_ties_and_small_pictures_by_hand(fmt, t):
    dt = R.sample_dtype(fmt)
    unit = t // 10

    def col(values):
        return (np.asarray(values, np.int64).astype(dt)[:, None],)
    base = 50 * unit
    # a difference of exactly T is not combed, T + 1 is, upwards and downwards; the comparison needs both neighbours on the same side
    assert frame(col([base, base + t, base]), None, fmt).match_stats() == (0, 0, 0, 0)
    assert frame(col([base, base + t + 1, base]), None, fmt, comb_limit=None).match_stats() == (1, 0, 0, 0)
    assert frame(col([base + t, base, base + t]), None, fmt).match_stats() == (0, 0, 0, 0)
    assert frame(col([base + t + 1, base, base + t + 1]), None, fmt, comb_limit=None).match_stats() == (1, 0, 0, 0)
    assert frame(col([base, base + t + 1, base + 2 * t + 2]), None, fmt).match_stats() == (0, 0, 0, 0)          # a slope is no comb
    assert frame(col([base, base + t + 1, base + 1]), None, fmt, comb_limit=None).match_stats() == (0, 0, 0, 0)  # one side within T
    assert M.stats(col([base, base + t + 1, base]), None, fmt, comb_limit=None) == (1, 0, 0, 0)
    # one sample of one tested row combed is 1000 per mille: the fallback, which without a previous picture interpolates the second field
    f = frame(col([base, base + t + 1, base]), None, fmt)
    assert f.match_stats() == (1, 0, 0, 3) and f.deinterlaced_planes()[0][:, 0].tolist() == [base, base, base]
    assert frame(col([base, base + t + 1, base]), None, fmt, comb_limit=1000).match_stats() == (1, 0, 0, 0)      # 1000 > 1000 is false
    # a tie takes c: the previous picture is the picture (every count equal), combed or not
    cur = col([base, base + 3 * t, base, base + 3 * t, base])
    assert frame(cur, cur, fmt, comb_limit=None).match_stats() == (3, 3, 3, 0)
    flat = col([base] * 5)
    assert frame(flat, col([base + 5 * t] * 5), fmt).match_stats() == (0, 3, 3, 0)
    # c combed, p1 and p2 tie at 0: p1.  Rows 0 2 4 of the picture and rows 1 3 of the previous one are one film picture, and so are
    # rows 0 2 4 of the previous picture with rows 1 3 of the picture: top field first takes p1 = C's first field with P's second
    lo, hi = base, base + 5 * t
    cur, prev = col([lo, hi, lo, hi, lo]), col([hi, lo, hi, lo, hi])
    f = frame(cur, prev, fmt)
    assert f.match_stats() == (3, 0, 0, 1) and f.deinterlaced_planes()[0][:, 0].tolist() == [lo] * 5
    g = frame(cur, prev, fmt, keep=1)
    assert g.match_stats() == (3, 0, 0, 1) and g.deinterlaced_planes()[0][:, 0].tolist() == [hi] * 5
    # p2 alone clean: the picture's second field with the previous picture's first
    prev = col([hi, 3 * hi // 2, hi, 3 * hi // 2, hi])
    f = frame(cur, prev, fmt)
    assert f.match_stats() == (3, 3, 0, 2) and f.deinterlaced_planes()[0][:, 0].tolist() == [hi] * 5
    # R < 3 counts 0 everywhere: choice c at R = 2; at R = 1 the bound w (R - 2) is negative and the fallback's output is the picture too
    for rows in (1, 2):
        cur, prev = col([lo, hi][:rows]), col([hi, lo][:rows])
        f = frame(cur, prev, fmt)
        assert f.match_stats()[:3] == (0, 0, 0) and f.match_stats()[3] == (0 if rows == 2 else 3) and equal_planes(f.deinterlaced_planes(), cur)
        assert frame(cur, prev, fmt, comb_limit=None).match_stats() == (0, 0, 0, 0)
        assert M.stats(cur, prev, fmt) == f.match_stats()
    # comb_limit None never falls back, whatever combs
    rng = np.random.default_rng(4)
    cur, prev = R.random_planes(rng, 9, 12, fmt), R.random_planes(rng, 9, 12, fmt)
    assert frame(cur, prev, fmt).match_stats()[3] == 3 and frame(cur, prev, fmt, comb_limit=None).match_stats()[3] in (0, 1, 2)
    assert frame(cur, None, fmt).match_stats()[3] == 3 and frame(cur, None, fmt, comb_limit=None).match_stats()[1:] == (0, 0, 0)


def test_frame_checks_its_match_arguments():
    fmt = (1, 1, 1, 8, 0, 0, 0)
    cur = R.random_planes(np.random.default_rng(1), 4, 6, fmt)
    for bad in (dict(comb_thresh=-1), dict(comb_thresh=256), dict(comb_thresh=1.5), dict(comb_thresh=True), dict(comb_limit=-1), dict(comb_limit=1001),
                dict(comb_limit=2.5), dict(comb_limit="off")):
        with pytest.raises(ValueError, match="comb"):
            frame(cur, None, fmt, **bad)
    with pytest.raises(ValueError, match="match_stats"):
        ingest.InterlacedYuvFrame(cur, 4, 6, product_format(fmt), cur).match_stats()
    f = frame(cur, cur, fmt, comb_thresh=3, comb_limit=None)[1:3]
    assert (f.mode, f.comb_thresh, f.comb_limit, f.y0, f.y1) == ("match", 3, None, 1, 3) and "match" in ingest.DEINTERLACE_MODES


def test_slices_count_over_the_band_the_device_is_handed():
    """A slice's counts are those of the reference on the packed band; where the slice and the whole frame choose alike the rows are the
    whole frame's, and in a static band (the candidates are equal) they always are."""
    fmt = (1, 1, 1, 8, 0, 0, 0)
    rng = np.random.default_rng(12)
    h, w = 46, 10
    like = R.random_planes(rng, h, w, fmt)
    film = [M.smooth_planes(rng, like, fmt, k) for k in range(4)]
    woven, _ = synth.telecine(film, "32b")
    for k in range(1, 5):
        f = frame(woven[k], woven[k - 1], fmt)
        whole = f.to_bgr()
        for a, b in ((0, 46), (23, 46), (0, 23), (11, 40), (12, 13), (45, 46), (1, 2)):
            g = f[a:b]
            lo, hi = g.band()
            sub_c, _ = R.sub_frame(woven[k], fmt, lo, hi)
            sub_p, _ = R.sub_frame(woven[k - 1], fmt, lo, hi)
            want, st = M.picture(sub_c, sub_p, fmt)
            assert g.match_stats() == st and st[3] == f.match_stats()[3]
            assert np.array_equal(g.to_bgr(), R.convert(want, fmt)[a - lo:b - lo]) and np.array_equal(g.to_bgr(), whole[a:b])
    # moving above, static below: the whole frame is matched (p2 here), the static band ties and takes c; the rows are the same
    cur, prev = tuple(p.copy() for p in woven[2]), tuple(p.copy() for p in woven[1])
    for p, q in zip(cur, prev):
        q[p.shape[0] // 2:] = p[p.shape[0] // 2:]
    f = frame(cur, prev, fmt, comb_limit=None)
    g = f[32:44]
    assert f.match_stats()[3] == 2 and g.match_stats()[3] == 0 and np.array_equal(g.to_bgr(), f.to_bgr()[32:44])


# ---- the film's pictures come back ---------------------------------------------------------------------------------------------------
_film = {}


def film_clip():
    """tests/test_change_select.py's clip as film: the BGR pictures, their (Y, U, V) triples and the truth."""
    if not _film:
        bgr, truth = synth.make_clip(SCHEDULE, 360, 640, seed=5)
        _film.update(bgr=bgr, yuv=[ingest.bgr_to_yuv420(f) for f in bgr], truth=truth)
    return _film


def matched_frames(woven, order="tff", mode="match"):
    pf = product_format(FMT420)
    h, w = woven[0][0].shape
    return [ingest.InterlacedYuvFrame(f, h, w, pf, woven[k - 1] if k else None, order, mode) for k, f in enumerate(woven)]


def test_telecine_deals_the_fields():
    film = film_clip()["yuv"][:9]
    for order, keep in (("tff", 0), ("bff", 1)):
        for pattern, want in (("32", [(0, 0), (1, 1), (1, 2), (2, 3), (3, 3), (4, 4), (5, 5), (5, 6), (6, 7), (7, 7), (8, 8)]),
                              ("32b", [(0, 0), (1, 1), (2, 1), (3, 2), (3, 3), (4, 4), (5, 5), (6, 5), (7, 6), (7, 7), (8, 8)]),
                              ("shift", [(k, max(k - 1, 0)) for k in range(9)])):
            woven, pairs = synth.telecine(film, pattern, order)
            assert pairs == want and len(woven) == len(pairs)
            for planes, (a, b) in zip(woven, pairs):
                for p, first, second in zip(planes, film[a], film[b]):
                    assert p.dtype == first.dtype and np.array_equal(p[keep::2], first[keep::2]) and np.array_equal(p[1 - keep::2], second[1 - keep::2])
    assert len(synth.telecine(film_clip()["yuv"], "32")[0]) == 65
    for bad in (dict(pattern="23"), dict(field_order="auto")):
        with pytest.raises(ValueError):
            synth.telecine(film, **bad)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_every_frame_is_a_picture_of_the_film(pattern, order):
    """Every frame after the first comes out byte-equal to one of the pictures whose fields it or its predecessor holds, and the choices
    repeat with the pattern's period."""
    film = film_clip()["yuv"]
    woven, pairs = synth.telecine(film, pattern, order)
    frames = matched_frames(woven, order)
    choices = []
    for k, f in enumerate(frames):
        st = f.match_stats()
        choices.append(st[3])
        if k:
            got = f.deinterlaced_planes()
            assert st[3] < 3 and any(equal_planes(got, film[i]) for i in set(pairs[k] + pairs[k - 1])), (k, st, pairs[k])
            # the right weave stays below 9.2 per mille of the samples tested; a wrong one (there always is one) combs in a third of them
            assert min(st[:3]) * 1000 <= 9.2 * 640 * 358 and max(st[:3]) * 1000 > 300 * 640 * 358, (k, st)
    period = 1 if pattern == "shift" else 5
    assert choices[1:-period] == choices[1 + period:], choices
    assert set(choices[1:]) == {"32": {0, 1}, "32b": {0, 2}, "shift": {2}}[pattern]


def test_the_interval_table_of_the_second_phase():
    """On "32b" mode adaptive puts every interval that begins or ends on a mixed frame one frame early; matching gives the film's own."""
    clip = film_clip()
    woven, pairs = synth.telecine(clip["yuv"], "32b")
    pf = product_format(FMT420)

    def intervals(frames):
        return [(s, e) for s, e, _r in frame_select.ChangeFrameSelector(NumpyCounter(), batch=8).run(list(frames), CHANGE_AREA)]
    matched = intervals(f.to_bgr() for f in matched_frames(woven))
    film = intervals(ingest.YuvFrame(clip["yuv"][min(p)], 360, 640, pf).to_bgr() for p in pairs)        # the picture each frame should be
    adaptive = intervals(deinterlaced_bgr(woven))
    print("matched", matched, "\nfilm", film, "\nadaptive", adaptive)
    assert matched == film == FILM_32B
    assert adaptive == ADAPTIVE_32B


def test_true_video_takes_the_fallback():
    clip = interlaced_clip()
    frames = matched_frames(clip["woven"])
    adaptive = deinterlaced_bgr(clip["woven"])
    for k, f in enumerate(frames):
        st = f.match_stats()
        if k:
            assert st[3] == 3 and all(335 * 640 * 358 <= c * 1000 <= 364 * 640 * 358 for c in st[:3]), (k, st)
        assert np.array_equal(f.to_bgr(), adaptive[k]), k


# ---- sources, headers and the command lines --------------------------------------------------------------------------------------------
def stored_truth(truth, pairs):
    """The film's truth [(start, end, text)] in the numbers of the stored frames, frame k showing picture min(pairs[k])."""
    texts = [next((t for s, e, t in truth if s <= min(p) + 1 <= e), None) for p in pairs]
    out = []
    for no, t in enumerate(texts, 1):
        if t is not None and out and out[-1][2] == t and out[-1][1] == no - 1:
            out[-1] = (out[-1][0], no, t)
        elif t is not None:
            out.append((no, no, t))
    return out


def test_sources_take_match_as_they_take_adaptive(tmp_path):
    fmt = (1, 1, 1, 8, 0, 0, 0)
    rng = np.random.default_rng(5)
    frames = [R.random_planes(rng, 6, 8, fmt) for _ in range(4)]
    path = y4m_file(tmp_path, "It", frames)
    src = ingest.Y4mSource(path, wide=True, deinterlace="match", comb_thresh=7, comb_limit=None)
    with open(path, "rb") as fp:
        stream = ingest.Y4mStream(fp, wide=True, deinterlace="match", comb_thresh=7, comb_limit=None)
        raws = [list(src.raw_frames()), list(stream.raw_frames())]
    opened = ingest.open_source(path, wide=True, deinterlace="match", comb_thresh=7, comb_limit=None)
    raws.append(list(opened.raw_frames()))
    for got in raws:
        for k, raw in enumerate(got):
            assert type(raw) is ingest.InterlacedYuvFrame and (raw.field_order, raw.mode, raw.comb_thresh, raw.comb_limit) == ("tff", "match", 7, None)
            want, st = M.picture(frames[k], frames[k - 1] if k else None, fmt, 0, 7, None)
            assert raw.match_stats() == st and np.array_equal(raw.to_bgr(), R.convert(want, fmt))
    assert np.array_equal(src.read(3), raws[0][2].to_bgr())
    src.close()
    opened.close()
    # wide=True and a field order exactly as adaptive needs them
    for kw in (dict(deinterlace="match"), dict(deinterlace="match", wide=False, field_order="tff")):
        with pytest.raises(ValueError, match="wide"):
            ingest.Y4mSource(path, **kw)
        with pytest.raises(ValueError, match="wide"):
            ingest.open_source(path, **kw)
        with open(path, "rb") as fp, pytest.raises(ValueError, match="wide"):
            ingest.Y4mStream(fp, **kw)
    mixed = y4m_file(tmp_path, "Im", frames, name="im.y4m")
    with pytest.raises(ValueError, match="Im"):
        ingest.Y4mSource(mixed, wide=True, deinterlace="match")
    assert ingest.Y4mSource(mixed, wide=True, deinterlace="match", field_order="bff").field_order == "bff"
    raw_path = str(tmp_path / "clip.raw")
    ingest.write_yuv(raw_path, frames, product_format(fmt))
    with pytest.raises(ValueError, match="field order"):
        ingest.YuvSource(raw_path, 8, 6, 25.0, product_format(fmt), deinterlace="match")
    headerless = ingest.YuvSource(raw_path, 8, 6, 25.0, product_format(fmt), deinterlace="match", field_order="bff", comb_limit=5)
    assert (headerless.read_raw(2).mode, headerless.read_raw(2).keep, headerless.read_raw(2).comb_limit) == ("match", 1, 5)
    headerless.close()
    # bad values, and the options without the mode
    for kw in (dict(comb_thresh=256), dict(comb_thresh=-1), dict(comb_limit=1001), dict(comb_limit=-1), dict(comb_limit=0.5)):
        for make in (lambda: ingest.Y4mSource(path, wide=True, deinterlace="match", **kw), lambda: ingest.open_source(path, wide=True, deinterlace="match", **kw),
                     lambda: ingest.YuvSource(raw_path, 8, 6, 25.0, product_format(fmt), deinterlace="match", field_order="tff", **kw)):
            with pytest.raises(ValueError, match="comb"):
                make()
    for kw in (dict(deinterlace="adaptive", comb_thresh=5), dict(comb_limit=None), dict(deinterlace="interpolate", comb_limit=30)):
        with pytest.raises(ValueError, match="belong to deinterlace"):
            ingest.open_source(path, wide=True, **kw)
    # without the opt-in every refusal and message is what it was
    for kw in ({}, {"wide": True}, {"wide": True, "field_order": "tff"}):
        for make in (lambda: ingest.Y4mSource(path, **kw), lambda: ingest.open_source(path, **kw)):
            with pytest.raises(ValueError) as e:
                make()
            assert str(e.value) == f"{path}: interlaced video (It) is not supported"
    for name in ("clip.yuv", "clip.npy", "clip.avi"):
        with pytest.raises(ValueError, match="deinterlace"):
            ingest.open_source(str(tmp_path / name), size=(8, 6), fps=25.0, deinterlace="match", field_order="tff")


@pytest.fixture(scope="module")
def telecined_y4m(tmp_path_factory):
    clip = film_clip()
    woven, pairs = synth.telecine(clip["yuv"], "32b")
    path = str(tmp_path_factory.mktemp("film") / "film32b.y4m")
    ingest.write_yuv(path, woven, product_format(FMT420), fps=FPS, y4m=True, interlace="t")
    return path, woven, stored_truth(clip["truth"], pairs)


@pytest.mark.parametrize("batch", [7, 64])
def test_one_pass_equals_several_passes_on_a_telecined_y4m(host_stack, telecined_y4m, batch):
    path, woven, truth = telecined_y4m
    src = ingest.Y4mSource(path, wide=True, deinterlace="match")
    assert src.field_order == "tff"
    decoded = list(src.frames())
    assert all(np.array_equal(a, f.to_bgr()) for a, f in zip(decoded, matched_frames(woven)))
    _, want = run(src, decoded, truth, "change", batch, None, sub_area=CHANGE_AREA)
    with open(path, "rb") as fp:
        data = fp.read()
    pipe, th = piped(data, 65536)
    stream = ingest.Y4mStream(pipe, wide=True, deinterlace="match")
    ex, got = run(stream, decoded, truth, "change", batch, None, sub_area=CHANGE_AREA)
    th.join()
    pipe.close()
    assert ex.one_pass and got == want and ex.clamped_intervals == 0 and stream.frame_count == len(decoded) == 65
    assert [(s, e) for s, e, _r in got[0]] == FILM_32B and got[3].count(" --> ") >= 2
    src.close()


def test_extractor_command_line_matches(host_stack, telecined_y4m, capsys):
    path, woven, truth = telecined_y4m
    src = ingest.Y4mSource(path, wide=True, deinterlace="match", comb_thresh=12, comb_limit=30)
    decoded = list(src.frames())
    _, want = run(src, decoded, truth, "change", 8, None, sub_area=CHANGE_AREA)
    src.close()
    area = f"{CHANGE_AREA.ymin},{CHANGE_AREA.ymax},{CHANGE_AREA.xmin},{CHANGE_AREA.xmax}"
    common = ["--area", area, "--selector", "change", "--batch", "8"]
    for more in (["--comb-thresh", "12", "--comb-limit", "30"], ["--comb-limit", "off"], []):
        ocr = LookupOcr(decoded, truth, text_box(CHANGE_AREA))
        assert extractor.main([path, "--deinterlace", "match"] + more + common, ocr=ocr, counter=NumpyCounter()) == 0
        assert capsys.readouterr().out == want[3] and ocr.seen == want[1] and want[3].count(" --> ") >= 2


def test_command_line_argument_errors_exit_with_status_2(tmp_path, capsys):
    frames = [R.random_planes(np.random.default_rng(2), 4, 6, FMT420)]
    it, im = y4m_file(tmp_path, "It", frames, name="it.y4m"), y4m_file(tmp_path, "Im", frames, name="im.y4m")
    ocr = LookupOcr([], [], None)
    mains = ((lambda argv: extractor.main(argv, ocr=ocr, counter=NumpyCounter()), "extractor: "),
             (lambda argv: area_locator.main(argv, cells_fn=lambda *a, **k: None), "area_locator: "))
    for main, prefix in mains:
        for argv in ([it, "--deinterlace", "match", "--comb-thresh", "ten"], [it, "--deinterlace", "match", "--comb-thresh"],
                     [it, "--deinterlace", "matching"], [it, "--deinterlace", "match", "--comb-limit"]):
            with pytest.raises(SystemExit) as e:
                main(argv)
            assert e.value.code == 2
            capsys.readouterr()
        for argv, word in (([it, "--comb-thresh", "5"], "--deinterlace match"), ([it, "--deinterlace", "adaptive", "--comb-limit", "5"], "--deinterlace match"),
                           ([it, "--deinterlace", "match", "--comb-thresh", "256"], "0..255"), ([it, "--deinterlace", "match", "--comb-thresh", "-1"], "0..255"),
                           ([it, "--deinterlace", "match", "--comb-limit", "1001"], "0..1000"), ([it, "--deinterlace", "match", "--comb-limit", "never"], "0..1000"),
                           ([it, "--deinterlace", "match", "--comb-limit", "-3"], "0..1000"), ([im, "--deinterlace", "match"], "Im"),
                           ([it, "--field-order", "tff"], "--deinterlace"), ([it], "interlaced video (It) is not supported")):
            assert main(argv) == 2, argv
            err = capsys.readouterr().err
            assert err.startswith(prefix) and word in err, (argv, err)
    assert ocr.seen == []
