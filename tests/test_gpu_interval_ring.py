"""vse_interval_ring_rank on the MI355X: every patch equals the numpy restatement (tests/interval_ring_ref.py) and vse_interval_rank on
the same frames stacked contiguously, byte for byte, for every width and row padding, every bucket edge of n, the ranks at both ends
and in the middle, samples across the ring's wrap with frame numbers far beyond cap, 1, 2 and 8 groups per call with permuted patch
indices and holes; nothing outside the named patches is written and the state is not written at all; refusals touch nothing;
frame_select.EngineRingRanker under StreamingQuantile equals the numpy path; and SubtitleExtractor in one pass with the streaming
quantile on the engine equals the several-pass quantile run."""
import ctypes as C

import numpy as np
import pytest

import interval_rank_ref
import interval_ring_ref
from test_one_pass import piped

pytestmark = pytest.mark.gpu
FILL = 0xA5
FAR = 10 ** 9 + 3


def clip_frames(seed, n, h=11, w=37):
    """Random bytes with ties forced: two pixel columns in three take one of two values, so equal samples meet every rank."""
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    frames[:, :, 0::3] = rng.choice(np.array([7, 200], np.uint8), size=frames[:, :, 0::3].shape)
    frames[:, :, 1::3] = rng.choice(np.array([0, 128, 255], np.uint8), size=frames[:, :, 1::3].shape)
    return frames


class Parked:
    """`frames` (host [N,H,W,3]; row k is frame base + 1 + k) parked in a device state and in the reference ring, in batches."""

    def __init__(self, ctx, frames, area, cap, base=0, batch=64):
        import torch
        self.ctx, self.host, self.area, self.cap, self.base = ctx, frames, area, cap, base
        self.dev = torch.from_numpy(frames).to(ctx.tdev)
        y0, y1, x0, x1 = area
        self.ah, self.aw = y1 - y0, x1 - x0
        self.state = ctx.interval_stream_state(self.ah, self.aw, cap)
        self.ref = interval_ring_ref.Ring(cap)
        for k in range(0, len(frames), batch):
            ctx.interval_stream(self.dev[k:k + batch], area, self.state, cap, base + k, [], base + k + 1, "min")
            self.ref.store(frames[k:k + batch, y0:y1, x0:x1], base + k)
        self.fed = base + len(frames)
        self.before = self.state.clone()

    def window(self):
        return list(range(max(self.base + 1, self.fed - self.cap + 1), self.fed + 1))

    def check(self, groups, out=None):
        """One call -> its patches, after holding each against the reference ring and against vse_interval_rank on the stacked frames."""
        import torch
        got = self.ctx.interval_ring_rank(self.state, self.ah, self.aw, self.cap, self.fed, groups, out=out).cpu().numpy()
        want = self.ref.rank(groups, self.fed)
        for k, g in enumerate(groups):
            o = g[2] if len(g) > 2 else k
            assert got[o].dtype == np.uint8 and np.array_equal(got[o], want[o]), (self.area, self.cap, g)
            stack = torch.stack([self.dev[f - self.base - 1] for f in g[0]])
            flat = self.ctx.interval_rank(stack, self.area, g[1]).cpu().numpy()
            assert np.array_equal(got[o], flat), (self.area, self.cap, g)
        assert torch.equal(self.state, self.before), "the state was written"
        return got


@pytest.mark.parametrize("area_h", [1, 2, 9])
def test_every_width_and_row_padding(ctx, area_h):
    """area_w 1..17 at x0 0..5: 3 area_w = 3..51 bytes per row, every padding 1..15 to the slot's 16-byte rows and every short last
    dword; 12 frames through a ring of 5, so the samples 8..12 lie across the wrap (slots 3, 4, 0, 1, 2)."""
    frames = clip_frames(area_h, 12)
    pads = set()
    for area_w in range(1, 18):
        pads.add(-3 * area_w % 16)
        for x0 in range(6):
            p = Parked(ctx, frames, (1, 1 + area_h, x0, x0 + area_w), 5)
            assert p.window() == [8, 9, 10, 11, 12]
            p.check([([8, 9, 10, 11, 12], (area_w + x0) % 5), ([9, 12], x0 % 2), ([10], 0)])
    assert pads >= set(range(1, 16))


def spread(rng, window, n):
    """n frames of the window, its first and last among them (n >= 2), ascending."""
    if n == 1:
        return [int(rng.choice(window))]
    inner = rng.choice(window[1:-1], size=n - 2, replace=False).tolist() if n > 2 else []
    return sorted([window[0], window[-1]] + [int(f) for f in inner])


@pytest.mark.parametrize("base", [0, FAR])
@pytest.mark.parametrize("cap", [3, 5, 64, 70])
def test_every_bucket_edge_and_rank_across_the_wrap(ctx, cap, base):
    """75 frames pass through the ring in batches of 64 and 11, so the window of the last `cap` wraps; n at both sides of every bucket
    edge with the ranks 0, (n - 1) // 2 and n - 1; calls of 8, 2 and 1 groups that mix the buckets, patch indices permuted with holes."""
    rng = np.random.default_rng(cap)
    p = Parked(ctx, clip_frames(cap + 100, 75), (1, 10, 2, 19), cap, base)
    window = p.window()
    assert len(window) == cap and window[-1] == base + 75 and (window[0] % cap) > (window[-1] % cap)          # the window wraps
    groups = []
    for n in sorted({1, 2, 7, 8, 9, 16, 17, 32, 33, 63, min(cap, 63)}):             # (a small ring: up to all of its frames)
        if n <= cap:
            groups += [(spread(rng, window, n), r) for r in sorted({0, (n - 1) // 2, n - 1})]
    assert len(groups) >= 6
    order = rng.permutation(len(groups))
    k = 0
    for size in [8, 2, 1] * len(groups):
        part = [groups[i] for i in order[k:k + size]]
        if not part:
            break
        k += size
        outs = rng.permutation(len(part) + 3)[:len(part)]                  # permuted, with holes
        p.check([(nos, r, int(o)) for (nos, r), o in zip(part, outs)])
        p.check(part)
    # the same frames in every group: n times the same sample set at every rank gives the sorted stack
    nos = spread(rng, window, min(cap, 8))
    got = p.check([(nos, r) for r in range(len(nos))])
    y0, y1, x0, x1 = p.area
    assert np.array_equal(got, np.sort(p.host[[f - base - 1 for f in nos], y0:y1, x0:x1], axis=0))


def test_a_large_area_at_63_samples(ctx):
    """120 x 320 pixels, 28800 dwords: many blocks; 66 frames through a ring of 64."""
    rng = np.random.default_rng(63)
    p = Parked(ctx, clip_frames(63, 66, 124, 330), (2, 122, 5, 325), 64)
    window = p.window()
    p.check([(window[1:], 31), (spread(rng, window, 63), 62, 2)])


def test_only_the_named_patches_are_written(ctx):
    """Patches 4, 0 and 2 of a 6-patch buffer filled with 0xA5, with a padded pitch and a lead: the other patches, the padding, the
    rows around and the bytes beside every row stay as they were."""
    import torch
    p = Parked(ctx, clip_frames(5, 9), (2, 7, 3, 26), 7)
    ah, aw = p.ah, p.aw
    groups = [([3, 5, 9], 1, 4), ([4, 5, 6, 7, 8], 0, 0), (list(range(3, 10)), 6, 2)]
    want = p.ref.rank(groups, p.fed)
    for lead, pitch in ((5, 3 * aw + 7), (16, 3 * aw + 11), (0, 3 * aw), (1, 3 * aw + 1)):
        buf = torch.full((6, ah + 2, pitch + lead), FILL, dtype=torch.uint8, device=ctx.tdev)
        out = buf.as_strided((6, ah, aw, 3), ((ah + 2) * (pitch + lead), pitch + lead, 3, 1), pitch + lead + lead)
        assert ctx.interval_ring_rank(p.state, ah, aw, p.cap, p.fed, groups, out=out) is out
        host = buf.cpu().numpy()
        got = host[:, 1:1 + ah, lead:lead + 3 * aw].reshape(6, ah, aw, 3)
        for o in (4, 0, 2):
            assert np.array_equal(got[o], want[o]), (lead, pitch, o)
            host[o, 1:1 + ah, lead:lead + 3 * aw] = FILL
        assert (host == FILL).all(), (lead, pitch)
        assert torch.equal(p.state, p.before)
    assert np.array_equal(p.dev.cpu().numpy(), p.host)


def test_no_groups_is_no_launch(ctx):
    import torch
    p = Parked(ctx, clip_frames(1, 4), (0, 3, 0, 5), 3)
    got = ctx.interval_ring_rank(p.state, 3, 5, 3, p.fed, [])
    assert tuple(got.shape) == (0, 3, 5, 3) and torch.equal(p.state, p.before)
    out = torch.full((2, 3, 5, 3), FILL, dtype=torch.uint8, device=ctx.tdev)
    assert ctx.interval_ring_rank(p.state, 3, 5, 3, p.fed, [], out=out) is out
    assert int((out != FILL).sum()) == 0


def test_refusals_touch_nothing(ctx):
    import torch
    from vse_amd import engine
    lib = engine.load_library()
    st = torch.full((1 << 14,), FILL, dtype=torch.uint8, device=ctx.tdev)
    out = torch.full((1 << 14,), FILL, dtype=torch.uint8, device=ctx.tdev)
    assert st.data_ptr() % 16 == 0

    def call(groups=(([8, 9, 10], 1, 0),), ah=4, aw=5, cap=3, fed=10, ngroups=None, handle=True, state=True, state_at=0, d_out=True,
             out_pitch=15, n=None, pass_groups=True):
        recs = (engine.IntervalRingGroup * max(len(groups), 1))()
        for k, g in enumerate(groups):
            recs[k].n, recs[k].rank, recs[k].out = (len(g[0]) if n is None else n), g[1], g[2]
            recs[k].frames[:len(g[0])] = g[0]
        return lib.vse_interval_ring_rank(ctx.handle if handle else None, C.c_void_p(st.data_ptr() + state_at) if state else None, ah, aw,
                                          cap, fed, recs if pass_groups else None, len(groups) if ngroups is None else ngroups,
                                          C.c_void_p(out.data_ptr()) if d_out else None, out_pitch, 60, ctx.stream())

    nine = tuple(([10], 0, k) for k in range(9))
    bad = [dict(handle=False), dict(state=False), dict(state_at=8), dict(d_out=False),
           dict(ah=0), dict(aw=0), dict(ah=-1), dict(cap=0), dict(cap=-1), dict(fed=-1), dict(fed=(1 << 62) + 1, groups=()),
           dict(ngroups=-1), dict(groups=nine), dict(ngroups=9), dict(pass_groups=False),
           dict(n=0), dict(n=64), dict(n=-1), dict(groups=(([8, 9, 10], 3, 0),)), dict(groups=(([8, 9, 10], -1, 0),)),
           dict(groups=(([8, 8, 9], 1, 0),)),                                       # not strictly ascending
           dict(groups=(([9, 8, 10], 1, 0),)),                                      # descending
           dict(groups=(([7, 8, 9], 1, 0),)),                                       # frame 7 = fed - cap is behind the window
           dict(groups=(([9, 10, 11], 1, 0),)),                                     # beyond fed
           dict(groups=(([0, 1], 0, 0),), fed=2),                                   # frame 0: numbers are 1-based
           dict(groups=(([-1, 1], 0, 0),), fed=2),
           dict(groups=(([8, 9, 10], 1, 0), ([8, 9, 11], 1, 1))),                   # the second group's
           dict(groups=(([8, 9, 10], 1, -1),)), dict(out_pitch=14)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "vse_interval_ring_rank" in lib.vse_last_error().decode(), kw
    torch.cuda.synchronize()
    assert int((st != FILL).sum()) == 0 and int((out != FILL).sum()) == 0          # nothing was enqueued
    # the limits themselves are accepted: 8 groups, the window's first and last frame, no groups at all (with or without a pointer)
    assert call(groups=nine[:8]) == 0 and call(groups=(([8], 0, 0), ([10], 0, 1))) == 0 and call(groups=(([1, 2], 1, 0),), fed=2) == 0
    assert call(groups=()) == 0 and call(groups=(), pass_groups=False) == 0 and call(fed=1 << 62, groups=()) == 0
    torch.cuda.synchronize()
    assert int((st != FILL).sum()) == 0
    with pytest.raises(engine.VseError, match="groups"):
        ctx.interval_ring_rank(st, 4, 5, 3, 10, [([10], 0)] * 9)
    with pytest.raises(engine.VseError, match="frames"):
        ctx.interval_ring_rank(st, 4, 5, 70, 70, [(list(range(1, 65)), 0)])
    with pytest.raises(engine.VseError, match="vse_interval_ring_rank"):
        ctx.interval_ring_rank(st, 4, 5, 3, 10, [([7, 8], 0)])


# ---- the host side on the engine ----------------------------------------------------------------------------------------------------
def test_engine_ring_ranker_equals_the_numpy_path(ctx):
    """StreamingQuantile over EngineRingRanker against the same over NumpyRingRanker on synth.make_clip, batches of 7 (a ring that
    wraps: ring_seconds 0.5 at 12 fps) and samples 15; and the state may not change in mid-clip."""
    from frame_change_ref import NumpyCounter
    from test_one_pass import AREA, FPS, clip
    from vse_amd import frame_select
    frames, truth = clip("change")
    runs = []
    for fn in (frame_select.EngineRingRanker(ctx), interval_ring_ref.NumpyRingRanker()):
        comp = frame_select.StreamingQuantile(fn, quantile=0.5, samples=15, trim_seconds=0.1, ring_seconds=0.5, batch=7)
        sel = frame_select.ChangeFrameSelector(NumpyCounter(), batch=7, compositor=comp)
        intervals = sel.run(list(frames), AREA, fps=FPS)
        assert [(s, e) for s, e, _r in intervals] == [(s, e) for s, e, _t in truth] and comp.cap == 6 + 1 + 0 + 7 + 1 < len(frames)
        runs.append((intervals, comp.patches, comp.clamped))
    assert runs[0][0] == runs[1][0] and runs[0][2] == runs[1][2] == 0 and sorted(runs[0][1]) == sorted(runs[1][1])
    want = frame_select.IntervalQuantile(interval_rank_ref.NumpyRanker(), quantile=0.5, samples=15, trim_seconds=0.1).run(
        list(frames), AREA, runs[0][0], FPS)
    for rep in want:
        assert runs[0][1][rep].dtype == np.uint8 and np.array_equal(runs[0][1][rep], runs[1][1][rep]), rep
        assert np.array_equal(runs[0][1][rep], want[rep]), rep
    fn = frame_select.EngineRingRanker(ctx)
    band = np.zeros((2, 4, 8, 3), np.uint8)
    fn(band, (0, 4, 0, 8), 5, 0, 2, [])
    with pytest.raises(ValueError, match="EngineRingRanker"):
        fn(band, (0, 4, 0, 8), 6, 2, 2, [])


def test_one_pass_streaming_quantile_on_engine(ctx, tmp_path):
    """The clip of test_gpu_one_pass (real detector, stand-in recogniser, drop_score 0, batch 8) as a Y4M file: one pass over a pipe with
    the streaming quantile against several passes with the quantile's own pass: equal patches, intervals, raw.txt lines and SRT."""
    from oracle import net_ref, pipeline_ref as P
    from test_gpu_interval_stream import PlainOcr
    from vse_amd import extractor, frame_select, ingest, pipeline, staging, synth
    pipe_ocr = pipeline.OcrPipeline(ctx, net_ref.get_weights("V3_ch_det_fast"), net_ref.get_weights("V4_en_rec_fast"), P.en_charset(),
                                    rec_mode="reference")
    h, w = 360, 640
    frames, truth = synth.make_clip([(None, 3), ("the quick brown fox", 9), ("seven wizards quietly box", 7), (None, 4),
                                     ("near frozen lakes", 8), (None, 2)], h, w, seed=6)
    kw = dict(sub_area=extractor.SubtitleArea(ymin=int(0.75 * h), ymax=h, xmin=0, xmax=w), frame_selector="change", interval_image="quantile")
    path = str(tmp_path / "clip.y4m")
    ingest.write_y4m(path, [ingest.bgr_to_yuv420(f) for f in frames], 12)
    src = ingest.Y4mSource(path)
    with open(path, "rb") as fp:
        data = fp.read()
    up = staging.Uploader(ctx.tdev, ctx=ctx)
    runs = []
    try:
        for one_pass in (False, True):
            fp, th = piped(data, 1 << 16) if one_pass else (None, None)
            source = ingest.Y4mStream(fp) if one_pass else src
            params = ({"streaming": True, "keep_patches": True, "samples": 5, "ring_seconds": 60,
                       "ring_fn": frame_select.EngineRingRanker(ctx)} if one_pass
                      else {"samples": 5, "rank_fn": frame_select.EngineRanker(ctx)})
            ocr = PlainOcr(pipe_ocr)
            ex = extractor.SubtitleExtractor(source, ocr, mode="auto", drop_score=0.0, batch=8, uploader=up,
                                             change_counter=frame_select.EngineCounter(ctx), composite_params=params, **kw)
            assert ex.one_pass == one_pass
            text = ex.run()
            runs.append((ex.intervals, ex.raw_lines, text, ex.interval_patches, ocr.frames))
            if one_pass:
                th.join()
                fp.close()
                assert ex.clamped_intervals == 0 and ex.clamped_quantiles == 0 and 0 < ex.peak_retained < len(frames)
    finally:
        up.close()
        src.close()
    for k, what in enumerate(("intervals", "raw_lines", "SRT")):
        assert runs[0][k] == runs[1][k], what
    assert [(s, e) for s, e, _r in runs[1][0]] == [(s, e) for s, e, _t in truth] and runs[0][4] == runs[1][4] == len(truth)
    want, got = runs[0][3], runs[1][3]
    assert sorted(got) == sorted(want) == [(s + e) // 2 for s, e, _t in truth]
    decoded = np.stack(list(ingest.Y4mSource(path).frames()))
    for (s, e, _t), rep in zip(truth, sorted(want)):
        nos, _pos = frame_select.fuse_samples(s, e, rep, 12, 5, 0.25)
        ref = interval_rank_ref.rank(decoded[[f - 1 for f in nos]], (int(0.75 * h), h, 0, w), frame_select.quantile_rank(0.5, len(nos)))
        assert got[rep].dtype == np.uint8 and np.array_equal(got[rep], want[rep]) and np.array_equal(got[rep], ref), rep
