"""vse_interval_stream on the MI355X: every patch equals the numpy restatement (tests/interval_stream_ref.py) byte for byte, for every
width and byte alignment, through the 16-byte and the general loads, with segments in the ring, in the batch and across both, slots
reused, stores that replace what the same call reads, CONTINUE across calls, n = 0 calls and a batch passed twice; nothing outside the
patches and the state is written; refusals touch nothing; and SubtitleExtractor in one pass with the streaming composite on the engine
equals the several-pass composite run."""
import ctypes as C

import numpy as np
import pytest

import interval_ref
import interval_stream_ref
from interval_stream_ref import CONTINUE, EMIT
from test_gpu_interval_composite import padded_view
from test_one_pass import piped

pytestmark = pytest.mark.gpu
MODES = interval_ref.MODES
FILL = 0xA5


def run_both(ctx, dev, host, area, cap, calls, mode, state=None):
    """calls: [(fed, n, segs, store_from)] on the frames dev / host [N,H,W,3] (frame f is row f - 1), through one device state and one
    reference Stream -> the patches of every call; each call's are compared as it returns."""
    y0, y1, x0, x1 = area
    state = ctx.interval_stream_state(y1 - y0, x1 - x0, cap) if state is None else state
    ref = interval_stream_ref.Stream(cap)
    outs = []
    for fed, n, segs, store_from in calls:
        got = ctx.interval_stream(dev[fed:fed + n], area, state, cap, fed, segs, store_from, mode).cpu().numpy()
        want = ref.stream(host[fed:fed + n], area, fed, segs, store_from, mode)
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), (area, cap, mode, fed, n, segs)
        outs.append(got)
    return outs, ref, state


def ring_rows(ctx, state, area, cap):
    """The ring of a state as the header lays it out: cap slots of area_h rows padded to 16 bytes, behind 6 such planes -> uint8
    [cap, area_h, 3 area_w] (the area's bytes of every slot)."""
    y0, y1, x0, x1 = area
    ah, rb = y1 - y0, 3 * (x1 - x0)
    rb16 = -(-rb // 16) * 16
    assert ctx.lib.vse_interval_stream_state_bytes(ah, x1 - x0, cap) == ah * rb16 * (6 + cap)
    host = state.cpu().numpy()
    return host[6 * ah * rb16:(6 + cap) * ah * rb16].reshape(cap, ah, rb16)[:, :, :rb]


# a clip of five frames through a ring of three: ring only, across ring and batch, batch only, an open fold that a later call continues
FIVE = [(0, 3, [(1, 2, EMIT, 2)], 2),
        (3, 2, [(2, 3, EMIT, 2), (4, 4, 0, 0)], 4),
        (5, 0, [(5, 5, CONTINUE | EMIT, 2)], 6)]


@pytest.mark.parametrize("area_h", [1, 2, 9])
def test_every_width_and_alignment(ctx, area_h):
    """area_w 1..17 at x0 0..5 on 11 x 37 frames (pitch 111: every row starts on another residue), packed and in a padded view."""
    import torch
    frames = np.random.default_rng(area_h).integers(0, 256, size=(5, 11, 37, 3), dtype=np.uint8)
    packed = torch.from_numpy(frames).to(ctx.tdev)
    padded = padded_view(ctx, frames, 5, 3, 2)
    for area_w in range(1, 18):
        for x0 in range(6):
            area = (1, 1 + area_h, x0, x0 + area_w)
            mode = MODES[(area_w + x0) % 3]
            run_both(ctx, packed, frames, area, 3, FIVE, mode)
            run_both(ctx, padded, frames, area, 3, FIVE, mode)


@pytest.mark.parametrize("x0, area_w", [(0, 64), (16, 37), (0, 63), (32, 32)])
def test_wide_loads_equal_general_loads(ctx, x0, area_w):
    """16-byte aligned base, pitch and stride with 3 x0 a multiple of 16: the 16-byte loads; the same pixels 3 bytes further: the general ones."""
    import torch
    n, h, w = 11, 6, 64
    frames = np.random.default_rng(x0 + area_w).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    area = (0, h, x0, x0 + area_w)
    aligned = torch.from_numpy(frames).to(ctx.tdev)
    assert aligned.data_ptr() % 16 == 0 and aligned.stride(1) % 16 == 0 and aligned.stride(0) % 16 == 0 and 3 * x0 % 16 == 0
    flat = torch.zeros(frames.size + 16, dtype=torch.uint8, device=ctx.tdev)
    shifted = flat[3:3 + frames.size].view(n, h, w, 3)
    shifted.copy_(aligned)
    assert shifted.data_ptr() % 16 == 3
    calls = [(0, 4, [(1, 1, EMIT, 1), (2, 3, EMIT, 2)], 3),
             (4, 7, [(3, 9, EMIT, 7), (10, 11, 0, 0)], 9),
             (11, 0, [], 12)]
    for mode in MODES:
        a, _, _ = run_both(ctx, aligned, frames, area, 4, calls, mode)
        b, _, _ = run_both(ctx, shifted, frames, area, 4, calls, mode)
        assert all(np.array_equal(p, q) for p, q in zip(a, b))
        st = interval_ref.accumulate(None, frames[2:9], area)
        assert np.array_equal(a[1][0], interval_ref.composite(st, 7, mode))


@pytest.mark.parametrize("cap", [1, 3, 8])
def test_slots_are_reused(ctx, cap):
    """30 frames in batches of 4, everything stored: the ring always holds the last `cap` frames, whose numbers pass several multiples
    of cap; every call reads all of them and its own batch."""
    import torch
    frames = np.random.default_rng(cap).integers(0, 256, size=(30, 5, 21, 3), dtype=np.uint8)
    dev = torch.from_numpy(frames).to(ctx.tdev)
    area = (1, 5, 2, 19)
    calls = []
    for fed in range(0, 30, 4):
        n = min(4, 30 - fed)
        first = max(1, fed - cap + 1)
        calls.append((fed, n, [(first, fed + n, EMIT, fed + n - first + 1)], 0))
    calls.append((30, 0, [(31 - cap, 30, EMIT, cap)], 31))
    _, ref, state = run_both(ctx, dev, frames, area, cap, calls, "mean")
    ring = ring_rows(ctx, state, area, cap)
    for slot, (f, pixels) in ref.ring.items():
        assert f > 30 - cap and np.array_equal(ring[slot], pixels.reshape(4, -1)), (cap, slot, f)


@pytest.mark.parametrize("aligned", [True, False])
def test_a_clip_fed_in_pieces(ctx, aligned):
    """75 frames as 1 + 7 + 64 + 3: one fold CONTINUEd through the four calls equals the composite of the whole."""
    import torch
    n, h, w = 75, 5, 48 if aligned else 45
    frames = np.random.default_rng(75).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    area = (1, 4, 0, w) if aligned else (1, 4, 2, 43)
    dev = torch.from_numpy(frames).to(ctx.tdev)
    whole = interval_ref.accumulate(None, frames, area)
    for mode in MODES:
        calls = [(0, 1, [(1, 1, 0, 0)], 2), (1, 7, [(2, 8, CONTINUE, 0)], 9), (8, 64, [(9, 72, CONTINUE, 0)], 73),
                 (72, 3, [(73, 75, CONTINUE | EMIT, 75)], 76)]
        outs, _, _ = run_both(ctx, dev, frames, area, 2, calls, mode)
        assert np.array_equal(outs[3][0], interval_ref.composite(whole, 75, mode)), mode


def test_three_emits_and_an_open_fold_in_one_call(ctx):
    """Ring of 8: a segment in the ring only, one across ring and batch, one in the batch only, then the open fold, which the next call
    CONTINUEs and EMITs."""
    import torch
    frames = np.random.default_rng(13).integers(0, 256, size=(13, 6, 40, 3), dtype=np.uint8)
    dev = torch.from_numpy(frames).to(ctx.tdev)
    area = (0, 6, 3, 38)
    calls = [(0, 6, [], 1),
             (6, 5, [(2, 4, EMIT, 3), (5, 8, EMIT, 4), (9, 10, EMIT, 2), (11, 11, 0, 0)], 12),
             (11, 2, [(12, 13, CONTINUE | EMIT, 3)], 14)]
    for mode in MODES:
        outs, _, _ = run_both(ctx, dev, frames, area, 8, calls, mode)
        assert outs[1].shape[0] == 3 and outs[2].shape[0] == 1
        assert np.array_equal(outs[2][0], interval_ref.composite(interval_ref.accumulate(None, frames[10:13], area), 3, mode))


def test_sums_past_sixteen_bits(ctx):
    """CONTINUE across four calls of 75 frames of 255 (and of random bright bytes) on a 3 x 5 area: the sums pass 65535."""
    import torch
    area = (0, 3, 0, 5)
    for frames in (np.full((300, 3, 5, 3), 255, np.uint8), np.random.default_rng(1).integers(200, 256, size=(300, 3, 5, 3), dtype=np.uint8)):
        dev = torch.from_numpy(frames).to(ctx.tdev)
        calls = [(k * 75, 75, [(k * 75 + 1, k * 75 + 75, (CONTINUE if k else 0) | (EMIT if k == 3 else 0), 300)], 301) for k in range(4)]
        outs, _, _ = run_both(ctx, dev, frames, area, 1, calls, "mean")
        sm = frames.astype(np.int64).sum(0)
        assert sm.min() > 65535 and np.array_equal(outs[3][0], (2 * sm + 300) // 600)
    assert (outs[3][0] >= 200).all()


def test_store_from_none_some_all_and_the_state_canary(ctx):
    """Ring of 8 in a state with a canary behind it: a batch stored whole, one not at all (the ring keeps the first), one in part; the
    ring's bytes are the reference's slot by slot, slots never stored keep their fill, and the bytes behind the state theirs."""
    import torch
    frames = np.random.default_rng(8).integers(0, 256, size=(12, 4, 23, 3), dtype=np.uint8)
    dev = torch.from_numpy(frames).to(ctx.tdev)
    area = (0, 4, 1, 22)
    nbytes = ctx.lib.vse_interval_stream_state_bytes(4, 21, 8)
    state = torch.full((nbytes + 256,), 0xC3, dtype=torch.uint8, device=ctx.tdev)
    calls = [(0, 4, [], -5),                                        # all of frames 1..4
             (4, 4, [], 9),                                         # none of 5..8
             (8, 0, [(1, 4, EMIT, 4)], 9),                          # the first batch is still there
             (8, 4, [(3, 4, EMIT, 2)], 11),                         # 11 and 12 replace 3 and 4, which this call reads first
             (12, 0, [(11, 12, EMIT, 2)], 13)]
    _, ref, state = run_both(ctx, dev, frames, area, 8, calls, "min", state=state)
    ring = ring_rows(ctx, state[:nbytes], area, 8)
    assert sorted(f for f, _p in ref.ring.values()) == [1, 2, 11, 12]
    for slot in range(8):
        if slot in ref.ring:
            assert np.array_equal(ring[slot], ref.ring[slot][1].reshape(4, -1)), slot
        else:
            assert (ring[slot] == 0xC3).all(), slot
    assert bool((state[nbytes:] == 0xC3).all())
    assert np.array_equal(dev.cpu().numpy(), frames)                # the input is read only


def test_a_store_replaces_what_the_call_reads(ctx):
    """Ring of 2: frames 3 and 4 go where 1 and 2 are, in the call whose segment reads 1..4."""
    import torch
    frames = np.random.default_rng(4).integers(0, 256, size=(4, 3, 18, 3), dtype=np.uint8)
    dev = torch.from_numpy(frames).to(ctx.tdev)
    area = (0, 3, 0, 18)
    for mode in MODES:
        outs, _, _ = run_both(ctx, dev, frames, area, 2, [(0, 2, [], 1), (2, 2, [(1, 4, EMIT, 4)], 3), (4, 0, [(3, 4, EMIT, 2)], 5)], mode)
        assert np.array_equal(outs[1][0], interval_ref.composite(interval_ref.accumulate(None, frames, area), 4, mode))


def test_the_same_batch_twice(ctx):
    """A batch passed with some segments and no store, then again with the rest and the stores, then that call once more: equal patches,
    an equal ring."""
    import torch
    frames = np.random.default_rng(6).integers(0, 256, size=(9, 4, 30, 3), dtype=np.uint8)
    dev = torch.from_numpy(frames).to(ctx.tdev)
    area = (1, 4, 4, 27)
    last = (3, 6, [(6, 7, EMIT, 2), (8, 9, EMIT, 2)], 7)
    calls = [(0, 3, [], 2), (3, 6, [(2, 3, EMIT, 2), (4, 5, EMIT, 2)], 10), last, last, (9, 0, [(7, 9, EMIT, 3)], 10)]
    outs, ref, state = run_both(ctx, dev, frames, area, 4, calls, "max")
    assert np.array_equal(outs[2], outs[3])
    ring = ring_rows(ctx, state, area, 4)
    assert all(np.array_equal(ring[slot], pixels.reshape(3, -1)) for slot, (_f, pixels) in ref.ring.items())


def test_mean_rounds_halves_up(ctx):
    import torch
    a = np.arange(255, dtype=np.uint8).reshape(1, 85, 3)
    four = np.stack([a, a + 1, a + 1, a])                            # sm = 4 a + 2: the mean is a + 1/2
    dev = torch.from_numpy(four).to(ctx.tdev)
    area = (0, 1, 0, 85)
    outs, _, _ = run_both(ctx, dev, four, area, 2, [(0, 2, [(1, 2, EMIT, 2)], 1), (2, 2, [(1, 4, EMIT, 4)], 5)], "mean")
    assert np.array_equal(outs[0][0], a + 1) and np.array_equal(outs[1][0], a + 1)


def test_writes_only_the_patches(ctx):
    """Patches in a buffer of canaries: rows longer than 3 area_w, patches further apart than their rows, a lead in front; explicit `out`
    numbers in another order than the segments."""
    import torch
    frames = np.random.default_rng(2).integers(0, 256, size=(6, 7, 29, 3), dtype=np.uint8)
    dev = torch.from_numpy(frames).to(ctx.tdev)
    area = (2, 7, 3, 26)
    ah, aw = 5, 23
    segs = [(1, 2, EMIT, 2, 2), (3, 5, EMIT, 3, 0), (6, 6, EMIT, 1, 1)]
    for lead, pitch in ((5, 3 * aw + 7), (16, 3 * aw + 11), (0, 3 * aw)):
        for mode in MODES:
            want = interval_stream_ref.Stream(2).stream(frames, area, 0, segs, 7, mode)
            buf = torch.full((3, ah + 2, pitch + lead), FILL, dtype=torch.uint8, device=ctx.tdev)
            out = buf.as_strided((3, ah, aw, 3), ((ah + 2) * (pitch + lead), pitch + lead, 3, 1), pitch + lead + lead)
            state = ctx.interval_stream_state(ah, aw, 2)
            assert ctx.interval_stream(dev, area, state, 2, 0, segs, 7, mode, out=out) is out
            host = buf.cpu().numpy()
            got = host[:, 1:1 + ah, lead:lead + 3 * aw].reshape(3, ah, aw, 3)
            assert np.array_equal(got, want), (lead, pitch, mode)
            host[:, 1:1 + ah, lead:lead + 3 * aw] = FILL
            assert (host == FILL).all(), (lead, pitch, mode)
    assert np.array_equal(dev.cpu().numpy(), frames)


def test_refusals_touch_nothing(ctx):
    import torch
    from vse_amd import engine
    lib = engine.load_library()
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=ctx.tdev)                    # far larger than any of the frames below
    st = torch.full((1 << 14,), FILL, dtype=torch.uint8, device=ctx.tdev)
    out = torch.full((1 << 14,), FILL, dtype=torch.uint8, device=ctx.tdev)

    def call(segs=((1, 2, EMIT, 2, 0),), n=4, h=10, w=20, pitch=60, fstride=600, y0=0, y1=10, x0=0, x1=20, cap=3, fed=0, nseg=None, store_from=1,
             mode=0, d_out=True, out_pitch=60, state_at=0, d_bgr=True):
        recs = (engine.IntervalSeg * max(len(segs), 1))(*[engine.IntervalSeg(*g) for g in segs])
        return lib.vse_interval_stream(ctx.handle, C.c_void_p(buf.data_ptr()) if d_bgr else None, n, h, w, pitch, fstride, y0, y1, x0, x1,
                                       C.c_void_p(st.data_ptr() + state_at), cap, fed, recs, len(segs) if nseg is None else nseg, store_from,
                                       mode, C.c_void_p(out.data_ptr()) if d_out else None, out_pitch, 600, ctx.stream())

    many = tuple((k + 1, k + 1, EMIT, 1, 0) for k in range(33))
    bad = [dict(y0=4, y1=4), dict(x0=7, x1=7), dict(y0=5, y1=3), dict(y0=-1), dict(x0=-1), dict(y1=11), dict(x1=21),      # empty / outside
           dict(n=-1), dict(n=65536), dict(pitch=59), dict(fstride=599), dict(d_bgr=False),                                 # frames, pitch, stride
           dict(cap=0), dict(cap=-1), dict(fed=-1), dict(fed=(1 << 62) + 1, n=0, segs=()), dict(nseg=-1), dict(segs=many, n=40, fstride=600), dict(nseg=33),
           dict(segs=((2, 1, EMIT, 1, 0),)),                                    # first > last
           dict(segs=((1, 2, EMIT, 2, 0), (2, 3, EMIT, 2, 1))),                 # overlap
           dict(segs=((3, 4, EMIT, 2, 0), (1, 2, EMIT, 2, 1))),                 # unordered
           dict(segs=((1, 5, EMIT, 5, 0),)),                                    # beyond fed + n
           dict(segs=((2, 4, EMIT, 3, 0),), fed=5, n=0),                        # frame 2 = fed - cap is behind the window
           dict(segs=((0, 1, EMIT, 2, 0),)),                                    # frame 0: numbers are 1-based
           dict(segs=((1, 1, EMIT, 1, 0), (2, 2, CONTINUE | EMIT, 2, 1))),      # CONTINUE on the second
           dict(segs=((1, 1, 0, 0, 0), (2, 2, EMIT, 1, 0))),                    # no EMIT, and not the last
           dict(segs=((1, 1, 4 | EMIT, 1, 0),)),                                # an unknown flag
           dict(mode=3), dict(mode=-1), dict(mode=2, segs=((1, 2, EMIT, 0, 0),)), dict(mode=2, segs=((1, 2, EMIT, 4194305, 0),)),
           dict(out_pitch=59), dict(d_out=False), dict(segs=((1, 2, EMIT, 2, -1),)), dict(state_at=8)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "vse_interval_stream" in lib.vse_last_error().decode(), kw
    torch.cuda.synchronize()
    assert int((st != FILL).sum()) == 0 and int((out != FILL).sum()) == 0 and int(buf.sum()) == 0      # nothing was enqueued
    assert lib.vse_interval_stream_state_bytes(0, 5, 3) == 0 and lib.vse_interval_stream_state_bytes(5, 0, 3) == 0
    assert lib.vse_interval_stream_state_bytes(2, 5, 0) == 0 and lib.vse_interval_stream_state_bytes(2, 5, -1) == 0
    assert lib.vse_interval_stream_state_bytes(2, 5, 3) == 2 * 16 * 9 and lib.vse_interval_stream_state_bytes(3, 16, 1) == 3 * 48 * 7
    # the limits themselves are accepted: 32 segments, the window's first frame, frames 2^22, n = 0 without frames, no EMIT without d_out
    assert call(segs=many[:32], n=40) == 0 and call(segs=((3, 5, EMIT, 3, 0),), fed=5, n=0, d_bgr=False) == 0
    assert call(mode=2, segs=((1, 2, EMIT, 4194304, 0),)) == 0 and call(segs=((1, 2, 0, 0, 0),), d_out=False) == 0
    assert call(segs=(), n=0, d_bgr=False) == 0 and call(segs=(), store_from=5) == 0
    torch.cuda.synchronize()
    with pytest.raises(engine.VseError, match="mode"):
        ctx.interval_stream(buf[:600].view(1, 10, 20, 3), (0, 10, 0, 20), st, 3, 0, [], 1, "median")
    with pytest.raises(engine.VseError):
        ctx.interval_stream_state(4, 5, 0)


# ---- the extractor ----------------------------------------------------------------------------------------------------------------
class PlainOcr:
    """The engine's recogniser on staged device batches."""

    def __init__(self, pipe):
        self.pipe, self.frames = pipe, 0

    def predict_batch(self, frames):
        import torch
        from vse_amd import shim
        assert torch.is_tensor(frames) and frames.dtype == torch.uint8 and frames.is_cuda
        self.frames += len(frames)
        return [shim.OcrRecogniser.arrange(b, r) for b, r in self.pipe.ocr(frames)]

    def predict(self, frame):
        import torch
        return self.predict_batch(torch.from_numpy(np.ascontiguousarray(frame)).cuda()[None])[0]


def test_one_pass_streaming_composite_on_engine(ctx, tmp_path):
    """The clip of test_gpu_one_pass (real detector, stand-in recogniser, drop_score 0, batch 8) as a Y4M file: one pass over a pipe with
    the streaming composite against several passes with the compositor's own pass: equal patches, intervals, raw.txt lines and SRT."""
    from oracle import net_ref, pipeline_ref as P
    from vse_amd import extractor, frame_select, ingest, pipeline, staging, synth
    pipe_ocr = pipeline.OcrPipeline(ctx, net_ref.get_weights("V3_ch_det_fast"), net_ref.get_weights("V4_en_rec_fast"), P.en_charset(),
                                    rec_mode="reference")
    h, w = 360, 640
    frames, truth = synth.make_clip([(None, 3), ("the quick brown fox", 9), ("seven wizards quietly box", 7), (None, 4),
                                     ("near frozen lakes", 8), (None, 2)], h, w, seed=6)
    kw = dict(sub_area=extractor.SubtitleArea(ymin=int(0.75 * h), ymax=h, xmin=0, xmax=w), frame_selector="change", interval_image="min")
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
            params = ({"streaming": True, "keep_patches": True, "stream_fn": frame_select.EngineStreamer(ctx)} if one_pass
                      else {"accumulate_fn": frame_select.EngineCompositor(ctx)})
            ocr = PlainOcr(pipe_ocr)
            ex = extractor.SubtitleExtractor(source, ocr, mode="auto", drop_score=0.0, batch=8, uploader=up,
                                             change_counter=frame_select.EngineCounter(ctx), composite_params=params, **kw)
            assert ex.one_pass == one_pass
            text = ex.run()
            runs.append((ex.intervals, ex.raw_lines, text, ex.interval_patches, ocr.frames))
            if one_pass:
                th.join()
                fp.close()
                assert ex.clamped_intervals == 0 and 0 < ex.peak_retained < len(frames)
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
        first, last = interval_ref.trim_range(s, e, 12, 0.25)
        ref = interval_ref.composite(interval_ref.accumulate(None, decoded[first - 1:last], (int(0.75 * h), h, 0, w)), last - first + 1, "min")
        assert got[rep].dtype == np.uint8 and np.array_equal(got[rep], want[rep]) and np.array_equal(got[rep], ref), rep
