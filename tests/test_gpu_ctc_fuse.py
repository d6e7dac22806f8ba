"""vse_ctc_fuse on the MI355X, through the C ABI: idx and maxp equal the numpy restatement (tests/ctc_fuse_ref.py) bit for bit for every
dictionary size, step count, row stride and base alignment, through the 16-byte and the dword loads alike; refusals launch nothing; a
malformed device table cannot reach outside the probabilities; and OcrPipeline.recognize_fused / SubtitleExtractor(interval_text="fused")
on top of it: identical frames give recognize()'s result exactly, the fused rows are the reference applied to the members' own
probabilities, and the members' probabilities do not depend on the batch they ride in."""
import ctypes as C

import numpy as np
import pytest

import ctc_fuse_ref
from oracle import net_ref
from oracle import pipeline_ref as P

pytestmark = pytest.mark.gpu

KS = (1, 2, 3, 5, 64)                                  # the groups of one call
GROUP = [0, 1, 3, 6, 11, 75]
assert [b - a for a, b in zip(GROUP, GROUP[1:])] == list(KS)


def call_fuse(ctx, probs_dev, b, t, ncls, stride, group_dev, g, tlen_dev, out_dev):
    from vse_amd import engine
    return engine.load_library().vse_ctc_fuse(ctx.handle, C.c_void_p(probs_dev.data_ptr()) if probs_dev is not None else None, b, t, ncls, stride,
                                              C.c_void_p(group_dev.data_ptr()) if group_dev is not None else None, g,
                                              C.c_void_p(tlen_dev.data_ptr()) if tlen_dev is not None else None,
                                              C.c_void_p(out_dev.data_ptr()) if out_dev is not None else None, ctx.stream())


def laid_out(ctx, probs, stride, lead, fill=np.nan):
    """probs float32 [B,T,ncls] in a device buffer with `stride` floats per (row, step) row, starting `lead` floats into a 16-byte aligned
    allocation; the gaps hold `fill` -> (the buffer, the view that starts at the first row)."""
    import torch
    b, t, ncls = probs.shape
    host = np.full(lead + b * t * stride + 8, fill, np.float32)
    host[lead:lead + b * t * stride].reshape(b * t, stride)[:, :ncls] = probs.reshape(b * t, ncls)
    buf = torch.from_numpy(host).to(ctx.tdev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[lead:]


def same(out_dev, want_idx, want_maxp, what):
    got = out_dev.cpu().numpy().view(np.int32)
    assert np.array_equal(got[..., 0], want_idx), what
    assert np.array_equal(got[..., 1], want_maxp.view(np.int32)), what


@pytest.mark.parametrize("t", [1, 5, 40])
@pytest.mark.parametrize("ncls", [1, 2, 97, 6625])
def test_kernel_equals_the_reference(ctx, ncls, t):
    """One call with groups of 1, 2, 3, 5 and 64 rows; row_stride ncls and ncls + 3; the base 16-byte aligned and 4 bytes behind that
    (with an odd ncls no row but the first is aligned then).  97 and 6625 are odd: with row_stride = ncls every fourth row takes the
    16-byte loads, the others the dword loads; ncls + 3 = 100 and 6628 make every row aligned.  Three groups end before t, and what
    lies behind their lengths, and in every gap, is NaN."""
    import torch
    rng = np.random.default_rng([ncls, t])
    b, g = GROUP[-1], len(KS)
    probs = rng.random((b, t, ncls), dtype=np.float32) + np.float32(1e-3)
    probs /= probs.sum(-1, keepdims=True, dtype=np.float32)
    tlen = np.array([t, max(t - 1, 0), t // 2, t, t - t // 3], np.int32)
    want_full = ctc_fuse_ref.fuse(probs, GROUP)
    want_short = ctc_fuse_ref.fuse(probs, GROUP, tlen)
    masked = probs.copy()
    for j in range(g):
        masked[GROUP[j]:GROUP[j + 1], tlen[j]:] = np.nan
    group_dev = torch.tensor(GROUP, dtype=torch.int32, device=ctx.tdev)
    tlen_dev = torch.from_numpy(tlen).to(ctx.tdev)
    for stride in (ncls, ncls + 3):
        for lead in (0, 1):
            what = (ncls, t, stride, lead)
            _buf, view = laid_out(ctx, probs, stride, lead)
            out = torch.full((g, t, 2), -7.0, dtype=torch.float32, device=ctx.tdev)
            assert call_fuse(ctx, view, b, t, ncls, stride, group_dev, g, None, out) == 0, what
            same(out, *want_full, what)
            _buf, view = laid_out(ctx, masked, stride, lead)
            out.fill_(-7.0)
            assert call_fuse(ctx, view, b, t, ncls, stride, group_dev, g, tlen_dev, out) == 0, what
            same(out, *want_short, what)
    if t > 1:
        assert not want_short[0][2, t // 2:].any() and not want_short[1][2, t // 2:].any()


def test_larger_dictionaries_loop_over_chunks(ctx):
    """ncls 7169 and 20000: one class and several chunks beyond the 7168 classes a block holds in registers at a time; the winner is
    planted in the last class, in the first class of the second chunk and in the last class of the first."""
    import torch
    for ncls in (7169, 20000):
        rng = np.random.default_rng(ncls)
        probs = rng.random((5, 3, ncls), dtype=np.float32) * np.float32(0.5)
        for s, c in enumerate((ncls - 1, 7168, 7167)):
            probs[:, s, c] = 0.75
        group = [0, 2, 5]
        want = ctc_fuse_ref.fuse(probs, group)
        assert want[0].tolist() == [[ncls - 1, 7168, 7167]] * 2
        for stride, lead in ((ncls, 0), ((ncls + 4) & ~3, 0), (ncls, 1)):
            _buf, view = laid_out(ctx, probs, stride, lead)
            out = torch.zeros((2, 3, 2), dtype=torch.float32, device=ctx.tdev)
            assert call_fuse(ctx, view, 5, 3, ncls, stride, torch.tensor(group, dtype=torch.int32, device=ctx.tdev), 2, None, out) == 0
            same(out, *want, (ncls, stride, lead))


@pytest.mark.parametrize("ncls, lo, hi", [(8, 2, 5), (6625, 1030, 6001), (6625, 4, 6624), (99, 3, 98)])
def test_equal_means_take_the_smaller_index(ctx, ncls, lo, hi):
    """Dyadic probabilities: classes lo < hi reach exactly the same mean from different member values (K = 2: 0.25 + 0.5 and 0.5 + 0.25;
    K = 3: 0.125 + 0.25 + 0.375 and three times 0.25), everything else is smaller.  lo and hi sit in different threads, waves and, in
    the 16-byte layout (the stride rounded up to a multiple of four floats aligns every row), in the slot behind the last whole vector
    (6624 of 6625, 98 of 99)."""
    import torch
    probs = np.full((5, 2, ncls), np.float32(1 / 64), np.float32)
    probs[0, :, lo], probs[1, :, lo] = 0.25, 0.5
    probs[0, :, hi], probs[1, :, hi] = 0.5, 0.25
    probs[2:5, :, hi] = 0.25
    probs[2, :, lo], probs[3, :, lo], probs[4, :, lo] = 0.125, 0.25, 0.375
    group = [0, 2, 5]
    want = ctc_fuse_ref.fuse(probs, group)
    assert (want[0] == lo).all() and want[1][0].tolist() == [0.375] * 2 and want[1][1].tolist() == [0.25] * 2
    flipped = probs.copy()                                   # the same with the larger index first in memory order of the members
    flipped[:, :, [lo, hi]] = probs[:, :, [hi, lo]]
    assert (ctc_fuse_ref.fuse(flipped, group)[0] == lo).all()
    for data in (probs, flipped):
        for stride, lead in ((ncls, 0), (ncls, 1), ((ncls + 3) & ~3, 0)):
            _buf, view = laid_out(ctx, data, stride, lead)
            out = torch.zeros((2, 2, 2), dtype=torch.float32, device=ctx.tdev)
            assert call_fuse(ctx, view, 5, 2, ncls, stride, torch.tensor(group, dtype=torch.int32, device=ctx.tdev), 2, None, out) == 0
            same(out, *want, (ncls, stride, lead))


def test_refusals_launch_nothing(ctx):
    import torch
    from vse_amd import engine
    lib = engine.load_library()
    probs = torch.full((4 * 3 * 10,), 0.1, dtype=torch.float32, device=ctx.tdev)
    group = torch.tensor([0, 2, 4], dtype=torch.int32, device=ctx.tdev)
    out = torch.full((2, 3, 2), -7.0, dtype=torch.float32, device=ctx.tdev)
    ok = dict(probs_dev=probs, b=4, t=3, ncls=10, stride=10, group_dev=group, g=2, tlen_dev=None, out_dev=out)
    for kw in (dict(probs_dev=None), dict(group_dev=None), dict(out_dev=None), dict(b=0), dict(t=0), dict(ncls=0), dict(g=0), dict(b=-1),
               dict(g=-2), dict(stride=9), dict(stride=0), dict(stride=-10)):
        assert call_fuse(ctx, **{**ok, **kw}) == -1, kw
        assert "vse_ctc_fuse" in lib.vse_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                                                       # nothing was enqueued
    assert call_fuse(ctx, **ok) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got.view(np.int32)[..., 0] == 0).all() and (got[..., 1] == np.float32(0.1)).all()


def test_context_checks_the_table(ctx):
    import torch
    from vse_amd import engine
    rng = np.random.default_rng(1)
    probs = rng.random((70, 1, 4, 9), dtype=np.float32)
    dev = torch.from_numpy(probs).to(ctx.tdev)
    for bad in ([0], [0, 0], [0, 3, 3], [3, 2], [-1, 2], [0, 71], [0, 65], [2, 1, 5]):
        with pytest.raises(engine.VseError):
            ctx.ctc_fuse(dev, bad)
    tlen = torch.tensor([4, 2, 0], dtype=torch.int32, device=ctx.tdev)
    got = ctx.ctc_fuse(dev, [1, 2, 6, 70], tlen)                                           # 1, 4 and 64 rows; it need not start at row 0
    assert tuple(got.shape) == (3, 1, 4, 2) and got.dtype == torch.float32
    same(got[:, 0], *ctc_fuse_ref.fuse(probs[:, 0], [1, 2, 6, 70], [4, 2, 0]), "Context.ctc_fuse")
    idx, ln, conf = (x.cpu().numpy() for x in ctx.ctc_collapse(got, tlen))                 # ... and decodes with the existing collapse
    for j in range(3):
        want_idx, want_maxp = (a[j] for a in ctc_fuse_ref.fuse(probs[:, 0], [1, 2, 6, 70], [4, 2, 0]))
        ids, _ = ctc_fuse_ref.ctc_greedy(want_idx, want_maxp, int(tlen[j]))
        assert idx[j, :ln[j]].tolist() == ids


def test_malformed_table_stays_inside_the_probabilities(ctx):
    """The library cannot check a device table: offsets beyond b, a group of 0 rows and one of 100 rows are clamped by the kernel.  The
    call only has to complete; the probabilities sit in the middle of a NaN-filled buffer and the results are finite, so nothing
    outside them was averaged."""
    import torch
    b, t, ncls = 6, 3, 97
    rng = np.random.default_rng(2)
    probs = rng.random((b, t, ncls), dtype=np.float32)
    pad = b * t * ncls
    host = np.full(3 * pad, np.nan, np.float32)
    host[pad:2 * pad] = probs.ravel()
    buf = torch.from_numpy(host).to(ctx.tdev)
    for table, tl in (([4, 9, 200], None), ([0, 0, 100], None), ([-50, 3, 2], None), ([2 ** 31 - 1, -2 ** 31, 5], None), ([0, 2, 6], [-4, 99])):
        group = torch.tensor(table, dtype=torch.int32, device=ctx.tdev)
        tlen = None if tl is None else torch.tensor(tl, dtype=torch.int32, device=ctx.tdev)
        out = torch.full((2, t, 2), -7.0, dtype=torch.float32, device=ctx.tdev)
        assert call_fuse(ctx, buf[pad:], b, t, ncls, ncls, group, 2, tlen, out) == 0
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert np.isfinite(got[..., 1]).all() and (got[..., 1] >= 0).all() and (got[..., 1] != -7.0).all(), table
        assert ((0 <= got.view(np.int32)[..., 0]) & (got.view(np.int32)[..., 0] < ncls)).all(), table
    same(out, *ctc_fuse_ref.fuse(probs, [0, 2, 6], [0, 3]), "lengths clamped into 0 .. t")


# ---- the pipeline on top ----------------------------------------------------------------------------------------------------------
def make_pipe(ctx, rec_id):
    from vse_amd import pipeline, shim
    det = net_ref.get_weights("V3_ch_det_fast")
    rec = net_ref.get_weights(rec_id)
    cs = P.en_charset() if rec_id == "V4_en_rec_fast" else P.standin_charset(shim._ncls(rec[0]))
    return pipeline.OcrPipeline(ctx, det, rec, cs)


@pytest.mark.parametrize("rec_id, ncls", [("V4_en_rec_fast", 97), ("V4_ch_rec_fast", 6625)])
def test_identical_frames_give_the_single_frame_result(ctx, rec_id, ncls):
    """(p + p) / 2 == p in float32: one frame stacked twice (and three times, and alone) gives recognize()'s text and score exactly."""
    import torch
    from vse_amd import pipeline, synth
    pipe = make_pipe(ctx, rec_id)
    assert len(pipe.charset) == ncls and getattr(pipe, "_fuse_rec", None) is None
    frame = synth.make_frames(1, 360, 640, seed=3, p_two_lines=1.0)
    one = torch.from_numpy(frame).to(ctx.tdev)
    boxes = pipeline.sorted_boxes(pipe.detect(one)[0])
    assert len(boxes) >= 1
    want = pipe.recognize(one, [boxes])[0]
    assert any(text for text, _ in want)
    assert getattr(pipe, "_fuse_rec", None) is None                                         # nothing of the second net exists before the first fusion
    three = torch.from_numpy(np.concatenate([frame] * 3)).to(ctx.tdev)
    assert pipe.recognize_fused(three[:2], [([0, 1], boxes)]) == [want]
    got = pipe.recognize_fused(three, [([0, 1, 2], boxes), ([1], boxes), ([2, 0], boxes[:1]), ([0], [])])
    assert got == [want, want, want[:1], []]
    assert pipe.recognize_fused(three, []) == []
    # a bound of one byte on the probability tensor: every quad's members still share a launch, one launch per quad
    res, parts = pipe.recognize_fused(three, [([0, 1, 2], boxes)], return_parts=True, max_fuse_bytes=1)
    assert res == [want] and len(parts) == len(boxes) and all(p["group"] == [0, 3] for p in parts)
    pipe.rec_mode = "reference"
    with pytest.raises(ValueError):
        pipe.recognize_fused(three, [([0, 1], boxes)])
    pipe.rec_mode = "ragged"
    for bad in ([], [3], [-1], list(range(3)) * 22):
        with pytest.raises(ValueError):
            pipe.recognize_fused(three, [(bad, boxes)])


def test_fused_rows_are_the_reference_on_the_members_own_probabilities(ctx):
    """Three frames that differ by the noise of synth.make_moving_clip (its background held still): the returned idx_maxp equals the
    numpy restatement applied to the returned probabilities, bit for bit, and each member's probabilities equal those of the same crop
    recognised alone: the batch-independence of ragged rows that the replication rests on."""
    import torch
    from vse_amd import synth
    pipe = make_pipe(ctx, "V4_en_rec_fast")
    frames, _truth = synth.make_moving_clip([("seven wizards quietly box", 3)], pan=(0, 0), seed=5)
    assert not np.array_equal(frames[0], frames[1]) and not np.array_equal(frames[1], frames[2])
    white = (frames == 255).all(axis=(0, 3))                                                # the fill of the text, in every frame
    ys, xs = np.nonzero(white)
    y0, y1, x0, x1 = int(ys.min()) - 3, int(ys.max()) + 4, int(xs.min()) - 3, int(xs.max()) + 4
    xm = (x0 + x1) // 2
    quads = [np.array([[a, y0], [b, y0], [b, y1], [a, y1]], np.float32) for a, b in ((x0, x1), (x0, xm), (xm - 20, x1))]
    dev = torch.from_numpy(frames).to(ctx.tdev)
    groups = [([0, 1, 2], quads), ([2, 0], quads[:2]), ([1], quads[2:])]
    res, parts = pipe.recognize_fused(dev, groups, return_parts=True)
    assert [len(r) for r in res] == [3, 2, 1] and sum(len(p["group"]) - 1 for p in parts) == 6
    net = pipe._fuse_net()
    differ = 0
    for part in parts:
        probs = part["probs"].cpu().numpy()[:, 0]
        tlen = part["tlen"].cpu().numpy()
        assert probs.dtype == np.float32 and probs.shape[2] == 97 and len(tlen) == len(part["group"]) - 1 == len(part["specs"])
        same(part["idx_maxp"][:, 0], *ctc_fuse_ref.fuse(probs, part["group"], tlen), part["specs"])
        for j, (gi, slot) in enumerate(part["specs"]):
            rows = range(part["group"][j], part["group"][j + 1])
            assert [part["crops"][r]["frame"] for r in rows] == groups[gi][0]
            n = int(tlen[j])
            assert 0 < n <= probs.shape[1]
            for r in rows:
                x = ctx.rec_preprocess(dev, [part["crops"][r]], pipe.rec_h, part["img_w"])
                prog = net.program(1, pipe.rec_h, part["img_w"])
                alone = net.run(x, widths=np.asarray([part["widths"][r]], np.int32))[[o["kind"] for o in prog.outputs].index("probs")]
                assert np.array_equal(alone.cpu().numpy()[0, 0, :n].view(np.int32), probs[r, :n].view(np.int32)), (gi, slot, r)
            differ += int(len(rows) > 1 and not np.array_equal(probs[rows[0], :n], probs[rows[1], :n]))
            # the decoded text is the greedy decode of the fused row
            idx, maxp = (a[j] for a in ctc_fuse_ref.fuse(probs, part["group"], tlen))
            ids, conf = ctc_fuse_ref.ctc_greedy(idx, maxp, n)
            assert res[gi][slot][0] == "".join(pipe.charset[c] for c in ids) and abs(res[gi][slot][1] - conf) < 1e-6
    assert differ >= 1                                                                      # the members did not all show the same pixels


def test_extractor_fused_end_to_end(ctx):
    """Frames of synth.make_frames, each held for 12 frames with blank frames between them: interval_text="fused" on two samples of each
    interval writes the SRT of the default run (the samples show the same pixels), and keeps one result per interval."""
    from vse_amd import extractor, frame_select, shim, synth
    h, w = 360, 640
    lit = synth.make_frames(3, h, w, seed=4)
    dark = np.full((h, w, 3), 40, np.uint8)
    clip = [dark] * 2
    for f in lit:
        clip += [f] * 12 + [dark] * 3
    ocr = shim.OcrRecogniser()
    ocr.recogniser = shim.PaddleOCR.__new__(shim.PaddleOCR)
    ocr.recogniser.pipe = make_pipe(ctx, "V4_en_rec_fast")
    src = extractor.ArraySource(clip, 12.0)
    area = extractor.SubtitleArea(ymin=int(0.7 * h), ymax=h, xmin=0, xmax=w)
    kw = dict(sub_area=area, mode="fast", language="en", frame_selector="change", drop_score=0.0, batch=8)
    plain = extractor.SubtitleExtractor(src, ocr, change_counter=frame_select.EngineCounter(ctx), **kw)
    want = plain.run()
    assert plain.intervals == [(3 + 15 * k, 14 + 15 * k, 8 + 15 * k) for k in range(3)] and want.count(" --> ") >= 2
    fused = extractor.SubtitleExtractor(src, ocr, change_counter=frame_select.EngineCounter(ctx), interval_text="fused",
                                        fuse_params={"samples": 2, "trim_seconds": 0}, **kw)
    assert fused.run() == want and fused.raw_lines == plain.raw_lines and fused.intervals == plain.intervals
    assert sorted(fused.interval_results) == [r for _s, _e, r in fused.intervals]
    assert all(len(b) == len(r) >= 1 for b, r in fused.interval_results.values())
