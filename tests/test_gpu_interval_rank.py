"""vse_interval_rank on the MI355X: every byte equals the numpy restatement (tests/interval_rank_ref.py) for every width, byte
alignment, sample count 1..63 and rank, through the aligned and the general loads alike; ties; rank 0 and n - 1 equal the composite
kernel's min and max; nothing outside the output is written and the input stays as it was; refusals touch nothing; and
IntervalQuantile on the engine gives the patches of the run fed by the numpy restatement."""
import ctypes as C

import numpy as np
import pytest

import interval_rank_ref

pytestmark = pytest.mark.gpu


def padded_view(ctx, frames, row_pad, lead, frame_rows_extra):
    """The same pixels in a strided view: rows `row_pad` bytes longer, starting `lead` bytes into their row, frames further apart."""
    import torch
    n, h, w, _ = frames.shape
    pitch = 3 * w + row_pad
    buf = torch.full((n, h + frame_rows_extra, pitch), 0x5A, dtype=torch.uint8, device=ctx.tdev)
    view = buf[:, 1:1 + h, lead:lead + 3 * w].view(n, h, w, 3)
    view.copy_(torch.from_numpy(frames))
    assert view.stride(1) == pitch and (n == 1 or view.stride(0) == (h + frame_rows_extra) * pitch > h * pitch)      # (one frame: no stride)
    return view


def shifted_view(ctx, frames, by):
    """The same pixels `by` bytes into a flat buffer: packed, and misaligned when `by` is no multiple of 4."""
    import torch
    flat = torch.zeros(frames.size + 16, dtype=torch.uint8, device=ctx.tdev)
    view = flat[by:by + frames.size].view(frames.shape)
    view.copy_(torch.from_numpy(frames))
    return view


def check_all_ranks(ctx, views, frames, area, ranks, what):
    """Every view in `views` (the pixels of `frames` on the device) at every rank in `ranks` against the sort, computed once."""
    y0, y1, x0, x1 = area
    ordered = np.sort(frames[:, y0:y1, x0:x1], axis=0)
    for rank in ranks:
        for name, view in views:
            got = ctx.interval_rank(view, area, rank).cpu().numpy()
            assert got.dtype == np.uint8 and got.shape == ordered[rank].shape and np.array_equal(got, ordered[rank]), (what, name, area, rank)


@pytest.mark.parametrize("area_h", [1, 2, 9])
def test_every_width_and_alignment(ctx, area_h):
    """area_w 1..17 at x0 0..5: 3 x0 and 3 area_w take every residue mod 4; 11 x 37 frames (pitch 111, so every row starts on another
    residue), packed and in a view with a padded pitch (116 + an odd lead) and a frame stride above h * pitch; every rank 0..4."""
    import torch
    frames = np.random.default_rng(area_h).integers(0, 256, size=(5, 11, 37, 3), dtype=np.uint8)
    views = [("packed", torch.from_numpy(frames).to(ctx.tdev)), ("padded", padded_view(ctx, frames, 5, 3, 2))]
    assert {3 * x % 4 for x in range(6)} == {3 * w % 4 for w in range(1, 18)} == set(range(4))
    for area_w in range(1, 18):
        for x0 in range(6):
            check_all_ranks(ctx, views, frames, (1, 1 + area_h, x0, x0 + area_w), range(5), "widths")


def test_every_sample_count(ctx):
    """n 1..63 (the bucket edges 8|9, 16|17, 32|33 and the limit 63) at ranks 0, n // 2 and n - 1: (n, 3, 23, 3) frames are packed at
    69 bytes a row and 207 a frame, so odd n take the general loads from the second frame on; the same pixels with a 72-byte pitch and
    a 4-byte aligned frame stride take the aligned loads.  n = 1 has no frame stride to align."""
    import torch
    rng = np.random.default_rng(63)
    for n in range(1, 64):
        frames = rng.integers(0, 256, size=(n, 3, 23, 3), dtype=np.uint8)
        aligned = padded_view(ctx, frames, 3, 0, 1)
        assert aligned.stride(1) % 4 == 0 and aligned.stride(0) % 4 == 0 and aligned.data_ptr() % 4 == 0
        views = [("packed", torch.from_numpy(frames).to(ctx.tdev)), ("aligned pitch", aligned)]
        check_all_ranks(ctx, views, frames, (0, 3, 1, 22), sorted({0, n // 2, n - 1}), n)
        check_all_ranks(ctx, views[1:], frames, (0, 3, 4, 20), sorted({0, n // 2, n - 1}), (n, "aligned start"))       # 3 x0 = 12: the aligned loads


def test_ties(ctx):
    import torch
    rng = np.random.default_rng(7)
    area = (0, 4, 0, 19)
    for what, frames in (("three values", rng.choice(np.array([0, 128, 255], np.uint8), size=(9, 4, 19, 3))),
                         ("two neighbours", rng.choice(np.array([7, 8], np.uint8), size=(12, 4, 19, 3))),
                         ("all 0", np.zeros((5, 4, 19, 3), np.uint8)), ("all 255", np.full((17, 4, 19, 3), 255, np.uint8)),
                         ("255 below the pad", np.concatenate([np.full((3, 4, 19, 3), 255, np.uint8), np.zeros((2, 4, 19, 3), np.uint8)]))):
        frames = np.ascontiguousarray(frames)
        views = [("packed", torch.from_numpy(frames).to(ctx.tdev)), ("shifted", shifted_view(ctx, frames, 1))]
        check_all_ranks(ctx, views, frames, area, range(len(frames)), what)
    # a ramp: the 48 bytes of a 16-pixel run all differ (b -> b (5 + 2 f) + f mod 256, an odd factor) and move differently per frame
    b = np.arange(48, dtype=np.int64).reshape(16, 3)
    ramp = np.stack([np.stack([(b * (5 + 2 * f) + f + 11 * r) % 256 for r in range(2)]) for f in range(13)]).astype(np.uint8)
    assert all(len(set(ramp[f, r].ravel().tolist())) == 48 for f in range(13) for r in range(2))
    views = [("aligned", torch.from_numpy(ramp).to(ctx.tdev)), ("shifted", shifted_view(ctx, ramp, 1))]
    check_all_ranks(ctx, views, ramp, (0, 2, 0, 16), range(13), "ramp")


@pytest.mark.parametrize("n", [1, 5, 16, 33])
def test_rank_ends_equal_the_composite_kernel(ctx, n):
    import torch
    frames = np.random.default_rng(n).integers(0, 256, size=(n, 6, 29, 3), dtype=np.uint8)
    dev = torch.from_numpy(frames).to(ctx.tdev)
    area = (1, 6, 2, 27)
    state = ctx.interval_state(5, 25)
    ctx.interval_accumulate(dev, area, state, reset=True)
    assert torch.equal(ctx.interval_rank(dev, area, 0), ctx.interval_composite(state, 5, 25, n, "min"))
    assert torch.equal(ctx.interval_rank(dev, area, n - 1), ctx.interval_composite(state, 5, 25, n, "max"))


@pytest.mark.parametrize("x0, area_w", [(0, 64), (16, 37), (0, 63), (32, 32)])
def test_wide_loads_equal_general_loads(ctx, x0, area_w):
    """src_w 64 with aligned base, pitch and frame stride, 3 x0 a multiple of 4: the aligned loads.  The same pixels 3 bytes further
    into a buffer are misaligned and take the general loads: identical bytes."""
    import torch
    n, h, w = 11, 6, 64
    frames = np.random.default_rng(x0 + area_w).integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    area = (0, h, x0, x0 + area_w)
    aligned = torch.from_numpy(frames).to(ctx.tdev)
    assert aligned.data_ptr() % 16 == 0 and aligned.stride(1) % 16 == 0 and aligned.stride(0) % 16 == 0 and 3 * x0 % 16 == 0
    shifted = shifted_view(ctx, frames, 3)
    assert shifted.data_ptr() % 16 == 3
    check_all_ranks(ctx, [("wide", aligned), ("general", shifted)], frames, area, range(n), "wide / general")
    check_all_ranks(ctx, [("one frame", aligned[:1])], frames[:1], area, [0], "n = 1")


def test_writes_only_the_output(ctx):
    import torch
    frames = np.random.default_rng(2).integers(0, 256, size=(4, 7, 29, 3), dtype=np.uint8)
    dev = torch.from_numpy(frames).to(ctx.tdev)
    area = (2, 7, 3, 26)                                                              # the last row is the allocation's last row
    ah, aw = 5, 23
    ordered = np.sort(frames[:, 2:7, 3:26], axis=0)
    for lead, pitch in ((5, 3 * aw + 7), (16, 3 * aw + 11), (0, 3 * aw)):
        for rank in range(4):
            buf = torch.full((ah + 2, pitch + lead), 0xA5, dtype=torch.uint8, device=ctx.tdev)
            out = buf[1:1 + ah, lead:lead + 3 * aw].view(ah, aw, 3)
            assert ctx.interval_rank(dev, area, rank, out=out) is out
            host = buf.cpu().numpy()
            assert np.array_equal(host[1:1 + ah, lead:lead + 3 * aw].reshape(ah, aw, 3), ordered[rank]), (lead, pitch, rank)
            host[1:1 + ah, lead:lead + 3 * aw] = 0xA5
            assert (host == 0xA5).all(), (lead, pitch, rank)                           # row gaps and the rows around: the canary
    assert np.array_equal(dev.cpu().numpy(), frames)                                  # the input is read only
    # a tight input: the whole frame is the area, its last byte the allocation's last byte, n = 3 so the frames are misaligned
    tight = np.random.default_rng(3).integers(0, 256, size=(3, 5, 7, 3), dtype=np.uint8)
    check_all_ranks(ctx, [("tight", torch.from_numpy(tight).to(ctx.tdev))], tight, (0, 5, 0, 7), range(3), "tight")
    check_all_ranks(ctx, [("tight", torch.from_numpy(tight).to(ctx.tdev))], tight, (3, 5, 5, 7), range(3), "last rows, last columns")


def test_refusals_touch_nothing(ctx):
    import torch
    from vse_amd import engine
    lib = engine.load_library()
    assert engine.INTERVAL_RANK_MAX == 63
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=ctx.tdev)                    # far larger than any of the frames below
    out = torch.full((4096,), 0xA5, dtype=torch.uint8, device=ctx.tdev)

    def rank(n=1, h=10, w=20, pitch=60, fstride=600, y0=0, y1=10, x0=0, x1=20, rank=0, src=True, dst=True, out_pitch=60):
        return lib.vse_interval_rank(ctx.handle, C.c_void_p(buf.data_ptr()) if src else None, n, h, w, pitch, fstride, y0, y1, x0, x1, rank,
                                     C.c_void_p(out.data_ptr()) if dst else None, out_pitch, ctx.stream())

    for kw in (dict(y0=4, y1=4), dict(x0=7, x1=7), dict(y0=5, y1=3), dict(y0=-1), dict(x0=-1), dict(y1=11), dict(x1=21),      # empty / outside
               dict(n=0), dict(n=-1), dict(n=64), dict(n=65535), dict(pitch=59), dict(h=0), dict(w=0), dict(n=2, fstride=599),
               dict(n=63, fstride=0, h=1, w=1, pitch=3, y1=1, x1=1, out_pitch=3),                                              # frames may not overlap
               dict(rank=-1), dict(rank=1), dict(n=5, rank=5), dict(n=63, rank=63), dict(src=False), dict(dst=False), dict(out_pitch=59),
               dict(x1=10, out_pitch=29)):
        assert rank(**kw) == -1, kw
        assert "vse_interval_rank" in lib.vse_last_error().decode(), kw
    torch.cuda.synchronize()
    assert int((out != 0xA5).sum()) == 0 and int(buf.sum()) == 0                      # nothing was enqueued
    assert rank() == 0 and rank(n=63, rank=62) == 0 and rank(n=63, rank=0, x1=10, out_pitch=30) == 0       # the limits themselves are accepted
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0 and int((out[:600] != 0).sum()) == 0 and int((out[600:] != 0xA5).sum()) == 0
    with pytest.raises(engine.VseError, match="vse_interval_rank"):
        ctx.interval_rank(buf[:64 * 27].view(64, 3, 3, 3), (0, 3, 0, 3), 0)


@pytest.mark.parametrize("staged", [False, True])
def test_quantile_on_engine(ctx, staged):
    """IntervalQuantile with EngineRanker (area rows only, batches of 8, with and without the uploader) gives the patches of the run fed
    by the numpy restatement."""
    from vse_amd import extractor, frame_select, staging, synth
    h, w = 120, 200
    frames, truth = synth.make_clip([(None, 2), ("the quick brown fox", 9), ("seven wizards", 7, 2), (None, 3), ("near frozen lakes", 6)], h, w, seed=6)
    ivs = [(s, e, (s + e) // 2) for s, e, _t in truth]
    area = extractor.SubtitleArea(ymin=int(0.7 * h), ymax=h, xmin=7, xmax=w - 4)
    up = staging.Uploader(ctx.tdev) if staged else None
    for quantile, samples in ((0.5, 5), (0.1, 8), (1.0, 3)):
        want = frame_select.IntervalQuantile(interval_rank_ref.NumpyRanker(), quantile, samples, trim_seconds=0.1, batch=8).run(list(frames), area, ivs, 10.0)
        comp = frame_select.IntervalQuantile(frame_select.EngineRanker(ctx), quantile, samples, trim_seconds=0.1, batch=8)
        got = comp.run(list(frames), area, ivs, 10.0, uploader=up)
        assert sorted(got) == sorted(want) == [r for _s, _e, r in ivs]
        assert all(got[r].dtype == np.uint8 and np.array_equal(got[r], want[r]) for r in want), (quantile, samples)
    if up is not None:
        up.close()
