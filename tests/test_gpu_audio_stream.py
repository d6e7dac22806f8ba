"""vse_audio_stream_* on the GPU (csrc/audio_stream.hip): the uint8 stream, the clip levels' bits and the set sizes are the host's
(vse_amd.timeline_sync.AudioStream) for every path of the kernels: the copy path and the resampling one, 2- / 4-byte and whole
group loads, partial last seconds, the unwritten sample, heavy ties, empty sets, the ends of the bin range, unaligned buffers,
pieces in any order, a re-used workspace, and sync() end to end in both modes."""
import numpy as np
import pytest

import audio_stream_ref as ref
from vse_amd import engine, synth, timeline_sync as ts

pytestmark = pytest.mark.gpu
S = 12000
FILL = 0xA5


def host(tmp_path, pcm, rate, sample_rate=S):
    p = str(tmp_path / "h.wav")
    with open(p, "wb") as f:
        f.write(synth.wav_bytes(pcm, rate))
    return ts.AudioStream(p, sample_rate).data


def device(ctx, pcm, rate, sample_rate=S, pieces=None, reverse=False, ws=None, out=None, pcm_offset=0):
    """Feed pcm [F, C] (pieces: seconds per call, None = one call) and finish -> (stream bytes, record int32 [8], out tensor)."""
    t = ctx.torch
    frames, channels = pcm.shape
    args = (frames, channels, rate, sample_rate)
    if ws is None:
        ws = ctx.audio_stream_workspace(*args)
    seconds = -(-frames // rate)
    step = pieces or seconds
    firsts = list(range(0, seconds, step))
    for first in (firsts[::-1] if reverse else firsts):
        piece = np.ascontiguousarray(pcm[first * rate:(first + step) * rate]).reshape(-1)
        buf = t.zeros(len(piece) + pcm_offset, dtype=t.int16, device=ctx.tdev)
        buf[pcm_offset:] = t.from_numpy(piece).to(ctx.tdev)
        ctx.audio_stream_feed(buf[pcm_offset:], first, *args, ws)
    if out is None:
        out = t.full((ctx.audio_stream_length(*args),), FILL, dtype=t.uint8, device=ctx.tdev)
    _, rec = ctx.audio_stream_finish(*args, ws, out=out)
    return out.cpu().numpy(), rec.cpu().numpy(), out


def check(ctx, tmp_path, pcm, rate, sample_rate=S, **kw):
    got, rec, _ = device(ctx, pcm, rate, sample_rate, **kw)
    lo, hi, n_ge0, n_le0 = ref.host_float_levels(pcm, rate, sample_rate)
    print(f"rate {rate} -> {sample_rate}, {pcm.shape}: lo {lo} hi {hi} sets {n_ge0} {n_le0}; device record {rec[:5].tolist()}")
    assert (int(rec[2]), int(rec[3])) == (n_ge0, n_le0)
    assert rec[:2].copy().view(np.uint32).tolist() == [int(lo.view(np.uint32)), int(hi.view(np.uint32))] or (np.isnan(lo) or np.isnan(hi))
    silent = not (np.isfinite(lo) and np.isfinite(hi)) or np.float32(hi - lo) == 0
    assert int(rec[4]) == int(silent)
    if silent:
        assert np.isnan(lo) == np.isnan(rec[:1].copy().view(np.float32)[0]) and np.isnan(hi) == np.isnan(rec[1:2].copy().view(np.float32)[0])
        assert (got == FILL).all()                       # the stream is not written
        with pytest.raises(ts.TimelineSyncError, match="silence"):
            host(tmp_path, pcm, rate, sample_rate)
    else:
        want = host(tmp_path, pcm, rate, sample_rate)
        assert got.shape == want.shape and np.array_equal(got, want), int((got != want).sum())
    return got


# kind, channels, rate, sample_rate, frames
CASES = [
    ("speech", 1, 12000, S, 2 * 12000),                 # the copy path, one 8-byte load per group
    ("speech", 2, 12000, S, 2 * 12000 + 1),             # the copy path, one 16-byte load per group; a last second of one frame
    ("speech", 6, 12000, S, 2 * 12000 + 6000),
    ("speech", 1, 16000, S, 16000 + 7),
    ("speech", 2, 44100, S, 2 * 44100 + 22050),
    ("speech", 6, 44101, S, 44101 + 7),
    ("speech", 2, 48000, S, 2 * 48000 + 5),             # the chunk lengths sum to one short of sample_count
    ("speech", 1, 48000, 8000, 2 * 48000 + 24000),
    ("speech", 2, 48000, 24000, 48000 + 7),             # 7 frames * 0.5 = 3.5 -> 4 samples (ties to even)
    ("speech", 6, 48000, S, 2 * 48000),
    ("tiny", 1, 12000, S, 2 * 12000),                   # both ranks in one bin or in adjacent bins, even set sizes ...
    ("tiny", 1, 12000, S, 2 * 12000 + 1),               # ... and odd ones
    ("tiny", 2, 48000, S, 2 * 48000 + 24000),
    ("tiny", 6, 16000, S, 16000 + 7),
    ("nonneg", 1, 16000, S, 2 * 16000),                 # the <= 0 set is zeros only
    ("nonneg", 2, 48000, S, 2 * 48000 + 5),
    ("positive", 2, 48000, S, 48000 + 7),               # the <= 0 set is empty: the host's silence
    ("ends", 1, 12000, S, 2 * 12000),                   # sums at both ends of the bin range
    ("ends", 2, 48000, S, 2 * 48000 + 24000),
    ("ends", 6, 44100, S, 44100 + 7),
    ("full", 6, 48000, 24000, 2 * 48000 + 24000),
    ("zero", 1, 12000, S, 2 * 12000),                   # silence: status 1, the output keeps its fill pattern
    ("zero", 2, 48000, S, 48000 + 7),
]


@pytest.mark.parametrize("kind,channels,rate,sample_rate,frames", CASES)
def test_stream_levels_and_set_sizes_are_the_hosts(ctx, tmp_path, kind, channels, rate, sample_rate, frames):
    check(ctx, tmp_path, ref.make_pcm(kind, frames, channels, seed=frames % 97 + channels), rate, sample_rate)


def test_tiny_values_cover_even_and_odd_set_sizes():
    sizes = set()
    for frames in (2 * 12000, 2 * 12000 + 1, 2 * 12000 + 2, 2 * 12000 + 3):
        _, _, _, n_ge0, n_le0, _ = ref.integer_stream(ref.make_pcm("tiny", frames, 1, seed=frames % 97 + 1), 12000, S)
        sizes |= {("ge", n_ge0 & 1), ("le", n_le0 & 1)}
    assert len(sizes) == 4


@pytest.mark.parametrize("frames", [2 * 12000 + 2, 2 * 12000 + 3])
def test_tiny_values_other_parities(ctx, tmp_path, frames):
    check(ctx, tmp_path, ref.make_pcm("tiny", frames, 1, seed=frames % 97 + 1), 12000)


@pytest.mark.parametrize("channels,rate", [(1, 12000), (2, 12000), (2, 48000), (6, 44100)])
def test_pieces_in_any_order_and_unaligned_buffers(ctx, tmp_path, channels, rate):
    t = ctx.torch
    frames = 4 * rate + rate // 2
    pcm = ref.make_pcm("speech", frames, channels, seed=21)
    want = host(tmp_path, pcm, rate)
    args = (frames, channels, rate, S)
    nbytes = ctx.lib.vse_audio_stream_workspace_bytes(*args)
    length = ctx.audio_stream_length(*args)
    assert length == len(want)
    big_ws = t.full((nbytes + 512,), 0x5A, dtype=t.uint8, device=ctx.tdev)
    assert big_ws.data_ptr() % 256 == 0
    ws = big_ws[:nbytes]
    for kw in (dict(), dict(pieces=1), dict(pieces=1, reverse=True), dict(pieces=3, reverse=True), dict(pieces=1, pcm_offset=1),
               dict(pieces=2, pcm_offset=3), dict(pcm_offset=2)):
        for off in (0, 1, 4, 7):
            big_out = t.full((length + 64,), FILL, dtype=t.uint8, device=ctx.tdev)
            out = big_out[off:off + length]
            got, rec, _ = device(ctx, pcm, rate, ws=ws, out=out, **kw)
            assert rec[4] == 0 and np.array_equal(got, want), (kw, off, int((got != want).sum()))
            whole = big_out.cpu().numpy()
            assert (whole[:off] == FILL).all() and (whole[off + length:] == FILL).all(), (kw, off)
            if kw:
                break                                  # every output offset with one feeding, every feeding with one offset
    assert (big_ws[nbytes:].cpu().numpy() == 0x5A).all()


def test_workspace_serves_the_next_file(ctx, tmp_path):
    a = ref.make_pcm("speech", 3 * 48000 + 100, 2, seed=31)
    b = ref.make_pcm("tiny", 2 * 16000 + 9, 6, seed=32)
    ws = ctx.audio_stream_workspace(8 * 48000, 8, 48000, S)          # large enough for both
    for pcm, rate in ((a, 48000), (b, 16000), (a, 48000)):
        check(ctx, tmp_path, pcm, rate, ws=ws)


def test_sync_gives_the_same_searches_and_script_in_both_modes(ctx, tmp_path):
    sp = lambda x, y: ["speech", 51, 20, x, y]           # noqa: E731
    src = dict(pieces=[sp(0, 20)], rate=48000, channels=2)
    dst = dict(pieces=[["noise", 52, 1.5, 300], sp(0, 12), sp(13, 20)], rate=44100)
    paths = {}
    for name, r in (("src", src), ("dst", dst)):
        paths[name] = str(tmp_path / f"{name}.wav")
        with open(paths[name], "wb") as f:
            f.write(synth.audio_from_recipe(r))
    script = str(tmp_path / "in.srt")
    with open(script, "w") as f:
        f.write("\n".join(f"{k + 1}\n{ts.format_srt_time(1 + 2.5 * k)} --> {ts.format_srt_time(3 + 2.5 * k)}\nline {k}\n" for k in range(7)))
    search = ts.GpuSearch(ctx)
    logs, outs = [], []
    for mode in ("host", "device"):
        out = str(tmp_path / f"{mode}.srt")
        logs.append([(*q[:5], int(np.float32(q[5]).view(np.uint32))) for q in ts.sync(paths["src"], paths["dst"], script, out, search=search,
                                                                                       stream_build=mode)])
        outs.append(open(out, "rb").read())
    assert len(logs[0]) >= 7 and logs[0] == logs[1] and outs[0] == outs[1]
    dev = ts.DeviceAudioStream(paths["src"], ctx=ctx)
    assert dev.data.is_cuda and np.array_equal(dev.data.cpu().numpy(), ts.AudioStream(paths["src"]).data)
    search.load(dev.data, dev.data)
    assert search.src.data_ptr() == dev.data.data_ptr()                # taken as it is, no copy


def test_refusals_launch_nothing(ctx):
    t = ctx.torch
    lib = ctx.lib
    for frames, channels, rate, sample_rate in ((24000, 0, 12000, S), (24000, 9, 12000, S), (24000, 1, 11999, S), (0, 1, 12000, S),
                                                (2 ** 33, 1, 12000, S), (2 ** 31 - 1 - 20 * 12000 + 1, 1, 12000, S)):
        assert lib.vse_audio_stream_length(frames, channels, rate, sample_rate) == 0
        assert lib.vse_audio_stream_workspace_bytes(frames, channels, rate, sample_rate) == 0
    assert lib.vse_audio_stream_length(2 ** 31 - 1 - 20 * 12000, 1, 12000, S) == 2 ** 31 - 1
    good = (3 * 12000, 1, 12000, S)
    nbytes = lib.vse_audio_stream_workspace_bytes(*good)
    ws = t.full((nbytes,), 0x5A, dtype=t.uint8, device=ctx.tdev)
    pcm = t.ones(3 * 12000 * 9, dtype=t.int16, device=ctx.tdev)
    out = t.full((ctx.audio_stream_length(*good),), FILL, dtype=t.uint8, device=ctx.tdev)
    rec = t.full((8,), -7, dtype=t.int32, device=ctx.tdev)

    def refused(call, text):
        with pytest.raises(engine.VseError, match="rc=-1") as e:
            call()
        assert text in str(e.value), str(e.value)

    for frames, channels, rate, sample_rate in ((24000, 0, 12000, S), (24000, 9, 12000, S), (24000, 1, 11999, S), (0, 1, 12000, S),
                                                (2 ** 33, 1, 12000, S)):
        n = max(channels, 1) * 12000
        refused(lambda: ctx.audio_stream_feed(pcm[:n], 0, frames, channels, rate, sample_rate, ws), "bad arguments")
        rc = lib.vse_audio_stream_finish(ctx.handle, frames, channels, rate, sample_rate, ws.data_ptr(), ws.numel(), out.data_ptr(),
                                         rec.data_ptr(), ctx.stream())
        assert rc == -1 and b"bad arguments" in lib.vse_last_error()
    refused(lambda: ctx.audio_stream_feed(pcm[:12005], 0, *good, ws), "whole seconds")            # not whole seconds, not the last
    refused(lambda: ctx.audio_stream_feed(pcm[:12000], 3, *good, ws), "whole seconds")            # outside the file
    refused(lambda: ctx.audio_stream_feed(pcm[:24001], 2, *good, ws), "whole seconds")            # runs past the end
    refused(lambda: ctx.audio_stream_feed(pcm[:12000], 0, *good, ws[:nbytes - 1]), "workspace")    # one byte short
    refused(lambda: ctx.audio_stream_finish(*good, ws[:nbytes - 1], out=out, result=rec), "workspace")
    refused(lambda: ctx.audio_stream_feed(pcm[:12000], 0, *good, ws[256 + 1:]), "workspace")       # not aligned (and short)
    refused(lambda: ctx.audio_stream_feed(pcm[:2 * 48000 + 1], 0, 2 * 48000 + 1, 1, 48000, S,
                                          t.empty(lib.vse_audio_stream_workspace_bytes(2 * 48000 + 1, 1, 48000, S), dtype=t.uint8,
                                                  device=ctx.tdev)), "too few to resample")
    t.cuda.synchronize()
    assert (ws.cpu().numpy() == 0x5A).all() and (out.cpu().numpy() == FILL).all() and (rec.cpu().numpy() == -7).all()
