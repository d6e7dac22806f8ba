"""The device form of the WAV -> uint8 stream step of timeline sync, on the CPU: the integer restatement the kernels implement
(tests/audio_stream_ref.py) gives AudioStream's bytes over a grid of channel counts, rates, lengths and amplitudes, refusals
included; DeviceAudioStream over a numpy builder gives the same stream, attributes, windows and error texts however the file is cut
into pieces, and leaves irregular files to AudioStream; the stream_build option of sync()."""
import logging
import math

import numpy as np
import pytest

import audio_stream_ref as ref
from audio_match_ref import NumpySearch
from vse_amd import synth, timeline_sync as ts

S = 12000


def wav(tmp_path, pcm, rate, name="a.wav"):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(synth.wav_bytes(pcm, rate))
    return p


def host_outcome(path, sample_rate=S):
    """("ok", bytes) or ("error", text) of the host path."""
    try:
        return "ok", ts.AudioStream(path, sample_rate).data
    except ts.TimelineSyncError as e:
        return "error", str(e)


LENGTHS = {"whole": lambda r: 2 * r, "one_more": lambda r: 2 * r + 1, "half_more": lambda r: 2 * r + r // 2,
           "second_and_7": lambda r: r + 7, "five": lambda r: 5}


@pytest.mark.parametrize("rate", [12000, 12001, 16000, 44100, 44101, 48000])
@pytest.mark.parametrize("channels", [1, 2, 3, 6, 8])
def test_integer_form_gives_the_hosts_bytes(tmp_path, channels, rate):
    seen = set()
    for li, (lname, length) in enumerate(LENGTHS.items()):
        for ai, kind in enumerate(["tiny", "nonneg", "speech", "full"]):
            pcm = ref.make_pcm(kind, length(rate), channels, seed=100 * li + ai)
            kind_, want = host_outcome(wav(tmp_path, pcm, rate))
            try:
                got, lo, hi, n_ge0, n_le0, status = ref.integer_stream(pcm, rate, S)
            except ref.Refused as e:
                assert e.kind == "too few" and kind_ == "error" and want.endswith(str(e)), (lname, kind, want)
                seen.add("too few")
                continue
            if status:
                assert got is None and kind_ == "error" and "silence" in want, (lname, kind, want)
                seen.add("silence")
                continue
            assert kind_ == "ok", (lname, kind, want)
            assert got.dtype == np.uint8 and np.array_equal(got, want), (lname, kind, int((got != want).sum()))
            assert n_ge0 + n_le0 >= len(got)
            seen.add("ok")
    assert "ok" in seen
    if rate > 2 * S:
        assert "too few" in seen          # one frame beyond two seconds resamples to nothing (rint(S / rate) == 0)


def test_grid_reaches_the_silence_refusal_and_the_short_sum(tmp_path):
    pcm = ref.make_pcm("positive", 48000 + 7, 2, seed=5)      # no sample <= 0 and nothing unwritten: the <= 0 set is empty
    assert ref.integer_stream(pcm, 48000, S)[5] == 1
    assert "silence" in host_outcome(wav(tmp_path, pcm, 48000))[1]
    pcm = ref.make_pcm("positive", 2 * 48000 + 5, 1, seed=6)  # the chunk lengths sum to one short: one zero, which then pads the end
    got, lo, hi, n_ge0, n_le0, status = ref.integer_stream(pcm, 48000, S)
    assert status == 0 and n_le0 == 1 + 480000 and np.array_equal(got, host_outcome(wav(tmp_path, pcm, 48000))[1])


CASES = [("speech", 2, 48000, 4 * 48000 + 24000), ("speech", 1, 12000, 4 * 12000 + 7), ("tiny", 3, 44101, 3 * 44101 + 9),
         ("positive", 1, 48000, 2 * 48000 + 5), ("full", 6, 16000, 5 * 16000)]


@pytest.mark.parametrize("kind,channels,rate,frames", CASES)
def test_device_audio_stream_over_the_numpy_builder(tmp_path, kind, channels, rate, frames):
    pcm = ref.make_pcm(kind, frames, channels, seed=11)
    path = wav(tmp_path, pcm, rate)
    host = ts.AudioStream(path)
    builders = []

    def build(*a):
        builders.append(ref.NumpyBuilder(*a))
        return builders[-1]

    want_levels = ref.integer_stream(pcm, rate, S)[1:3]
    for kw in (dict(), dict(piece_seconds=1), dict(piece_seconds=3), dict(piece_seconds=1, piece_order=lambda x: x[::-1]),
               dict(piece_seconds=3, piece_order=lambda x: x[::-1])):
        dev = ts.DeviceAudioStream(path, build=build, **kw)
        assert np.array_equal(dev.data, host.data), kw
        assert (dev.sample_rate, dev.sample_count, dev.padding_size, dev.duration_seconds) == \
            (host.sample_rate, host.sample_count, host.padding_size, host.duration_seconds)
        assert len(dev.data) == len(host.data)
        assert dev.levels[0].dtype == np.float32 and [x.view(np.uint32) for x in dev.levels] == [x.view(np.uint32) for x in want_levels]
        for t in (-3.0, 0.0, 1.25, 100.0):
            assert dev.sample_for_time(t) == host.sample_for_time(t)
            assert dev.window(t, 1.5, 700) == host.window(t, 1.5, 700)
            assert dev.substream(t, t + 0.8) == host.substream(t, t + 0.8)
    seconds = -(-frames // rate)
    assert [len(b.fed) for b in builders] == [1, seconds, -(-seconds // 3), seconds, -(-seconds // 3)]
    assert builders[3].fed[0][0] == seconds - 1 and builders[1].fed[0][0] == 0


def test_device_audio_stream_raises_the_hosts_texts(tmp_path):
    for name, pcm, rate in (("z.wav", ref.make_pcm("zero", 24000, 1), 12000), ("p.wav", ref.make_pcm("positive", 48007, 2, 3), 48000),
                            ("t.wav", ref.make_pcm("speech", 2 * 48000 + 1, 2, 4), 48000)):
        path = wav(tmp_path, pcm, rate, name)
        kind, want = host_outcome(path)
        assert kind == "error"
        with pytest.raises(ts.TimelineSyncError) as e:
            ts.DeviceAudioStream(path, build=ref.NumpyBuilder)
        assert str(e.value) == want
    assert "too few to resample" in want
    low = wav(tmp_path, ref.make_pcm("speech", 16000, 1, 5), 8000, "low.wav")
    with pytest.raises(ts.TimelineSyncError, match="below the search rate"):
        ts.DeviceAudioStream(low, build=ref.NumpyBuilder)


def test_device_audio_stream_defers_irregular_files_to_the_host(tmp_path, caplog):
    def no_build(*a):
        raise AssertionError("the builder must not be used")

    nine = wav(tmp_path, ref.make_pcm("speech", 30000, 9, 7), 12000, "nine.wav")
    with caplog.at_level(logging.INFO, logger="vse_amd.timeline_sync"):
        dev = ts.DeviceAudioStream(nine, build=no_build)
    assert np.array_equal(dev.data, ts.AudioStream(nine).data) and dev.levels is None
    assert len([r for r in caplog.records if "built on the host" in r.getMessage()]) == 1 and "9 channels" in caplog.text

    for cut in (12000 * 2 * 2 + 1000, 12000 * 2):           # a data chunk cut mid-second, and one that lost a whole second
        full = synth.wav_bytes(ref.make_pcm("speech", 36000, 2, 8), 12000)
        p = str(tmp_path / f"cut{cut}.wav")
        with open(p, "wb") as f:
            f.write(full[:len(full) - cut])
        caplog.clear()
        try:
            with caplog.at_level(logging.INFO, logger="vse_amd.timeline_sync"):
                got = ("ok", ts.DeviceAudioStream(p, build=no_build).data)
        except ts.TimelineSyncError as e:
            got = ("error", str(e))
        want = host_outcome(p)
        assert got[0] == want[0] and (np.array_equal(got[1], want[1]) if got[0] == "ok" else got[1] == want[1])
        assert "shorter than its header claims" in caplog.text


def test_sync_stream_build_option(tmp_path):
    a = wav(tmp_path, ref.make_pcm("speech", 36000, 1, 1), 12000, "a.wav")
    b = wav(tmp_path, ref.make_pcm("speech", 36000, 1, 2), 12000, "b.wav")
    srt = str(tmp_path / "in.srt")
    with open(srt, "w") as f:
        f.write("1\n00:00:01,000 --> 00:00:02,000\nx\n")
    out = str(tmp_path / "out.srt")
    with pytest.raises(ts.TimelineSyncError, match="--stream-build device needs the GPU searcher"):
        ts.sync(a, b, srt, out, search=NumpySearch(), stream_build="device")
    with pytest.raises(ts.TimelineSyncError, match="--stream-build nonsense"):
        ts.sync(a, b, srt, out, search=NumpySearch(), stream_build="nonsense")
    ts.sync(a, b, srt, out, search=NumpySearch(), stream_build="host")
    args = ts._parser().parse_args(["--src", a, "--dst", b, "--script", srt, "--stream-build", "device"])
    assert args.stream_build == "device" and ts._parser().parse_args(["--src", a, "--dst", b, "--script", srt]).stream_build == "host"


def test_size_queries_follow_the_geometry(built_lib):
    """The library's host half without a GPU: the stream length is the restatement's, the workspace holds the int32 samples (padded
    to 256 bytes) and whole 1024-lane segments of the 65535 C + 1 bins, and what is refused gives 0."""
    from vse_amd import engine
    lib = engine.load_library()
    for channels in (1, 2, 3, 6, 8):
        for rate in (12000, 12001, 16000, 44100, 44101, 48000):
            for frames in (1, 5, rate + 7, 2 * rate, 2 * rate + 1, 2 * rate + rate // 2, 2 * 60 * 60 * rate):
                for s in (S, 8000, rate):
                    try:
                        length = ref.geometry(frames, channels, rate, s)["L"]
                    except ref.Refused as e:            # a tail too short to resample is feed's refusal, not the size query's
                        assert e.kind == "too few"
                        length = 20 * rate + math.ceil(frames / float(rate) * s)
                    assert lib.vse_audio_stream_length(frames, channels, rate, s) == length
                    seg = -(-(-(-(65535 * channels + 1) // 1024)) // 4) * 4
                    assert lib.vse_audio_stream_workspace_bytes(frames, channels, rate, s) == -(-4 * length // 256) * 256 + seg * 1024 * 4
    for frames, channels, rate, s in ((24000, 0, 12000, S), (24000, 9, 12000, S), (24000, 1, 11999, S), (0, 1, 12000, S), (-5, 1, 12000, S),
                                      (2 ** 33, 1, 12000, S), (2 ** 31 - 20 * 12000, 1, 12000, S), (24000, 1, 12000, 0)):
        assert lib.vse_audio_stream_length(frames, channels, rate, s) == 0
        assert lib.vse_audio_stream_workspace_bytes(frames, channels, rate, s) == 0
    assert lib.vse_audio_stream_length(2 ** 31 - 1 - 20 * 12000, 1, 12000, S) == 2 ** 31 - 1
