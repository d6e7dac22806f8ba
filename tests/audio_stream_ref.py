"""The integer form of vse_amd.timeline_sync.AudioStream (include/vse_hip.h, the vse_audio_stream_* section) in numpy: what the
device kernels compute, restated on the host.  integer_stream is the whole specification in one function; NumpyBuilder has the
feed / finish contract of DeviceAudioStream's `build`, so the class runs without a GPU.  Both are held equal to AudioStream's own
bytes by tests/test_audio_stream.py."""
import math

import numpy as np


class Refused(Exception):
    """What the size queries answer with 0 (`kind` = "arguments") and what feed refuses for the last chunk ("too few")."""

    def __init__(self, kind, text):
        super().__init__(text)
        self.kind = kind


def geometry(frames, channels, rate, sample_rate):
    """-> dict of sample_count, P, L, K, n_last, new_last; Refused for what the entry points refuse."""
    if not 1 <= channels <= 8 or rate < sample_rate or frames < 1:
        raise Refused("arguments", f"{frames} frames, {channels} channels, {rate} Hz -> {sample_rate} Hz")
    sample_count = math.ceil(frames / float(rate) * sample_rate)
    length = 20 * rate + sample_count
    if length > 2 ** 31 - 1:
        raise Refused("arguments", f"stream length {length}")
    chunks = -(-frames // rate)
    n_last = frames - (chunks - 1) * rate
    new_last = int(round(n_last * (sample_rate / float(rate))))
    if new_last == 0 and sample_rate != rate:
        raise Refused("too few", f"the last {n_last} frames are too few to resample")
    return dict(sample_count=sample_count, P=10 * rate, L=length, K=chunks, n_last=n_last, new_last=new_last)


def chunk_samples(pcm, rate, sample_rate, new_k):
    """pcm: int16 [n_k, C] of one chunk -> the int32 sums of its new_k samples."""
    s = pcm.astype(np.int32).sum(axis=1, dtype=np.int32)
    if sample_rate == rate:
        return s
    n_k = len(s)
    scale = 1.0 / (new_k / n_k)
    idx = np.minimum(np.floor(np.arange(new_k, dtype=np.int64).astype(np.float64) * scale).astype(np.int64), n_k - 1)
    return s[idx]


def level(s, channels):
    """f(s): the float32 the host holds for the integer sum s."""
    x = np.asarray(s).astype(np.float32)
    return x if channels == 1 else x / np.float32(channels)


def median3(sorted_ints, channels):
    """3 x the float32 median of f over a non-empty ascending int array."""
    n = len(sorted_ints)
    if n & 1:
        m = np.float32(level(sorted_ints[n // 2], channels))
    else:
        m = np.float32(np.float32(level(sorted_ints[n // 2 - 1], channels)) + np.float32(level(sorted_ints[n // 2], channels))) / np.float32(2)
    return np.float32(m * np.float32(3))


def levels_and_stream(samples, padding, channels):
    """samples: int32 [L] with the chunks written and the paddings still unset -> (uint8 stream or None, lo, hi, n_ge0, n_le0, status)."""
    s = samples
    s[:padding] = s[padding]
    s[len(s) - padding:] = s[len(s) - padding - 1]
    ge, le = np.sort(s[s >= 0]), np.sort(s[s <= 0])
    nan = np.float32(np.nan)
    hi = median3(ge, channels) if len(ge) else nan
    lo = median3(le, channels) if len(le) else nan
    if not len(ge) or not len(le) or np.float32(hi - lo) == 0:
        return None, lo, hi, len(ge), len(le), 1
    x = level(s, channels)
    x = np.minimum(np.maximum(x, lo), hi)
    y = ((x - lo) / np.float32(hi - lo)) * np.float32(255.0) + np.float32(0.5)
    assert y.dtype == np.float32
    return y.astype(np.int32).astype(np.uint8), lo, hi, len(ge), len(le), 0


def integer_stream(pcm, rate, sample_rate):
    """pcm: int16 [F, C] -> (uint8 stream or None, lo, hi, n_ge0, n_le0, status); Refused as geometry."""
    frames, channels = pcm.shape
    g = geometry(frames, channels, rate, sample_rate)
    s = np.zeros(g["L"], np.int32)
    for k in range(g["K"]):
        chunk = pcm[k * rate:(k + 1) * rate]
        new_k = sample_rate if len(chunk) == rate else g["new_last"]
        at = g["P"] + k * sample_rate
        s[at:at + new_k] = chunk_samples(chunk, rate, sample_rate, new_k)
    return levels_and_stream(s, g["P"], channels)


class NumpyBuilder:
    """`build` of DeviceAudioStream on the host: build(frames, channels, rate, sample_rate) -> an object with
    feed(pcm int16 [n, C], first_second) and finish() -> (stream, lo, hi, n_ge0, n_le0, status).  Unfed samples hold a value no audio
    can reach, so a chunk that was never fed shows in the bytes."""

    def __init__(self, frames, channels, rate, sample_rate):
        self.g = geometry(frames, channels, rate, sample_rate)
        self.frames, self.channels, self.rate, self.sample_rate = frames, channels, rate, sample_rate
        self.s = np.full(self.g["L"], 32767 * channels, np.int32)
        self.fed = []

    def feed(self, pcm, first_second):
        pcm = np.asarray(pcm)
        assert pcm.dtype == np.int16 and pcm.ndim == 2 and pcm.shape[1] == self.channels and len(pcm) >= 1
        start = first_second * self.rate
        assert 0 <= first_second < self.g["K"] and start + len(pcm) <= self.frames
        assert len(pcm) % self.rate == 0 or start + len(pcm) == self.frames, "a piece is whole seconds unless it ends the file"
        self.fed.append((first_second, len(pcm)))
        g = self.g
        for c in range(-(-len(pcm) // self.rate)):
            k = first_second + c
            chunk = pcm[c * self.rate:(c + 1) * self.rate]
            last = k == g["K"] - 1
            new_k = g["new_last"] if last else self.sample_rate
            at = g["P"] + k * self.sample_rate
            self.s[at:at + new_k] = chunk_samples(chunk, self.rate, self.sample_rate, new_k)
            if last:
                self.s[at + new_k:g["P"] + g["sample_count"]] = 0

    def finish(self):
        return levels_and_stream(self.s.copy(), self.g["P"], self.channels)


def make_pcm(kind, frames, channels, seed=0):
    """Test audio, int16 [frames, channels].  tiny: -3..3 (heavy ties); nonneg: 0..40; positive: 1..40; speech: a normal
    distribution of deviation 3000; full: every value of int16; ends: -32768 or 32767 on all channels of a frame at once, so the
    sums sit at both ends of the bin range; zero: silence."""
    rng = np.random.default_rng(seed)
    shape = (frames, channels)
    if kind == "tiny":
        x = rng.integers(-3, 4, shape)
    elif kind == "nonneg":
        x = rng.integers(0, 41, shape)
    elif kind == "positive":
        x = rng.integers(1, 41, shape)
    elif kind == "speech":
        x = np.clip(np.rint(rng.normal(0.0, 3000.0, shape)), -32768, 32767)
    elif kind == "full":
        x = rng.integers(-32768, 32768, shape)
    elif kind == "ends":
        x = np.repeat(np.where(rng.integers(0, 2, (frames, 1)) == 1, 32767, -32768), channels, axis=1)
    elif kind == "zero":
        x = np.zeros(shape)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, dtype=np.int16)


def host_float_levels(pcm, rate, sample_rate):
    """(lo, hi, n_ge0, n_le0) as AudioStream's own float pipeline has them (it keeps none of them): the same calls in the same
    order on the same float32 array, up to the medians."""
    from vse_amd import timeline_sync as ts
    frames, channels = pcm.shape
    sample_count = math.ceil(frames / float(rate) * sample_rate)
    padding = 10 * rate
    data = np.zeros(20 * rate + sample_count, np.float32)
    at = padding
    for k in range(-(-frames // rate)):
        chunk = ts._downmix(pcm[k * rate:(k + 1) * rate].tobytes(), channels)
        new_length = int(round(len(chunk) * (sample_rate / float(rate))))
        if sample_rate != rate:
            chunk = ts._resize_nearest(chunk, new_length)
        data[at:at + new_length] = chunk
        at += new_length
    data[0:padding] = data[padding]
    data[-padding:] = data[-padding - 1]
    ge, le = data[data >= 0], data[data <= 0]
    with np.errstate(all="ignore"):
        hi = np.float32(np.median(ge) * 3) if len(ge) else np.float32(np.nan)
        lo = np.float32(np.median(le) * 3) if len(le) else np.float32(np.nan)
    return lo, hi, len(ge), len(le)
