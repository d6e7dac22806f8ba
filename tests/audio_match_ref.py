"""The audio template search of timeline sync in numpy (the contract of vse_audio_match, include/vse_hip.h), and NumpySearch, a
searcher with the call signature of the engine's (vse_amd.timeline_sync.GpuSearch).  For a uint8 pattern p[0..m) and window
w[0..n+m-1), per offset k:
    X_k = sum p[i] w[k+i], S_k = sum w[k+i]^2, P = sum p[i]^2                 (exact int64)
    num = float64(max(S_k - 2 X_k + P, 0)), den = sqrt(float64 S_k) * sqrt(float64 P)
    v_k = float32(num / den) if num < den else 1.0
-> (first argmin k, v_k).  The cross term comes from a float64 FFT correlation rounded to int64 (direct int64 for small sizes)."""
import math

import numpy as np


def cross_terms(p, w):
    """int64 X_k for k in [0, len(w) - len(p) + 1)."""
    p = np.asarray(p, np.int64)
    w = np.asarray(w, np.int64)
    m = len(p)
    n = len(w) - m + 1
    if m * n <= 1 << 22:
        return np.array([int(np.dot(p, w[k:k + m])) for k in range(n)], np.int64) if n < 64 else \
            np.lib.stride_tricks.sliding_window_view(w, m)[:n] @ p
    size = 1 << int(math.ceil(math.log2(len(w) + m)))
    x = np.fft.irfft(np.fft.rfft(w.astype(np.float64), size) * np.conj(np.fft.rfft(p.astype(np.float64), size)), size)[:n]
    xi = np.rint(x).astype(np.int64)
    err = np.abs(x - xi).max()
    assert err < 0.25, f"FFT cross term not exact enough: {err}"
    return xi


def values(p, w):
    """float32 v_k of every offset."""
    p = np.asarray(p, np.int64)
    w = np.asarray(w, np.int64)
    m = len(p)
    n = len(w) - m + 1
    x = cross_terms(p, w)
    c = np.concatenate([[0], np.cumsum(w * w)])
    s = c[m:m + n] - c[:n]
    pp = int((p * p).sum())
    num = np.maximum(s - 2 * x + pp, 0).astype(np.float64)
    den = np.sqrt(s.astype(np.float64)) * math.sqrt(float(pp))
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(num < den, num / np.where(den > 0, den, 1.0), 1.0)
    return v.astype(np.float32)


def match(p, w):
    """(first argmin offset, float32 value)."""
    v = values(p, w)
    k = int(np.argmin(v))
    return k, v[k]


class NumpySearch:
    """Searcher over two uint8 streams: load(src, dst), then __call__([(src_off, m, dst_off, win_len), ...]) ->
    [(index, float32 value), ...], as the engine's searcher."""

    def load(self, src, dst):
        self.src = np.ascontiguousarray(src, np.uint8)
        self.dst = np.ascontiguousarray(dst, np.uint8)

    def __call__(self, queries):
        out = []
        for so, m, do, wl in queries:
            assert m >= 1 and wl >= m and 0 <= so <= len(self.src) - m and 0 <= do <= len(self.dst) - wl
            out.append(match(self.src[so:so + m], self.dst[do:do + wl]))
        return out
