"""numpy restatement of vse_ctc_fuse (include/vse_hip.h), bit for bit: per group and step the member rows' probabilities are summed in
float32 in member order, divided once by (float)K, and the first index of the largest mean is taken; steps at or behind a group's
length give {0, 0.0}.  Plus the greedy CTC decode of such a row."""
import numpy as np


def fuse(probs, group, tlen=None):
    """probs: float32 [B, T, ncls]; group: g + 1 ascending row offsets; tlen: g lengths or None -> (idx int32 [g, T], maxp float32 [g, T])."""
    probs = np.asarray(probs)
    assert probs.dtype == np.float32 and probs.ndim == 3
    g, T = len(group) - 1, probs.shape[1]
    idx, maxp = np.zeros((g, T), np.int32), np.zeros((g, T), np.float32)
    for j in range(g):
        rows = range(group[j], group[j + 1])
        n = T if tlen is None else min(max(int(tlen[j]), 0), T)
        acc = probs[rows[0], :n].copy()
        for r in rows[1:]:
            acc = acc + probs[r, :n]                       # float32 + float32, rounded once per add
        m = acc / np.float32(len(rows))                    # a correctly rounded float32 divide
        assert m.dtype == np.float32
        if n:
            idx[j, :n] = m.argmax(axis=1)                  # the first index of the largest value
            maxp[j, :n] = m[np.arange(n), idx[j, :n]]
    return idx, maxp


def ctc_greedy(idx, maxp, n=None):
    """One row -> (kept class ids, mean of their maxp as float32 or 0.0): keep step t when idx[t] != 0 and idx[t] != idx[t-1]."""
    idx, maxp = np.asarray(idx)[:n], np.asarray(maxp)[:n]
    keep = (idx != 0) & (idx != np.concatenate([[-1], idx[:-1]]))
    ids = [int(v) for v in idx[keep]]
    return ids, float(np.float32(maxp[keep].astype(np.float32).sum() / len(ids))) if ids else 0.0
