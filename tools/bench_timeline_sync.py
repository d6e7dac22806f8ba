#!/usr/bin/env python3
"""Timeline sync cost on a synthesized long pair (vse_amd.timeline_sync).

Default run: a 45-minute pair at 12 kHz mono (about 65 MB per WAV) whose destination has an offset, an inserted segment and a
cut, with one line every ~3 s; a 5-minute and a 30-minute 48 kHz stereo pair for the cost of downmixing and resampling.  Reports
  * stream preparation (WAV -> uint8 stream) per file, on the host (AudioStream) and on the device (DeviceAudioStream: file read,
    upload, kernels and the read-back that waits for them), the two alternating, three times each after a warm-up: median and
    spread (max - min);
  * GPU search time: device events around every vse_audio_match call, per call class and in total;
  * end-to-end sync() time with the GPU searcher in both stream_build modes, alternating in the same way, and the share of it that
    preparation takes in each;
  * the same run with the numpy searcher (tests/audio_match_ref.py: float64 FFT, not cv2), the queries of a call on a pool of
    --threads threads.
--kernels: only fixed series of calls per class (small window, normal step of 3 queries, max-window step), for a separate
`rocprofv3 --kernel-trace --stats` run; --trace <kernel_trace.csv> then joins that trace to the classes and prints kernel time,
MACs (m x offsets, from the shapes) and the share of the i8 dense MFMA peak.

usage: python tools/bench_timeline_sync.py [--minutes 45] [--sizes hd48k,main,hd30] [--threads 16] [--no-numpy] [--kernels [--reps 20]]
       [--trace CSV]"""
import argparse
import csv
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

from vse_amd import synth, timeline_sync as ts  # noqa: E402

I8_PEAK_MACS = 2.5e15       # i8 MFMA, dense: twice the BF16 rate (~2.5 PFLOPS), MI355X_MICROARCH.md Matrix cores
RATE = 12000
CLASSES = {"small": 3.0, "normal": 20.0, "max": 60.0}     # window widths in seconds (+-1.5, +-10, +-30)


def long_pair(minutes, rate=RATE, channels=1, seed=41):
    """Recipes: destination = 2 s lead-in, source up to 40 %, a 12 s insert, the rest minus a 7 s cut at 70 %."""
    secs = minutes * 60
    a, b = round(secs * 0.4), round(secs * 0.7)
    sp = lambda x, y: ["speech", seed, secs, x, y]           # noqa: E731
    src = dict(pieces=[sp(0, secs)], rate=rate, channels=channels)
    dst = dict(pieces=[["noise", seed + 1, 2.0, 300], sp(0, a), ["noise", seed + 2, 12.0, 3000], sp(a, b), sp(b + 7, secs)],
               rate=rate if channels == 1 else 44100)
    return src, dst


def script(minutes):
    lines, s, k = [], 1.0, 0
    while s + 2.2 < minutes * 60:
        lines.append(f"{k + 1}\n{ts.format_srt_time(s)} --> {ts.format_srt_time(s + 2.2)}\nline {k}\n")
        s += 2.6 + (k % 4) * 0.3
        k += 1
    return "\n".join(lines), k


class TimedGpuSearch(ts.GpuSearch):
    def __init__(self, ctx):
        super().__init__(ctx)
        self.calls = []

    def __call__(self, queries):
        t = self.ctx.torch
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        need = self.ctx.audio_match_workspace_bytes(queries)
        if self.ws is None or self.ws.numel() < need:
            self.ws = t.empty(max(need, 256), dtype=t.uint8, device=self.ctx.tdev)
        e0.record()
        out = self.ctx.audio_match(self.src, self.dst, queries, workspace=self.ws)
        e1.record()
        out = out.cpu().numpy()
        macs = sum(m * (wl - m + 1) for _, m, _, wl in queries)
        self.calls.append((len(queries), max(wl - m + 1 for _, m, _, wl in queries), macs, e0.elapsed_time(e1)))
        vals = out[:, 1].copy().view(np.float32)
        return [(int(k), vals[i]) for i, k in enumerate(out[:, 0])]


class ThreadedNumpySearch:
    def __init__(self, threads):
        from audio_match_ref import NumpySearch
        self.inner = NumpySearch()
        self.pool = ThreadPoolExecutor(threads)

    def load(self, src, dst):
        self.inner.load(src, dst)

    def __call__(self, queries):
        return list(self.pool.map(lambda q: self.inner([q])[0], queries))


def call_class(nq, offsets):
    if nq == 1:
        return "small"
    return "max" if offsets > 30 * RATE * 1.5 else "normal"


def run_sync(tmp, search, stream_build="host"):
    t0 = time.perf_counter()
    log = ts.sync(os.path.join(tmp, "src.wav"), os.path.join(tmp, "dst.wav"), os.path.join(tmp, "in.srt"), os.path.join(tmp, "out.srt"),
                  search=search, stream_build=stream_build)
    return time.perf_counter() - t0, log


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def spread(xs):
    """Three repeats -> their median, and (max - min) as the spread."""
    return round(sorted(xs)[len(xs) // 2], 4), round(max(xs) - min(xs), 4)


# name -> (minutes, recipe pair): the 5-minute 48 kHz stereo pair, the long 12 kHz mono pair, a 30-minute 48 kHz stereo pair
def sizes(a):
    return {"hd48k": (5, long_pair(5, 48000, 2, seed=43)), "main": (a.minutes, long_pair(a.minutes)),
            "hd30": (30, long_pair(30, 48000, 2, seed=47))}


def measure_pair(ctx, name, minutes, pair, a, res):
    """Stream preparation per file on the host and on the device, and sync() end to end in both modes: the two modes alternate,
    three times each after a warm-up, in this one process.  The device figure is a host clock around DeviceAudioStream: file
    read (from the page cache: the WAVs were just written), upload, kernels and the read-back of the result record, which waits for
    the device."""
    with tempfile.TemporaryDirectory() as tmp:
        for side, r in zip(("src", "dst"), pair):
            with open(os.path.join(tmp, f"{side}.wav"), "wb") as f:
                f.write(synth.audio_from_recipe(r))
        text, nlines = script(minutes)
        with open(os.path.join(tmp, "in.srt"), "w") as f:
            f.write(text)
        for side in ("src", "dst"):
            p = os.path.join(tmp, f"{side}.wav")
            res[f"wav_{name}_{side}_MB"] = round(os.path.getsize(p) / 1e6, 1)
            dev = ts.DeviceAudioStream(p, ctx=ctx)                  # warm-up (module load, allocator) and the byte check
            res[f"same_bytes_{name}_{side}"] = bool(np.array_equal(dev.data.cpu().numpy(), ts.AudioStream(p).data))
            del dev
            host, device = [], []
            for _ in range(3):
                host.append(timed(lambda: ts.AudioStream(p)))
                device.append(timed(lambda: ts.DeviceAudioStream(p, ctx=ctx)))
            res[f"prep_{name}_{side}_s"], res[f"prep_{name}_{side}_spread_s"] = spread(host)
            res[f"prep_device_{name}_{side}_s"], res[f"prep_device_{name}_{side}_spread_s"] = spread(device)
        gs = TimedGpuSearch(ctx)
        run_sync(tmp, gs, "device")                                 # warm-up (module load, workspace)
        times = {"host": [], "device": []}
        logs = {}
        for _ in range(3):
            for mode in ("host", "device"):
                gs.calls.clear()
                t, logs[mode] = run_sync(tmp, gs, mode)
                times[mode].append(t)
        key = "sync_gpu" if name == "main" else f"sync_gpu_{name}"
        res[f"{key}_s"], res[f"{key}_spread_s"] = spread(times["host"])
        res[f"{key}_device_build_s"], res[f"{key}_device_build_spread_s"] = spread(times["device"])
        res[f"same_searches_{name}"] = logs["host"] == logs["device"]
        res[f"lines_{name}"] = nlines
        res[f"search_gpu_total_{name}_s"] = round(sum(c[3] for c in gs.calls) / 1e3, 4)
        for mode, pre in (("host", "prep"), ("device", "prep_device")):
            prep = res[f"{pre}_{name}_src_s"] + res[f"{pre}_{name}_dst_s"]
            total = res[f"{key}_s"] if mode == "host" else res[f"{key}_device_build_s"]
            res[f"prep_share_of_sync_{name}_{mode}"] = round(prep / total, 3)
        if name != "main":
            return
        per = {}
        for nq, offs, macs, ms in gs.calls:
            c = per.setdefault(call_class(nq, offs), [0, 0.0, 0])
            c[0] += 1
            c[1] += ms
            c[2] += macs
        for k, (n, ms, macs) in per.items():
            res[f"calls_{k}"] = n
            res[f"search_{k}_ms_per_call"] = round(ms / n, 4)
            res[f"search_{k}_GMAC_per_call"] = round(macs / n / 1e9, 2)
        res["lines"] = nlines
        res["search_gpu_total_s"] = res["search_gpu_total_main_s"]
        res["searches"] = len(logs["host"])
        if not a.no_numpy:
            res["sync_numpy_fft_not_cv2_s"], nlog = run_sync(tmp, ThreadedNumpySearch(a.threads))
            res["numpy_threads"] = a.threads
            res["numpy_same_searches"] = [x[:5] for x in nlog] == [x[:5] for x in logs["host"]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=45)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--sizes", default="hd48k,main,hd30", help="which pairs to run, of hd48k, main, hd30")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", default=None)
    a = ap.parse_args()
    if a.trace:
        return summarize_trace(a.trace, a.reps)
    from vse_amd import engine
    ctx = engine.Context(0)
    if a.kernels:
        return kernel_series(ctx, a.reps)
    res = {}
    table = sizes(a)
    for name in a.sizes.split(","):
        minutes, pair = table[name]
        measure_pair(ctx, name, minutes, pair, a, res)
        print(f"{name} done: {json.dumps(res)}", file=sys.stderr, flush=True)      # (progress; the result is the last line)
    print(json.dumps(res))


def kernel_series(ctx, reps):
    """reps calls per class, classes in order small, normal, max; 3 s (36 000-sample) groups on 45-minute-like streams."""
    rng = np.random.default_rng(1)
    n = 10 * 60 * RATE
    src = rng.integers(90, 166, n, dtype=np.uint8)
    dst = rng.integers(90, 166, n, dtype=np.uint8)
    gs = TimedGpuSearch(ctx)
    gs.load(src, dst)
    m = 3 * RATE
    out = {}
    for cls, width in CLASSES.items():
        w = int(width * RATE)
        for r in range(reps):
            so, do = 100000 + 7919 * r, 200000 + 6007 * r
            if cls == "small":
                q = [(so, m, do, w + m)]
            else:
                q = [(so, m, do, w + m), (so, m // 2, do, w + m // 2), (so + m // 2, m - m // 2, do + m // 2, w + m - m // 2)]
            gs(q)
        calls = gs.calls[-reps:]
        out[cls] = {"calls": reps, "GMAC_per_call": round(calls[0][2] / 1e9, 3),
                    "event_ms_per_call": round(sorted(c[3] for c in calls)[reps // 2], 4)}
    print(json.dumps(out))


def summarize_trace(path, reps):
    """Kernel durations of a --kernels run, per class: the two kernels of each call, in launch order."""
    rows = [r for r in csv.DictReader(open(path)) if "audio_match" in r.get("Kernel_Name", "")]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    calls = [(rows[i], rows[i + 1]) for i in range(0, len(rows) - 1, 2)]
    m = 3 * RATE
    out = {}
    for ci, (cls, width) in enumerate(CLASSES.items()):
        mine = calls[ci * reps:(ci + 1) * reps]
        w = int(width * RATE)
        macs = m * (w + 1) if cls == "small" else m * (w + 1) + 2 * (m // 2) * (w + 1)
        main_us = sorted((int(a["End_Timestamp"]) - int(a["Start_Timestamp"])) / 1e3 for a, _ in mine)[len(mine) // 2]
        fin_us = sorted((int(b["End_Timestamp"]) - int(b["Start_Timestamp"])) / 1e3 for _, b in mine)[len(mine) // 2]
        out[cls] = {"GMAC": round(macs / 1e9, 3), "main_us": round(main_us, 2), "finalize_us": round(fin_us, 2),
                    "i8_peak_share_main": round(macs / (main_us * 1e-6) / I8_PEAK_MACS, 3),
                    "i8_peak_share_both": round(macs / ((main_us + fin_us) * 1e-6) / I8_PEAK_MACS, 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
