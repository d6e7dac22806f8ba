#!/usr/bin/env python3
"""Generates tests/golden/timeline_sync.json by RUNNING the reference's own Sushi (backend/sushi: create_arg_parser() and run(args),
the WAV path of the GUI's Timeline Sync tab) in-process on synthesized WAV pairs and scripts.

Stubs for what this container lacks, each restating a documented behaviour:
  * cv2.matchTemplate(TM_SQDIFF_NORMED) -> tests/audio_match_ref.py (the exact-integer form of the value; cv2's own float32
    DFT can differ in the last bits and on near-ties);
  * cv2.resize(INTER_NEAREST) -> src index = min(floor(j * (1 / (dst / src))), src - 1);
  * chardet.detect -> utf-8-sig when the bytes start with a BOM, else utf-8;
  * imageio_ffmpeg.get_ffmpeg_exe -> a path that is never run (WAV inputs need no ffmpeg);
  * numpy.empty inside wav.py -> numpy.zeros: a sample no chunk writes holds 0.0, what a fresh allocation holds in practice
    (memory reused from an earlier scenario would otherwise leave it to chance).
Per scenario the JSON holds the synth recipes and SHA-256 of both WAVs, the options, the input script, the expected output and
every search the reference made: [src_off, m, dst_off, win_len] -> [index, float32 bits].  Only inputs and outputs are written
(data, not source).  Needs /root/reference; not run on the GPU box and never by pytest.
"""
import hashlib
import json
import logging
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
OUT = os.path.join(HERE, "timeline_sync.json")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import audio_match_ref  # noqa: E402
from vse_amd import synth  # noqa: E402

SEARCHES = []
STREAMS = []          # (data array, name) of every WavStream made, in order


def _offset(view):
    for arr, name in STREAMS:
        base = arr.ctypes.data
        if base <= view.ctypes.data < base + arr.nbytes:
            return name, view.ctypes.data - base
    raise AssertionError("array outside the registered streams")


def _match_template(image, templ, method):
    (_, do), (_, so) = _offset(image), _offset(templ)
    v = audio_match_ref.values(templ[0], image[0])
    k = int(np.argmin(v))
    SEARCHES.append([so, templ.shape[1], do, image.shape[1], k, int(v[k].view(np.uint32))])
    return v[None]


def _resize(a, dsize, interpolation=0):
    w, src = dsize[0], a.shape[1]
    idx = np.minimum(np.floor(np.arange(w) * (1.0 / (w / src))).astype(np.int64), src - 1)
    return a[:, idx]


def install_stubs():
    cv2 = types.ModuleType("cv2")
    cv2.TM_SQDIFF_NORMED, cv2.INTER_NEAREST = 1, 0
    cv2.matchTemplate, cv2.resize = _match_template, _resize
    chardet = types.ModuleType("chardet")
    chardet.detect = lambda raw: {"encoding": "utf-8-sig" if raw.startswith(b"\xef\xbb\xbf") else "utf-8"}
    ff = types.ModuleType("imageio_ffmpeg")
    ff.get_ffmpeg_exe = lambda: "ffmpeg-is-not-run-for-wav"
    sys.modules.update({"cv2": cv2, "chardet": chardet, "imageio_ffmpeg": ff})
    sys.path.insert(0, os.path.join(REF, "backend"))
    import sushi
    from sushi import wav
    class ZeroedNumpy:
        empty = staticmethod(np.zeros)

        def __getattr__(self, name):
            return getattr(np, name)
    wav.np = ZeroedNumpy()
    orig = wav.WavStream.__init__

    def init(self, path, *a, **k):
        orig(self, path, *a, **k)
        STREAMS.append((self.data, path))
    wav.WavStream.__init__ = init
    sushi.WavStream = wav.WavStream
    return sushi


# ---- scenarios -------------------------------------------------------------------------------------------------------------------

def speech(seed, seconds, a, b):
    return ["speech", seed, seconds, a, b]


def noise(seed, seconds, level):
    return ["noise", seed, seconds, level]


def srt(lines):
    return "\n".join(f"{i + 1}\n{t(s)} --> {t(e)}\n{text}\n" for i, (s, e, text) in enumerate(lines))


def t(sec):
    ms = int(round(sec * 1000))
    return f"{ms // 3600000:02d}:{ms // 60000 % 60:02d}:{ms // 1000 % 60:02d},{ms % 1000:03d}"


def regular_lines(first, last, step=4.0, dur=2.5):
    out, s, k = [], first, 0
    while s + dur <= last:
        out.append((s, s + dur, f"line {k}"))
        s += step + (k % 3) * 0.35
        k += 1
    return out


def ass(events, bom=True):
    head = ("[Script Info]\n; made for the timeline sync tests\nTitle: sync\nScriptType: v4.00+\nPlayResX: 640\nPlayResY: 360\n\n"
            "[V4+ Styles]\nFormat: Name, Fontname, Fontsize, PrimaryColour, SecondaryColour, OutlineColour, BackColour, Bold, Italic, "
            "Underline, StrikeOut, ScaleX, ScaleY, Spacing, Angle, BorderStyle, Outline, Shadow, Alignment, MarginL, MarginR, MarginV, "
            "Encoding\nStyle: Default,Arial,20,&H00FFFFFF,&H000000FF,&H00000000,&H00000000,0,0,0,0,100,100,0,0,1,2,2,2,10,10,10,1\n"
            "Style: Sign,Arial,16,&H00FFFFFF,&H000000FF,&H00000000,&H00000000,0,0,0,0,100,100,0,0,1,2,2,8,10,10,10,1\n\n"
            "[Events]\nFormat: Layer, Start, End, Style, Name, MarginL, MarginR, MarginV, Effect, Text\n")

    def at(sec):
        cs = int(round(sec * 100))
        return f"{cs // 360000}:{cs // 6000 % 60:02d}:{cs // 100 % 60:02d}.{cs % 100:02d}"
    body = "".join(f"{kind}: 0,{at(s)},{at(e)},{style},,0,0,0,,{text}\n" for kind, s, e, style, text in events)
    tail = "\n[Fonts]\nfontname: none.ttf\n\n[Aegisub Project Garbage]\nActive Line: 3\n"
    return ("\ufeff" if bom else "") + head + body + tail


def scenarios():
    S = []
    base = [speech(11, 80, 0, 80)]
    lines = regular_lines(2.0, 76.0)

    S.append(dict(name="constant_offset", src=dict(pieces=base), dst=dict(pieces=[noise(21, 2.5, 300)] + base),
                  script=srt(lines), ext=".srt", args=[]))
    S.append(dict(name="inserted_segment", src=dict(pieces=base),
                  dst=dict(pieces=[noise(22, 1.0, 300), speech(11, 80, 0, 36), noise(23, 18.0, 4000), speech(11, 80, 36, 80)]),
                  script=srt(lines), ext=".srt", args=[]))
    S.append(dict(name="removed_segment", src=dict(pieces=base),
                  dst=dict(pieces=[speech(11, 80, 0, 30), speech(11, 80, 36, 80)]), script=srt(lines), ext=".srt", args=[]))
    S.append(dict(name="destination_shorter", src=dict(pieces=base), dst=dict(pieces=[noise(24, 1.0, 300), speech(11, 80, 0, 50)]),
                  script=srt(lines), ext=".srt", args=[]))
    S.append(dict(name="gain_and_noise", src=dict(pieces=base),
                  dst=dict(pieces=[noise(25, 1.2, 300)] + base, gain=[1, 2], noise=[26, 400]), script=srt(lines), ext=".srt", args=[]))
    S.append(dict(name="rates_48k_stereo_vs_44k1_mono",
                  src=dict(pieces=[speech(12, 61, 0, 61)], rate=48000, channels=2, trim=48000 - 5, extensible=True),
                  dst=dict(pieces=[noise(27, 0.75, 300), speech(12, 61, 0, 61)], rate=44100, trim=33075 - 5,
                           list_chunk=True),
                  script=srt(regular_lines(1.5, 57.0)), ext=".srt", args=[]))
    tricky = [(2.0, 4.5, "first"), (4.0, 6.0, "overlaps the first"), (8.0, 8.0, "zero duration"), (10.0, 12.5, "twice"),
              (10.0, 12.5, "twice (same times)"), (14.0, 14.2, "short a"), (14.25, 14.4, "short b"), (14.3, 14.35, "short c"),
              (18.0, 20.0, "after"), (22.0, 26.0, "long"), (23.0, 24.0, "inside long"), (30.0, 32.0, "next"),
              (31.0, 31.3, "short inside"), (36.0, 38.5, "tail"), (44.0, 46.0, "more"), (52.0, 54.0, "end")]
    S.append(dict(name="srt_tricky_lines", src=dict(pieces=base), dst=dict(pieces=[noise(28, 3.3, 300)] + base), script=srt(tricky),
                  ext=".srt", args=[]))
    ev = [("Comment", 0.0, 0.0, "Default", "comment at the top"), ("Dialogue", 2.0, 4.5, "Default", "hello, world"),
          ("Dialogue", 6.0, 8.0, "Sign", "{\\pos(10,10)}a sign"), ("Comment", 9.0, 10.0, "Default", "a comment"),
          ("Dialogue", 11.0, 13.5, "Default", "line three"), ("Dialogue", 12.0, 12.3, "Sign", "short sign"),
          ("Dialogue", 16.0, 18.0, "Default", "four"), ("Dialogue", 20.0, 23.0, "Default", "five"),
          ("Dialogue", 26.0, 28.0, "Default", "six"), ("Dialogue", 31.0, 33.0, "Default", "seven"),
          ("Dialogue", 37.0, 40.0, "Default", "eight"), ("Dialogue", 44.0, 46.0, "Default", "nine"),
          ("Comment", 70.0, 71.0, "Default", "last comment")]
    S.append(dict(name="ass_bom_comments_sections", src=dict(pieces=base), dst=dict(pieces=[noise(29, 1.7, 300)] + base),
                  script=ass(ev), ext=".ass", args=[]))
    S.append(dict(name="no_grouping", src=dict(pieces=base),
                  dst=dict(pieces=[noise(30, 0.5, 300), speech(11, 80, 0, 40), noise(31, 2.0, 3000), speech(11, 80, 40, 80)]),
                  script=srt(lines), ext=".srt", args=["--no-grouping"]))
    S.append(dict(name="small_windows", src=dict(pieces=base),
                  dst=dict(pieces=[speech(11, 80, 0, 30), noise(32, 9.0, 4000), speech(11, 80, 30, 80)]), script=srt(lines), ext=".srt",
                  args=["--window", "5", "--max-window", "15", "--rewind-thresh", "3"]))
    S.append(dict(name="smooth_radius_0", src=dict(pieces=base), dst=dict(pieces=[noise(33, 2.0, 300)] + base, noise=[34, 900]),
                  script=srt(lines), ext=".srt", args=["--smooth-radius", "0"]))
    S.append(dict(name="sample_rate_8000", src=dict(pieces=base), dst=dict(pieces=[noise(35, 1.4, 300)] + base), script=srt(lines),
                  ext=".srt", args=["--sample-rate", "8000"]))
    return S


def run_one(sushi, sc, tmp):
    from sushi.__main__ import create_arg_parser
    paths = {}
    rec = {"name": sc["name"], "args": sc["args"], "ext": sc["ext"], "script": sc["script"]}
    for side in ("src", "dst"):
        data = synth.audio_from_recipe(sc[side])
        paths[side] = os.path.join(tmp, f"{sc['name']}_{side}.wav")
        with open(paths[side], "wb") as f:
            f.write(data)
        rec[side] = {"recipe": sc[side], "sha256": hashlib.sha256(data).hexdigest()}
    script = os.path.join(tmp, sc["name"] + "_in" + sc["ext"])
    out = os.path.join(tmp, sc["name"] + "_out" + sc["ext"])
    with open(script, "wb") as f:
        f.write(sc["script"].encode("utf-8"))
    del SEARCHES[:], STREAMS[:]
    args = create_arg_parser().parse_args(["--src", paths["src"], "--dst", paths["dst"], "--script", script, "-o", out] + sc["args"])
    sushi.run(args)
    with open(out, "rb") as f:
        rec["output"] = f.read().decode("utf-8")
    rec["searches"] = list(SEARCHES)
    return rec


def main():
    logging.disable(logging.CRITICAL)
    sushi = install_stubs()
    recs = []
    with tempfile.TemporaryDirectory() as tmp:
        for sc in scenarios():
            recs.append(run_one(sushi, sc, tmp))
            print(f"{sc['name']}: {len(recs[-1]['searches'])} searches", file=sys.stderr)
    with open(OUT, "w") as f:
        json.dump({"scenarios": recs}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)", file=sys.stderr)


if __name__ == "__main__":
    main()
