#!/usr/bin/env python3
"""Generates tests/golden/timeline_sync_keyframes.json by RUNNING the reference's own Sushi (backend/sushi) in-process, with
keyframes and timecodes, on synthesized WAV pairs and scripts.  The stubs for what this container lacks are those of
make_timeline_sync_golden.py (imported: it only defines them).

Per scenario the JSON holds the synth recipes and SHA-256 of both WAVs, the input script, the keyframes of both sides (frame
numbers and frame counts; the files handed to the reference are written with vse_amd.keyframes.write_keyframes), the timecodes
file texts, the options, every search the reference made ([src_off, m, dst_off, win_len] -> [index, float32 bits]), the expected
output and how often the reference logged each snapping step.  Beside the scenarios: probes of the reference's Timecodes
(constant fps, v1, v2) and one keyframes file with what the reference's parse_keyframes returns for it.  Only inputs and outputs
are written (data, not source).  Needs the reference checkout make_timeline_sync_golden.py points at; never run by pytest.
"""
import hashlib
import json
import logging
import math
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_timeline_sync_golden as base  # noqa: E402
from make_timeline_sync_golden import ass, noise, speech, srt  # noqa: E402
from vse_amd import keyframes as kfmod, synth  # noqa: E402

OUT = os.path.join(HERE, "timeline_sync_keyframes.json")
NTSC = 24000.0 / 1001.0
SECONDS = 80
SHIFT = 2.5


class Collect(logging.Handler):
    def __init__(self):
        super().__init__()
        self.messages = []

    def emit(self, record):
        self.messages.append(record.getMessage())


# ---- keyframes placed around the lines -----------------------------------------------------------------------------------------

def first_frame_at(t, fps):
    return int(math.ceil(t * fps - 1e-9))


#              (source frames off the line's first frame, destination jitter in frames; None: no keyframe on that side)
START_PLACES = [(0, 0), (-1, 1), (3, 0), None, (0, -1), (0, None), (1, 2)]
END_PLACES = [(0, 1), None, (1, 0), (4, 0), (0, -2)]


def place_keyframes(lines, src_time, dst_frame, shift=SHIFT, extra=()):
    """lines: [(start, end)] -> (src frames, dst frames).  src_time(frame) -> s; dst_frame(t) -> nearest destination frame.
    extra: (source frame, jitter) pairs placed as they are."""
    src, dst = {0}, {0}

    def put(frame, jitter):
        src.add(frame)
        if jitter is not None:
            dst.add(dst_frame(src_time(frame) + shift) + jitter)

    def src_frame_at(t):          # first source frame starting at or after t
        f = 0
        while src_time(f) < t - 1e-9:
            f += 1
        return f
    for k, (s, e) in enumerate(lines):
        p = START_PLACES[k % len(START_PLACES)]
        if p:
            put(src_frame_at(s) + p[0], p[1])
        p = END_PLACES[k % len(END_PLACES)]
        if p:
            put(src_frame_at(e) + 1 + p[0], p[1])
    for frame, jitter in extra:
        put(frame, jitter)
    return sorted(src), sorted(dst)


def cfr_time(fps):
    return lambda f: f / fps


def cfr_frame(fps):
    return lambda t: int(round(t * fps))


def v2_times(count, switch, fps_a, fps_b):
    """ms time stamps of `count` frames: fps_a up to frame `switch`, fps_b after it (a variable-frame-rate release)."""
    out, t = [], 0.0
    for f in range(count):
        out.append(t)
        t += 1000.0 / (fps_a if f < switch else fps_b)
    return out


def v2_text(times_ms):
    return "# timecode format v2\n" + "\n".join("%.3f" % t for t in times_ms) + "\n"


def nearest_frame(times_s):
    import bisect

    def f(t):
        i = bisect.bisect_left(times_s, t)
        if i == 0:
            return 0
        if i == len(times_s):
            return len(times_s) - 1
        return i if times_s[i] - t < t - times_s[i - 1] else i - 1
    return f


def lines_of(first, last, step=4.0, dur=2.5):
    out, s, k = [], first, 0
    while s + dur <= last:
        out.append((s, s + dur, f"line {k}"))
        s += step + (k % 3) * 0.35
        k += 1
    return out


def scenarios():
    S = []
    base_audio = [speech(11, 80, 0, SECONDS)]
    shifted = dict(pieces=[noise(21, SHIFT, 300)] + base_audio)
    lines = lines_of(2.0, SECONDS - 3.0)
    spans = [(s, e) for s, e, _ in lines]
    n_src, n_dst = int(SECONDS * NTSC) + 1, int((SECONDS + SHIFT) * NTSC) + 1
    kf = place_keyframes(spans, cfr_time(NTSC), cfr_frame(NTSC))

    def sc(name, ext=".srt", script=None, src=None, dst=None, keyframes=kf, counts=(n_src, n_dst), fps=(NTSC, NTSC), timecodes=(None, None),
           **options):
        S.append(dict(name=name, ext=ext, script=script or srt(lines), src=src or dict(pieces=base_audio), dst=dst or shifted,
                      keyframes=dict(src=[k for k in keyframes[0] if k < counts[0]], dst=[k for k in keyframes[1] if k < counts[1]]),
                      frame_count=dict(src=counts[0], dst=counts[1]),
                      fps=dict(src=fps[0], dst=fps[1]), timecodes=dict(src=timecodes[0], dst=timecodes[1]), options=options))

    sc("srt_cfr_all")
    sc("srt_cfr_shift", kf_mode="shift")
    sc("srt_cfr_snap", kf_mode="snap")
    sc("srt_max_kf_distance_0", max_kf_distance=0)
    sc("srt_max_kf_distance_3_5", max_kf_distance=3.5)
    sc("srt_no_grouping", grouping=False)

    # destination with v2 timecodes: 23.976 fps up to frame 500, 29.97 after it; the file ends at frame 1299 (47.5 s), and every
    # later frame takes the last time
    ms = v2_times(1300, 500, NTSC, 30000.0 / 1001.0)
    secs = [float("%.3f" % t) / 1000.0 for t in ms]
    sc("srt_v2_destination", keyframes=place_keyframes(spans, cfr_time(NTSC), nearest_frame(secs)), counts=(n_src, len(ms)),
       fps=(NTSC, None), timecodes=(None, v2_text(ms)))

    # source with v1 timecodes: 23.976 fps with frames 0..239 at 29.97; destination at 25 fps
    v1 = "# timecode format v1\nAssume 23.976\n0,239,29.97\n"
    over = 240 / 29.97

    def v1_time(f):
        return f / 29.97 if f <= 240 else over + (f - 240) / 23.976
    sc("srt_v1_source_25fps_destination", keyframes=place_keyframes(spans, v1_time, cfr_frame(25.0)),
       counts=(n_src + 60, int((SECONDS + SHIFT) * 25) + 1), fps=(None, 25.0), timecodes=(v1, None))

    # two groups (a segment inserted in the destination), keyframes of the second group displaced with it
    first = [x for x in spans if x[1] < 36.0]
    second = [x for x in spans if x[0] > 36.0]
    a = place_keyframes(first, cfr_time(NTSC), cfr_frame(NTSC), shift=1.0)
    b = place_keyframes(second, cfr_time(NTSC), cfr_frame(NTSC), shift=19.0)
    sc("srt_two_groups", dst=dict(pieces=[noise(22, 1.0, 300), speech(11, 80, 0, 36), noise(23, 18.0, 4000), speech(11, 80, 36, SECONDS)]),
       keyframes=(sorted(set(a[0] + b[0])), sorted(set(a[1] + b[1]))), counts=(n_src, int((SECONDS + 19.0) * NTSC) + 1))

    # ASS: comments and lines with identical times (linked events), a zero-duration line, and typesetting groups (short lines close
    # together) whose first and last keyframes are displaced differently in the destination
    ev = [("Comment", 0.0, 0.0, "Default", "comment at the top"), ("Dialogue", 2.0, 4.5, "Default", "hello, world"),
          ("Dialogue", 6.0, 6.3, "Sign", "{\\pos(10,10)}sign a"), ("Dialogue", 6.35, 6.7, "Sign", "sign b"), ("Dialogue", 6.75, 7.1, "Sign", "sign c"),
          ("Comment", 9.0, 10.0, "Default", "a comment"), ("Dialogue", 11.0, 13.5, "Default", "line three"),
          ("Dialogue", 11.0, 13.5, "Default", "line three again (same times)"), ("Dialogue", 15.0, 15.0, "Default", "zero duration"),
          ("Dialogue", 16.0, 18.0, "Default", "four"), ("Dialogue", 20.0, 20.4, "Sign", "sign d"), ("Dialogue", 20.45, 20.8, "Sign", "sign e"),
          ("Dialogue", 23.0, 25.0, "Default", "five"), ("Dialogue", 27.0, 29.5, "Default", "six"), ("Dialogue", 31.0, 33.0, "Default", "seven"),
          ("Dialogue", 32.0, 32.3, "Sign", "short sign inside seven"), ("Dialogue", 36.0, 38.0, "Default", "eight"),
          ("Dialogue", 40.0, 42.5, "Default", "nine"), ("Comment", 44.0, 45.0, "Default", "last comment")]
    plain = [(s, e) for kind, s, e, style, _ in ev if kind == "Dialogue" and style == "Default" and e > s]

    def fr(t):
        return first_frame_at(t, NTSC)
    extra = [(fr(6.0), 0), (fr(7.1) + 1, 1), (fr(20.0), -1), (fr(20.8) + 1, 1)]          # start / end of the two sign groups
    sc("ass_linked_and_typesetting", ext=".ass", script=ass(ev), keyframes=place_keyframes(plain, cfr_time(NTSC), cfr_frame(NTSC), extra=extra))
    return S


def cli_args(sc, paths):
    o = sc["options"]
    args = ["--src-keyframes", paths["src_kf"], "--dst-keyframes", paths["dst_kf"]]
    for side in ("src", "dst"):
        if sc["fps"][side] is not None:
            args += [f"--{side}-fps", repr(sc["fps"][side])]
        else:
            args += [f"--{side}-timecodes", paths[side + "_tc"]]
    if "kf_mode" in o:
        args += ["--kf-mode", o["kf_mode"]]
    if "max_kf_distance" in o:
        args += ["--max-kf-distance", repr(o["max_kf_distance"])]
    if o.get("grouping") is False:
        args += ["--no-grouping"]
    return args


def run_one(sushi, sc, tmp, collect):
    from sushi.__main__ import create_arg_parser
    paths = {}
    rec = {k: sc[k] for k in ("name", "ext", "script", "keyframes", "frame_count", "fps", "timecodes", "options")}
    for side in ("src", "dst"):
        data = synth.audio_from_recipe(sc[side])
        paths[side] = os.path.join(tmp, f"{sc['name']}_{side}.wav")
        with open(paths[side], "wb") as f:
            f.write(data)
        rec[side] = {"recipe": sc[side], "sha256": hashlib.sha256(data).hexdigest()}
        paths[side + "_kf"] = kfmod.write_keyframes(os.path.join(tmp, f"{sc['name']}_{side}.kf.txt"), sc["keyframes"][side],
                                                    sc["frame_count"][side])
        if sc["timecodes"][side] is not None:
            paths[side + "_tc"] = os.path.join(tmp, f"{sc['name']}_{side}.tc.txt")
            with open(paths[side + "_tc"], "w") as f:
                f.write(sc["timecodes"][side])
    script = os.path.join(tmp, sc["name"] + "_in" + sc["ext"])
    out = os.path.join(tmp, sc["name"] + "_out" + sc["ext"])
    with open(script, "wb") as f:
        f.write(sc["script"].encode("utf-8"))
    del base.SEARCHES[:], base.STREAMS[:], collect.messages[:]
    args = create_arg_parser().parse_args(["--src", paths["src"], "--dst", paths["dst"], "--script", script, "-o", out] + cli_args(sc, paths))
    sushi.run(args)
    with open(out, "rb") as f:
        rec["output"] = f.read().decode("utf-8")
    rec["searches"] = [list(x) for x in base.SEARCHES]
    m = collect.messages
    rec["reference_log"] = {"corrected": sum("corrected by" in x for x in m), "snapped": sum(x.startswith("Snapping ") for x in m),
                            "typesetting_mismatch": sum(x.startswith("Typesetting group at") for x in m)}
    return rec


def timecode_probes(sushi):
    from sushi.demux import Timecodes
    ms = v2_times(40, 20, NTSC, 30.0)
    cases = [dict(kind="cfr", fps=NTSC), dict(kind="cfr", fps=25.0), dict(kind="file", text="# timecode format v1\nAssume 23.976\n"),
             dict(kind="file", text="# timecode format v1\nassume 29.970\n0,9,23.976\n20,29,59.94\n"),
             dict(kind="file", text=v2_text(ms)), dict(kind="file", text="# timestamp format v2\n0\n41.708\n83.417\n125.125")]
    out = []
    for c in cases:
        tc = Timecodes.cfr(c["fps"]) if c["kind"] == "cfr" else Timecodes.parse(c["text"])
        numbers = [0, 1, 5, 9, 10, 11, 19, 29, 30, 31, 39, 40, 41, 100, 1000]
        stamps = [0.0, 0.01, 0.0417, 0.2, 0.41, 0.4171, 0.5, 0.83, 1.0, 1.2, 1.61, 1.7, 3.0, 41.7, 100.0]
        c = dict(c)
        c["frame_time"] = [[n, tc.get_frame_time(n)] for n in numbers]
        c["frame_number"] = [[t, tc.get_frame_number(t)] for t in stamps]
        c["frame_size"] = [[t, tc.get_frame_size(t)] for t in stamps]
        out.append(c)
    return out


def keyframes_files(sushi, tmp):
    from sushi import keyframes as ref_kf
    out = []
    for kf, count in (([0, 7, 8, 19, 39], 40), ([3, 4, 30], 31), ([], 5)):
        path = kfmod.write_keyframes(os.path.join(tmp, "kf.txt"), kf, count)
        with open(path) as f:
            text = f.read()
        out.append(dict(keyframes=kf, frame_count=count, text=text, parsed=ref_kf.parse_keyframes(path)))
    return out


def main():
    collect = Collect()
    logging.root.addHandler(collect)
    logging.root.setLevel(logging.INFO)
    sushi = base.install_stubs()
    recs = []
    with tempfile.TemporaryDirectory() as tmp:
        for sc in scenarios():
            recs.append(run_one(sushi, sc, tmp, collect))
            print(f"{sc['name']}: {len(recs[-1]['searches'])} searches, {recs[-1]['reference_log']}", file=sys.stderr)
        doc = {"scenarios": recs, "timecodes": timecode_probes(sushi), "keyframes_files": keyframes_files(sushi, tmp)}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)", file=sys.stderr)


if __name__ == "__main__":
    main()
