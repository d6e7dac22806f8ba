"""vse_amd.timeline_sync on the CPU (numpy searcher, tests/audio_match_ref.py): every golden scenario (tests/golden/timeline_sync.json,
recorded from the reference's own Sushi) gives the reference's output byte for byte and makes the same searches with the same
results; the WAV reader, the script round trips and the CLI refusals."""
import hashlib
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from audio_match_ref import NumpySearch
from vse_amd import synth, timeline_sync as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "timeline_sync.json")))["scenarios"]


def materialize(sc, tmp):
    """Write the scenario's WAVs (checked against the recorded SHA-256) and script -> (src, dst, script, output) paths."""
    paths = []
    for side in ("src", "dst"):
        data = synth.audio_from_recipe(sc[side]["recipe"])
        assert hashlib.sha256(data).hexdigest() == sc[side]["sha256"], f"{sc['name']} {side}: synth bytes changed"
        p = os.path.join(tmp, f"{side}.wav")
        open(p, "wb").write(data)
        paths.append(p)
    script = os.path.join(tmp, "in" + sc["ext"])
    open(script, "wb").write(sc["script"].encode("utf-8"))
    return paths[0], paths[1], script, os.path.join(tmp, "out" + sc["ext"])


def options(args):
    """Sushi's CLI options of a scenario -> sync() keywords."""
    kw, it = {}, iter(args)
    for a in it:
        if a == "--no-grouping":
            kw["grouping"] = False
        else:
            kw[a[2:].replace("-", "_")] = int(next(it))
    return kw


def run_scenario(sc, tmp, search):
    src, dst, script, out = materialize(sc, tmp)
    got_log = ts.sync(src, dst, script, out, search=search, **options(sc["args"]))
    return open(out, "rb").read(), [[a, b, c, d, k, int(np.float32(v).view(np.uint32))] for a, b, c, d, k, v in got_log]


@pytest.mark.parametrize("sc", GOLDEN, ids=[s["name"] for s in GOLDEN])
def test_golden_scenario_numpy(sc, tmp_path):
    out, searches = run_scenario(sc, str(tmp_path), NumpySearch())
    assert searches == sc["searches"]
    assert out == sc["output"].encode("utf-8")


def test_golden_covers_the_paths():
    by = {s["name"]: s for s in GOLDEN}
    assert any(q[3] > 50 * 12000 for q in by["inserted_segment"]["searches"])           # widened to max_window (30 s)
    assert any(q[3] > 25 * 12000 for q in by["small_windows"]["searches"])              # widened to --max-window 15
    assert by["destination_shorter"]["output"].count("-->") == by["destination_shorter"]["script"].count("-->")
    assert by["ass_bom_comments_sections"]["output"].startswith("\ufeff[Script Info]")
    assert "[Aegisub Project Garbage]" in by["ass_bom_comments_sections"]["output"]


# ---- WAV reader -----------------------------------------------------------------------------------------------------------------

def write(tmp_path, name, data):
    p = str(tmp_path / name)
    open(p, "wb").write(data)
    return p


def test_wav_extensible_list_chunk_and_odd_chunk(tmp_path):
    x = synth.render_audio(synth.speech_content(3, 5), 12000, 1)
    plain = ts.AudioStream(write(tmp_path, "a.wav", synth.wav_bytes(x, 12000)))
    ext = ts.AudioStream(write(tmp_path, "b.wav", synth.wav_bytes(x, 12000, extensible=True,
                                                                 chunks_before_data=[(b"LIST", b"odd"), (b"junk", b"x" * 6)])))
    assert np.array_equal(plain.data, ext.data)
    assert plain.sample_count == 36000 and plain.padding_size == 120000 and len(plain.data) == 36000 + 240000


def test_wav_stereo_downmix_is_the_float32_mean(tmp_path):
    rng = np.random.default_rng(0)
    st = rng.integers(-20000, 20000, size=(24000, 2)).astype(np.int16)
    s = ts.AudioStream(write(tmp_path, "s.wav", synth.wav_bytes(st, 12000)))
    mono = (st[:, 0].astype(np.float32) + st[:, 1].astype(np.float32)) / np.float32(2)
    d = np.zeros(24000 + 240000, np.float32)
    d[120000:144000] = mono
    d[:120000] = d[120000]
    d[-120000:] = d[-120001]
    hi = np.median(d[d >= 0]) * 3
    lo = np.median(d[d <= 0]) * 3
    want = ((np.clip(d, lo, hi) - lo) / (hi - lo) * 255.0 + 0.5).astype(np.uint8)
    assert np.array_equal(s.data, want)


def test_wav_resample_leaves_the_unwritten_sample_zero(tmp_path):
    x = synth.render_audio(synth.speech_content(3, 6), 48000, 1)[:2 * 48000 + 5]
    s = ts.AudioStream(write(tmp_path, "r.wav", synth.wav_bytes(x, 48000)))
    assert s.sample_count == 24002 and len(s.data) == 24002 + 960000


@pytest.mark.parametrize("bits", [8, 24, 32])
def test_wav_refuses_other_sample_widths(tmp_path, bits):
    fmt = struct.pack("<HHIIHH", 1, 1, 12000, 12000 * bits // 8, bits // 8, bits)
    data = b"\x00" * 3000
    body = b"WAVEfmt " + struct.pack("<I", 16) + fmt + b"data" + struct.pack("<I", len(data)) + data
    with pytest.raises(ts.TimelineSyncError, match=f"{bits}-bit"):
        ts.AudioStream(write(tmp_path, "w.wav", b"RIFF" + struct.pack("<I", len(body)) + body))


def test_wav_refuses_low_rate_silence_and_non_wav(tmp_path):
    x = synth.render_audio(synth.speech_content(2, 7), 8000, 1)
    with pytest.raises(ts.TimelineSyncError, match="below the search rate"):
        ts.AudioStream(write(tmp_path, "low.wav", synth.wav_bytes(x, 8000)))
    with pytest.raises(ts.TimelineSyncError, match="silence"):
        ts.AudioStream(write(tmp_path, "z.wav", synth.wav_bytes(np.zeros((24000, 1), np.int16), 12000)))
    with pytest.raises(ts.TimelineSyncError, match="RIFF"):
        ts.AudioStream(write(tmp_path, "n.wav", b"OggS" + b"\x00" * 100))
    mkv = write(tmp_path, "a.mkv", b"\x1a\x45\xdf\xa3")
    wav = write(tmp_path, "b.wav", synth.wav_bytes(synth.render_audio(synth.speech_content(2, 8), 12000), 12000))
    srt = write(tmp_path, "c.srt", b"1\n00:00:01,000 --> 00:00:02,000\nx\n")
    with pytest.raises(ts.TimelineSyncError, match="only WAV"):
        ts.sync(mkv, wav, srt, str(tmp_path / "o.srt"), search=NumpySearch())


# ---- scripts -------------------------------------------------------------------------------------------------------------------

def test_srt_round_trip_crlf_bom_and_times():
    text = "\ufeff1\r\n00:00:01,000 --> 00:00:02,500\r\nhello\r\nworld\r\n\r\n2\r\n0:0:3,25 --> 00:00:04,000\r\nbye\r\n"
    s = ts.SrtScript.from_text(text.lstrip("\ufeff"))
    assert [(e.source_index, e.start, e.end, e.text) for e in s.events] == [(1, 1.0, 2.5, "hello\r\nworld"), (2, 3.25, 4.0, "bye")]
    assert s.to_text() == "1\n00:00:01,000 --> 00:00:02,500\nhello\r\nworld\n\n2\n00:00:03,250 --> 00:00:04,000\nbye"
    assert ts.format_srt_time(3725.0005) == "01:02:05,000" and ts.format_time(3725.125) == "1:02:05.12"


def test_ass_round_trip_keeps_sections_and_comments():
    sc = next(s for s in GOLDEN if s["ext"] == ".ass")
    a = ts.AssScript.from_text(sc["script"].lstrip("\ufeff"))
    assert sum(e.is_comment for e in a.events) == 3 and "[Fonts]" in a.other
    again = ts.AssScript.from_text(a.to_text())
    assert again.to_text() == a.to_text()
    assert a.to_text().splitlines()[:2] == ["[Script Info]", "; made for the timeline sync tests"]


def test_non_utf8_script_is_refused(tmp_path):
    p = write(tmp_path, "latin.srt", "1\n00:00:01,000 --> 00:00:02,000\ncaf\xe9\n".encode("latin-1"))
    with pytest.raises(ts.TimelineSyncError, match="UTF-8"):
        ts.SrtScript.from_file(p)


# ---- CLI -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra", [["--src-keyframes", "k.txt", "--dst-keyframes", "k2.txt"], ["--chapters", "none"], ["--dst-fps", "23.976"],
                                   ["--src-timecodes", "t.txt"], ["--src-audio", "1"], ["--sample-type", "float32"],
                                   ["--test-shift-plot", "p.png"], ["--kf-mode", "snap"], ["--temp-dir", "/tmp"], ["--no-cleanup"]])
def test_cli_refuses_unsupported_options(tmp_path, extra):
    r = subprocess.run([sys.executable, "-m", "vse_amd.timeline_sync", "--src", "a.wav", "--dst", "b.wav", "--script", "c.srt"] + extra,
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 2
    assert extra[0] in r.stderr


def test_cli_refuses_a_missing_file_with_status_2(tmp_path):
    r = subprocess.run([sys.executable, "-m", "vse_amd.timeline_sync", "--src", str(tmp_path / "no.wav"), "--dst", "b.wav", "--script",
                        "c.srt"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 2 and "doesn't exist" in r.stderr
