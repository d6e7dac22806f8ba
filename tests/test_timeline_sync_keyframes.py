"""Keyframe snapping of vse_amd.timeline_sync on the CPU: every scenario of tests/golden/timeline_sync_keyframes.json (recorded from
the reference's own Sushi run with keyframes and timecodes) gives the reference's output byte for byte with the recorded searches
replayed; the Timecodes forms give the reference's values; the CLI refusals."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from vse_amd import keyframes, synth, timeline_sync as ts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOC = json.load(open(os.path.join(ROOT, "tests", "golden", "timeline_sync_keyframes.json")))
GOLDEN = DOC["scenarios"]
BY_NAME = {s["name"]: s for s in GOLDEN}


class ReplaySearch:
    """The searcher of a recorded run: every query must be one the reference made, and gets the reference's result."""

    def __init__(self, searches):
        self.table = {tuple(q[:4]): (q[4], np.array(q[5], np.uint32).view(np.float32)) for q in searches}

    def load(self, src, dst):
        pass

    def __call__(self, queries):
        return [self.table[tuple(int(v) for v in q)] for q in queries]


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


def sync_kwargs(sc, tmp, as_lists=False):
    """The scenario's keyframes (files in Sushi's format, or lists), timecodes files and options -> sync() keywords."""
    kw = dict(sc["options"])
    for side in ("src", "dst"):
        kf = sc["keyframes"][side]
        kw[side + "_keyframes"] = list(kf) if as_lists else keyframes.write_keyframes(os.path.join(tmp, side + ".kf.txt"), kf,
                                                                                       sc["frame_count"][side])
        if sc["fps"][side] is not None:
            kw[side + "_fps"] = sc["fps"][side]
        else:
            p = os.path.join(tmp, side + ".tc.txt")
            open(p, "w").write(sc["timecodes"][side])
            kw[side + "_timecodes"] = p
    return kw


def run_scenario(sc, tmp, **more):
    src, dst, script, out = materialize(sc, tmp)
    log = ts.sync(src, dst, script, out, search=ReplaySearch(sc["searches"]), **sync_kwargs(sc, tmp, **more))
    return open(out, "rb").read(), [[a, b, c, d, k, int(np.float32(v).view(np.uint32))] for a, b, c, d, k, v in log]


@pytest.mark.parametrize("sc", GOLDEN, ids=[s["name"] for s in GOLDEN])
def test_golden_scenario_replayed(sc, tmp_path):
    out, searches = run_scenario(sc, str(tmp_path))
    assert searches == sc["searches"]
    assert out == sc["output"].encode("utf-8")


def test_keyframes_as_lists_of_frame_numbers(tmp_path):
    sc = BY_NAME["srt_cfr_all"]
    out, _ = run_scenario(sc, str(tmp_path), as_lists=True)
    assert out == sc["output"].encode("utf-8")


def test_golden_covers_the_paths(tmp_path):
    assert {s["ext"] for s in GOLDEN} == {".srt", ".ass"}
    modes = {s["options"].get("kf_mode", "all") for s in GOLDEN}
    assert modes == {"all", "shift", "snap"}
    assert any(s["options"].get("grouping") is False for s in GOLDEN)
    assert any((s["timecodes"]["dst"] or "").startswith("# timecode format v2") for s in GOLDEN)
    assert any((s["timecodes"]["src"] or "").startswith("# timecode format v1") and s["timecodes"]["src"].count(",") >= 2 for s in GOLDEN)
    # the reference logged each snapping step somewhere, the start / end mismatch of a typesetting group among them
    assert BY_NAME["srt_cfr_all"]["reference_log"]["corrected"] == 1 and BY_NAME["srt_cfr_snap"]["reference_log"]["snapped"] > 0
    assert BY_NAME["ass_linked_and_typesetting"]["reference_log"]["typesetting_mismatch"] > 0
    assert BY_NAME["srt_two_groups"]["reference_log"]["corrected"] == 2
    # the modes and the distances change the result; max_kf_distance 0 is the run without keyframes
    outs = {n: BY_NAME[n]["output"] for n in ("srt_cfr_all", "srt_cfr_shift", "srt_cfr_snap", "srt_max_kf_distance_0", "srt_max_kf_distance_3_5")}
    assert len(set(outs.values())) >= 4
    sc = BY_NAME["srt_max_kf_distance_0"]
    src, dst, script, out = materialize(sc, str(tmp_path))
    ts.sync(src, dst, script, out, search=ReplaySearch(sc["searches"]))
    assert open(out, "rb").read() == sc["output"].encode("utf-8") != BY_NAME["srt_cfr_all"]["output"].encode("utf-8")
    # linked events (comments, identical times, a zero duration) went through resolve_link and were shifted
    a = BY_NAME["ass_linked_and_typesetting"]
    assert "Comment: 0,0:00:00.00,0:00:00.00" not in a["output"] and a["output"].count("Comment:") == 3


def test_snapping_limit_both_sides_of_it():
    """Keyframes closer than and further than the snapping limit from a line's start and end: lines whose times moved by the plain
    audio shift only, and lines that were snapped, both exist in the constant-fps scenario in snap mode (in the other modes a
    line without a keyframe nearby takes a correction interpolated from its neighbours)."""
    sc, plain = BY_NAME["srt_cfr_snap"], BY_NAME["srt_max_kf_distance_0"]
    a = ts.SrtScript.from_text(sc["output"]).events
    b = ts.SrtScript.from_text(plain["output"]).events
    starts = [round(x.start - y.start, 3) for x, y in zip(a, b)]
    ends = [round(x.end - y.end, 3) for x, y in zip(a, b)]
    assert any(d == 0 for d in starts) and any(d != 0 for d in starts)
    assert any(d == 0 for d in ends) and any(d != 0 for d in ends)
    assert max(abs(d) for d in starts + ends) < 2 * 1001 / 24000.0          # nothing moves further than max_kf_distance frames


@pytest.mark.parametrize("case", DOC["timecodes"], ids=lambda c: c["kind"] + "-" + (repr(c["fps"]) if c["kind"] == "cfr" else c["text"][:30].strip()))
def test_timecodes_give_the_reference_values(case):
    tc = ts.Timecodes.cfr(case["fps"]) if case["kind"] == "cfr" else ts.Timecodes.parse(case["text"])
    for n, want in case["frame_time"]:
        assert tc.get_frame_time(n) == want, ("frame_time", n)
    for t, want in case["frame_number"]:
        assert tc.get_frame_number(t) == want, ("frame_number", t)
    for t, want in case["frame_size"]:
        assert tc.get_frame_size(t) == want, ("frame_size", t)


def test_timecodes_refusals(tmp_path):
    with pytest.raises(ts.TimelineSyncError, match="not supported"):
        ts.Timecodes.parse("# timecode format v3\n1\n")
    with pytest.raises(ts.TimelineSyncError, match="not supported"):
        ts.Timecodes.parse("")
    with pytest.raises(ts.TimelineSyncError, match="Malformed"):
        ts.Timecodes.parse("# timecode format v2\n0\nabc\n")
    with pytest.raises(ts.TimelineSyncError, match="not found"):
        ts.Timecodes.from_file(str(tmp_path / "none.txt"))


def test_interpolate_nones_and_closest_keyframe():
    assert ts.interpolate_nones([None, None], [1.0, 2.0]) == []
    assert ts.interpolate_nones([1.0, 2.0], [1.0, 2.0]) == [1.0, 2.0]
    assert ts.interpolate_nones([0.0, None, 1.0, None], [0.0, 1.0, 2.0, 5.0]) == [0.0, 0.5, 1.0, 1.0]
    kt = [0.0, 1.0, 2.0]
    assert ts.get_distance_to_closest_kf(-1.0, kt) == 1.0 and ts.get_distance_to_closest_kf(5.0, kt) == -3.0
    assert ts.get_distance_to_closest_kf(1.5, kt) == -0.5          # a tie goes to the earlier keyframe
    assert ts.get_distance_to_closest_kf(1.75, kt) == 0.25


def test_sync_refuses_keyframe_option_mistakes(tmp_path):
    sc = BY_NAME["srt_cfr_all"]
    src, dst, script, out = materialize(sc, str(tmp_path))
    search = ReplaySearch(sc["searches"])
    for kw, word in ((dict(src_keyframes=[0, 5]), "--dst-keyframes"), (dict(src_fps=25.0), "--src-fps"),
                     (dict(src_keyframes=[0], dst_keyframes=[0], src_fps=25.0), "--dst-keyframes needs"),
                     (dict(src_keyframes=[0], dst_keyframes=[0], src_fps=25.0, dst_fps=25.0, dst_timecodes=script), "--dst-timecodes"),
                     (dict(src_keyframes=[0], dst_keyframes=[0], src_fps=25.0, dst_fps=25.0, kf_mode="none"), "--kf-mode"),
                     (dict(src_keyframes=script, dst_keyframes=[0], src_fps=25.0, dst_fps=25.0), "Unsupported keyframes type")):
        with pytest.raises(ts.TimelineSyncError, match=word):
            ts.sync(src, dst, script, out, search=search, **kw)


# ---- CLI -----------------------------------------------------------------------------------------------------------------------

def cli(*extra):
    # the WAVs and the script do not exist: every refusal below comes before those checks
    return subprocess.run([sys.executable, "-m", "vse_amd.timeline_sync", "--src", "a.wav", "--dst", "b.wav", "--script", "c.srt", *extra],
                          cwd=ROOT, capture_output=True, text=True)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("kf")
    kf = keyframes.write_keyframes(str(d / "kf.txt"), [0, 10], 20)
    tc = str(d / "tc.txt")
    open(tc, "w").write("# timecode format v1\nAssume 23.976\n")
    return kf, tc, str(d / "missing.txt")


def test_cli_refusals_name_the_option(files):
    kf, tc, missing = files
    both = ["--src-keyframes", kf, "--dst-keyframes", kf]
    cases = [
        (["--src-keyframes", missing, "--dst-keyframes", kf, "--src-fps", "25", "--dst-fps", "25"], "--src-keyframes"),
        (["--src-keyframes", kf, "--dst-keyframes", missing, "--src-fps", "25", "--dst-fps", "25"], "--dst-keyframes"),
        (both + ["--src-timecodes", missing, "--dst-fps", "25"], "--src-timecodes"),
        (both + ["--src-fps", "25", "--dst-timecodes", missing], "--dst-timecodes"),
        (["--src-keyframes", kf, "--src-fps", "25"], "--dst-keyframes"),
        (["--dst-keyframes", kf, "--dst-fps", "25"], "--src-keyframes"),
        (["--src-keyframes", "auto", "--dst-keyframes", kf, "--src-fps", "25", "--dst-fps", "25"], "--src-keyframes auto"),
        (["--src-keyframes", kf, "--dst-keyframes", "make", "--src-fps", "25", "--dst-fps", "25"], "--dst-keyframes make"),
        (both + ["--dst-fps", "25"], "--src-keyframes needs --src-fps or --src-timecodes"),
        (both + ["--src-timecodes", tc], "--dst-keyframes needs --dst-fps or --dst-timecodes"),
        (both + ["--src-fps", "25", "--src-timecodes", tc, "--dst-fps", "25"], "--src-fps and --src-timecodes"),
        (both + ["--src-fps", "25", "--dst-timecodes", tc, "--dst-fps", "25"], "--dst-fps and --dst-timecodes"),
        (["--src-fps", "25"], "--src-fps"), (["--dst-fps", "25"], "--dst-fps"), (["--src-timecodes", tc], "--src-timecodes"),
        (["--dst-timecodes", tc], "--dst-timecodes"), (["--kf-mode", "all"], "--kf-mode"), (["--max-kf-distance", "2"], "--max-kf-distance"),
        (["--chapters", "none"], "--chapters"), (["--src-audio", "1"], "--src-audio"), (["--dst-audio", "1"], "--dst-audio"),
        (["--src-script", "1"], "--src-script"), (["--test-shift-plot", "p.png"], "--test-shift-plot"), (["--temp-dir", "t"], "--temp-dir"),
        (["--no-cleanup"], "--no-cleanup"),
    ]
    for extra, word in cases:
        r = cli(*extra)
        assert r.returncode == 2, (extra, r.stderr)
        assert word in r.stderr, (extra, r.stderr)
        assert "doesn't exist" not in r.stderr or "keyframes" in r.stderr or "timecodes" in r.stderr, (extra, r.stderr)
    r = cli("--src-keyframes", "auto", "--dst-keyframes", kf, "--src-fps", "25", "--dst-fps", "25")
    assert "python -m vse_amd.keyframes" in r.stderr


def test_cli_accepts_complete_keyframe_options(files):
    kf, tc, _ = files
    r = cli("--src-keyframes", kf, "--dst-keyframes", kf, "--src-fps", "23.976", "--dst-timecodes", tc, "--kf-mode", "snap",
            "--max-kf-distance", "3")
    assert r.returncode == 2 and "Source file doesn't exist" in r.stderr          # the options passed; the WAV check came next


def test_cli_end_to_end_with_keyframes(tmp_path):
    """The CLI with keyframes files gives the reference's script (the numpy searcher stands in for the GPU one in-process)."""
    from audio_match_ref import NumpySearch
    sc = BY_NAME["srt_v1_source_25fps_destination"]
    src, dst, script, out = materialize(sc, str(tmp_path))
    kw = sync_kwargs(sc, str(tmp_path))
    real = ts.GpuSearch
    ts.GpuSearch = NumpySearch
    try:
        rc = ts.main(["--src", src, "--dst", dst, "--script", script, "-o", out, "--src-keyframes", kw["src_keyframes"], "--dst-keyframes",
                      kw["dst_keyframes"], "--src-timecodes", kw["src_timecodes"], "--dst-fps", "25"])
    finally:
        ts.GpuSearch = real
    assert rc == 0
    assert open(out, "rb").read() == sc["output"].encode("utf-8")
