"""vse_audio_match on the MI355X: the first argmin offset and the float32 bits of its value equal the numpy restatement of the
contract (tests/audio_match_ref.py) on random, constant and periodic streams; three queries in one call equal three calls;
invalid queries are refused without a launch; and timeline sync on the engine's searcher reproduces the reference's golden
scenarios byte for byte."""
import numpy as np
import pytest

import audio_match_ref as ref

pytestmark = pytest.mark.gpu


def dev(ctx, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.uint8)).to(ctx.tdev)


def run(ctx, src, dst, queries):
    """-> [(index, float32 bits)] of one call."""
    out = ctx.audio_match(dev(ctx, src), dev(ctx, dst), queries).cpu().numpy()
    return [(int(r[0]), int(np.uint32(r[1]))) for r in out]


def want(src, dst, queries):
    got = []
    for so, m, do, wl in queries:
        k, v = ref.match(src[so:so + m], dst[do:do + wl])
        got.append((k, int(np.float32(v).view(np.uint32))))
    return got


def audio_like(rng, n):
    """Noise bursts over a floor, centred on 128 like a prepared stream."""
    env = np.repeat(rng.random(n // 600 + 1) > 0.5, 600)[:n] * 50 + 6
    return np.clip(128 + rng.standard_normal(n) * env, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("m", [1, 63, 64, 65, 4095, 4097, 36001, 140001])
def test_random_streams(ctx, m):
    rng = np.random.default_rng(m)
    n = 3000 if m > 100000 else 50000
    src = rng.integers(0, 256, m + 777, dtype=np.uint8)
    dst = audio_like(rng, n + m + 999)
    k = n // 3
    dst[500 + k:500 + k + m] = src[100:100 + m] if m < 100 else np.clip(src[100:100 + m].astype(int) + rng.integers(-3, 4, m), 0, 255)
    q = [(100, m, 500, n + m - 1)]
    assert run(ctx, src, dst, q) == want(src, dst, q)


def test_wide_window_720k_offsets_touching_both_ends(ctx):
    rng = np.random.default_rng(7)
    m, n = 36000, 720001
    src = audio_like(rng, m)
    dst = audio_like(rng, n + m - 1)
    dst[654321:654321 + m] = np.clip(src.astype(int) + rng.integers(-2, 3, m), 0, 255)
    q = [(0, m, 0, n + m - 1)]                 # pattern = the whole source, window = the whole destination
    got = run(ctx, src, dst, q)
    assert got == want(src, dst, q)
    assert got[0][0] == 654321


@pytest.mark.parametrize("fill", [0, 255])
def test_constant_streams(ctx, fill):
    """All-0 streams give den == 0 (v = 1 everywhere, index 0); all-255 ones hit the bias extreme (v = 0 everywhere)."""
    m = 70000
    src = np.full(m + 5, fill, np.uint8)
    dst = np.full(m + 20000, fill, np.uint8)
    q = [(5, m, 3, m + 19990)]
    got = run(ctx, src, dst, q)
    assert got == want(src, dst, q)
    assert got[0][0] == 0


def test_mixed_constant_pattern_on_random_window(ctx):
    rng = np.random.default_rng(11)
    src = np.zeros(5000, np.uint8)
    dst = rng.integers(0, 256, 40000, dtype=np.uint8)
    dst[1000:9000] = 0
    q = [(0, 5000, 0, 40000)]
    assert run(ctx, src, dst, q) == want(src, dst, q)


@pytest.mark.parametrize("period,m", [(97, 3001), (256, 4096), (1000, 20000)])
def test_periodic_ties_take_the_first_index(ctx, period, m):
    rng = np.random.default_rng(period)
    cyc = rng.integers(0, 256, period, dtype=np.uint8)
    dst = np.tile(cyc, (m + 50000) // period + 2)
    src = dst[37:37 + m].copy()
    q = [(0, m, 0, m + 40000)]
    got = run(ctx, src, dst, q)
    assert got == want(src, dst, q)
    assert got[0][0] == 37 % period and got[0][1] == 0


def test_three_queries_equal_three_calls(ctx):
    rng = np.random.default_rng(5)
    src = audio_like(rng, 200000)
    dst = audio_like(rng, 500000)
    dst[100000:136000] = src[50000:86000]
    qs = [(50000, 36000, 60000, 240000 + 36000 - 1), (50000, 18000, 80000, 36000 + 18000 - 1), (68000, 18000, 0, 500000)]
    together = run(ctx, src, dst, qs)
    alone = [run(ctx, src, dst, [q])[0] for q in qs]
    assert together == alone == want(src, dst, qs)


@pytest.mark.parametrize("queries", [[(0, 0, 0, 10)], [(0, 10, 0, 9)], [(-1, 10, 0, 100)], [(95, 10, 0, 100)], [(0, 10, 1, 1000)],
                                     [(0, 10, -1, 100)], [], [(0, 10, 0, 100)] * 4])
def test_invalid_queries_are_refused(ctx, queries):
    from vse_amd import engine
    src = np.zeros(100, np.uint8)
    dst = np.zeros(1000, np.uint8)
    with pytest.raises(engine.VseError):
        ctx.audio_match(dev(ctx, src), dev(ctx, dst), queries)


def test_small_workspace_is_refused(ctx):
    import torch
    from vse_amd import engine
    q = [(0, 1000, 0, 50000)]
    need = ctx.audio_match_workspace_bytes(q)
    assert need > 0
    ws = torch.empty(need - 256, dtype=torch.uint8, device=ctx.tdev)
    with pytest.raises(engine.VseError, match="workspace"):
        ctx.audio_match(dev(ctx, np.zeros(1000, np.uint8)), dev(ctx, np.zeros(50000, np.uint8)), q, workspace=ws)


# ---- timeline sync on the engine's searcher ----------------------------------------------------------------------------------

def test_golden_scenarios_on_the_gpu_searcher(ctx, tmp_path):
    """Every scenario of tests/golden/timeline_sync.json (recorded from the reference's Sushi) through sync() with the GPU
    searcher: the same searches with the same index and float32 bits, and the reference's output byte for byte."""
    from test_timeline_sync import GOLDEN, run_scenario
    from vse_amd import timeline_sync as ts
    search = ts.GpuSearch(ctx)
    for sc in GOLDEN:
        d = tmp_path / sc["name"]
        d.mkdir()
        out, searches = run_scenario(sc, str(d), search)
        assert searches == sc["searches"], sc["name"]
        assert out == sc["output"].encode("utf-8"), sc["name"]


def test_cli_on_the_gpu(ctx, tmp_path):
    import subprocess
    import sys
    from test_timeline_sync import GOLDEN, ROOT, materialize
    sc = GOLDEN[0]
    src, dst, script, out = materialize(sc, str(tmp_path))
    r = subprocess.run([sys.executable, "-m", "vse_amd.timeline_sync", "--src", src, "--dst", dst, "--script", script, "--output", out],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == sc["output"].encode("utf-8")
