"""vse_scene_change on the MI355X: the device counts equal the numpy restatement (tests/scene_cut_ref.py) as identical integers in
all three columns, batches chained through the state equal one batch, every refused argument returns without a launch, and the
keyframes found on the engine (and the script snapped to them) equal those of the numpy counter."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from scene_cut_ref import NumpySceneCounter, counts as ref_counts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#         H     W     s  R  n
SHAPES = [(16, 16, 1, 0, 5),          # one block
          (16, 16, 1, 8, 5),          # every nonzero vector clipped
          (52, 70, 1, 8, 9),          # plane remainders on both axes
          (33, 47, 1, 3, 9),
          (97, 131, 2, 8, 9),         # source remainder under the box filter
          (360, 640, 1, 8, 5),
          (1081, 1923, 3, 8, 3)]
IDS = ["%dx%d-s%d-R%d-n%d" % s for s in SHAPES]


def dev_counts(ctx, frames, scale, search, bias, batches=None, reset_first=True):
    """frames: cuda uint8 [n,H,W,3] view -> host int32 [n,3], fed in batches of `batches` frames through one state."""
    n, h, w, _ = frames.shape
    state = ctx.scene_change_state(h, w, scale)
    step = batches or n
    out = [ctx.scene_change(frames[i:i + step], scale, search, bias, state, reset=(reset_first and i == 0)).cpu().numpy()
           for i in range(0, n, step)]
    return np.concatenate(out)


def random_frames(n, h, w, seed):
    """Noise, a displaced copy of the frame before (so nonzero vectors win), and a held frame."""
    rng = np.random.default_rng(seed)
    f = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
    if n > 2:
        f[2] = np.roll(f[1], (1, -2), (0, 1))
    f[n - 1] = f[n - 2]
    return f


def generator_clip(n, h, w, scale, search, seed):
    """Pans within the search range, a hold and a cut (at least 4 frames: three kinds of transition)."""
    from vse_amd import synth
    n = max(n, 4)
    r = max(scale * search, 1)
    pans = [(0, r), (-(r // 2), r // 3), (r, 0), (-1, 1)]
    frames, cuts = synth.make_scenes([dict(frames=n - 1, pan=pans[:max(n - 3, 1)] + [(0, 0)], hold=[n - 2]), dict(frames=1)], h, w, seed=seed)
    assert cuts == [0, n - 1]
    return frames


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("kind", ["random", "generator"])
def test_counts_match_numpy(ctx, shape, kind):
    import torch
    h, w, s, r, n = shape
    frames = random_frames(n, h, w, seed=h + w) if kind == "random" else generator_clip(n, h, w, s, r, seed=h + w)
    bias = 1024 if kind == "generator" else 300
    want, _ = ref_counts(frames, s, r, bias)
    got = dev_counts(ctx, torch.from_numpy(frames).cuda(), s, r, bias)
    assert got.dtype == np.int32 and np.array_equal(got, want), (shape, kind, got.tolist(), want.tolist())
    bh, bw = h // s // 16, w // s // 16
    assert tuple(want[0][:2]) == (bh * bw, 0)
    if kind == "generator":
        assert want[-1][0] * 10 >= 9 * bh * bw and want[-2][0] == 0          # the cut changes 90 % of the blocks, the held frame none


@pytest.mark.parametrize("search", range(9))
def test_every_search_radius(ctx, search):
    """The window's left edge is rounded down to a dword of the plane row: each radius mod 4 lays the lanes out differently."""
    import torch
    frames = np.concatenate([random_frames(4, 52, 70, seed=search), generator_clip(5, 52, 70, 1, search, seed=40 + search)])
    want, _ = ref_counts(frames, 1, search, 500)
    assert np.array_equal(dev_counts(ctx, torch.from_numpy(frames).cuda(), 1, search, 500), want), (search, want.tolist())


@pytest.mark.parametrize("scale", range(1, 9))
def test_every_scale(ctx, scale):
    """Source remainders under every box size, rows of an odd byte length (the plane pass fetches whole aligned dwords around them)."""
    import torch
    h, w = 17 * scale + scale - 1, 69 * scale + scale // 2          # plane 17 x 69: a second tile of 5 columns, a fifth tile row of one row
    frames = random_frames(3, h, w, seed=scale)
    want, _ = ref_counts(frames, scale, 2, 100)
    assert np.array_equal(dev_counts(ctx, torch.from_numpy(frames).cuda(), scale, 2, 100), want), (scale, want.tolist())
    padded = torch.zeros((3, h + 2, w * 3 + 7), dtype=torch.uint8, device=ctx.tdev)          # an odd pitch: rows start at every alignment
    view = padded[:, 1:h + 1, 5:5 + w * 3].view(3, h, w, 3)
    view.copy_(torch.from_numpy(frames))
    assert np.array_equal(dev_counts(ctx, view, scale, 2, 100), want), (scale, "padded")


@pytest.mark.parametrize("bias", [0, 65535])
def test_bias_extremes(ctx, bias):
    import torch
    frames = generator_clip(6, 97, 131, 2, 8, seed=5)
    want, _ = ref_counts(frames, 2, 8, bias)
    assert np.array_equal(dev_counts(ctx, torch.from_numpy(frames).cuda(), 2, 8, bias), want)
    if bias == 0:
        assert want[-1, 0] > 0 and want[-2, 0] == 0          # the cut still counts, the held frame (inter 0) never does


def test_counts_padded_pitch_and_stride(ctx):
    import torch
    frames = random_frames(6, 52, 70, seed=7)
    want, _ = ref_counts(frames, 1, 8, 300)
    padded = torch.zeros((6, 57, 83 * 3 + 5), dtype=torch.uint8, device=ctx.tdev)     # padded rows inside padded frames
    view = padded[:, 3:55, 6:6 + 210].view(6, 52, 70, 3)
    view.copy_(torch.from_numpy(frames))
    assert view.stride(1) == 83 * 3 + 5 and view.stride(0) == 57 * (83 * 3 + 5)
    assert np.array_equal(dev_counts(ctx, view, 1, 8, 300), want)
    frames2 = random_frames(4, 97, 131, seed=8)
    want2, _ = ref_counts(frames2, 2, 8, 300)
    padded2 = torch.zeros((4, 100, 140 * 3 + 1), dtype=torch.uint8, device=ctx.tdev)
    view2 = padded2[:, 2:99, 3:3 + 393].view(4, 97, 131, 3)
    view2.copy_(torch.from_numpy(frames2))
    assert np.array_equal(dev_counts(ctx, view2, 2, 8, 300), want2)


@pytest.mark.parametrize("batch", [1, 7, None])
def test_batches_chain_through_state(ctx, batch):
    import torch
    from vse_amd import synth
    frames, _ = synth.make_scenes([dict(frames=6, pan=(2, -3)), dict(frames=5, pan=(0, 4), hold=[2]), dict(frames=5)], 100, 150, seed=3)
    want, _ = ref_counts(frames, 1, 8, 1024)
    dev = torch.from_numpy(frames).cuda()
    assert np.array_equal(dev_counts(ctx, dev, 1, 8, 1024, batches=batch), want)
    # a fresh (zero-filled) state without `reset` is the same: the first frame has no predecessor
    assert np.array_equal(dev_counts(ctx, dev, 1, 8, 1024, batches=batch, reset_first=False), want)


def test_reset(ctx):
    import torch
    frames = random_frames(8, 40, 90, seed=11)
    dev = torch.from_numpy(frames).cuda()
    state = ctx.scene_change_state(40, 90, 1)
    ws = torch.empty(8 * 40 * 92, dtype=torch.uint8, device=ctx.tdev)
    chained = ctx.scene_change(dev[:5], 1, 4, 300, state, workspace=ws).cpu().numpy()
    chained = np.concatenate([chained, ctx.scene_change(dev[5:], 1, 4, 300, state, workspace=ws).cpu().numpy()])
    assert np.array_equal(chained, ref_counts(frames, 1, 4, 300)[0])
    again = ctx.scene_change(dev[5:], 1, 4, 300, state, reset=True, workspace=ws).cpu().numpy()
    want, _ = ref_counts(frames[5:], 1, 4, 300)
    assert np.array_equal(again, want)
    assert tuple(again[0]) == (2 * 5, 0, want[0, 2]) and want[0, 2] > 0


def test_rejects_invalid_arguments(ctx):
    from vse_amd import engine
    lib = engine.load_library()
    import torch
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=ctx.tdev)        # far larger than any of the frames below
    st = torch.zeros(1 << 16, dtype=torch.uint8, device=ctx.tdev)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=ctx.tdev)
    cnt = torch.full((3,), -7, dtype=torch.int32, device=ctx.tdev)

    def call(h=64, w=64, scale=1, search=8, bias=1024, ws_bytes=1 << 16, n=1):
        return lib.vse_scene_change(ctx.handle, C.c_void_p(buf.data_ptr()), n, h, w, w * 3, h * w * 3, scale, search, bias,
                                    C.c_void_p(st.data_ptr()), 0, C.c_void_p(ws.data_ptr()), ws_bytes, C.c_void_p(cnt.data_ptr()),
                                    ctx.stream())
    bad = [dict(scale=0), dict(scale=9), dict(search=-1), dict(search=9), dict(bias=-1), dict(bias=65536), dict(h=15), dict(w=15),
           dict(h=31, scale=2), dict(w=127, scale=8), dict(ws_bytes=64 * 64 - 1), dict(n=2, ws_bytes=64 * 64 * 2 - 1), dict(n=0)]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert "vse_scene_change" in lib.vse_last_error().decode()
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [-7, -7, -7] and int(st.sum()) == 0      # nothing was enqueued
    # aw * ah > 2^23: 2900 x 2900 = 8.41 M > 8388608 (no such buffer is needed: the call returns before it touches one)
    rc = lib.vse_scene_change(ctx.handle, C.c_void_p(buf.data_ptr()), 1, 2900, 2900, 2900 * 3, 2900 * 2900 * 3, 1, 8, 1024,
                              C.c_void_p(st.data_ptr()), 0, C.c_void_p(ws.data_ptr()), 1 << 30, C.c_void_p(cnt.data_ptr()), ctx.stream())
    assert rc == -1 and "2^23" in lib.vse_last_error().decode()
    assert lib.vse_scene_change_state_bytes(2900, 2900, 1) == 0 and lib.vse_scene_change_state_bytes(2900, 2900, 2) == 16 + 1450 * 1452
    assert lib.vse_scene_change_state_bytes(15, 64, 1) == 0 and lib.vse_scene_change_state_bytes(33, 47, 1) == 16 + 33 * 48
    assert lib.vse_scene_change_workspace_bytes(3, 97, 131, 2) == 3 * 48 * 68 and lib.vse_scene_change_workspace_bytes(0, 97, 131, 2) == 0
    assert call() == 0
    torch.cuda.synchronize()
    assert cnt.cpu().tolist() == [16, 0, 0] and int(st[0]) == 1          # the valid call ran: 4 x 4 flat blocks, the flag is set


# ---- end to end ----------------------------------------------------------------------------------------------------------------

def three_cut_clip():
    from vse_amd import synth
    return synth.make_scenes([dict(frames=9, pan=(0, 3)), dict(frames=8, pan=(2, -2), hold=[3, 4]),
                              dict(frames=10, text=("seven wizards quietly box", 3, 8)), dict(frames=6, pan=(-4, 0))], 180, 320, seed=9)


def test_find_keyframes_engine_equals_numpy(ctx, tmp_path):
    from vse_amd import ingest, keyframes
    frames, cuts = three_cut_clip()
    np.save(tmp_path / "clip.npy", frames)
    src = ingest.open_source(str(tmp_path / "clip.npy"), fps=24.0)
    want = keyframes.find_keyframes(src, ctx=NumpySceneCounter(), batch=7)
    got = keyframes.find_keyframes(src, ctx=ctx, batch=7)
    assert got == want == cuts and len(cuts) == 4


def test_cli_writes_a_file_parse_keyframes_reads(ctx, tmp_path):
    from vse_amd import ingest, keyframes
    frames, cuts = three_cut_clip()
    avi = str(tmp_path / "clip.avi")
    ingest.write_avi_bgr24(avi, frames, 24.0)
    out = str(tmp_path / "keyframes.txt")
    r = subprocess.run([sys.executable, "-m", "vse_amd.keyframes", avi, "-o", out, "--batch", "16"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert keyframes.parse_keyframes(out) == cuts
    assert len(open(out).read().splitlines()) == 3 + len(frames)


def test_sync_with_engine_keyframes_equals_numpy_path(ctx, tmp_path):
    """One fixture scenario (constant fps on both sides): two generator clips are cut where the scenario's keyframes are, the
    detector finds the keyframes in them, and the script is snapped to those.  The GPU search with the engine's keyframes gives the
    script of the reference search with the numpy counter's keyframes, which is the reference's own output."""
    from audio_match_ref import NumpySearch
    from test_timeline_sync_keyframes import BY_NAME, materialize, sync_kwargs
    from vse_amd import keyframes, synth, timeline_sync as ts
    sc = BY_NAME["srt_cfr_all"]
    src, dst, script, out = materialize(sc, str(tmp_path))
    kw = sync_kwargs(sc, str(tmp_path))
    found = {}
    for side in ("src", "dst"):
        bounds = sc["keyframes"][side] + [sc["frame_count"][side]]
        scenes = [dict(frames=b - a, pan=(0, 1)) for a, b in zip(bounds[:-1], bounds[1:])]
        frames, cuts = synth.make_scenes(scenes, 48, 64, seed=len(side) + 3)
        assert cuts == sc["keyframes"][side]
        clip = _Frames(frames)
        found[side] = (keyframes.find_keyframes(clip, ctx=NumpySceneCounter(), batch=256, search=2),
                       keyframes.find_keyframes(clip, ctx=ctx, batch=256, search=2))
        assert found[side][0] == found[side][1] == cuts
    outs = []
    for which, search in ((0, NumpySearch()), (1, ts.GpuSearch(ctx))):
        kw.update(src_keyframes=found["src"][which], dst_keyframes=found["dst"][which])
        ts.sync(src, dst, script, out, search=search, **kw)
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1] == sc["output"].encode("utf-8")


class _Frames:
    def __init__(self, frames):
        self._f = frames
        self.frame_count = len(frames)

    def frames(self):
        return iter(self._f)
