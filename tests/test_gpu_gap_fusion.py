"""A 1x1 conv of conv_gemm_kernel's unmasked form sums, in its epilogue, the partials of the global-average pool behind it (the plan
decides: conv_gap_select, csrc/conv_select.hip); the pool's own pass over the tensor is then not run, only gap_finish_kernel.

One-conv + pool graphs through engine.Net: a 1x1 lift of the 3-channel feed to `cin` channels (t0), the 1x1 conv + bias + relu under
test (t3), its global average (g).  Both g and t3 are fetched, so every check reads the fp16 conv output THE SAME RUN stored.

Which launches ran is read off the partial sums the run left in the workspace: the conv's epilogue and gap_partial_kernel group and
order an image's pixels differently, both orders are restated below in fp32, and the slots must hold the BITS of the one the selector
(tests/plan_select.py) announces.  That pins the summation order too: an image's sums depend on the image alone.

Shapes.  The four shapes of the issue (64 or 128 input channels) are served by conv_smallm_kernel / conv_pw_kernel (conv_select sends
1x1 convs with at most 256 input channels and at most 4096 wave tiles there), so their pairs stay two launches: they are kept as refused
cases.  The cases they were meant to exercise are rebuilt with 320 input channels, which reaches conv_gemm_kernel, on every row tile:
  256 x 64   3 x 17 x 30 -> 40    two tiles per image, the second 254 rows live, one slot: two contributors; cout tail in the N tile
  256 x 64   2 x 16 x 16 -> 64    one full tile per image: plain stores, no memset
  256 x 64   2 x 40 x 40 -> 64    6 slots, 7 tiles
  256 x 32   2 x 20 x 20 -> 24    the 32-cout tile
  128 x 128  3 x 32 x 32 -> 128   4 slots, 8 tiles of 128 rows
  256 x 192  12 x 34 x 60 -> 320  7 slots, 8 tiles: slot 0 takes tiles 0 and 7; two N tiles, the second half empty; 8 waves along M
  256 x 256  6 x 68 x 120 -> 256  the server detector's tile (16 waves, 64-deep K tiles): 31 slots, 32 tiles, the last 224 rows live
Refused: 3 x 17 x 30 -> 72 on the 128-row tile (four tiles for one slot), a ragged plan, 1 x 64 x 64 and the issue's four shapes."""
import re

import numpy as np
import pytest

import plan_select

GAP = {"pooling_type": "avg", "ksize": [1, 1], "strides": [1, 1], "paddings": [0, 0], "ceil_mode": False, "exclusive": True,
       "adaptive": True, "global_pooling": False, "padding_algorithm": "EXPLICIT"}
F32 = np.float32


def _graph(cin, cout, pool, keep_t0, seed, post=0):
    """pool: fetch g (0), t3 (1) and, with keep_t0, t0 (2): t0 then outlives the conv, so the pool's scratch is not laid over the conv's
    input; else fetch t3 alone.  post: a 1x1 conv of t3 to `post` channels (t4) behind the pool, fetched last: a later dense output."""
    conv1 = lambda a, f, b: {"type": "conv2d", "in": {"Input": [a], "Filter": [f]}, "out": {"Output": [b]},      # noqa: E731
                             "attrs": {"strides": [1, 1], "paddings": [0, 0], "groups": 1}}
    ops = [{"type": "feed", "in": {"X": ["feed"]}, "out": {"Out": ["x"]}, "attrs": {"col": 0}}, conv1("x", "w0", "t0"), conv1("t0", "w1", "t1"),
           {"type": "elementwise_add", "in": {"X": ["t1"], "Y": ["b1"]}, "out": {"Out": ["t2"]}, "attrs": {"axis": 1}},
           {"type": "relu", "in": {"X": ["t2"]}, "out": {"Out": ["t3"]}, "attrs": {}}]
    fetch = lambda a, c: {"type": "fetch", "in": {"X": [a]}, "out": {"Out": ["fetch"]}, "attrs": {"col": c}}      # noqa: E731
    if pool:
        ops += [{"type": "pool2d", "in": {"X": ["t3"]}, "out": {"Out": ["g"]}, "attrs": dict(GAP)}]
        ops += [conv1("t3", "w4", "t4")] if post else []
        names = ["g", "t3"] + (["t0"] if keep_t0 else []) + (["t4"] if post else [])
        ops += [fetch(a, c) for c, a in enumerate(names)]
        cols = tuple(range(len(names)))
    else:
        ops += [fetch("t3", 0)]
        cols = (0,)
    rng = np.random.default_rng(seed)
    params = {"w0": (cin, 3, 1, 1), "w1": (cout, cin, 1, 1), "b1": (cout,)}
    if post:
        params["w4"] = (post, cout, 1, 1)
    desc = {"model": "unit", "ops": ops, "params": {n: {"dims": list(d), "dtype": 5} for n, d in params.items()},
            "var_shapes": {"t0": [-1, cin, -1, -1], "t1": [-1, cout, -1, -1], "t2": [-1, cout, -1, -1], "t3": [-1, cout, -1, -1],
                           "t4": [-1, post, -1, -1], "g": [-1, cout, 1, 1]}}
    wts = {"w0": rng.standard_normal(params["w0"]).astype(F32),
           "w1": (rng.standard_normal(params["w1"]) / np.sqrt(cin)).astype(F32),
           "b1": (rng.standard_normal(cout) * 0.5 + 0.5).astype(F32)}          # (mostly positive sums: the means are not near zero)
    if post:
        wts["w4"] = (rng.standard_normal(params["w4"]) / np.sqrt(cout)).astype(F32)
    return desc, wts, cols


def _input(n, h, w, seed):
    import torch
    from oracle import ir_emul
    x = np.random.default_rng(seed).uniform(-1, 1, (n, 3, h, w)).astype(np.float16).astype(F32)
    return torch.from_numpy(ir_emul.to_nhwc8(x).astype(np.float16)).cuda()


# ---- the two summation orders, restated in fp32 ----------------------------------------------------------------------------------

def partials_of_the_conv(x, bm, wm, splits):
    """conv_gemm_kernel's column sums of one image, x [hw, c] = the stored fp16 values as fp32 -> [slots, c].  Tile t holds rows
    t * bm ..; wave wm_ of WM holds bm / WM of them as TM row tiles of 32 lanes.  A lane adds its TM rows, the 16 lanes of a DPP row add
    by quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror, the 2 WM half-tiles are added in order, and slot
    t % splits takes the tile (a zeroed slot + at most two tiles)."""
    hw, c = x.shape
    tiles = -(-hw // bm)
    tm = bm // wm // 32
    xp = np.zeros((tiles * bm, c), F32)
    xp[:hw] = x                                                     # rows at or beyond the image add 0
    v = xp.reshape(tiles, wm, tm, 2, 16, c)
    cs = np.zeros((tiles, wm, 2, 16, c), F32)
    for i in range(tm):
        cs = cs + v[:, :, i]
    lane = np.arange(16)
    for perm in (lane ^ 1, lane ^ 2, (lane & 8) | (7 - (lane & 7)), 15 - lane):
        cs = cs + cs[:, :, :, perm]
    red = cs[:, :, :, 0].reshape(tiles, 2 * wm, c)
    s = np.zeros((tiles, c), F32)
    for r in range(2 * wm):
        s = s + red[:, r]
    assert tiles <= 2 * splits
    part = np.zeros((min(splits, tiles), c), F32)
    for t in range(tiles):
        part[t % splits] = part[t % splits] + s[t]
    return part


def partials_of_the_pool(x, splits):
    """gap_partial_kernel: slot s takes pixels [s * per, (s + 1) * per); lane pl of 32 adds pixels pl, pl + 32, .. of them in order, the 32
    lane sums are added in lane order."""
    hw, c = x.shape
    per = -(-hw // splits)
    part = np.zeros((splits, c), F32)
    for s in range(splits):
        seg = x[s * per:min(hw, (s + 1) * per)]
        k = -(-len(seg) // 32) if len(seg) else 0
        segp = np.zeros((k * 32, c), F32)
        segp[:len(seg)] = seg
        acc = np.zeros((32, c), F32)
        for r in segp.reshape(k, 32, c):
            acc = acc + r
        for q in range(32):
            part[s] = part[s] + acc[q]
    return part


def finish(part, hw):
    """gap_finish_kernel: the slots in index order, times 1 / hw, to fp16."""
    s = np.zeros(part.shape[1:], F32)
    for q in range(part.shape[0]):
        s = s + part[q]
    return (s * (F32(1.0) / F32(hw))).astype(np.float16)


# ---- one run -------------------------------------------------------------------------------------------------------------------------

class Run:
    def __init__(self, ctx, n, h, w, cin, cout, seed=0, keep_t0=True, ragged=False, xs=None, post=0):
        """Runs the pool graph once per input of xs (default: one random input) on ONE net and workspace; .g / .conv16 / .part hold the
        last run's pool output [n, c] (fp16 values), conv output [n, hw, c] (fp16) and partial sums as left in the workspace."""
        import torch
        from vse_amd import engine, ir
        self.shape = (n, h, w, cin, cout)
        desc, wts, cols = _graph(cin, cout, True, keep_t0, seed, post)
        self.net = net = engine.Net(ctx, desc, wts, fetch_cols=cols, ragged=ragged)
        prog = net.program(n, h, w)
        k = [i for i, o in enumerate(prog.ops) if int(o["kind"]) == ir.OP_GAP][0] - 1
        assert int(prog.ops[k]["kind"]) == ir.OP_CONV and np.array_equal(prog.ops[k]["out"], prog.ops[k + 1]["in0"])
        self.name = engine.op_kernel_names(prog.ops)[k]
        self.gap = plan_select.decisions(prog.ops)[0].get(k)
        self.splits = int(prog.ops[k + 1]["in2"]["h"])
        for x in (xs if xs is not None else [_input(n, h, w, seed + 1)]):
            outs = net.run(x)
            torch.cuda.synchronize()
        self.last = outs[-1].cpu().numpy()
        self.g = outs[0].cpu().numpy().reshape(n, -1)[:, :cout].astype(np.float16)
        self.conv16 = outs[1].cpu().numpy()[..., :cout].reshape(n, h * w, cout).astype(np.float16)
        assert np.array_equal(self.conv16.astype(F32), outs[1].cpu().numpy()[..., :cout].reshape(n, h * w, cout))     # (fp16 values, fetched as fp32)
        ws = net.ws[((n, h, w), 0)][0]
        off = self.gap["off"] if self.gap else int(prog.ops[k + 1]["in2"]["off"])
        self.part = ws[off:off + n * self.splits * cout * 4].cpu().numpy().view(F32).reshape(n, self.splits, cout)

    def check_mean(self):
        """(a) against the fp64 mean of the stored conv output: fp32 summation, hw * 2^-24 * max|x|, plus half an fp16 ulp of the result."""
        n, h, w, _, _ = self.shape
        ref = self.conv16.astype(np.float64).mean(axis=1)
        got = self.g.astype(np.float64)
        bound = h * w * 2.0 ** -24 * np.abs(self.conv16.astype(np.float64)).max() + np.spacing(np.abs(self.g)).astype(np.float64) / 2
        err = np.abs(got - ref)
        print(f"{self.shape} {self.name}: fused {self.gap}; mean error max {err.max():.3e}, max error / bound {(err / bound).max():.3f}, "
              f"means {np.abs(ref).min():.3f} .. {np.abs(ref).max():.3f}")
        assert np.abs(ref).max() > 0.05 and (err <= bound).all()

    def check_order(self):
        """The slots hold the bits of the announced order, and the output is gap_finish_kernel's of them."""
        n, h, w, _, _ = self.shape
        x = self.conv16.astype(F32)
        if self.gap:
            m = re.fullmatch(r"conv_gemm_kernel<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+), 0>", self.name)
            assert m and int(m.group(1)) == self.gap["bm"], self.name
            want = [partials_of_the_conv(x[i], self.gap["bm"], int(m.group(3)), self.splits) for i in range(n)]
            other = [partials_of_the_pool(x[i], self.splits) for i in range(n)]
        else:
            want = [partials_of_the_pool(x[i], self.splits) for i in range(n)]
            other = None
        for i in range(n):
            slots = want[i].shape[0]
            assert np.array_equal(self.part[i, :slots], want[i]), (self.shape, i)
            assert np.array_equal(self.g[i], finish(want[i], h * w)), (self.shape, i)
        if other is not None:      # the restated orders are told apart by these inputs: the conv's sums are not gap_partial_kernel's
            assert any(o.shape != w_.shape or not np.array_equal(o, w_) for o, w_ in zip(other, want))


FUSED = [
    # n, h, w, cin, cout, kernel the conv record names, tiles per image, slots the finish pass reads, two contributors
    (3, 17, 30, 320, 40, "conv_gemm_kernel<256, 64, 4, 1, 32, 3, 0>", 2, 1, 1),
    (2, 16, 16, 320, 64, "conv_gemm_kernel<256, 64, 4, 1, 32, 3, 0>", 1, 1, 0),
    (2, 40, 40, 320, 64, "conv_gemm_kernel<256, 64, 4, 1, 32, 3, 0>", 7, 6, 1),
    (2, 20, 20, 320, 24, "conv_gemm_kernel<256, 32, 4, 1, 32, 3, 0>", 2, 1, 1),
    (3, 32, 32, 320, 128, "conv_gemm_kernel<128, 128, 2, 2, 32, 3, 0>", 8, 4, 1),
    (12, 34, 60, 320, 320, "conv_gemm_kernel<256, 192, 8, 2, 64, 2, 0>", 8, 7, 1),
    (6, 68, 120, 320, 256, "conv_gemm_kernel<256, 256, 4, 4, 64, 2, 0>", 32, 31, 1),
]
REFUSED = [
    # n, h, w, cin, cout, start of the kernel name, ragged
    (3, 17, 30, 320, 72, "conv_gemm_kernel<128, 128, 2, 2, 32, 3, 0>", False),        # four 128-row tiles for one slot
    (2, 40, 40, 320, 64, "conv_gemm_kernel<256, 64, 4, 1, 32, 3, 0>", True),           # a ragged plan
    (1, 64, 64, 64, 64, "conv_pw_kernel<", False),
    (3, 17, 30, 64, 72, "conv_smallm_kernel<", False),                                # the issue's four shapes
    (3, 34, 60, 128, 320, "conv_smallm_kernel<", False),
    (2, 16, 16, 64, 64, "conv_pw_kernel<", False),
    (2, 40, 40, 64, 64, "conv_pw_kernel<", False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("n,h,w,cin,cout,name,tiles,slots,atomic", FUSED)
def test_fused_pool_sums(ctx, n, h, w, cin, cout, name, tiles, slots, atomic):
    from vse_amd import engine
    seed = cout + 1000 * h + w
    x = _input(n, h, w, seed + 1)
    r = Run(ctx, n, h, w, cin, cout, seed, xs=[x])
    assert r.name == name and r.gap is not None, (r.name, r.gap)
    assert (r.gap["tiles"], r.gap["slots"], r.gap["atomic"], r.gap["moved"]) == (tiles, slots, atomic, 0), r.gap
    r.check_mean()                                                                                   # (a)
    r.check_order()                                                                                  # the conv summed, in the restated order
    # (b) the conv's output is that of the same conv with no pool behind it
    desc, wts, cols = _graph(cin, cout, False, True, seed)
    alone = engine.Net(ctx, desc, wts, fetch_cols=cols).run(x)[0].cpu().numpy()[..., :cout].reshape(n, h * w, cout)
    assert np.array_equal(alone, r.conv16.astype(F32))
    # (c) an image gives the same bits at another batch position, beside other images
    import torch
    y = _input(n, h, w, seed + 2)
    y[n - 1] = x[0]
    moved = Run(ctx, n, h, w, cin, cout, seed, xs=[y])
    assert np.array_equal(moved.g[n - 1].view(np.uint16), r.g[0].view(np.uint16))
    assert np.array_equal(moved.part[n - 1, :slots].view(np.uint32), r.part[0, :slots].view(np.uint32))
    assert not np.array_equal(moved.g[0], r.g[0])
    # (d) a second run on the same workspace, after another input, equals a fresh run
    again = Run(ctx, n, h, w, cin, cout, seed, xs=[y, torch.flip(y, dims=[0]), x])
    assert np.array_equal(again.g.view(np.uint16), r.g.view(np.uint16))
    assert np.array_equal(again.part[:, :slots].view(np.uint32), r.part[:, :slots].view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("n,h,w,cin,cout,name,ragged", REFUSED)
def test_refused_pairs_run_as_two_launches(ctx, n, h, w, cin, cout, name, ragged):
    r = Run(ctx, n, h, w, cin, cout, seed=cout + h, ragged=ragged)
    assert r.name.startswith(name) and r.gap is None, (r.name, r.gap)
    r.check_mean()                                                                                   # (a)
    if not ragged:
        r.check_order()                                                                              # gap_partial_kernel's slots and order


@pytest.mark.gpu
def test_partials_move_when_the_scratch_lies_over_the_conv_input(ctx):
    """Without a later reader of t0 the compiler lays the pool's scratch over the conv's input, which the conv still reads while its
    blocks finish.  The plan then keeps the partials in bytes that are dead while the pair runs, here the head of t4, which the conv
    behind the pool overwrites.  Everything, t4 included, equals the run of the graph that keeps t0 alive (partials in the scratch)."""
    n, h, w, cin, cout, seed = 2, 40, 40, 320, 64, 7
    x = _input(n, h, w, seed + 1)
    kept = Run(ctx, n, h, w, cin, cout, seed, xs=[x], post=512)
    loose = Run(ctx, n, h, w, cin, cout, seed, keep_t0=False, xs=[x, x], post=512)
    print("scratch in its own bytes:", kept.gap, "\nscratch over the input:   ", loose.gap)
    assert kept.gap is not None and kept.gap["moved"] == 0 and loose.gap is not None and loose.gap["moved"] == 1
    assert np.array_equal(loose.conv16, kept.conv16) and np.abs(kept.last).max() > 0
    assert np.array_equal(loose.last, kept.last)
    assert np.array_equal(loose.g.view(np.uint16), kept.g.view(np.uint16))
    loose.check_mean()
