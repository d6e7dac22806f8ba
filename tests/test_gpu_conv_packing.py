"""Column packing of conv_c3_kernel / conv_col_kernel (csrc/conv_common.h): several images of a batch share one virtual row band, so
that the column tiles cover maps whose width is not a multiple of the tile width without half-empty tiles.  Packing only changes which
block and lane computes a pixel — never the values it sees or the order they are summed in — so a batch must equal, BIT FOR BIT, the
same images run one at a time (a batch of one cannot pack)."""
import re

import numpy as np
import pytest

from oracle import ir_emul
from test_gpu_nets import _up_res_graph

pytestmark = pytest.mark.gpu


def _conv_graph(cin, cout, k, rng):
    """test_conv_shapes' two-op graph: 1x1 lift to `cin` channels, then the 'same' k conv + bias + hard-swish."""
    desc = {"model": "unit", "ops": [
        {"type": "feed", "in": {"X": ["feed"]}, "out": {"Out": ["x"]}, "attrs": {"col": 0}},
        {"type": "conv2d", "in": {"Input": ["x"], "Filter": ["w0"]}, "out": {"Output": ["t0"]},
         "attrs": {"strides": [1, 1], "paddings": [0, 0], "groups": 1}},
        {"type": "conv2d", "in": {"Input": ["t0"], "Filter": ["w1"]}, "out": {"Output": ["t1"]},
         "attrs": {"strides": [1, 1], "paddings": [k[0] // 2, k[1] // 2], "groups": 1}},
        {"type": "elementwise_add", "in": {"X": ["t1"], "Y": ["b1"]}, "out": {"Out": ["t2"]}, "attrs": {"axis": 1}},
        {"type": "hard_swish", "in": {"X": ["t2"]}, "out": {"Out": ["t3"]}, "attrs": {"offset": 3.0, "scale": 6.0, "threshold": 6.0}},
        {"type": "fetch", "in": {"X": ["t3"]}, "out": {"Out": ["fetch"]}, "attrs": {"col": 0}}],
        "params": {"w0": {"dims": [cin, 3, 1, 1], "dtype": 5}, "w1": {"dims": [cout, cin, k[0], k[1]], "dtype": 5},
                   "b1": {"dims": [cout], "dtype": 5}},
        "var_shapes": {"t0": [-1, cin, -1, -1], "t1": [-1, cout, -1, -1]}}
    wts = {"w0": rng.standard_normal((cin, 3, 1, 1)).astype(np.float32),
           "w1": (rng.standard_normal((cout, cin, k[0], k[1])) / np.sqrt(cin * k[0] * k[1])).astype(np.float32),
           "b1": rng.standard_normal(cout).astype(np.float32) * 0.1}
    return desc, wts


def pack_group(images, ow, tw, spare, gap):
    """Mirror of conv_pack_group (csrc/conv_select.hip): images per virtual row band."""
    if ow % tw == 0 or images < 2:
        return 1
    tiles = lambda cols: -(-cols // tw)          # noqa: E731
    best, bg, g = images * tiles(ow), 1, 2
    while g <= 16 and g <= images:
        seams = max((min(x0 + tw, g * ow) - 1) // ow - x0 // ow for x0 in range(0, g * ow, tw))
        cost = images // g * tiles(g * ow) + tiles(images % g * ow)
        if seams * gap <= spare and cost < best:
            best, bg = cost, g
        g *= 2
    return bg


def big_conv_kernel(net, n, h, w, k):
    """(kernel name, images per group) of the program's k conv at batch n."""
    from vse_amd import engine, ir
    prog = net.program(n, h, w)
    names = engine.op_kernel_names(prog.ops)
    name = [nm for o, nm in zip(prog.ops, names) if int(o["kind"]) == ir.OP_CONV and (int(o["p"][ir.P_KH]), int(o["p"][ir.P_KW])) == k][0]
    m = re.fullmatch(r"conv_c3(n32)?_kernel<(\d), (\d)>", name)
    if m:
        return name, pack_group(n, w, 32 * int(m.group(3)), 6, 1)
    if name.startswith("conv_col_kernel<"):
        return name, pack_group(n, w, 32, 48 - (32 + k[1] - 1), k[1] // 2)
    return name, 1


def check_batch_equals_singles(ctx, desc, wts, rng, n, h, w, k, packs):
    import torch
    from vse_amd import engine
    net = engine.Net(ctx, desc, wts)
    name, g = big_conv_kernel(net, n, h, w, k)
    print(f"{k[0]}x{k[1]} {h}x{w} n={n}: {name}, {g} image(s) per column group")
    if packs:
        assert name.startswith(("conv_c3", "conv_col")) and g > 1, (name, g)
    x = rng.uniform(-1, 1, (n, 3, h, w)).astype(np.float16).astype(np.float32)
    xt = torch.from_numpy(ir_emul.to_nhwc8(x).astype(np.float16)).cuda()
    batch = net.run(xt)[0].cpu().numpy()
    assert batch.shape[0] == n and np.isfinite(batch).all() and np.abs(batch).max() > 0
    for i in range(n):
        single = net.run(xt[i:i + 1].contiguous())[0].cpu().numpy()
        assert np.array_equal(batch[i:i + 1], single), (i, np.abs(batch[i:i + 1].astype(np.float32) - single.astype(np.float32)).max())


# cin, cout, k, h, w, n, packs (the conv runs on a column kernel AND conv_pack_group puts several images into a group).
# The heights steer conv_c3_plan: 31 rows take 16 x 32 tiles, 39 rows 8 x 64, 33-35 rows 4 x 128 at these widths.
# Widths 33 and 70 tile too badly for the compiler to send them to a column kernel (conv_route.c3_tile_eff / RouteLimits.col_min_tile_eff judge the map
# unpacked), and 31 columns on 32-wide tiles leave nothing to gain: those cases check that the batch still equals its images.
# Tiles with several seams need maps narrower than half a tile, which the same routing keeps off these kernels.
CASES = [
    (32, 32, (3, 3), 31, 240, 2, True),        # conv_c3n32: 32 couts, 16 x 32 tiles; G capped by the batch
    (64, 64, (3, 3), 31, 240, 3, True),        # a pair + a short group of one
    (64, 64, (3, 3), 39, 240, 4, True),        # 8 x 64 tiles over 4 x 240 columns
    (64, 64, (3, 3), 39, 240, 5, True),        # ... + a short group of one
    (64, 64, (3, 3), 35, 240, 8, True),        # 4 x 128 tiles over 8 x 240 columns
    (128, 160, (3, 3), 17, 120, 16, True),     # three cout tiles, the last half empty (cout tail)
    (128, 160, (3, 3), 19, 120, 17, True),     # short last group (one image)
    (64, 64, (3, 3), 33, 60, 16, True),
    (48, 64, (3, 3), 31, 30, 16, True),        # 30-wide map: a seam inside most tiles
    (48, 64, (3, 3), 31, 30, 17, True),
    (64, 40, (3, 3), 39, 240, 4, True),        # cout tail (40 of 64)
    (64, 40, (3, 3), 33, 31, 3, False),
    (64, 64, (3, 3), 33, 31, 8, False),
    (48, 64, (3, 3), 19, 70, 2, False),
    (64, 64, (3, 3), 19, 33, 2, False),
    (64, 64, (3, 3), 35, 240, 3, False),       # 4 x 128 tiles: three images gain no tile
    (64, 64, (9, 9), 33, 240, 2, True),        # conv_col_kernel: gap of 4 columns
    (64, 64, (9, 9), 31, 240, 3, True),
    (48, 64, (9, 9), 31, 120, 8, True),        # odd chunk count
    (64, 64, (9, 9), 31, 60, 17, True),
    (32, 32, (7, 7), 33, 240, 4, True),
    (32, 32, (7, 7), 31, 30, 16, True),
    (64, 24, (5, 5), 31, 240, 5, True),        # cout tail (24 of 32)
    (64, 64, (5, 5), 31, 120, 4, True),
    (64, 40, (9, 5), 33, 60, 8, True),         # tall filter, 5 columns: gap of 2
    (16, 16, (7, 7), 33, 31, 3, False),
    (48, 64, (9, 9), 19, 33, 2, False),
    (128, 128, (3, 3), 136, 240, 8, True),     # full size: the detector's 128 -> 128 layers
    (256, 64, (9, 9), 136, 240, 8, True),      # ... and the large-kernel neck's 9 x 9
]


@pytest.mark.parametrize("cin,cout,k,h,w,n,packs", CASES)
def test_packed_batch_equals_single_images(ctx, cin, cout, k, h, w, n, packs):
    rng = np.random.default_rng(cin * 1000 + cout + w)
    desc, wts = _conv_graph(cin, cout, k, rng)
    check_batch_equals_singles(ctx, desc, wts, rng, n, h, w, k, packs)


@pytest.mark.parametrize("cin,cout,k,h,w,n", [(64, 64, (3, 3), 34, 120, 16), (128, 96, (3, 3), 34, 60, 16), (64, 64, (9, 9), 34, 120, 4),
                                              (32, 32, (5, 5), 32, 60, 8)])
def test_packed_batch_with_upsampled_input_and_residual(ctx, cin, cout, k, h, w, n):
    """The FPN pattern: input gathered through a nearest x2 upsample (P_INSHIFT: the group's images are half-size tensors) and a
    residual add in the epilogue (F_RES), which takes the lane's own image / row / column."""
    rng = np.random.default_rng(cin + cout + w)
    desc, wts = _up_res_graph(cin, cout, k, rng)
    check_batch_equals_singles(ctx, desc, wts, rng, n, h, w, k, True)


@pytest.mark.parametrize("cin,cout,k,h,w,n", [(192, 192, (3, 3), 34, 60, 16), (64, 64, (9, 9), 68, 120, 8)])
def test_packed_launch_race_screen(ctx, cin, cout, k, h, w, n):
    """test_column_kernels_race_screen's screen on packed launches: repeated under a competing stream, the outputs never change."""
    import torch
    from vse_amd import engine
    rng = np.random.default_rng(11)
    desc, wts = _conv_graph(cin, cout, k, rng)
    net = engine.Net(ctx, desc, wts)
    name, g = big_conv_kernel(net, n, h, w, k)
    assert name.startswith(("conv_c3", "conv_col")) and g > 1, (name, g)
    x = (torch.rand((n, h, w, 8), device="cuda") * 2 - 1).half()
    x[..., 3:] = 0
    first = net.run(x)[0].clone()
    side = torch.cuda.Stream()
    junk = torch.rand((4096, 4096), device="cuda")
    for rep in range(12):
        with torch.cuda.stream(side):
            for _ in range(1 + rep % 3):
                junk = junk @ junk * 1e-4           # competing load on another stream
        out = net.run(x)[0]
        assert torch.equal(out, first), rep
    torch.cuda.synchronize()
