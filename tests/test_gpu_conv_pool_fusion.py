"""A 3x3 conv whose only reader is a 3x3 / stride-2 max-pool runs with it as one kernel (csrc/conv_c3pool.hip; the plan decides,
conv_pool_select in csrc/conv_select.hip).  The fused kernel keeps the conv's K order and takes the maxima on the fp16 values the conv
would have stored, so its output must equal, BIT FOR BIT, the pool run on its own over the conv's output — for every map geometry, for
an output that is a channel slice of a concat buffer, for batches, and wherever the plan must NOT fuse (a second reader of the conv's
output, a ragged plan).

The kernel's tile / strip / carry index arithmetic is restated in Python below and checked against a plain max-pool on the CPU."""
import numpy as np
import pytest

POOL = {"pooling_type": "max", "ksize": [3, 3], "strides": [2, 2], "paddings": [1, 1], "ceil_mode": False, "exclusive": True,
        "adaptive": False, "global_pooling": False, "padding_algorithm": "EXPLICIT"}


def maxpool_3s2p1(a):
    """Plain 3x3 / stride-2 / pad-1 max-pool over axes (1, 2) of [n, h, w, c]; padding positions do not take part."""
    n, h, w, c = a.shape
    ph, pw = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out = np.empty((n, ph, pw, c), a.dtype)
    for r in range(ph):
        for q in range(pw):
            out[:, r, q] = a[:, max(2 * r - 1, 0):min(2 * r + 2, h), max(2 * q - 1, 0):min(2 * q + 2, w)].max(axis=(1, 2))
    return out


# ---- the kernel's index arithmetic, restated ------------------------------------------------------------------------------------

def strips(images, tiles_h, tiles_w, ntn):
    """conv_c3pool_strips: (tile rows per strip, strips)."""
    n = 1
    while images * tiles_w * ntn * n < 1024 and (tiles_h + n) // (n + 1) >= 4:
        n += 1
    seg = -(-tiles_h // n)
    return seg, -(-tiles_h // seg)


def fused_pool_by_tiles(a, images_for_strips):
    """What conv_c3pool_kernel's pool phase computes from conv values a [h, w] (one image, one channel): 8 x 32 tiles at conv column
    30 tx - 1, strips of tile rows with the column maxima of a tile's last row carried into the next, a strip that starts below the top
    running the tile above it for the carry alone; thread (pooled column pc < 15, row half rp) takes pooled rows 2 rp, 2 rp + 1."""
    h, w = a.shape
    lowest = -65504.0
    php, pwp = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    tiles_h, tiles_w = (h + 7) // 8, (pwp + 14) // 15
    seg, nseg = strips(images_for_strips, tiles_h, tiles_w, 1)
    assert nseg * seg >= tiles_h and (nseg - 1) * seg < tiles_h
    out = np.full((php, pwp), np.nan)
    for s in range(nseg):
        ty_first, ty_end = s * seg, min(s * seg + seg, tiles_h)
        for tx in range(tiles_w):
            ox0 = 30 * tx - 1
            carry = np.full(15, lowest)
            for ty in range(ty_first - 1 if ty_first > 0 else 0, ty_end):
                oy0 = 8 * ty
                tile = np.full((8, 32), np.nan)                   # the LDS tile: conv rows oy0 .. oy0 + 7, columns ox0 .. ox0 + 31
                for r in range(8):
                    for lc in range(32):
                        if 0 <= oy0 + r < h and 0 <= ox0 + lc < w:
                            tile[r, lc] = a[oy0 + r, ox0 + lc]

                def colmax(r, pc):
                    m = lowest
                    if oy0 + r >= h:
                        return m
                    for dc in range(3):
                        lc = 2 * pc + dc
                        if 0 <= ox0 + lc < w:
                            m = max(m, tile[r, lc])
                    return m
                new_carry = carry.copy()
                for pc in range(15):
                    for rp in range(2):
                        rb = 4 * rp
                        e = colmax(3 if rp else 7, pc)
                        first = e if rp else carry[pc]
                        va, vb, vc, vd = (colmax(rb + k, pc) for k in range(4))
                        if not rp:
                            new_carry[pc] = e
                        pcol, prow = 15 * tx + pc, 4 * ty + 2 * rp
                        if ty >= ty_first and pcol < pwp:
                            if prow < php:
                                assert np.isnan(out[prow, pcol])          # every pooled pixel is written once
                                out[prow, pcol] = max(first, va, vb)
                            if prow + 1 < php:
                                assert np.isnan(out[prow + 1, pcol])
                                out[prow + 1, pcol] = max(vb, vc, vd)
                carry = new_carry
    return out


SIZES = list(range(1, 41)) + [240, 272, 480]


@pytest.mark.parametrize("h", SIZES)
def test_tile_and_window_arithmetic_matches_a_plain_max_pool(h):
    """Heights and widths 1 .. 40, 240, 272, 480 (every height against a spread of widths that covers every residue of the 30-column
    tile step and both parities, and the reverse), at batch sizes that give one strip, a few strips and many strips."""
    rng = np.random.default_rng(h)
    if h <= 40:
        widths = SIZES
    else:
        widths = [1, 2, 15, 29, 30, 31, 32, 33, 59, 60, 61, 240, 272, 480]
    for w in widths:
        a = (rng.permutation(h * w).astype(np.float64).reshape(h, w) - (h * w) // 2) * (60000.0 / (h * w))    # distinct, both signs, fp16 range
        ref = maxpool_3s2p1(a[None, :, :, None])[0, :, :, 0]
        for images in ((1, 64, 4096) if h * w <= 41 * 480 else (1 if (h + w) % 2 else 64,)):
            got = fused_pool_by_tiles(a, images)
            assert np.array_equal(got, ref), (h, w, images)


def test_strip_plan():
    """The headline's stem (64 images, 34 x 16 tiles) runs whole column strips, half the batch two strips of 17 tile rows; no strip but a
    map's only one is shorter than 4."""
    assert strips(64, 34, 16, 1) == (34, 1)
    assert strips(32, 34, 16, 1) == (17, 2)
    for images in (1, 2, 3, 8, 64, 500):
        for th in range(1, 70):
            for tw in (1, 2, 16):
                seg, nseg = strips(images, th, tw, 1)
                assert (nseg - 1) * seg < th <= nseg * seg
                assert nseg == 1 or seg >= 4, (images, th, tw, seg, nseg)


# ---- on the GPU ---------------------------------------------------------------------------------------------------------------------

def _graph(cin, cout, mode, rng):
    """1x1 lift of the 3-channel feed to `cin` channels (t0), the 3x3 conv + bias + relu under test (t3) and, by mode:
    conv  fetch t3;
    dense p = maxpool(t3) -> fetch 0, q = maxpool(t0) -> fetch 1 (q keeps t0 alive behind the conv, so that p is not laid over it);
    slice concat(q, p) -> fetch: p's view is a channel slice of the concat buffer (ld > c);
    two_readers dense + fetch t3 itself: the conv's output has a second reader."""
    conv = [{"type": "feed", "in": {"X": ["feed"]}, "out": {"Out": ["x"]}, "attrs": {"col": 0}},
            {"type": "conv2d", "in": {"Input": ["x"], "Filter": ["w0"]}, "out": {"Output": ["t0"]},
             "attrs": {"strides": [1, 1], "paddings": [0, 0], "groups": 1}},
            {"type": "conv2d", "in": {"Input": ["t0"], "Filter": ["w1"]}, "out": {"Output": ["t1"]},
             "attrs": {"strides": [1, 1], "paddings": [1, 1], "groups": 1}},
            {"type": "elementwise_add", "in": {"X": ["t1"], "Y": ["b1"]}, "out": {"Out": ["t2"]}, "attrs": {"axis": 1}},
            {"type": "relu", "in": {"X": ["t2"]}, "out": {"Out": ["t3"]}, "attrs": {}}]
    pool = lambda a, b: {"type": "pool2d", "in": {"X": [a]}, "out": {"Out": [b]}, "attrs": dict(POOL)}          # noqa: E731
    fetch = lambda a, c: {"type": "fetch", "in": {"X": [a]}, "out": {"Out": ["fetch"]}, "attrs": {"col": c}}      # noqa: E731
    tail = {"conv": [fetch("t3", 0)],
            "dense": [pool("t3", "p"), pool("t0", "q"), fetch("p", 0), fetch("q", 1)],
            "slice": [pool("t3", "p"), pool("t0", "q"),
                      {"type": "concat", "in": {"X": ["q", "p"]}, "out": {"Out": ["c"]}, "attrs": {"axis": 1}}, fetch("c", 0)],
            "two_readers": [pool("t3", "p"), pool("t0", "q"), fetch("p", 0), fetch("q", 1), fetch("t3", 2)]}[mode]
    cols = {"conv": (0,), "dense": (0, 1), "slice": (0,), "two_readers": (0, 1, 2)}[mode]
    desc = {"model": "unit", "ops": conv + tail,
            "params": {"w0": {"dims": [cin, 3, 1, 1], "dtype": 5}, "w1": {"dims": [cout, cin, 3, 3], "dtype": 5}, "b1": {"dims": [cout], "dtype": 5}},
            "var_shapes": {"t0": [-1, cin, -1, -1], "t1": [-1, cout, -1, -1], "t2": [-1, cout, -1, -1], "t3": [-1, cout, -1, -1],
                           "p": [-1, cout, -1, -1], "q": [-1, cin, -1, -1], "c": [-1, cin + cout, -1, -1]}}
    wts = {"w0": rng.standard_normal((cin, 3, 1, 1)).astype(np.float32),
           "w1": (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(cin * 9)).astype(np.float32),
           "b1": rng.standard_normal(cout).astype(np.float32) * 0.1}
    return desc, wts, cols


def _run(ctx, cin, cout, mode, seed, x, ragged=False):
    """-> (outputs as numpy, kernel name of the 3x3 conv in a profiled run, ms of the pool behind it)."""
    from vse_amd import engine, ir
    desc, wts, cols = _graph(cin, cout, mode, np.random.default_rng(seed))
    net = engine.Net(ctx, desc, wts, fetch_cols=cols, ragged=ragged)
    outs = [o.cpu().numpy() for o in net.run(x)]
    ms, prog, names = net.profile(x)
    again = [o.cpu().numpy() for o in net.last_outs]
    assert all(np.array_equal(a, b) for a, b in zip(outs, again))
    k = [i for i, o in enumerate(prog.ops) if int(o["kind"]) == ir.OP_CONV and int(o["p"][ir.P_KH]) == 3][0]
    pool_ms = float(ms[k + 1]) if int(prog.ops[k + 1]["kind"]) == ir.OP_POOL else None
    unfused = engine.op_kernel_names(prog.ops)[k]
    assert unfused.startswith("conv_patch_kernel<8, ") and unfused.endswith(", 2>"), unfused       # the LIGHT family, by the record alone
    return outs, names[k], pool_ms


def _input(n, h, w, seed):
    import torch
    from oracle import ir_emul
    x = np.random.default_rng(seed).uniform(-1, 1, (n, 3, h, w)).astype(np.float16).astype(np.float32)
    return torch.from_numpy(ir_emul.to_nhwc8(x).astype(np.float16)).cuda()


# cin, cout, n, h, w.  64 input channels and 65 .. 128 couts are what the compiler sends to the LIGHT patch kernel's 128-cout tile (the
# stem's kernel); 64 couts reach its 64-cout tile only on maps that tile badly for conv_c3_kernel.
CASES = [
    (64, 128, 2, 272, 480),      # the detector stem's shape at a reduced batch: many strips, each with a carry-only tile
    (64, 128, 3, 40, 64),        # even height and width, batch 3
    (64, 128, 1, 41, 61),        # odd both: a tile row of ONE conv row, a tile column of ONE pooled column
    (64, 128, 2, 33, 63),        # one-row remainder, width one short of two full conv tiles
    (64, 128, 1, 80, 64),        # three strips of four tile rows in one image
    (64, 128, 1, 7, 30),         # smaller than one tile
    (64, 128, 2, 8, 31),         # exactly one tile row, 16 pooled columns: a second tile column for one of them
    (64, 96, 2, 25, 65),         # cout tail (96 of 128)
    (64, 64, 1, 7, 30),          # the 64-cout tile
    (64, 64, 4, 9, 31),
]


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,n,h,w", CASES)
@pytest.mark.parametrize("mode", ["dense", "slice"])
def test_fused_conv_pool_equals_the_pool_alone(ctx, cin, cout, n, h, w, mode):
    seed = cout + h * 1000 + w
    x = _input(n, h, w, seed)
    (conv,), cname, _ = _run(ctx, cin, cout, "conv", seed, x)                        # (b) the conv alone, fetched (fp32 of the same sums)
    conv16 = conv[..., :cout].astype(np.float16)                                     # ... as the fp16 tensor the pair passes on
    assert cname.startswith("conv_patch_kernel<8, ")
    # (c) the pool alone on (b)'s output: pool_kernel itself, in the graph whose conv output has a second reader and so cannot fuse
    (p_un, q_un, t3_un), uname, ums = _run(ctx, cin, cout, "two_readers", seed, x)
    assert uname.startswith("conv_patch_kernel<8, ") and ums > 0.0, (uname, ums)
    assert np.array_equal(t3_un[..., :cout], conv[..., :cout])
    assert np.array_equal(p_un[..., :cout], maxpool_3s2p1(conv16).astype(np.float32))
    # (a) conv -> pool, fused
    outs, fname, fms = _run(ctx, cin, cout, mode, seed, x)
    assert fname == "conv_c3pool_kernel<%d>" % (128 if cout > 64 else 64) and fms == 0.0, (fname, fms)
    if mode == "dense":
        p, q = outs[0][..., :cout], outs[1][..., :cin]
    else:
        assert outs[0].shape[3] >= cin + cout                                        # p = channels cin .. cin + cout of the concat buffer
        q, p = outs[0][..., :cin], outs[0][..., cin:cin + cout]
    print(f"{mode} {cin}->{cout} n{n} {h}x{w}: {fname}, pooled max {p.max():.3f}, differing values {(p != p_un[..., :cout]).sum()}")
    assert p.shape == p_un[..., :cout].shape and np.abs(p).max() > 0
    assert np.array_equal(p, p_un[..., :cout])
    assert np.array_equal(q, q_un[..., :cin])                                        # the neighbouring slice is untouched


@pytest.mark.gpu
def test_a_ragged_plan_is_not_fused(ctx):
    cin, cout, n, h, w = 64, 128, 2, 40, 64
    x = _input(n, h, w, 5)
    (p, q), name, ms = _run(ctx, cin, cout, "dense", 5, x, ragged=True)
    assert name.startswith("conv_patch_kernel<8, ") and ms > 0.0, (name, ms)
    (p_f, q_f), fname, _ = _run(ctx, cin, cout, "dense", 5, x)
    assert fname == "conv_c3pool_kernel<128>"
    assert np.array_equal(p, p_f) and np.array_equal(q, q_f)                         # (uniform widths: the ragged plan computes the same map)
