"""An SE gate multiply directly followed by the residual add that reads its product runs as ONE pass, half(half(x * s) + r)
(scale_add_kernel, csrc/simple_ops.hip; the plan decides: scale_add_select, csrc/conv_select.hip).  The product is rounded to fp16 before
the add, as the stored intermediate was, so the result must equal the unfused pair's BIT FOR BIT, and the intermediate is never written.

Graph: two 1x1 lifts of the 3-channel feed to c channels, t0 and r; s = mean(t0) over the map; m = t0 * s; o = m + r.  Fetching m as well
keeps the product alive behind the add, which forces the two launches."""
import numpy as np
import pytest

import plan_select

GAP = {"pooling_type": "avg", "ksize": [1, 1], "strides": [1, 1], "paddings": [0, 0], "ceil_mode": False, "exclusive": True,
       "adaptive": True, "global_pooling": False, "padding_algorithm": "EXPLICIT"}


def _graph(c, keep_product, seed):
    conv1 = lambda a, f, b: {"type": "conv2d", "in": {"Input": [a], "Filter": [f]}, "out": {"Output": [b]},      # noqa: E731
                             "attrs": {"strides": [1, 1], "paddings": [0, 0], "groups": 1}}
    fetch = lambda a, k: {"type": "fetch", "in": {"X": [a]}, "out": {"Out": ["fetch"]}, "attrs": {"col": k}}      # noqa: E731
    ops = [{"type": "feed", "in": {"X": ["feed"]}, "out": {"Out": ["x"]}, "attrs": {"col": 0}}, conv1("x", "w0", "t0"), conv1("x", "w1", "r"),
           {"type": "pool2d", "in": {"X": ["t0"]}, "out": {"Out": ["s"]}, "attrs": dict(GAP)},
           {"type": "elementwise_mul", "in": {"X": ["t0"], "Y": ["s"]}, "out": {"Out": ["m"]}, "attrs": {"axis": -1}},
           {"type": "elementwise_add", "in": {"X": ["m"], "Y": ["r"]}, "out": {"Out": ["o"]}, "attrs": {"axis": -1}},
           fetch("o", 0)] + ([fetch("m", 1)] if keep_product else [])
    rng = np.random.default_rng(seed)
    desc = {"model": "unit", "ops": ops, "params": {"w0": {"dims": [c, 3, 1, 1], "dtype": 5}, "w1": {"dims": [c, 3, 1, 1], "dtype": 5}},
            "var_shapes": {"t0": [-1, c, -1, -1], "r": [-1, c, -1, -1], "s": [-1, c, 1, 1], "m": [-1, c, -1, -1], "o": [-1, c, -1, -1]}}
    # (a mean of a few tenths and products of order one: roundings of the product to fp16 matter to the sum)
    wts = {"w0": (rng.standard_normal((c, 3, 1, 1)) + 1.5).astype(np.float32), "w1": rng.standard_normal((c, 3, 1, 1)).astype(np.float32)}
    return desc, wts, (0, 1) if keep_product else (0,)


def _input(n, h, w, seed, widths=None):
    import torch
    from oracle import ir_emul
    x = np.random.default_rng(seed).uniform(0, 1, (n, 3, h, w)).astype(np.float16).astype(np.float32)
    for i, wi in enumerate(widths if widths is not None else []):
        x[i, :, :, wi:] = 0                                   # a ragged batch is zero right of each sample
    return torch.from_numpy(ir_emul.to_nhwc8(x).astype(np.float16)).cuda()


def _pair(prog):
    from vse_amd import ir
    k = [i for i, o in enumerate(prog.ops) if int(o["kind"]) == ir.OP_SCALE]
    assert len(k) == 1 and int(prog.ops[k[0] + 1]["kind"]) == ir.OP_BINARY and np.array_equal(prog.ops[k[0]]["out"], prog.ops[k[0] + 1]["in0"])
    return k[0]


@pytest.mark.gpu
@pytest.mark.parametrize("n,h,w,c,widths", [(2, 5, 7, 24, None), (2, 6, 33, 768, None), (3, 4, 40, 64, [40, 13, 26])])
def test_fused_scale_add_equals_the_pair(ctx, n, h, w, c, widths):
    import torch
    from vse_amd import engine
    ragged = widths is not None
    wv = np.asarray(widths, np.int32) if ragged else None
    x = _input(n, h, w, c + w, widths)
    # the pair as two launches: the product has a second reader
    desc, wts, cols = _graph(c, True, c)
    two = engine.Net(ctx, desc, wts, fetch_cols=cols, ragged=ragged)
    k2 = _pair(two.program(n, h, w))
    assert k2 not in plan_select.decisions(two.program(n, h, w).ops)[1]
    o2, m2 = [t.cpu().numpy()[..., :c] for t in two.run(x, widths=wv)]
    ms2 = two.profile(x, widths=wv)[0]
    assert ms2[k2] > 0 and ms2[k2 + 1] > 0
    # ... and as one
    desc, wts, cols = _graph(c, False, c)
    one = engine.Net(ctx, desc, wts, fetch_cols=cols, ragged=ragged)
    prog = one.program(n, h, w)
    k = _pair(prog)
    assert plan_select.decisions(prog.ops)[1] == {k: "in1"}
    (o1,) = [t.cpu().numpy()[..., :c] for t in one.run(x, widths=wv)]
    differing = int((o1 != o2).sum())
    exact = m2.astype(np.float64) + (o2.astype(np.float64) - m2.astype(np.float64))      # o2 - m2 ~ r: only shows the product matters
    print(f"{n}x{h}x{w}x{c}{' ragged' if ragged else ''}: differing values {differing}, |o| max {np.abs(o1).max():.3f}, "
          f"|m| max {np.abs(m2).max():.3f}, sums the product's rounding moved {(exact != o2).sum()}")
    assert np.abs(m2).max() > 0.5 and np.abs(o1).max() > 0.5
    assert np.array_equal(o1.view(np.uint32), o2.view(np.uint32))
    # the intermediate's bytes are untouched: a pattern laid over them survives the run, and the result is the same again
    s = prog.ops[k]["out"]
    lo = int(s["off"])
    hi = lo + ((n * h * w - 1) * int(s["ld"]) + int(s["c"])) * 2
    ws = one.ws[((n, h, w), 0)][0]
    a, b = int(prog.ops[k + 1]["out"]["off"]), int(prog.ops[k]["in0"]["off"])
    assert not (lo <= a < hi) and not (lo <= b < hi)
    ws[lo:hi] = 0x5A
    (o3,) = [t.cpu().numpy()[..., :c] for t in one.run(x, widths=wv)]
    torch.cuda.synchronize()
    assert bool((ws[lo:hi] == 0x5A).all())
    assert np.array_equal(o3.view(np.uint32), o2.view(np.uint32))
    ms, _, _ = one.profile(x, widths=wv)
    assert ms[k] > 0 and ms[k + 1] == 0.0                 # the launch's time goes to the scale record
