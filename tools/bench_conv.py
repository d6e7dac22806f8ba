#!/usr/bin/env python3
"""Single-layer timing of the conv kernels on the GPU, per kernel family the compiler may route a layer to.

usage: python tools/bench_conv.py [--cfgs d,p,c] [--layers name,name...]
       python tools/bench_conv.py --pool [--layers name,name...]     (3x3 layers: conv + 3x3 / s2 max-pool, fused against the two launches)
  d: implicit GEMM only (conv_gemm_kernel, the launcher's tile configuration)
  p: + conv_patch_kernel / conv_col_kernel
  c: + conv_c3_kernel for any couts
Each layer is a two-op graph (1x1 stem lifting the 3-channel feed to `cin`, then the conv under test); the conv under
test is timed with HIP events (vse_plan_profile), min of 3."""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from vse_amd import engine
from vse_amd.conv_route import RouteLimits

LAYERS = {  # name: cin, cout, k, stride, pad, h, w, n
    "det_1x1_896_256": (896, 256, (1, 1), (1, 1), (0, 0), 136, 240, 64),
    "det_1x1_1216_512": (1216, 512, (1, 1), (1, 1), (0, 0), 68, 120, 64),
    "det_1x1_256_256": (256, 256, (1, 1), (1, 1), (0, 0), 136, 240, 64),
    "det_1x1_1920_768": (1920, 768, (1, 1), (1, 1), (0, 0), 34, 60, 64),
    "det_1x1_512_256": (512, 256, (1, 1), (1, 1), (0, 0), 68, 120, 64),
    "det_1x1_768_256": (768, 256, (1, 1), (1, 1), (0, 0), 34, 60, 64),
    "det_3x3_64_128": (64, 128, (3, 3), (1, 1), (1, 1), 272, 480, 64),
    "det_3x3_64_64": (64, 64, (3, 3), (1, 1), (1, 1), 272, 480, 64),
    "det_1x1_64_256": (64, 256, (1, 1), (1, 1), (0, 0), 272, 480, 64),
    "det_1x1_896_256": (896, 256, (1, 1), (1, 1), (0, 0), 136, 240, 64),
    "det_1x1_1216_512": (1216, 512, (1, 1), (1, 1), (0, 0), 68, 120, 64),
    "det_1x1_256_256": (256, 256, (1, 1), (1, 1), (0, 0), 136, 240, 64),
    "det_1x1_1920_768": (1920, 768, (1, 1), (1, 1), (0, 0), 34, 60, 64),
    "rec_1x1_1216_512": (1216, 512, (1, 1), (1, 1), (0, 0), 12, 256, 32),
    "rec_1x1_1920_768": (1920, 768, (1, 1), (1, 1), (0, 0), 6, 256, 32),
    "rec_1x1_896_256": (896, 256, (1, 1), (1, 1), (0, 0), 12, 512, 32),
    "rec_3x3_224_224": (224, 224, (3, 3), (1, 1), (1, 1), 3, 256, 32),
    "det_3x3_192_192": (192, 192, (3, 3), (1, 1), (1, 1), 34, 60, 64),
    "det_3x3_160_160": (160, 160, (3, 3), (1, 1), (1, 1), 68, 120, 64),
    "rec_3x3_192_192": (192, 192, (3, 3), (1, 1), (1, 1), 6, 256, 32),
    "rec_3x3_160_160": (160, 160, (3, 3), (1, 1), (1, 1), 12, 256, 32),
    "det_3x3_128_128": (128, 128, (3, 3), (1, 1), (1, 1), 136, 240, 64),
    "det_3x3_256_64": (256, 64, (3, 3), (1, 1), (1, 1), 136, 240, 64),
    "det_3x3_256_160": (256, 160, (3, 3), (1, 1), (1, 1), 68, 120, 64),
    "det_3x3_768_192": (768, 192, (3, 3), (1, 1), (1, 1), 34, 60, 64),
    "det_9x9_256_64": (256, 64, (9, 9), (1, 1), (4, 4), 136, 240, 64),
    "det_9x9_64_64": (64, 64, (9, 9), (1, 1), (4, 4), 136, 240, 64),
    "det_9x9_256_64_h68": (256, 64, (9, 9), (1, 1), (4, 4), 68, 120, 64),
    "det_9x9_256_64_h34": (256, 64, (9, 9), (1, 1), (4, 4), 34, 60, 64),
    "det_9x9_256_64_h17": (256, 64, (9, 9), (1, 1), (4, 4), 17, 30, 64),
    "det_9x9_64_64_h68": (64, 64, (9, 9), (1, 1), (4, 4), 68, 120, 64),
    "det_3x3_256_64_h68": (256, 64, (3, 3), (1, 1), (1, 1), 68, 120, 64),
    "det_3x3_224_224": (224, 224, (3, 3), (1, 1), (1, 1), 17, 30, 64),
    "det_3x3_32_32": (32, 32, (3, 3), (1, 1), (1, 1), 136, 240, 64),
    "det_3x3_32_32_h68": (32, 32, (3, 3), (1, 1), (1, 1), 68, 120, 64),
    "det_1x1_32_64": (32, 64, (1, 1), (1, 1), (0, 0), 136, 240, 64),
    "det_1x1_64_32": (64, 32, (1, 1), (1, 1), (0, 0), 136, 240, 64),
    "rec_3x3_128_128_w768": (128, 128, (3, 3), (1, 1), (1, 1), 12, 384, 28),
    "rec_3x3_160_160_w768": (160, 160, (3, 3), (1, 1), (1, 1), 12, 192, 28),
    "rec_3x3_192_192_w768": (192, 192, (3, 3), (1, 1), (1, 1), 6, 192, 28),
    "rec_3x3_768_192_w768": (768, 192, (3, 3), (1, 1), (1, 1), 6, 192, 28),
    "rec_3x3_224_224_w768": (224, 224, (3, 3), (1, 1), (1, 1), 3, 192, 28),
    "det_7x7_32_32": (32, 32, (7, 7), (1, 1), (3, 3), 136, 240, 64),
    "det_5x5_32_32": (32, 32, (5, 5), (1, 1), (2, 2), 136, 240, 64),
    "rec_3x3_128_128": (128, 128, (3, 3), (1, 1), (1, 1), 12, 512, 32),
    "rec_3x3_768_192": (768, 192, (3, 3), (1, 1), (1, 1), 6, 256, 32),
    "rec_3x3_256_160": (256, 160, (3, 3), (1, 1), (1, 1), 12, 256, 32),
    "rec_3x3_64_128": (64, 128, (3, 3), (1, 1), (1, 1), 24, 512, 32),
}


def graph(cin, cout, k, s, p):
    desc = {"model": "unit", "ops": [
        {"type": "feed", "in": {"X": ["feed"]}, "out": {"Out": ["x"]}, "attrs": {"col": 0}},
        {"type": "conv2d", "in": {"Input": ["x"], "Filter": ["w0"]}, "out": {"Output": ["t0"]},
         "attrs": {"strides": [1, 1], "paddings": [0, 0], "groups": 1}},
        {"type": "conv2d", "in": {"Input": ["t0"], "Filter": ["w1"]}, "out": {"Output": ["t1"]},
         "attrs": {"strides": list(s), "paddings": list(p), "groups": 1}},
        {"type": "elementwise_add", "in": {"X": ["t1"], "Y": ["b1"]}, "out": {"Out": ["t2"]}, "attrs": {"axis": 1}},
        {"type": "relu", "in": {"X": ["t2"]}, "out": {"Out": ["t3"]}, "attrs": {}},
        {"type": "fetch", "in": {"X": ["t3"]}, "out": {"Out": ["fetch"]}, "attrs": {"col": 0}}],
        "params": {"w0": {"dims": [cin, 3, 1, 1], "dtype": 5}, "w1": {"dims": [cout, cin, k[0], k[1]], "dtype": 5},
                   "b1": {"dims": [cout], "dtype": 5}},
        "var_shapes": {"t0": [-1, cin, -1, -1], "t1": [-1, cout, -1, -1]}}
    rng = np.random.default_rng(1)
    wts = {"w0": rng.standard_normal((cin, 3, 1, 1)).astype(np.float32),
           "w1": (rng.standard_normal((cout, cin, k[0], k[1])) / np.sqrt(cin * k[0] * k[1])).astype(np.float32),
           "b1": rng.standard_normal(cout).astype(np.float32) * 0.1}
    return desc, wts


def cfg_limits(c):
    """The routing thresholds of --cfgs letter c."""
    return RouteLimits(patch_min_k={"d": 1 << 30, "p": 500, "c": 100}[c],
                       patch_max_cout=256 if c == "p" else 64,       # "p": also try the patch kernel on wide layers (two+ cout tiles)
                       col3_max_cout=4096 if c == "c" else 0,        # 0: no layer (coutp >= 8) goes to conv_c3_kernel
                       col3_min_tile_eff=0.0, col3_wide_min_cin=0, col3_min_k=100)


def pool_graph(cin, cout, second_reader):
    """lift -> 3x3 conv + bias + relu (t3) -> p = 3x3 / s2 / p1 max-pool, fetched; q = the same pool of the lifted input keeps that tensor alive
    behind the conv (else the compiler lays p over it and the pair cannot run as one kernel).  second_reader: t3 is fetched too, which
    keeps the plan from fusing: the same conv and pool as two launches."""
    desc, wts = graph(cin, cout, (3, 3), (1, 1), (1, 1))
    pool = {"pooling_type": "max", "ksize": [3, 3], "strides": [2, 2], "paddings": [1, 1], "ceil_mode": False, "exclusive": True,
            "adaptive": False, "global_pooling": False, "padding_algorithm": "EXPLICIT"}
    desc["ops"] = desc["ops"][:-1] + [
        {"type": "pool2d", "in": {"X": ["t3"]}, "out": {"Out": ["p"]}, "attrs": dict(pool)},
        {"type": "pool2d", "in": {"X": ["t0"]}, "out": {"Out": ["q"]}, "attrs": dict(pool)},
        {"type": "fetch", "in": {"X": ["p"]}, "out": {"Out": ["fetch"]}, "attrs": {"col": 0}},
        {"type": "fetch", "in": {"X": ["q"]}, "out": {"Out": ["fetch"]}, "attrs": {"col": 1}},
        {"type": "fetch", "in": {"X": ["t3"]}, "out": {"Out": ["fetch"]}, "attrs": {"col": 2}}]
    desc["var_shapes"].update({"t2": [-1, cout, -1, -1], "t3": [-1, cout, -1, -1], "p": [-1, cout, -1, -1], "q": [-1, cin, -1, -1]})
    return desc, wts, (0, 1, 2) if second_reader else (0, 1)


def pool_main(names):
    """conv + max-pool as one kernel (conv_c3pool_kernel, where the plan fuses the pair) against conv and pool_kernel as two launches."""
    ctx = engine.Context(0)
    for name in names:
        cin, cout, k, s, p, h, w, n = LAYERS[name]
        if (k, s, p) != ((3, 3), (1, 1), (1, 1)):
            continue
        x = (torch.rand((n, h, w, 8), device="cuda") * 2 - 1).half()
        x[..., 3:] = 0
        row = []
        for second_reader in (True, False):
            desc, wts, cols = pool_graph(cin, cout, second_reader)
            net = engine.Net(ctx, desc, wts, fetch_cols=cols)
            net.run(x)
            torch.cuda.synchronize()
            best = (1e9, 0.0, 0.0, "")
            for _ in range(5):
                ms, prog, var = net.profile(x)
                best = min(best, (float(ms[1] + ms[2]), float(ms[1]), float(ms[2]), var[1]))
            row.append(f"{best[3]}: {best[1]:.3f} + pool {best[2]:.3f} = {best[0]:.3f} ms")
            del net
            torch.cuda.empty_cache()
        print(f"{name:20s} " + " | ".join(row), flush=True)


def main():
    if "--pool" in sys.argv:
        return pool_main(sys.argv[sys.argv.index("--layers") + 1].split(",") if "--layers" in sys.argv else ["det_3x3_64_128"])
    cfgs = sys.argv[sys.argv.index("--cfgs") + 1].split(",") if "--cfgs" in sys.argv else ["d"]
    if not set(cfgs) <= {"d", "p", "c"}:
        sys.exit(f"unknown --cfgs {cfgs}: d, p, c")
    names = sys.argv[sys.argv.index("--layers") + 1].split(",") if "--layers" in sys.argv else list(LAYERS)
    ctx = engine.Context(0)
    for name in names:
        cin, cout, k, s, p, h, w, n = LAYERS[name]
        desc, wts = graph(cin, cout, k, s, p)
        nets = {key: engine.Net(ctx, desc, wts, want_probs=False, limits=cfg_limits(key)) for key in cfgs}
        x = (torch.rand((n, h, w, 8), device="cuda") * 2 - 1).half()
        x[..., 3:] = 0
        oh = (h + 2 * p[0] - k[0]) // s[0] + 1
        ow = (w + 2 * p[1] - k[1]) // s[1] + 1
        flops = 2.0 * n * oh * ow * cout * cin * k[0] * k[1]
        row = []
        for c in cfgs:
            net = nets[c]
            net.run(x)
            torch.cuda.synchronize()
            best = 1e9
            for _ in range(3):
                ms, prog, var = net.profile(x)
                best = min(best, float(ms[1]))
            row.append(f"cfg{c}: {best:7.3f} ms {flops / best / 1e9:6.0f} TF/s")
        print(f"{name:20s} " + " | ".join(row), flush=True)
        del net, nets, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
