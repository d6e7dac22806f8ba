"""Graph compiler (fusion, BN folding, concat placement, NHWC/padding, weight tiling, buffer reuse, attention
matching) validated on CPU: compiled program run by the IR emulator vs the op-by-op oracle interpreter."""
import os
import numpy as np
import pytest

from oracle import ir_emul, net_ref
from vse_amd import compiler, ir

CASES = [("V4_ch_det", (1, 3, 64, 96)), ("V4_ch_det_fast", (1, 3, 64, 96)), ("V3_ch_det_fast", (1, 3, 64, 96)),
         ("V2_ch_det", (1, 3, 64, 64)), ("V4_ch_rec", (2, 3, 48, 96)), ("V4_ch_rec_fast", (1, 3, 48, 160)),
         ("V4_en_rec_fast", (2, 3, 48, 96)), ("V3_ch_rec_fast", (1, 3, 48, 96)), ("V3_korean_rec_fast", (1, 3, 48, 96)),
         ("V2_ch_rec", (2, 3, 32, 64))]


@pytest.mark.parametrize("mid,shape", CASES)
def test_program_matches_oracle(mid, shape):
    desc, w = net_ref.get_weights(mid)
    x = np.random.default_rng(0).uniform(-1, 1, shape).astype(np.float16).astype(np.float32)
    ref = net_ref.run_graph(desc, w, x)[0].numpy()
    prog = compiler.compile_model(desc, w, shape[0], shape[2], shape[3])
    out = ir_emul.Emulator(prog).run(ir_emul.to_nhwc8(x))
    if "_det" in mid:
        got, r = out[0][..., 0], ref[:, 0]
        if mid != "V3_ch_det_fast":            # real weights + noise input -> map is ~0 everywhere
            assert r.max() - r.min() > 0.2, "synthetic det head must not be saturated"
        assert np.abs(got - r).max() < 5e-3
    else:
        # fp16 WEIGHTS, fp32 activations (the emulator's default) against the fp32 interpreter: log-probabilities of every class, max
        # probability, arg-max outside near-ties — the bounds of tests/parity.py (the engine adds fp16 activation storage on top)
        from parity import check_rec_probs
        check_rec_probs(mid, out[0][:, 0], ref, idx=out[-1].view(np.int32)[:, 0, :, 0])
    assert len(prog.ops) < 0.5 * len(desc["ops"])        # fusion actually happened
    assert all(int(o["kind"]) in range(ir.OP_CONV, ir.OP_WSCALE + 1) for o in prog.ops)


@pytest.mark.parametrize("mid", ["V3_ch_det_fast", "V4_ch_det_fast", "V2_ch_det"])
def test_hilo_weights_track_the_fp32_reference(mid):
    """compile_model(hilo=True): fp16 hi + lo weight pairs.  With fp32 activations in the emulator the only deviation left
    is ~22-bit weight rounding: the map agrees with the fp32 interpreter an order of magnitude better than with fp16
    weights (the weight rounding, not the activation storage, is what moves box borders: DESIGN §4)."""
    desc, w = net_ref.get_weights(mid)
    if mid == "V3_ch_det_fast":
        from vse_amd import synth
        from oracle import pipeline_ref
        x, _ = pipeline_ref.det_preprocess(synth.make_frames(1, 270, 480, seed=5)[0])
    else:
        x = np.random.default_rng(0).uniform(-1, 1, (1, 3, 64, 96)).astype(np.float32)
    x = x.astype(np.float16).astype(np.float32)
    ref = net_ref.run_graph(desc, w, x)[0].numpy()[:, 0]
    err = {}
    for hilo in (False, True):
        prog = compiler.compile_model(desc, w, 1, x.shape[2], x.shape[3], hilo=hilo)
        assert all(bool(int(o["flags"]) & (ir.F_HILO | ir.F_HLSUM)) == hilo for o in prog.ops if int(o["kind"]) in (ir.OP_CONV, ir.OP_DWCONV))
        assert not any(int(o["flags"]) & (ir.F_PATCH | ir.F_UP2HEAD) for o in prog.ops) or not hilo
        err[hilo] = np.abs(ir_emul.Emulator(prog).run(ir_emul.to_nhwc8(x))[0][..., 0] - ref).max()
    # (the real-weight detector's head amplifies what is left ~15x: 5e-3 on the map instead of 4e-2 with fp16 weights)
    assert err[True] < 1e-2 and err[True] < 0.25 * err[False] + 1e-6, err


def test_gmacs_match_survey():
    # 194.70 GMAC / frame (server det @544x960), 10.14 GMAC / 48x320 crop (server rec)
    desc, w = net_ref.get_weights("V4_ch_rec")
    prog = compiler.compile_model(desc, w, 1, 48, 320)
    assert abs(prog.gmacs - 10.142) < 0.02
    desc, w = net_ref.get_weights("V4_ch_det_fast")
    prog = compiler.compile_model(desc, w, 1, 544, 960)
    assert abs(prog.gmacs - 2.935) < 0.01


def test_buffer_reuse_is_safe():
    desc, w = net_ref.get_weights("V4_ch_det_fast")
    x = np.random.default_rng(1).uniform(-1, 1, (1, 3, 64, 96)).astype(np.float16).astype(np.float32)
    a = compiler.compile_model(desc, w, 1, 64, 96, reuse=True)
    b = compiler.compile_model(desc, w, 1, 64, 96, reuse=False)
    assert a.ws_bytes < b.ws_bytes
    oa = ir_emul.Emulator(a).run(ir_emul.to_nhwc8(x))[0]
    ob = ir_emul.Emulator(b).run(ir_emul.to_nhwc8(x))[0]
    assert np.array_equal(oa, ob)


def test_weight_store_is_shape_independent():
    desc, w = net_ref.get_weights("V4_en_rec_fast")
    store = compiler.WeightStore()
    compiler.compile_model(desc, w, 1, 48, 320, store=store)
    n = len(store.blob)
    compiler.compile_model(desc, w, 4, 48, 640, store=store)
    assert len(store.blob) == n


def test_kernel_selection_and_head_fusion_at_full_size():
    """At the reference's det size the k x k stride-1 convs go to the LDS-resident-patch family (conv_patch_kernel, or the
    column-per-step kernels conv_col_kernel / conv_c3_kernel = F_COL), the DB head's
    1x1->1-channel conv + sigmoid is folded into its producer (F_DOT1) and the upsample+concat in front of it is a
    virtual 2-source gather (F_SRC2): no 64-channel 544x960 tensor is written or copied."""
    desc, w = net_ref.get_weights("V4_ch_det")
    prog = compiler.compile_model(desc, w, 1, 544, 960)
    flags = [int(o["flags"]) for o in prog.ops if int(o["kind"]) == ir.OP_CONV]
    assert sum(bool(f & (ir.F_PATCH | ir.F_COL)) for f in flags) >= 30 and sum(bool(f & ir.F_COL) for f in flags) >= 20
    # every column-kernel op obeys the kernels' preconditions (conv_col_ok / conv_c3_ok)
    for o in prog.ops:
        if int(o["kind"]) == ir.OP_CONV and int(o["flags"]) & ir.F_COL:
            p = o["p"]
            assert not int(o["flags"]) & (ir.F_PATCH | ir.F_SRC2 | ir.F_DOT1 | ir.F_HILO | ir.F_PIXSHUF)
            assert (p[ir.P_SH], p[ir.P_SW]) == (1, 1) and p[ir.P_CINP] % 16 == 0 and p[ir.P_KH] in (3, 5, 7, 9)
            assert p[ir.P_COUT] <= (192 if p[ir.P_KH] == 3 else 64) and p[ir.P_KTOT] == p[ir.P_KH] * p[ir.P_KW] * p[ir.P_CINP]
    assert sum(bool(f & ir.F_DOT1) for f in flags) == 1 and sum(bool(f & ir.F_SRC2) for f in flags) == 1
    # ... and that last conv runs on the LOW-RES grid with folded 2x2 taps (conv_head.hip): same algorithmic MACs reported
    assert sum(bool(f & ir.F_UP2HEAD) for f in flags) == 1
    assert not any(int(o["kind"]) == ir.OP_RESIZE and int(o["out"]["h"]) == 544 for o in prog.ops)
    assert abs(prog.gmacs - 194.703) < 0.05                      # 194.70 GMAC per 544x960 frame
    assert prog.outputs[0]["kind"] == "map" and prog.outputs[0]["esize"] == 4 and prog.outputs[0]["c"] == 1
    # every patch op obeys the kernel's preconditions
    for o in prog.ops:
        if int(o["kind"]) == ir.OP_CONV and int(o["flags"]) & ir.F_PATCH:
            p = o["p"]
            assert (p[ir.P_SH], p[ir.P_SW]) == (1, 1) and p[ir.P_KH] * p[ir.P_KW] >= 5
            assert (8 + p[ir.P_KH] - 1) * (32 + p[ir.P_KW] - 1) <= 640 and p[ir.P_COUT] <= 128


def test_head_up2_folding_is_exact():
    """conv3x3(concat[u, up2(x)]) == per-parity 2x2 convs over x with the folded weights + 3x3 over u (fp64 identity that
    conv_head_up2_kernel relies on), including the zero padding at the map border."""
    import torch
    import torch.nn.functional as F
    rng = np.random.default_rng(3)
    cout, hl, wl = 5, 6, 7
    w = rng.standard_normal((cout, 65, 3, 3))
    x = rng.standard_normal((2, 64, hl, wl))
    u = rng.standard_normal((2, 1, 2 * hl, 2 * wl))
    full = torch.cat([torch.from_numpy(u), torch.from_numpy(x).repeat_interleave(2, 2).repeat_interleave(2, 3)], 1)
    ref = F.conv2d(full, torch.from_numpy(w), None, 1, 1).numpy()
    # matrix in the compiler's K order: (tap, physical channel) with u at physical channel 0 and x at 8..71
    mat = np.zeros((8, 9 * 72))
    m4 = mat.reshape(8, 3, 3, 72)
    m4[:cout, :, :, 0] = w[:, 0]
    m4[:cout, :, :, 8:72] = np.transpose(w[:, 1:], (0, 2, 3, 1))
    stream = compiler.Compiler.head_up2_weights(mat, 72).astype(np.float64)      # fp16-rounded folded weights
    wx = stream[:2 * 4 * 4 * 64 * 32].reshape(2, 4, 4, 64, 32)
    wu = stream[2 * 4 * 4 * 64 * 32:].reshape(64, 32)[:cout, :9].reshape(cout, 1, 3, 3)
    got = F.conv2d(torch.from_numpy(u), torch.from_numpy(wu), None, 1, 1).numpy()
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    for a in range(2):
        for b in range(2):
            wk = np.concatenate([wx[0, a * 2 + b], wx[1, a * 2 + b]], axis=2)[:, :cout]          # [tap][cout][64]
            w4 = np.ascontiguousarray(wk.reshape(2, 2, cout, 64).transpose(2, 3, 0, 1))
            z = F.conv2d(torch.from_numpy(xp[:, :, a:a + hl + 1, b:b + wl + 1]), torch.from_numpy(w4)).numpy()
            got[:, :, a::2, b::2] += z
    # the only difference is the fp16 rounding of the (summed) weights
    assert np.abs(got - ref).max() < 2e-2 * np.abs(ref).max()
    # exactness of the folding itself: repeat with weights that are exactly representable in fp16
    w_q = np.round(w * 8) / 8
    m4[:] = 0
    m4[:cout, :, :, 0] = w_q[:, 0]
    m4[:cout, :, :, 8:72] = np.transpose(w_q[:, 1:], (0, 2, 3, 1))
    stream = compiler.Compiler.head_up2_weights(mat, 72).astype(np.float64)
    wx = stream[:2 * 4 * 4 * 64 * 32].reshape(2, 4, 4, 64, 32)
    wu = stream[2 * 4 * 4 * 64 * 32:].reshape(64, 32)[:cout, :9].reshape(cout, 1, 3, 3)
    ref = F.conv2d(full, torch.from_numpy(w_q), None, 1, 1).numpy()
    got = F.conv2d(torch.from_numpy(u), torch.from_numpy(wu), None, 1, 1).numpy()
    for a in range(2):
        for b in range(2):
            wk = np.concatenate([wx[0, a * 2 + b], wx[1, a * 2 + b]], axis=2)[:, :cout]
            w4 = np.ascontiguousarray(wk.reshape(2, 2, cout, 64).transpose(2, 3, 0, 1))
            got[:, :, a::2, b::2] += F.conv2d(torch.from_numpy(xp[:, :, a:a + hl + 1, b:b + wl + 1]), torch.from_numpy(w4)).numpy()
    assert np.abs(got - ref).max() < 1e-9


def test_light_patch_variant_selection():
    """3x3 stride-1 convs with up to 128 couts on well-tiling maps take the LIGHT patch variant: taps are padded to 2
    (two taps per step).  The tall filters of the large-kernel neck (9x9, and the 7x7 / 5x5 IntraCL merges) go to the
    column-per-step kernel (F_COL): no tap padding, K = taps x channels exactly."""
    desc, w = net_ref.get_weights("V4_ch_det")
    prog = compiler.compile_model(desc, w, 1, 544, 960)
    seen, col = set(), set()
    for o in prog.ops:
        p = o["p"]
        taps = int(p[ir.P_KH]) * int(p[ir.P_KW])
        if int(o["kind"]) == ir.OP_CONV and int(o["flags"]) & ir.F_PATCH and not int(o["flags"]) & ir.F_UP2HEAD:
            ptaps = int(p[ir.P_KTOT]) // ((int(p[ir.P_CINP]) + 31) // 32 * 32)
            seen.add((taps, ptaps))
        if int(o["kind"]) == ir.OP_CONV and int(o["flags"]) & ir.F_COL:
            assert not int(o["flags"]) & ir.F_PATCH and int(p[ir.P_KTOT]) == taps * int(p[ir.P_CINP])
            col.add(taps)
    # (the 17x30 maps of the coarsest pyramid level tile badly into 16-row tiles and stay on the 8-row patch variant)
    # (... and the 3x3 layers with more than 64 couts over 64 input channels stay on LIGHT; the other 3x3 layers up to 192 couts
    # run on conv_c3_kernel)
    assert (9, 10) in seen and col == {81, 49, 25, 9}


@pytest.mark.parametrize("optype,attr,value", [("conv2d", "dilations", [2, 2]), ("conv2d", "padding_algorithm", "SAME"),
                                               ("hard_swish", "offset", 2.0), ("nearest_interp_v2", "align_corners", True),
                                               ("depthwise_conv2d", "dilations", [1, 2])])
def test_unsupported_attribute_values_fail_loudly(optype, attr, value):
    """A descriptor converted from another export (SAME padding, dilated conv, ...) must not compile into a program that
    silently computes different values: the lowering hard-codes these attributes, so it refuses anything else."""
    import copy
    desc, w = net_ref.get_weights("V4_ch_det_fast")
    desc = copy.deepcopy(desc)
    op = next(o for o in desc["ops"] if o["type"] == optype)
    op["attrs"][attr] = value
    with pytest.raises(compiler.UnsupportedGraph, match=attr):
        compiler.compile_model(desc, w, 1, 64, 96)


def _load_fuzz_graph():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("fuzz_graph", os.path.join(os.path.dirname(__file__), "..", "tools", "fuzz_graph.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    return fz


def test_random_graphs_compile_and_match_the_interpreter():
    """A fixed-seed sample of tools/fuzz_graph.py on the CPU emulator: random graphs over the reference models' operator set
    (nested concats, odd channel counts, squeeze-excite gates, upsample + lateral adds, transposed convs ...) either match the
    fp32 interpreter or are refused with UnsupportedGraph — never a bare assert or a wrong result (the tool ran 700 graphs here
    and 600 on the GPU engine)."""
    fz = _load_fuzz_graph()
    rng = np.random.default_rng(5)
    ok = refused = 0
    for _ in range(10):
        h, w = int(rng.integers(2, 6)) * 16, int(rng.integers(2, 7)) * 16
        desc, wts, cout = fz.random_graph(rng, h, w)
        x = rng.uniform(-1, 1, (1, 3, h, w)).astype(np.float16).astype(np.float32)
        ref = net_ref.run_graph(desc, wts, x)[0].numpy()
        try:
            prog = compiler.compile_model(desc, wts, 1, h, w)
        except compiler.UnsupportedGraph:
            refused += 1
            continue
        got = np.transpose(ir_emul.Emulator(prog).run(ir_emul.to_nhwc8(x))[0][..., :cout], (0, 3, 1, 2))
        assert got.shape == ref.shape and np.abs(got - ref).max() < 5e-3 * max(1.0, np.abs(ref).max())
        ok += 1
    assert ok >= 7


def test_segmented_concat_views_are_handled_or_refused_loudly():
    """A concat of parts that are not multiples of 8 channels leaves gaps in the buffer: convolutions read it through their
    channel map, a nested concat of 8-multiples is simply dense, and consumers that address channels linearly refuse."""
    fz = _load_fuzz_graph()
    rng = np.random.default_rng(1)

    def build(c1, c2, tail, nested=True):
        g = fz.G(rng)
        a = g.act(g.bn(g.conv("x", 3, c1, (3, 3), (2, 2), (1, 1)), c1), c1, "relu")
        b = g.act(g.bn(g.conv(a, c1, c2, (3, 3), (1, 1), (1, 1)), c2), c2, "relu")
        cat, c = g.concat([a, b], c1 + c2), c1 + c2
        if nested:
            cat, c = g.concat([cat, a], c + c1), c + c1
        if tail == "conv":
            out = g.act(g.bias(g.conv(cat, c, 8, (1, 1), (1, 1), (0, 0)), 8), 8, "sigmoid")
            return g.finish(out) + (8,)
        out = g.pool(cat, c, "max", 2, 2, 0)
        return g.finish(out) + (c,)
    x = rng.uniform(-1, 1, (1, 3, 32, 48)).astype(np.float16).astype(np.float32)
    for c1, c2, tail, nested in ((16, 24, "conv", True), (16, 24, "pool", True), (12, 20, "conv", False)):
        desc, wts, cout = build(c1, c2, tail, nested)
        ref = net_ref.run_graph(desc, wts, x)[0].numpy()
        prog = compiler.compile_model(desc, wts, 1, 32, 48)
        got = np.transpose(ir_emul.Emulator(prog).run(ir_emul.to_nhwc8(x))[0][..., :cout], (0, 3, 1, 2))
        assert np.abs(got - ref).max() < 5e-3 * max(1.0, np.abs(ref).max()), (c1, c2, tail)
    for tail, nested, what in (("pool", False, "segments"), ("conv", True, "8-channel boundaries")):
        desc, wts, _ = build(12, 20, tail, nested)
        with pytest.raises(compiler.UnsupportedGraph, match=what):
            compiler.compile_model(desc, wts, 1, 32, 48)


def test_se_gate_folds_into_consumers_unless_the_fold_is_refused(monkeypatch):
    """An SE output read only by the next stage's depthwise conv and by 1x1 convs (the detector's stage outputs: stage transition +
    FPN lateral) is never materialised: the depthwise conv applies the gate on load (F_GATE), each 1x1 conv reads per-image
    weights W * gate (OP_WSCALE + F_IMGW, M tiles aligned to images).  Same result within the net tolerance; without the fold
    (Compiler._gate_foldable refusing) the separate multiply comes back."""
    desc, w = net_ref.get_weights("V4_ch_det")
    x = np.random.default_rng(3).uniform(-1, 1, (2, 3, 128, 160)).astype(np.float16).astype(np.float32)
    ref = net_ref.run_graph(desc, w, x)[0].numpy()[:, 0]
    prog = compiler.compile_model(desc, w, 2, 128, 160)
    kinds = [int(o["kind"]) for o in prog.ops]
    assert kinds.count(ir.OP_WSCALE) == 2 and kinds.count(ir.OP_SCALE) == 3
    imgw = [o for o in prog.ops if int(o["kind"]) == ir.OP_CONV and int(o["flags"]) & ir.F_IMGW]
    assert len(imgw) == 2 and all(int(o["p"][ir.P_KH]) == 1 and int(o["in2"]["n"]) == 2 for o in imgw)
    gated = [o for o in prog.ops if int(o["kind"]) == ir.OP_DWCONV and int(o["flags"]) & ir.F_GATE]
    assert len(gated) == 2
    got = ir_emul.Emulator(prog).run(ir_emul.to_nhwc8(x))[0][..., 0]
    assert np.abs(got - ref).max() < 5e-3
    monkeypatch.setattr(compiler.Compiler, "_gate_foldable", lambda *a: False)
    plain = compiler.compile_model(desc, w, 2, 128, 160)
    k2 = [int(o["kind"]) for o in plain.ops]
    assert k2.count(ir.OP_WSCALE) == 0 and k2.count(ir.OP_SCALE) == 5
    assert np.abs(ir_emul.Emulator(plain).run(ir_emul.to_nhwc8(x))[0][..., 0] - ref).max() < 5e-3


RAGGED_CASES = [("V4_ch_rec", 48, (96, 131, 77)), ("V4_en_rec_fast", 48, (97, 64, 160)), ("V3_ch_rec_fast", 48, (80, 123, 99)),
                ("V2_ch_rec", 32, (64, 101, 88))]


@pytest.mark.parametrize("mid,h,widths", RAGGED_CASES)
def test_ragged_plan_gives_every_sample_its_own_width(mid, h, widths):
    """compile_model(ragged=True): samples of different widths share one batch tensor, and each receives what the oracle
    computes for a batch of exactly its width (paddleocr pads a chunk of <= 6 crops of ONE frame to the chunk's widest crop,
    backend/tools/ocr.py:99 + backend/config.py:58; the padded width, not the neighbours, is what a crop's logits depend on)."""
    from parity import check_rec_probs
    desc, w = net_ref.get_weights(mid)
    rng = np.random.default_rng(3)
    wmax = max(widths) + 9                                  # the tensor may be wider than every sample
    x = np.zeros((len(widths), 3, h, wmax), np.float32)
    for n, wn in enumerate(widths):
        x[n, :, :, :wn] = rng.uniform(-1, 1, (3, h, wn))
    x = x.astype(np.float16).astype(np.float32)
    prog = compiler.compile_model(desc, w, len(widths), h, wmax, ragged=True)
    assert prog.wlevels is not None and len(prog.wlevels) >= 3
    tab = prog.width_table(widths)
    out = ir_emul.Emulator(prog).run(ir_emul.to_nhwc8(x), widths=widths)
    probs, idx = out[0][:, 0], out[-1].view(np.int32)[:, 0, :, 0]
    for n, wn in enumerate(widths):
        ref = net_ref.run_graph(desc, w, x[n:n + 1, :, :, :wn])[0].numpy()[0]        # [T_n, classes]
        tn = int(tab[prog.out_level][n])
        assert ref.shape[0] == tn
        check_rec_probs(mid, probs[n, :tn], ref, idx=idx[n, :tn])
    # the same kernel family per layer whatever the batch and its widest sample (a layer sums its products in one order)
    def families(p):       # op kinds and every flag (kernel family, gate folding, weight tiling ...), layer by layer
        return [(int(o["kind"]), int(o["flags"])) for o in p.ops]
    assert families(prog) == families(compiler.compile_model(desc, w, 48, h, 1283, ragged=True)) \
        == families(compiler.compile_model(desc, w, 1, h, 320, ragged=True))


def test_ragged_plan_refuses_detector_graphs():
    desc, w = net_ref.get_weights("V4_ch_det_fast")
    with pytest.raises(compiler.UnsupportedGraph):
        compiler.compile_model(desc, w, 1, 64, 96, ragged=True)


@pytest.mark.parametrize("mid,hilo", [("V3_ch_det_fast", True), ("V4_ch_det_fast", False), ("V4_ch_det", False), ("V2_ch_det", False)])
def test_input_norm_folded_into_the_stem(mid, hilo):
    """compile_model(input_norm=(mean, std)): the plan takes the RAW resized pixels (integers, exact in fp16) + a ones channel
    and computes what the oracle computes on (u/255 - mean)/std in fp32 (paddleocr NormalizeImage, App. C.1) — closer than
    the plan fed the fp16-rounded normalised image."""
    from oracle import pipeline_ref
    from vse_amd import synth
    desc, w = net_ref.get_weights(mid)
    frame = synth.make_frames(1, 96, 160, seed=5)[0]
    x, _ = pipeline_ref.det_preprocess(frame)                 # fp32 normalised, what the reference feeds
    ref = net_ref.run_graph(desc, w, x)[0].numpy()[:, 0]
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    raw = np.zeros((1, 96, 160, 8), np.float32)
    raw[..., :3] = frame[None].astype(np.float32)             # no resize at this size: det_preprocess is the identity on pixels
    raw[..., 3] = 1.0
    chk = (raw[0, ..., :3] / 255.0 - np.asarray(mean, np.float32)) / np.asarray(std, np.float32)
    assert np.abs(chk.transpose(2, 0, 1) - x[0]).max() < 1e-5
    prog = compiler.compile_model(desc, w, 1, 96, 160, hilo=hilo, input_norm=(mean, std))
    got = ir_emul.Emulator(prog).run(raw)[0][..., 0]
    prog0 = compiler.compile_model(desc, w, 1, 96, 160, hilo=hilo)
    got0 = ir_emul.Emulator(prog0).run(ir_emul.to_nhwc8(x))[0][..., 0]
    e, e0 = np.abs(got - ref).max(), np.abs(got0 - ref).max()
    assert e < 5e-3, e
    if hilo:                           # with ~22-bit weights the fp16 rounding of the INPUT is the error that is left: gone
        assert e < 0.5 * e0 + 1e-6, (e, e0)
    # compiling twice from the same descriptor must not see the first compile's rewritten stem
    compiler.compile_model(desc, w, 1, 96, 160, hilo=hilo, input_norm=(mean, std))
    # fuse_preprocess: the same program with the stem marked to resize the uint8 frames itself (the emulator is fed the resized
    # pixels either way; the GPU test compares the two routes bit for bit)
    fused = compiler.compile_model(desc, w, 1, 96, 160, hilo=hilo, input_norm=(mean, std), fuse_preprocess=True)
    marked = [int(o["flags"]) & ir.F_U8SRC for o in fused.ops]
    assert sum(1 for m in marked if m) == 1 and marked[0] and int(fused.ops[0]["flags"]) & ir.F_STEM
    assert np.array_equal(ir_emul.Emulator(fused).run(raw)[0], ir_emul.Emulator(prog).run(raw)[0])
    with pytest.raises(compiler.UnsupportedGraph):
        compiler.compile_model(desc, w, 1, 96, 160, hilo=hilo, fuse_preprocess=True)          # needs input_norm


@pytest.mark.parametrize("mid", ["V3_ch_det_fast", "V4_ch_det_fast"])
def test_mobile_detector_chains_and_gated_laterals(mid):
    """compile_model(hilo=True) for the mobile detectors (the reference's default mode, paddle_model_config.py:53-58):
    runs of 1x1 / depthwise convs become OP_CHAIN records (chains.py), tensors that feed a chain are fp16 hi + lo pairs, and the
    RSE-FPN laterals (1x1 conv + SE block with shortcut + top-down add) become ONE gated conv each (F_OGATE, residual in the
    epilogue).  The emulator decodes the chain blob the kernel reads (descriptor words, MFMA fragments in lane order, depthwise
    records) and must agree with the fp32 interpreter; the byte-exact fp16 mode must stay within the fp16 budget."""
    desc, w = net_ref.get_weights(mid)
    x = np.random.default_rng(3).uniform(-1, 1, (2, 3, 96, 160)).astype(np.float16).astype(np.float32)
    ref = net_ref.run_graph(desc, w, x)[0].numpy()[:, 0]
    prog = compiler.compile_model(desc, w, 2, 96, 160, hilo=True)
    plain = compiler.compile_model(desc, w, 2, 96, 160, hilo=True, chain=False)
    kinds = [int(o["kind"]) for o in prog.ops]
    chains = [o for o in prog.ops if int(o["kind"]) == ir.OP_CHAIN]
    assert len(chains) >= 3 and len(prog.ops) < len(plain.ops)              # (where the path is cut follows the time model: chains.py)
    gated = [o for o in prog.ops if int(o["kind"]) == ir.OP_CONV and int(o["flags"]) & ir.F_OGATE]
    assert len(gated) == 4 and sum(bool(int(o["flags"]) & ir.F_RES) for o in gated) == 3      # four laterals, three top-down adds
    assert ir.OP_SCALE not in [int(o["kind"]) for o in prog.ops if int(o["out"]["c"]) == 96]        # no 96-channel SE multiply is left
    # the neck's 3x3 96 -> 24 convs take their hi and lo weights in ONE pass (64-row stages [hi 32 | lo 32], F_HLSUM) in both programs
    # (at the reference's detector input size: on this test's small maps they fall to the implicit GEMM)
    for pr in (compiler.compile_model(desc, w, 1, 544, 960, hilo=True), compiler.compile_model(desc, w, 1, 544, 960, hilo=True, chain=False)):
        hl = [o for o in pr.ops if int(o["kind"]) == ir.OP_CONV and int(o["flags"]) & ir.F_HLSUM]
        assert len(hl) == 4 and all(int(o["p"][ir.P_KH]) == 3 and int(o["p"][ir.P_COUT]) <= 32 and not int(o["flags"]) & ir.F_HILO for o in hl)
    for o in chains:
        hdr = np.frombuffer(bytes(prog.weights.blob[int(o["w_off"]):int(o["w_off"]) + 4 * ir.CH_HDR]), np.int32)
        assert hdr[ir.CHH_MAGIC] == ir.CH_MAGIC and 2 <= hdr[ir.CHH_NSTAGES] <= 8 and hdr[ir.CHH_LDS_TOTAL] <= 160 * 1024
        final_h = min(int(o[k]["h"]) for k in ("out", "out2", "in2") if int(o[k]["n"]) > 0)       # tiles cover the LAST stage's output
        if int(o["out"]["esize"]) == 4:
            final_h //= 4               # the head tail stores 4 x 4 map pixels per pixel of its last stage (CHS_SHUF)
        assert int(o["p"][ir.P_CH_TILES_H]) * hdr[ir.CHH_TH] >= final_h and int(o["p"][ir.P_CH_LDS]) == hdr[ir.CHH_LDS_TOTAL]
    # the DB head's tail (the last op of both programs) is flagged for the register form chain_pw2_kernel, image size in the record;
    # the layer-by-layer program keeps exactly that one chain record
    for pr in (prog, plain):
        tail = pr.ops[-1]
        hdr = np.frombuffer(bytes(pr.weights.blob[int(tail["w_off"]):int(tail["w_off"]) + 4 * ir.CH_HDR]), np.int32)
        assert int(tail["kind"]) == ir.OP_CHAIN and int(tail["p"][ir.P_CH_PW2]) == 1 and int(tail["p"][ir.P_CH_IMG]) == hdr[ir.CHH_LDSW_BYTES] <= 64 * 1024
    assert [int(o["kind"]) for o in plain.ops].count(ir.OP_CHAIN) == 1
    # depthwise filter tables are fp32 [taps][C] = fp16 hi + fp16 lo summed (round 4): the emulator and the kernels read them as such
    dw = [o for o in plain.ops if int(o["kind"]) == ir.OP_DWCONV]
    assert dw
    for o in dw[:3]:
        taps, cp = int(o["p"][ir.P_KH]) * int(o["p"][ir.P_KW]), int(o["in0"]["c"])
        tab = np.frombuffer(bytes(plain.weights.blob[int(o["w_off"]):int(o["w_off"]) + 4 * taps * cp]), np.float32)
        hi = tab.astype(np.float16).astype(np.float32)
        lo = (tab - hi).astype(np.float16).astype(np.float32)
        assert np.isfinite(tab).all() and np.abs(tab).max() > 0 and np.array_equal(hi + lo, tab)      # exactly a hi + lo pair
    # a tensor that feeds a chain is a pair: its producer stores the lo half, the chain reads it at the same offset
    lo_in = [int(o["p"][ir.P_CH_LO_IN]) for o in chains]
    assert any(lo_in) and all(v % 8 == 0 for v in lo_in)
    err32 = np.abs(ir_emul.Emulator(prog).run(ir_emul.to_nhwc8(x))[0][..., 0] - ref).max()
    err16 = np.abs(ir_emul.Emulator(prog, round_f16=True).run(ir_emul.to_nhwc8(x))[0][..., 0] - ref).max()
    err16_plain = np.abs(ir_emul.Emulator(plain, round_f16=True).run(ir_emul.to_nhwc8(x))[0][..., 0] - ref).max()
    assert err32 < 1e-2 and err16 < 3e-2, (err32, err16, err16_plain)
    print(f"{mid}: {len(plain.ops)} -> {len(prog.ops)} ops, {len(chains)} chains; max |map - fp32 interpreter|: fp32 emulation {err32:.2e}, "
          f"fp16-exact emulation chained {err16:.2e} vs unchained {err16_plain:.2e}")


def _lateral_graph(tail):
    """feed -> 1x1 (3 -> 16) -> relu -> LATERAL 1x1 (16 -> 24, no bias) -> SE block with shortcut (x + x * hsigmoid(fc2(relu(fc1(gap(x))))))
    -> `tail` ops -> fetch: the pattern _rewrite_se_laterals turns into one gated conv (F_OGATE)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("fuzz_graph", os.path.join(os.path.dirname(__file__), "..", "tools", "fuzz_graph.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    g = fz.G(np.random.default_rng(5))
    t = g.act(g.conv("x", 3, 16, (1, 1), (1, 1), (0, 0)), 16, "relu")
    x = g.conv(t, 16, 24, (1, 1), (1, 1), (0, 0))
    gp = g.pool(x, 24, "avg", 1, 1, 0, glob=True)
    h = g.act(g.bias(g.conv(gp, 24, 8, (1, 1), (1, 1), (0, 0)), 8), 8, "relu")
    gate = g.act(g.bias(g.conv(h, 8, 24, (1, 1), (1, 1), (0, 0)), 24), 24, "hard_sigmoid")
    o = g.binary(x, g.binary(x, gate, 24, "elementwise_mul"), 24)
    for kind in tail:
        o = g.bn(o, 24) if kind == "bn" else g.bias(o, 24) if kind == "bias" else g.scale(o, 24) if kind == "scale" else g.act(o, 24, kind)
    return g.finish(o)


@pytest.mark.parametrize("tail", [(), ("bn",), ("hard_swish",), ("relu",), ("scale",)])
def test_gated_lateral_falls_back_when_something_rides_behind_the_se_add(tail):
    """the gated conv evaluates (conv + bias) * (1 + gate) + residual, so a BN / bias / activation that the epilogue
    would absorb BEHIND the SE add cannot ride in it ((conv * s + b) * (1 + g) != (conv * (1 + g)) * s + b).  Such a graph must compile
    WITHOUT the rewrite (it did before the rewrite existed) and compute the graph's values; the plain pattern keeps the gated conv."""
    desc, w = _lateral_graph(tail)
    x = np.random.default_rng(1).uniform(-1, 1, (2, 3, 16, 32)).astype(np.float16).astype(np.float32)
    ref = net_ref.run_graph(desc, w, x)[0].numpy()
    try:
        prog = compiler.compile_model(desc, w, 2, 16, 32)
    except NotImplementedError:
        # a tail the compiler has no lowering for behind an element-wise add (a stand-alone batch_norm): refused loudly with or without
        # the rewrite — what must never happen is a program that folds it into the gated conv
        with pytest.raises(NotImplementedError):
            compiler.Compiler(desc, w, 2, 16, 32, se_lateral=False).compile()
        return
    gated = [o for o in prog.ops if int(o["kind"]) == ir.OP_CONV and int(o["flags"]) & ir.F_OGATE]
    if not tail:
        assert len(gated) == 1
    elif tail[0] in ("hard_swish", "relu"):          # an activation the epilogue would have absorbed behind the gate: no gated conv
        assert len(gated) == 0, (tail, len(gated))    # (a `scale` op is lowered on its own: the gated conv in front of it stays valid)
    got = np.transpose(ir_emul.Emulator(prog).run(ir_emul.to_nhwc8(x))[0][..., :24], (0, 3, 1, 2))
    assert np.abs(got - ref).max() < 5e-3 * max(1.0, np.abs(ref).max()), (tail, np.abs(got - ref).max())


def test_head_tail_fusion_and_its_fallback_without_the_head_form(monkeypatch):
    """F_TAIL2: the server detector's second head deconv (64 -> 1, the base map) rides in the first one's launch and its map is stored
    densely (ld 1) for the F_UP2HEAD conv.  The emulator decodes stage B from the MFMA fragments the kernel reads; with fp16 rounding
    of every stored tensor the fused and the separate programs give the same map.  A graph whose dense map would reach any other
    reader (here: the head conv without the fused 1-channel projection the head kernel needs) compiles with the two launches instead
    (Tail2Unsupported -> retry)."""
    desc, w = net_ref.get_weights("V4_ch_det")
    x = np.random.default_rng(3).uniform(-1, 1, (1, 3, 64, 96)).astype(np.float16).astype(np.float32)
    outs = {}
    for t2 in (None, False):
        prog = compiler.compile_model(desc, w, 1, 64, 96, tail2=t2)
        tails = [o for o in prog.ops if int(o["flags"]) & ir.F_TAIL2]
        assert len(tails) == (1 if t2 is None else 0)
        if tails:
            o = tails[0]
            assert int(o["flags"]) & ir.F_PW and int(o["flags"]) & ir.F_PIXSHUF and int(o["out2"]["ld"]) == 1 and int(o["out2"]["esize"]) == 2
            assert (int(o["out2"]["h"]), int(o["out2"]["w"])) == (64, 96)
            head = [q for q in prog.ops if int(q["flags"]) & ir.F_UP2HEAD]
            assert len(head) == 1 and int(head[0]["in0"]["ld"]) == 1 and int(head[0]["in0"]["off"]) == int(o["out2"]["off"])
        outs[t2] = ir_emul.Emulator(prog, round_f16=True).run(ir_emul.to_nhwc8(x))[0]
    assert np.abs(outs[None] - outs[False]).max() < 2e-6 and outs[None].std() > 0
    monkeypatch.setattr(compiler.Compiler, "_try_fuse_dot1", lambda *a: None)
    store, fb = compiler.WeightStore(), {}
    prog = compiler.compile_model(desc, w, 1, 64, 96, store=store, fallbacks=fb)
    assert not any(int(o["flags"]) & (ir.F_TAIL2 | ir.F_UP2HEAD) for o in prog.ops)
    # the abandoned attempt leaves nothing behind in the shared store, and the outcome is remembered for the next shape
    direct = compiler.WeightStore()
    compiler.compile_model(desc, w, 1, 64, 96, store=direct, tail2=False)
    assert fb == {"tail2": False} and len(store.blob) == len(direct.blob) and set(store.index) == set(direct.index)
    fb2 = {}
    prog2 = compiler.compile_model(desc, w, 1, 96, 128, store=store, tail2=fb["tail2"], fallbacks=fb2)
    assert fb2 == {} and not any(int(o["flags"]) & ir.F_TAIL2 for o in prog2.ops)        # no failed attempt this time
    ref = net_ref.run_graph(desc, w, x)[0].numpy()[:, 0]
    assert np.abs(ir_emul.Emulator(prog).run(ir_emul.to_nhwc8(x))[0][..., 0] - ref).max() < 5e-3
