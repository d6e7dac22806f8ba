"""One-record OP_CHAIN cases (csrc/chain.hip: chain_kernel and chain_pw2_kernel) at the smallest shapes that reach each path of the kernel:
every tile of chains.CHAIN_TILES, every stage pattern, the channel paddings, the epilogues, plain / pair inputs and outputs, the persistent
tile loop and the DB head's tail.  tests/test_gpu_chain_ops.py runs them on the GPU, tests/test_chain_records.py on the emulator; both
through op_harness.run_case.

A case is a Spec: the stages (pw(...) / dw(...)), the input map, the FORCED tile.  build(spec, mode) plans it with chains.chain_plan(...,
tiles=[tile]), packs it with chains.chain_pack, asserts the form it was written for (tile, buffer kinds, blocks per CU at its LDS size,
kernel, P_CH_PW2, tile count, input vectors per region) and returns one run of the record:

  * the EXACT run.  Inputs on {-2 .. 2} / 2 (the lo half of a pair input {-1, 0, 1} / 4 on the odd channels), biases on the same grid,
    1x1 weights sparse in {+-1, +-1/2} with NNZ non-zeros per cout, depthwise weights three taps per channel of the same set, activations
    none / relu.  A 1x1 weight gets +-2^-12 added — so that its lo fragment carries information — only in a column whose input channel is
    COARSE (every value of it an fp16 number, no stage with lo weights in front of it): the kernel runs W_hi x_hi + W_lo x_hi + W_hi x_lo and leaves W_lo x_lo out, which is then
    identically zero.  Three conditions, asserted from the generated tensors by every exact check (exact_conditions): the chain on the
    ABSOLUTE values, in units of the product of the grids, stays below 2^24 at every stage (every partial sum in any order is exact in
    fp32); every channel-minor intermediate is exactly a hi + lo pair; no column with a lo weight meets a lo input.  The results then equal
    float16(ref64), the hi / lo split of ref64, or float32(ref64) BIT FOR BIT.
  * the REAL run.  Seeded normal inputs, weights scaled 1 / sqrt(K), non-zero normal biases, the nonlinear activations, held to
    op_harness.ratio with e32 = |ref_chain in float32 - ref_chain in float64| (a Spec with e_pair adds the hi + lo rounding of the LDS
    intermediates, from ref_chain(pair=True) in float64: 8 (e32 + e_pair)).

Every stored output is a channel slice of a wider buffer pre-filled with NaN: the check asserts that everything outside the slice is still
the pre-fill.  build(..., mutate=) hands a MUTATED stage list / weight / blob to the planner, the packer and the kernel and the unmutated
one to the reference (tests/test_chain_records.py: the checks must fail)."""
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

import op_harness as H
from vse_amd import chains, ir

A = ir
F16_NAN = 0x7E00
MUTATIONS = ("dw_taps", "cout", "res", "pad", "lo_pass", "shuf")
REAL_MUST_FAIL = ("dw_taps", "cout", "res", "shuf")          # (lo_pass in the real run: caught where the output is a pair or the fp32 map)


@dataclass(frozen=True)
class S:
    """One stage of a Spec."""
    kind: str
    cin: int
    cout: int
    k: int = 1
    s: int = 1
    act: int = A.ACT_RELU               # the exact run (none / relu); the real run uses real_act
    real_act: int = A.ACT_HSWISH
    res: int = -1
    act2: int = A.ACT_NONE
    post: bool = False
    store: Optional[str] = None         # None | "plain" | "pair" | "map" (the last stage: "plain" unless said otherwise)
    dview: int = 0                      # the output view has this many channels more (or fewer) than the stage
    nnz: int = 4                        # exact run: non-zero weights per cout
    unit1: bool = False                 # exact run: weights +-1 only (long chains: one bit of growth per stage)
    wlo: bool = True                    # exact run: lo weights where the condition allows them


def pw(cin, cout, **kw):
    return S("pw", cin, cout, **kw)


def dw(c, k=3, s=1, **kw):
    return S("dw", c, c, k=k, s=s, **kw)


@dataclass(frozen=True)
class Spec:
    name: str
    tile: Tuple[int, int]
    n: int
    h: int
    w: int
    stages: Tuple[S, ...]
    in_lo: bool = False
    in_ld_extra: int = 0
    kinds: Optional[str] = None         # the LDS buffer kinds the case was written for, e.g. "010" (0 channel-minor, 1 planar)
    bcu: int = 3                        # blocks per CU at the plan's LDS size (3: < ~51 KiB, 2: < ~78 KiB, 1: above)
    form: str = "generic"               # "generic" | "pw2": the kernel the launcher runs for the record as the compiler would flag it
    tiles: Optional[Tuple[int, int]] = None        # the tile count lies in [lo, hi]
    tiles_cu: int = 0                   # GPU test: more tiles than this many times the device's CUs
    vecs: Optional[str] = None          # "lt256" | "gt512": 16-byte input vectors of a tile's region (the prefetch covers 512)
    e_pair: bool = False                # the real run's bound is 8 (e32 + e_pair)
    res_alt: int = -1                   # mutation "res": the buffer handed to the kernel instead
    batch_of: int = 0                   # batch independence: image 0 of this 1-image spec again as image 2 of a batch of 3
    both_kernels: bool = False          # head tail: P_CH_PW2 = 1 and 0 on the same blob, bit-identical maps


def rup(x, m):
    return (x + m - 1) // m * m


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _same_bits(got, want64, what):
    want = np.asarray(want64).astype(got.dtype)
    ok = _bits(got) == _bits(want)
    assert ok.all(), (what, "not bit-identical at", tuple(int(v) for v in np.argwhere(~ok)[0]), "of", got.shape, "got",
                      float(got[tuple(np.argwhere(~ok)[0])]), "want", float(want[tuple(np.argwhere(~ok)[0])]), int((~ok).sum()), "differ")


def _grid(rng, shape, lo, hi, unit):
    return rng.integers(lo, hi + 1, shape).astype(np.float64) * unit


def _slice(flat, shape_pix, c, ld, off, coff=0):
    npix = int(np.prod(shape_pix))
    return flat[off:off + npix * ld].reshape(tuple(shape_pix) + (ld,))[..., coff:coff + c]


def _buffer(shape_pix, ld, off, dtype, nan=True):
    flat = np.zeros(off + int(np.prod(shape_pix)) * ld + 8, dtype)
    if nan:
        if dtype == np.float16:
            flat.view(np.uint16)[:] = F16_NAN
        else:
            flat[:] = np.nan
    return flat


def _is_f16(v):
    return v.astype(np.float16).astype(np.float64) == v


@dataclass
class Built:
    run: H.Run
    rec: np.ndarray
    check: object                       # check(arenas) -> worst error / bound (exact run: 0.0)
    plan: dict
    stages: list                        # the reference's stages (chain_stage dicts with w_ref)
    x: tuple                            # (hi, lo or None) of the input
    weights: dict                       # name -> the float64 array handed to the packer (unmutated)
    outs: list                          # the stored outputs: tensor, layout, stage
    note: dict


def build(sp: Spec, mode: str, mutate: Optional[str] = None, pw2: Optional[int] = None, like: Optional[Built] = None) -> Built:
    """mode: "exact" | "real".  mutate (MUTATIONS): the kernel's side is mutated, the reference's is not.  pw2: P_CH_PW2 (None: as the
    compiler sets it).  like: the weights and biases are this build's, and image 2 of the batch is its image 0."""
    exact = mode == "exact"
    rng = np.random.default_rng(sum(map(ord, sp.name)) * 7 + (1 if exact else 2))
    n, h, w, ns = sp.n, sp.h, sp.w, len(sp.stages)
    c0 = sp.stages[0].cin
    if mutate not in (None,) + MUTATIONS:
        raise ValueError(mutate)

    # ---- the input
    shape = (n, h, w, c0)
    if exact:
        xhi = _grid(rng, shape, -2, 2, 0.5).astype(np.float16)
        xlo = (rng.integers(-1, 2, shape) / 4.0 * (np.arange(c0) & 1)).astype(np.float16) if sp.in_lo else None
    else:
        v = rng.normal(0, 1, shape)
        xhi = v.astype(np.float16)
        xlo = (v - xhi.astype(np.float64)).astype(np.float16) if sp.in_lo else None
    if like is not None:
        xhi[2] = like.x[0][0]
        if sp.in_lo:
            xlo[2] = like.x[1][0]
    x64 = xhi.astype(np.float64) + (xlo.astype(np.float64) if sp.in_lo else 0.0)
    in_ld = (2 * c0 if sp.in_lo else c0) + sp.in_ld_extra
    xb = _buffer((n, h, w), in_ld, 0, np.float16, nan=False)
    _slice(xb, (n, h, w), c0, in_ld, 0)[...] = xhi
    if sp.in_lo:
        _slice(xb, (n, h, w), c0, in_ld, 0, coff=c0)[...] = xlo
    in0 = H.view(H.ext(0), n, h, w, c0, ld=in_ld)

    # ---- the stages, one after the other: the weights of the exact run depend on which input channels are coarse
    # has_lo[j]: per channel of buffer j, whether any pixel carries a lo half (the input: as given; an intermediate: as the kernel splits it)
    has_lo = [(xlo != 0).reshape(-1, c0).any(0) if sp.in_lo else np.zeros(c0, bool)]
    stages, weights, bufs, absb = [], {}, [x64], [np.abs(x64)]
    units, caps, lo_cols = [0.25 if sp.in_lo else 0.5], [], []
    g = 0
    for j, s in enumerate(sp.stages):
        act = s.act if exact else s.real_act
        act_a, act_b = (0.25, 0.5) if act == A.ACT_HSIGMOID else (0.0, 0.0)
        post_a, post_b = ((0.5, 1.0) if exact else (0.75, -0.125)) if s.post else (1.0, 0.0)
        bias = (_grid(rng, s.cout, -2, 2, 0.5) if exact else rng.normal(0, 0.5, s.cout)).astype(np.float32)
        if like is not None:
            bias = like.stages[j]["ep"]["shift"]
        store = s.store or ("plain" if j == ns - 1 else None)
        name = f"w{j}"
        st = H.chain_stage(s.kind, s.cin, s.cout, s.k, s.s, act, act_a, act_b, post_a, post_b, s.res, s.act2 if s.res >= 0 else A.ACT_NONE,
                           g if store else -1, int(store == "map"), name, bias)
        g += bool(store)
        if s.kind == "pw":
            wm = np.zeros((s.cout, s.cin), np.float64)
            if exact:
                # (lo weights once per chain: behind a stage that had them the grid is 2^-12 finer, and a second factor 2^-12 leaves fp32)
                coarse = ~has_lo[-1] if s.wlo and units[-1] >= 2.0 ** -6 else np.zeros(s.cin, bool)
                for co in range(s.cout):
                    sel = rng.choice(s.cin, size=min(s.nnz, s.cin), replace=False)
                    wm[co, sel] = rng.choice([1.0, -1.0] if s.unit1 else [1.0, -1.0, 0.5, -0.5], size=len(sel))
                    wm[co, sel] += 2.0 ** -12 * rng.choice([1.0, -1.0], size=len(sel)) * coarse[sel]
            else:
                wm = rng.normal(0, 1, (s.cout, s.cin)) / np.sqrt(s.cin)
            if like is not None:
                wm = like.weights[name].reshape(s.cout, s.cin)
            st["w_ref"] = H.pair64(wm)              # what the kernel sees: f16(w) + f16(w - f16(w))
            lo_cols.append((st["w_ref"] != wm.astype(np.float16).astype(np.float64)).any(0))
            wu = 2.0 ** -12 if lo_cols[-1].any() else (1.0 if s.unit1 else 0.5)
            weights[name] = wm.reshape(s.cout, s.cin, 1, 1)
        else:
            k2 = s.k * s.k
            if exact:
                wd = np.zeros((s.cin, k2), np.float64)
                for c in range(s.cin):
                    sel = rng.choice(k2, size=3, replace=False)
                    wd[c, sel] = rng.choice([1.0, -1.0] if s.unit1 else [1.0, -1.0, 0.5, -0.5], size=3)
            else:
                wd = rng.normal(0, 1, (s.cin, k2)) / s.k
            if like is not None:
                wd = like.weights[name].reshape(s.cin, k2)
            wd = wd.astype(np.float32)
            wu = 1.0 if s.unit1 else 0.5
            st["w_ref"] = np.ascontiguousarray(wd.T)
            lo_cols.append(None)
            weights[name] = wd.reshape(s.cin, 1, s.k, s.k)
        stages.append(st)
        bufs.append(H.ref_chain_stage(bufs, st, np.float64))
        has_lo.append((~_is_f16(bufs[-1])).reshape(-1, s.cout).any(0))
        if exact:
            sa = dict(st, w_ref=np.abs(st["w_ref"]), ep=dict(st["ep"], act=A.ACT_NONE, act2=A.ACT_NONE, shift=np.abs(bias), post_a=abs(post_a),
                                                            post_b=abs(post_b)))
            absb.append(H.ref_chain_stage(absb, sa, np.float64))
            units.append(units[-1] * wu * (0.5 if s.post else 1.0))
            caps.append(float(absb[-1].max()) / units[-1])

    def exact_conditions():
        """-> the largest partial sum in grid units (< 2^24), over the stages."""
        for j, s in enumerate(sp.stages):
            assert caps[j] < 2.0 ** 24, (sp.name, "stage", j, "sum |x w| in grid units", caps[j])
            if j + 1 < ns and sp.stages[j + 1].kind == "pw":
                assert (H.pair64(bufs[j + 1]) == bufs[j + 1]).all(), (sp.name, "output of stage", j, "is no exact hi + lo pair")
            if s.kind == "pw":
                assert not (has_lo[j] & lo_cols[j]).any(), (sp.name, "stage", j, "a lo weight meets a lo input: the kernel leaves that product out")
        return max(caps)

    # ---- what the kernel is handed
    k_stages = [dict(st) for st in stages]
    k_weights = dict(weights)
    if mutate == "dw_taps":
        j = next((j for j, s in enumerate(sp.stages) if s.kind == "dw"), None)
        if j is None:
            raise ValueError("dw_taps: no depthwise stage")
        k_weights[f"w{j}"] = np.ascontiguousarray(weights[f"w{j}"].transpose(0, 1, 3, 2))
    elif mutate == "cout":
        j = next((j for j, s in enumerate(sp.stages) if s.kind == "pw" and s.cout > 32), None)
        if j is None:
            raise ValueError("cout: no rows on both sides of a 32-boundary")
        k_weights[f"w{j}"] = weights[f"w{j}"].copy()
        k_weights[f"w{j}"][[31, 32]] = weights[f"w{j}"][[32, 31]]
    elif mutate == "res":
        j = next((j for j, s in enumerate(sp.stages) if s.res >= 0), None)
        if j is None or sp.res_alt < 0:
            raise ValueError("res: no residual, or no other buffer it could come from")
        k_stages[j]["res_buf"] = k_stages[j]["res_abs"] = sp.res_alt
    elif mutate == "shuf":
        if sp.stages[-1].store != "map":
            raise ValueError("shuf: no shuffle stage")
        j = ns - 1
        k_weights[f"w{j}"] = weights[f"w{j}"].copy()
        k_weights[f"w{j}"][[1, 2]] = weights[f"w{j}"][[2, 1]]
        sh = stages[j]["ep"]["shift"].copy()
        sh[[1, 2]] = sh[[2, 1]]
        k_stages[j]["ep"] = dict(stages[j]["ep"], shift=sh)
    plan = chains.chain_plan(k_stages, h, w, sp.in_lo, tiles=[sp.tile])
    assert plan is not None, (sp.name, "no plan at tile", sp.tile)
    cblob, img_bytes, _meta, _macs = chains.chain_pack(k_stages, plan, k_weights)
    words = cblob[:4 * (ir.CH_HDR + (ns + 1) * ir.CH_BUF + ns * ir.CH_STAGE)].view(np.int32)
    img_off = int(words[ir.CHH_LDSIMG_OFF])
    if mutate == "pad":
        j = next((j for j, s in enumerate(sp.stages) if s.kind == "dw" and s.s == 2), None)
        if j is None:
            raise ValueError("pad: no stride-2 stage")
        words[ir.CH_HDR + (ns + 1) * ir.CH_BUF + j * ir.CH_STAGE + ir.CHS_PAD] = 0
    elif mutate == "lo_pass":
        j = next((j for j, s in enumerate(sp.stages) if s.kind == "pw" and (not exact or lo_cols[j].any())), None)
        if j is None:
            raise ValueError("lo_pass: no 1x1 stage with lo weights")
        half = k_stages[j]["nct"] * k_stages[j]["nks"] * 1024
        cblob[img_off + k_stages[j]["w_lds"] + half:img_off + k_stages[j]["w_lds"] + 2 * half] = 0

    # ---- the form the case was written for
    oh, ow = plan["dims"][-1]
    tiles_h, tiles_w = -(-oh // plan["th"]), -(-ow // plan["tw"])
    ntiles = n * tiles_h * tiles_w
    b0 = plan["bufs"][0]
    vecs = b0["P"] * ((b0["Cp"] if b0["kind"] == 0 else b0["C"]) // 8)
    kinds = "".join(str(b["kind"]) for b in plan["bufs"])
    last = sp.stages[-1]
    shuf = last.store == "map"
    flag = int(bool(shuf and ns == 2 and all(s.kind == "pw" for s in sp.stages) and c0 <= 64 and last.cout <= 32))
    if mutate is None:
        assert (plan["th"], plan["tw"]) == sp.tile, (sp.name, plan["th"], plan["tw"])
        assert kinds == (sp.kinds or "".join("0" if s.kind == "pw" else "1" for s in sp.stages)), (sp.name, kinds)
        assert sp.tiles is None or sp.tiles[0] <= ntiles <= sp.tiles[1], (sp.name, ntiles, sp.tiles)
        assert sp.vecs is None or (vecs < 256 if sp.vecs == "lt256" else vecs > 512 and vecs % 256), (sp.name, vecs, sp.vecs)

    # ---- the outputs
    tensors, views, lo_out, outs = [xb], [None, None, None], [0, 0, 0], []
    for j, st in enumerate(stages):
        s, gi = sp.stages[j], st["gout"]
        if gi < 0:
            continue
        oh_, ow_ = plan["dims"][j + 1]
        if st["shuf"]:
            ob = _buffer((n, 4 * oh_, 4 * ow_), 1, 0, np.float32)
            views[gi] = H.view(H.ext(1 + gi), n, 4 * oh_, 4 * ow_, 1, ld=1, esize=4)
            outs.append(dict(j=j, g=gi, map=True, shape=(n, 4 * oh_, 4 * ow_), ld=1, off=0, c=1, cw=1, pair=False))
        else:
            pair = (s.store or "plain") == "pair"
            assert not (pair and s.dview)
            cv = s.cout + s.dview
            ld, off = (2 * s.cout if pair else max(cv, s.cout)) + 8, 8
            ob = _buffer((n, oh_, ow_), ld, off, np.float16)
            views[gi] = H.view(H.ext(1 + gi), n, oh_, ow_, cv, ld=ld, off=off * 2)
            lo_out[gi] = s.cout if pair else 0
            outs.append(dict(j=j, g=gi, map=False, shape=(n, oh_, ow_), ld=ld, off=off, c=s.cout, cw=min(cv, s.cout), pair=pair))
        tensors.append(ob)
    while len(tensors) < 4:
        tensors.append(np.zeros(8, np.float16))
    blob = H.Blob()
    blob.add(np.zeros(64, np.uint8))                   # (the chain's blob does not start the weight arena)
    w_off = blob.add(cblob)
    rec = H.chain_op(in0, views[0], (tiles_h, tiles_w), plan["lds_total"], ns, img_bytes, w_off, out2=views[1], out3=views[2],
                     pw2=flag if pw2 is None else pw2, lo_in=c0 if sp.in_lo else 0, lo_out=lo_out)
    if mutate is None:
        form = H.chain_form(rec)
        assert form[0] == (sp.form if pw2 is None or pw2 == flag else "generic"), (sp.name, form, sp.form)
        assert H.chain_form(H.chain_op(in0, views[0], (tiles_h, tiles_w), plan["lds_total"], ns, img_bytes, w_off))[1] == sp.bcu, \
            (sp.name, "lds_total", plan["lds_total"], "blocks per CU", sp.bcu)
    run = H.Run(rec, blob.array(), tensors)
    note = dict(ntiles=ntiles, vecs=vecs, lds=plan["lds_total"], kinds=kinds, last=last.kind,
                pattern="".join("p" if s.kind == "pw" else "d" for s in sp.stages))

    # ---- the reference
    memo = {}

    def references():
        if not memo:
            if exact:
                memo["r"] = bufs, None, None
            else:
                r32 = H.ref_chain(x64.astype(np.float32), stages, np.float32)
                e32 = [float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(r32, bufs)]
                rp = H.ref_chain(x64, stages, np.float64, pair=True)
                memo["r"] = bufs, e32, [float(np.abs(a - b).max()) for a, b in zip(rp, bufs)]
        return memo["r"]

    def check(arenas):
        r64, e32, epair = references()
        worst = 0.0
        if exact:
            exact_conditions()
        for o in outs:
            flat = arenas[1 + o["g"]].reshape(-1)
            y64 = r64[o["j"] + 1]
            what = (sp.name, mode, "output", o["g"], "of stage", o["j"])
            keep = np.ones(flat.shape, bool)
            _slice(keep, o["shape"], o["cw"], o["ld"], o["off"])[...] = False
            got = _slice(flat, o["shape"], o["cw"], o["ld"], o["off"])
            e = None if exact else e32[o["j"] + 1] + (epair[o["j"] + 1] if sp.e_pair else 0.0)
            if o["map"]:
                y64 = H.ref_shuffle(y64)
                if exact:
                    _same_bits(got, y64, what)
                else:
                    worst = max(worst, H.ratio(got, y64, e, what))
            elif o["pair"]:
                lo = _slice(flat, o["shape"], o["cw"], o["ld"], o["off"], coff=o["c"])
                _slice(keep, o["shape"], o["cw"], o["ld"], o["off"], coff=o["c"])[...] = False
                if exact:
                    _same_bits(got, y64, what + ("hi half",))
                    _same_bits(lo, y64 - y64.astype(np.float16).astype(np.float64), what + ("lo half",))
                else:
                    worst = max(worst, H.ratio(got.astype(np.float64) + lo.astype(np.float64), y64, e, what + ("hi + lo",), pair=True))
            else:
                y64 = y64[..., :o["cw"]]
                if exact:
                    _same_bits(got, y64, what)
                else:
                    worst = max(worst, H.ratio(got, y64, e, what))
            pre = F16_NAN if flat.dtype == np.float16 else 0x7FC00000
            assert (_bits(flat)[keep] == pre).all(), what + ("bytes outside the output view were written",)
        if not exact:
            note["e32"], note["e_pair"] = max(e32[o["j"] + 1] for o in outs), max(epair[o["j"] + 1] for o in outs)
        return worst

    return Built(run, rec, check, plan, stages, (xhi, xlo), weights, outs, note)


def _equal_outputs(a, b, what):
    for k, (ta, tb) in enumerate(zip(a[1:], b[1:])):
        assert np.array_equal(_bits(ta), _bits(tb)), what + (f"tensor {k + 1}: not the same bits",)


def _equal_image(one, three, a, b, what):
    """Image 0 of the 1-image run and image 2 of the batch: every byte of the output buffers' pixels."""
    for o1, o3 in zip(one.outs, three.outs):
        npix = int(np.prod(o1["shape"])) * o1["ld"]
        ta = a[1 + o1["g"]].reshape(-1)[o1["off"]:o1["off"] + npix]
        tb = b[1 + o3["g"]].reshape(-1)[o3["off"] + 2 * npix:o3["off"] + 3 * npix]
        assert np.array_equal(_bits(ta), _bits(tb)), what + (f"output {o1['g']}: image 2 of the batch differs from the image alone",)


def case(sp: Spec, mutate=None, modes=("exact", "real")):
    """The op_harness.Case of a spec: the exact and the real run, each of them
      * twice for a head tail (both_kernels): P_CH_PW2 = 1 and 0 on the same blob, whose maps must be the same bits;
      * twice for batch independence (batch_of): the 1-image spec, and its image again as image 2 of 3."""
    built, pairs = [], []
    for m in modes:
        if sp.both_kernels:
            built += [build(sp, m, mutate, pw2=1), build(sp, m, mutate, pw2=0)]
            pairs.append((len(built) - 2, len(built) - 1))
        elif sp.batch_of:
            one = build(sp, m, mutate)
            three = build(Spec(**dict(sp.__dict__, n=sp.batch_of, batch_of=0)), m, mutate, like=one)
            built += [one, three]
            pairs.append((len(built) - 2, len(built) - 1))
        else:
            built.append(build(sp, m, mutate))

    def check(outs):
        worst = max(b.check(o) for b, o in zip(built, outs))
        for i, j in pairs:
            if sp.batch_of:
                _equal_image(built[i], built[j], outs[i], outs[j], (sp.name, "runs", i, j))
            else:
                _equal_outputs(outs[i], outs[j], (sp.name, "runs", i, j))
        return worst
    return H.Case(sp.name, [b.run for b in built], check, note=built[-1].note)


# ---------------------------------------------------------------------------------------------------------------- the groups
LEAN = dict(unit1=True, nnz=2)           # exact run of a long chain: +-1 weights, two per cout: one bit of growth per stage


def _unit(cin, mid, cout, k=3, s=1, res=-1, lean=False, **kw):
    """pw -> dw -> pw: the inverted-residual unit."""
    e = LEAN if lean else {}
    return (pw(cin, mid, real_act=A.ACT_HSWISH, **e), dw(mid, k, s, real_act=A.ACT_HSWISH, unit1=lean),
            pw(mid, cout, act=A.ACT_NONE, real_act=A.ACT_NONE, res=res, **e, **kw))


def group_tiles():
    out = []
    for th, tw in chains.CHAIN_TILES:
        # a tail in both directions; (8, 32) and (16, 16) have regions of more than 512 input vectors, (2, 8) of fewer than 256
        out.append(Spec(f"tile {th}x{tw} pw-dw3-pw tails", (th, tw), 1, th + 1, 2 * tw + 3, _unit(16, 32, 16), kinds="010",
                        bcu={(8, 32): 1, (16, 16): 1, (8, 16): 2, (4, 32): 2}.get((th, tw), 3),
                        vecs={(8, 32): "gt512", (16, 16): "gt512"}.get((th, tw))))
    out.append(Spec("tile 16x16 image 7x9 smaller than the tile", (16, 16), 2, 7, 9, _unit(16, 32, 16), kinds="010", bcu=1, tiles=(2, 2)))
    out.append(Spec("tile 8x32 image 5x7 smaller than the tile", (8, 32), 1, 5, 7, _unit(8, 16, 8), kinds="010", bcu=2, tiles=(1, 1)))
    # the product's squeeze-and-excite chains: 1 x 1 pixels, a (4, 16) tile almost entirely outside the image
    out.append(Spec("tile 4x16 image 1x1 squeeze-excite", (4, 16), 3, 1, 1, (pw(32, 8, real_act=A.ACT_RELU), pw(8, 32, act=A.ACT_NONE, real_act=A.ACT_HSIGMOID)),
                    kinds="00", tiles=(3, 3)))
    out.append(Spec("tile 2x8 image 1x1 pair in", (2, 8), 1, 1, 1, (pw(16, 8, real_act=A.ACT_RELU), pw(8, 16, act=A.ACT_NONE, real_act=A.ACT_HSIGMOID)),
                    in_lo=True, kinds="00", vecs="lt256"))
    return out


def group_patterns():
    R, N = A.ACT_RELU, A.ACT_NONE
    six = _unit(16, 48, 16, lean=True) + (pw(16, 48, **LEAN), dw(48, unit1=True), pw(48, 16, act=N, real_act=N, res=3, **LEAN))
    eight = (pw(16, 24, **LEAN), dw(24, unit1=True), pw(24, 16, **LEAN), pw(16, 24, **LEAN), dw(24, real_act=R, unit1=True),
             pw(24, 16, real_act=A.ACT_SWISH, **LEAN), pw(16, 32, **LEAN), pw(32, 16, act=N, real_act=N, res=6, act2=R, **LEAN))
    return [
        Spec("pw-pw", (4, 16), 1, 5, 19, (pw(16, 32), pw(32, 16, real_act=A.ACT_SIGMOID)), kinds="00"),
        Spec("pw-pw first output stored", (4, 8), 1, 5, 19, (pw(16, 32, store="plain"), pw(32, 16, real_act=A.ACT_SWISH)), kinds="00"),
        Spec("dw-pw planar input", (4, 16), 1, 6, 21, (dw(16), pw(16, 24)), kinds="10"),
        Spec("dw-pw planar input pair", (4, 16), 1, 6, 21, (dw(16, 5), pw(16, 24)), in_lo=True, kinds="10"),
        Spec("pw-dw depthwise last", (4, 8), 1, 6, 13, (pw(16, 24), dw(24)), kinds="01"),
        Spec("pw-dw5 s2 depthwise last odd map", (4, 8), 1, 11, 19, (pw(16, 24), dw(24, 5, 2)), kinds="01"),
        Spec("pw-dw-pw residual from the input", (4, 8), 1, 6, 13, _unit(16, 40, 16, res=0, act2=R), kinds="010", res_alt=-1),
        Spec("pw-pw residual same halo", (4, 16), 1, 5, 19, (pw(16, 24), pw(24, 16, act=N, real_act=N, res=0)), kinds="00"),
        Spec("pw-pw-pw residual of two candidates", (4, 8), 1, 5, 11, (pw(16, 16), pw(16, 16), pw(16, 16, act=N, real_act=N, res=1)), kinds="000", res_alt=2),
        Spec("six stages residual from buffer 3", (2, 8), 1, 5, 13, six, kinds="010010", bcu=2, res_alt=0),
        Spec("eight stages", (2, 8), 1, 3, 11, eight, kinds="01001000", res_alt=3),
        Spec("pw-dw5 s1-pw", (4, 8), 1, 6, 13, _unit(16, 24, 16, k=5), kinds="010"),
        Spec("pw-dw3 s2-pw even map", (4, 8), 1, 12, 20, _unit(16, 24, 16, s=2), kinds="010"),
        Spec("pw-dw3 s2-pw odd map", (4, 8), 1, 11, 19, _unit(16, 24, 16, s=2), kinds="010"),
        Spec("pw-dw5 s2-pw even map", (2, 8), 1, 8, 20, _unit(16, 24, 16, k=5, s=2), kinds="010"),
        Spec("pw-dw5 s2-pw odd map", (4, 8), 1, 9, 17, _unit(16, 24, 16, k=5, s=2), kinds="010"),
    ]


def group_channels():
    N = A.ACT_NONE
    return [
        Spec("cin 8 of 16", (4, 8), 1, 5, 11, (pw(8, 16), pw(16, 8)), kinds="00"),
        Spec("cin 24 of 32 pw-dw-pw", (4, 8), 1, 5, 11, _unit(24, 40, 24), kinds="010"),
        Spec("dw 24 into a 32-deep buffer", (4, 8), 1, 5, 11, (pw(16, 24), dw(24), pw(24, 16)), kinds="010"),
        Spec("pw 40 into a 48-deep buffer", (4, 8), 1, 5, 11, (pw(16, 40), pw(40, 56), pw(56, 48, act=N, real_act=N)), kinds="000"),
        Spec("couts 72 and 40 two K slices", (4, 8), 1, 5, 11, (pw(40, 72), pw(72, 40)), kinds="00", bcu=2),
        Spec("8 channels throughout", (2, 8), 1, 3, 11, _unit(8, 8, 8), kinds="010", vecs="lt256"),
        Spec("dw 8 first", (2, 8), 1, 3, 11, (dw(8), pw(8, 8)), kinds="10", vecs="lt256"),
    ]


def group_epilogues():
    out = []
    for name, a in (("relu", A.ACT_RELU), ("hswish", A.ACT_HSWISH), ("swish", A.ACT_SWISH), ("sigmoid", A.ACT_SIGMOID),
                    ("hsigmoid", A.ACT_HSIGMOID), ("none", A.ACT_NONE)):
        out.append(Spec(f"act {name} on both stage types", (4, 8), 1, 5, 11, (pw(16, 24, real_act=a), dw(24, real_act=a), pw(24, 16, real_act=a)), kinds="010"))
    out.append(Spec("post affine on both stage types", (4, 8), 1, 5, 11, (pw(16, 24, post=True), dw(24, post=True), pw(24, 16, post=True)), kinds="010"))
    out.append(Spec("relu after the residual", (4, 8), 1, 5, 11, (pw(16, 24), pw(24, 16, act=A.ACT_NONE, real_act=A.ACT_NONE, res=0, act2=A.ACT_RELU)),
                    kinds="00"))
    # a 1x1 stage with a non-zero bias and NO activation in front of a 5x5 depthwise stage: without S_MASK the halo pixels outside the image
    # would carry the bias instead of the zero padding, and every border pixel of the output would change
    out.append(Spec("bias in front of a depthwise stage", (4, 8), 1, 4, 8, (pw(16, 24, act=A.ACT_NONE, real_act=A.ACT_NONE), dw(24, 5), pw(24, 16)),
                    kinds="010"))
    return out


def group_io():
    u = _unit(16, 24, 16)
    st = lambda a, b, c: (pw(16, 24, store=a), dw(24, store=b), pw(24, 16, store=c))          # noqa: E731
    return [
        Spec("pair input", (4, 8), 1, 5, 11, u, in_lo=True, kinds="010"),
        Spec("batch of 3", (4, 8), 3, 5, 11, u, kinds="010"),
        Spec("input a slice of a wider tensor", (4, 8), 2, 5, 11, u, in_ld_extra=24, kinds="010"),
        Spec("pair input in a wider tensor", (4, 8), 2, 5, 11, (pw(16, 24), pw(24, 16)), in_lo=True, in_ld_extra=8, kinds="00"),
        Spec("one pair output", (4, 8), 1, 5, 11, st(None, None, "pair"), kinds="010"),
        Spec("two outputs plain pair", (4, 8), 1, 5, 11, st("plain", None, "pair"), kinds="010"),
        Spec("two outputs pair plain depthwise stored", (4, 8), 1, 5, 11, st(None, "pair", "plain"), kinds="010"),
        Spec("three outputs plain", (4, 8), 2, 5, 11, st("plain", "plain", "plain"), kinds="010"),
        Spec("three outputs pairs", (4, 8), 1, 5, 11, st("pair", "pair", "pair"), kinds="010"),
        Spec("output view wider than cout", (4, 8), 1, 5, 11, (pw(16, 24, store="plain", dview=8), dw(24), pw(24, 16, dview=8)), kinds="010"),
        Spec("output view narrower than cout", (4, 8), 1, 5, 11, (pw(16, 24), dw(24, dview=-8)), kinds="01"),
    ]


def group_persistent():
    u8 = _unit(8, 8, 8)
    return [
        Spec("9 tiles on 8 blocks", (2, 8), 1, 6, 24, _unit(16, 24, 16), kinds="010", tiles=(9, 9)),
        Spec("15 tiles on 8 blocks batch 3", (2, 8), 3, 2, 40, _unit(16, 24, 16), kinds="010", tiles=(15, 15)),
        Spec("13 tiles pair input", (4, 8), 1, 52, 8, (pw(16, 16), pw(16, 16)), in_lo=True, kinds="00", tiles=(13, 13)),
        # more tiles than three blocks on each of 256 CUs hold: every block walks its tile loop
        Spec("832 tiles of 2x8", (2, 8), 2, 64, 104, u8, kinds="010", tiles=(832, 832), tiles_cu=3, vecs="lt256"),
        # one block per CU (LDS above 79 KiB) and more tiles than CUs
        Spec("one block per CU 272 tiles", (2, 8), 1, 32, 136, (pw(64, 256, nnz=2), pw(256, 64, nnz=2)), kinds="00", bcu=1, tiles=(272, 272),
             tiles_cu=1),
    ]


def _tail(c0, mid, **kw):
    return (pw(c0, mid, real_act=A.ACT_RELU), pw(mid, 16, act=A.ACT_NONE, real_act=A.ACT_SIGMOID, store="map", **kw))


def group_tail():
    """pw(c0 -> 4 c1p) -> pw(-> 16) with the pixel-shuffle store; 3 x 5 x 7 = 105 and 2 x 9 x 31 = 558 pixels: no multiple of 32 or 256."""
    out = []
    for c0, mid in ((8, 32), (24, 32), (64, 96)):
        for lo in (False, True):
            out.append(Spec(f"tail {c0}-{mid}-16{' pair in' if lo else ''}", (4, 16), 3, 5, 7, _tail(c0, mid), in_lo=lo, kinds="00", form="pw2",
                            bcu={(64, False): 2, (64, True): 1}.get((c0, lo), 3), both_kernels=True))
    out.append(Spec("tail 24-32-16 558 pixels", (4, 16), 2, 9, 31, _tail(24, 32), kinds="00", form="pw2", both_kernels=True))
    # the launcher keeps these on the generic kernel whatever the flag says
    out.append(Spec("tail 72 channels stays generic", (4, 16), 1, 5, 7, _tail(72, 32), kinds="00", both_kernels=True))
    out.append(Spec("tail image above 64 KiB stays generic", (2, 8), 1, 5, 7, _tail(64, 256), kinds="00", bcu=1, both_kernels=True))
    return out


def group_batch():
    return [
        Spec("batch independence pw-dw-pw", (4, 8), 1, 5, 11, _unit(16, 24, 16), kinds="010", batch_of=3),
        Spec("batch independence pair in two outputs", (2, 8), 1, 5, 11, (pw(16, 24, store="pair"), pw(24, 16)), in_lo=True, kinds="00", batch_of=3),
        Spec("batch independence tail", (4, 16), 1, 5, 7, _tail(24, 32), kinds="00", form="pw2", batch_of=3),
    ]


def group_product():
    """The stage patterns of the fast detectors' chains at the tiles their programs choose (tests/test_chain_records.py lists the pairs),
    with the product's outputs and residuals, on small maps."""
    N, R = A.ACT_NONE, A.ACT_RELU

    def pdpp(k):
        return (pw(16, 40), dw(40, k), pw(40, 16, act=N, real_act=N, res=0, store="plain"), pw(16, 40, store="pair"))
    se = (pw(24, 96, real_act=R), pw(96, 24, real_act=R), pw(24, 96, act=N, real_act=A.ACT_HSIGMOID))
    return [
        Spec("dw3 s2-pw at 4x8", (4, 8), 1, 9, 17, (dw(24, 3, 2), pw(24, 16, act=N, real_act=N)), in_lo=True, kinds="10"),
        Spec("dw5 s2-pw at 8x16", (8, 16), 1, 17, 35, (dw(16, 5, 2), pw(16, 24, act=N, real_act=N)), in_lo=True, kinds="10", bcu=2, vecs="gt512"),
        Spec("pw-dw-pw-pw at 2x8", (2, 8), 1, 3, 11, pdpp(3), in_lo=True, kinds="0100"),
        Spec("pw-dw-pw-pw at 4x8", (4, 8), 2, 5, 11, pdpp(3), in_lo=True, kinds="0100"),
        Spec("pw-dw5-pw-pw at 4x16", (4, 16), 1, 5, 19, pdpp(5), in_lo=True, kinds="0100", bcu=2),
        Spec("pw-pw two outputs at 8x16", (8, 16), 1, 9, 19, (pw(40, 24, act=N, real_act=N, store="plain"), pw(24, 64, store="pair")), in_lo=True,
             kinds="00", bcu=2),
        Spec("squeeze-excite of three at 4x16", (4, 16), 2, 1, 1, se, kinds="000", bcu=2),
        Spec("squeeze-excite of three at 4x32", (4, 32), 2, 1, 1, se, kinds="000", bcu=1),
    ]


GROUPS = {"product": group_product, "tiles": group_tiles, "patterns": group_patterns, "channels": group_channels, "epilogues": group_epilogues, "io": group_io,
          "persistent": group_persistent, "tail": group_tail, "batch": group_batch}


# ---------------------------------------------------------------------------------------------------------------- refused records
# Each is a valid record but for one property.  All are refused by HOST code before any kernel starts: vse_plan_create (csrc/vse_runtime.hip:
# the descriptor inside the blob, 4-byte aligned, magic, stages, buffers and LDS bytes equal to the record's, the LDS image inside the blob) and
# the top of launch_chain (at most CH_MAX_STAGES = 8 stages; more than 158 KiB of LDS: VSE_E_UNSUPPORTED).
def refused_cases():
    sp = Spec("refused base", (4, 8), 1, 5, 11, (pw(16, 16), pw(16, 16)), kinds="00")
    nw = ir.CH_HDR + 3 * ir.CH_BUF + 2 * ir.CH_STAGE

    def make(name, rc, fn):
        b = build(sp, "exact")
        rec, blob = b.rec.copy(), b.run.blob.copy()
        off = int(rec["w_off"][0])
        rec, blob = fn(rec, blob, off, blob[off:off + 4 * nw].view(np.int32))
        return name, rc, H.Case(name, [H.Run(rec, blob, b.run.tensors)], refused=True, note={"want_rc": rc})

    def setp(slot, delta):
        def fn(rec, blob, off, words):
            rec["p"][0, slot] += delta
            return rec, blob
        return fn

    def magic(rec, blob, off, words):
        words[ir.CHH_MAGIC] ^= 1
        return rec, blob

    def desc_past_end(rec, blob, off, words):
        rec["w_off"] = blob.nbytes - 64
        return rec, blob

    def image_past_end(rec, blob, off, words):
        return rec, blob[:blob.nbytes - 256].copy()

    def misaligned(rec, blob, off, words):
        rec["w_off"] = off + 2
        return rec, np.concatenate([blob[:off], np.zeros(2, np.uint8), blob[off:]])

    def nine_stages(rec, blob, off, words):
        hdr, bw, sw = words[:ir.CH_HDR].copy(), words[ir.CH_HDR:ir.CH_HDR + 3 * ir.CH_BUF], words[ir.CH_HDR + 3 * ir.CH_BUF:]
        img = blob[off + int(hdr[ir.CHH_LDSIMG_OFF]):]
        hdr[ir.CHH_NSTAGES], hdr[ir.CHH_NBUFS] = 9, 10
        w2 = np.concatenate([hdr, bw, np.zeros(7 * ir.CH_BUF, np.int32), sw, np.zeros(7 * ir.CH_STAGE, np.int32)])
        w2[ir.CHH_LDSIMG_OFF] = rup(w2.nbytes, 16)
        rec["p"][0, ir.P_CH_NSTAGES], rec["p"][0, ir.P_CH_NBUFS] = 9, 10
        return rec, np.concatenate([blob[:off], w2.view(np.uint8), np.zeros(rup(w2.nbytes, 16) - w2.nbytes, np.uint8), img])

    def too_much_lds(rec, blob, off, words):
        words[ir.CHH_LDS_TOTAL] = rec["p"][0, ir.P_CH_LDS] = 159 * 1024
        return rec, blob
    return [make("wrong magic", H.VSE_E_INVAL, magic),
            make("stages differ from the header", H.VSE_E_INVAL, setp(ir.P_CH_NSTAGES, 1)),
            make("buffers differ from the header", H.VSE_E_INVAL, setp(ir.P_CH_NBUFS, 1)),
            make("LDS bytes differ from the header", H.VSE_E_INVAL, setp(ir.P_CH_LDS, 16)),
            make("descriptor past the end of the blob", H.VSE_E_INVAL, desc_past_end),
            make("LDS image past the end of the blob", H.VSE_E_INVAL, image_past_end),
            make("w_off not a multiple of 4", H.VSE_E_INVAL, misaligned),
            make("nine stages with a matching header", H.VSE_E_INVAL, nine_stages),
            make("LDS above 158 KiB", H.VSE_E_UNSUPPORTED, too_much_lds)]


REFUSED = {"chain": refused_cases}
