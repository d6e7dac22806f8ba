"""CPU half of the one-record chain tests (tests/chain_cases.py; the GPU half is tests/test_gpu_chain_ops.py):

  1. every case on the emulator (oracle/ir_emul.py, round_f16=True: it models the hi + lo rounding of the LDS intermediates) under the same
     two checks as on the GPU: the exact run bit for bit — which proves that the dyadic inputs meet their three conditions — and the real run
     under op_harness.ratio (no case needs the e_pair term: the largest e_pair over all cases is 3.8e-7, its e32 8.3e-7, and the worst
     error / bound stays at the 0.5 of one fp16 rounding);
  2. the hand-built records speak the compiler's format: every OP_CHAIN record of the fast detectors at five input sizes is rebuilt from
     its decoded stage list and weights through chain_stage / chain_plan (forced to the program's tile) / chain_pack / chain_op — the record
     fields and the blob bytes must be identical, and the default tile list must choose the program's tile;
  3. the checks bite: six mutations of what the kernel is handed, never of the reference, must fail (the dropped padding of a stride-2
     stage is a descriptor word the kernel does not read — its regions carry the padding —: the emulator's own check of the regions against
     the stage's geometry is what fails).  Not representable on the emulator,
     and therefore only a comment: S_MASK (the emulator pads inside conv2d; on the GPU the case "bias in front of a depthwise stage" has no
     activation between a non-zero bias and a 5x5 depthwise stage, so a missing mask changes every border pixel), the prefetch registers and
     the tile loop (the emulator has no tiles), and the W_lo x_lo product the kernel leaves out;
  4. reach: the cases cover every tile of chains.CHAIN_TILES, both kernels, both stage types as last stage, regions of fewer than 256 and of
     more than 512 input vectors, 9 .. 15 tiles, and every (stage pattern, tile) pair of the product programs of 2."""
import numpy as np
import pytest

import chain_cases as CC
import op_harness as H
from oracle import net_ref
from vse_amd import chains, compiler, ir

SIZES = ((544, 960), (96, 160), (224, 352), (32, 608), (64, 64))
FAST = ("V3_ch_det_fast", "V4_ch_det_fast")


# ---- 1. the emulator leg ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", sorted(CC.GROUPS))
def test_emulator_matches_fp64_reference(built_lib, group):
    worst, n, e32, ep = 0.0, 0, 0.0, 0.0
    for sp in CC.GROUPS[group]():
        c = CC.case(sp)
        r = H.run_case(c, H.run_emulator)
        assert r is not None, sp.name
        print(f"  {sp.name}: {r:.3f}  e32 {c.note['e32']:.2e} e_pair {c.note['e_pair']:.2e}")
        worst, n, e32, ep = max(worst, r), n + 1, max(e32, c.note["e32"]), max(ep, c.note["e_pair"])
    print(f"{group}: {n} cases, worst error / bound {worst:.3f}, largest e32 {e32:.2e}, largest e_pair {ep:.2e}")
    assert n > 0


def test_refused_records_build(built_lib):
    """The records the library must refuse (GPU test) are one-record OP_CHAIN plans with a negative expectation."""
    seen = set()
    for name, rc, c in CC.REFUSED["chain"]():
        assert c.refused and len(c.runs) == 1 and c.runs[0].ops.dtype == ir.OP_DT and int(c.runs[0].ops["kind"][0]) == ir.OP_CHAIN and rc < 0
        seen.add(rc)
    assert seen == {H.VSE_E_INVAL, H.VSE_E_UNSUPPORTED}


# ---- 2. the hand-built records against the compiler's -----------------------------------------------------------------------------------
def _i2f(v):
    return float(np.asarray([v], np.int32).view(np.float32)[0])


def decode_chain(blob, r):
    """-> (stages as chain_stage dicts, weights, tile, the blob's bytes) of an OP_CHAIN record, from the descriptor and the LDS image."""
    off = int(r["w_off"])
    hdr = blob[off:off + 4 * ir.CH_HDR].view(np.int32)
    n, nb = int(hdr[ir.CHH_NSTAGES]), int(hdr[ir.CHH_NBUFS])
    sw = blob[off + 4 * (ir.CH_HDR + nb * ir.CH_BUF):off + 4 * (ir.CH_HDR + nb * ir.CH_BUF + n * ir.CH_STAGE)].view(np.int32).reshape(n, ir.CH_STAGE)
    img = off + int(hdr[ir.CHH_LDSIMG_OFF])
    lane = np.arange(64)
    rows = np.array([chains.conv_wrow(int(f)) for f in lane & 31])
    stages, weights = [], {}
    for j, s in enumerate(sw):
        cin, cout, k = int(s[ir.CHS_CIN]), int(s[ir.CHS_COUT]), int(s[ir.CHS_K])
        if int(s[ir.CHS_TYPE]) == ir.CH_PW:
            nks, nct = int(s[ir.CHS_NKS]), int(s[ir.CHS_NCT])
            o = img + int(s[ir.CHS_WLDS])
            fr = blob[o:o + 2 * nct * nks * 1024].view(np.float16).astype(np.float64).reshape(2, nct, nks, 64, 8)
            # (a lo half of -0: the weight lay below hi by less than fp16 can hold; -2^-30 rounds to the same -0)
            fr[1][np.signbit(fr[1]) & (fr[1] == 0)] = -2.0 ** -30
            wm = np.zeros((nct * 32, nks * 16), np.float64)
            for ct in range(nct):
                for ks in range(nks):
                    k0 = ks * 16 + 8 * (lane >> 5)
                    # (a weight whose split is (hi, lo): hi + lo itself can be a tie that rounds to hi's neighbour — lo = half a step of hi,
                    # about one weight in 4000 —, so lo is shortened by 2^-20 of itself, which neither fp16(w) nor fp16(w - hi) sees)
                    wm[(ct * 32 + rows)[:, None], k0[:, None] + np.arange(8)[None, :]] = fr[0, ct, ks] + fr[1, ct, ks] * (1.0 - 2.0 ** -20)
            o = img + int(s[ir.CHS_BLDS])
            bias = blob[o:o + 4 * cout].view(np.float32).copy()
            weights[f"w{j}"] = wm[:cout, :cin].reshape(cout, cin, 1, 1)
        else:
            nrec = chains.dw_rec(k)
            o = img + int(s[ir.CHS_WLDS])
            rec = blob[o:o + 4 * cin * nrec].view(np.float32).reshape(cin, nrec)
            bias = rec[:, k * k].copy()
            weights[f"w{j}"] = rec[:, :k * k].astype(np.float64).reshape(cin, 1, k, k)
        stages.append(H.chain_stage("pw" if int(s[ir.CHS_TYPE]) == ir.CH_PW else "dw", cin, cout, k, int(s[ir.CHS_S]), int(s[ir.CHS_ACT]),
                                    _i2f(s[ir.CHS_ACT_A]), _i2f(s[ir.CHS_ACT_B]), _i2f(s[ir.CHS_POST_A]), _i2f(s[ir.CHS_POST_B]),
                                    int(s[ir.CHS_RES]), int(s[ir.CHS_ACT2]), int(s[ir.CHS_GOUT]), int(s[ir.CHS_SHUF]), f"w{j}", bias))
    size = int(hdr[ir.CHH_LDSIMG_OFF]) + int(hdr[ir.CHH_LDSW_BYTES])
    return stages, weights, (int(hdr[ir.CHH_TH]), int(hdr[ir.CHH_TW])), blob[off:off + size]


def _absent(v):
    return None if int(v["n"]) == 0 else v


def product_chains():
    """(what, record, blob) of every OP_CHAIN record of the fast detectors' hi + lo programs at SIZES."""
    for mid in FAST:
        desc, w = net_ref.get_weights(mid)
        for h, wd in SIZES:
            prog = compiler.compile_model(desc, w, 2, h, wd, hilo=True)
            blob = prog.weights.array()
            for i, r in enumerate(prog.ops):
                if int(r["kind"]) == ir.OP_CHAIN:
                    yield (mid, h, wd, i), r, blob


def _pattern(stages):
    return "".join("p" if st["type"] == "pw" else "d" for st in stages)


def test_chain_records_and_blobs_match_the_compiler():
    nrec, pairs = 0, set()
    for what, r, blob in product_chains():
        stages, weights, tile, theirs = decode_chain(blob, r)
        p = r["p"]
        in_lo = bool(int(p[ir.P_CH_LO_IN]))
        H_, W_ = int(r["in0"]["h"]), int(r["in0"]["w"])
        free = chains.chain_plan([dict(st) for st in stages], H_, W_, in_lo)
        assert (free["th"], free["tw"]) == tile, (what, "the default tile list chooses", free["th"], free["tw"], "the program", tile)
        plan = chains.chain_plan(stages, H_, W_, in_lo, tiles=[tile])
        mine, img_bytes, _meta, _macs = chains.chain_pack(stages, plan, weights)
        assert np.array_equal(mine, theirs), (what, "the repacked blob differs", int((mine != theirs).sum()) if mine.shape == theirs.shape else "size")
        oh, ow = plan["dims"][-1]
        n = len(stages)
        shuf = bool(stages[-1]["shuf"])
        pw2 = int(shuf and n == 2 and all(st["type"] == "pw" for st in stages) and stages[0]["cin"] <= 64 and stages[1]["cout"] <= 32)
        rec = H.chain_op(r["in0"], r["out"], (-(-oh // tile[0]), -(-ow // tile[1])), plan["lds_total"], n, img_bytes, int(r["w_off"]),
                         out2=_absent(r["out2"]), out3=_absent(r["in2"]), pw2=pw2, lo_in=int(p[ir.P_CH_LO_IN]),
                         lo_out=[int(p[ir.P_CH_LO_OUT0 + g]) for g in range(3)])
        for fld in ("kind", "flags", "p", "f", "in0", "in1", "in2", "out", "out2", "w_off", "b_off", "aux_off"):
            assert np.array_equal(r[fld], rec[0][fld]), (what, fld, r[fld], rec[0][fld])
        assert H.chain_form(rec)[0] == ("pw2" if shuf else "generic"), what
        nrec += 1
        pairs.add((_pattern(stages), tile))
    assert nrec >= 60 and len(pairs) >= 13, (nrec, sorted(pairs))


# ---- 3. the checks bite ---------------------------------------------------------------------------------------------------------------
# (group, case name): the mutations applied to it.  Where a mutation means nothing for a case (no depthwise stage, no residual, ..) build()
# raises ValueError.
MUTATED = {
    ("tiles", "tile 4x8 pw-dw3-pw tails"): ("dw_taps", "lo_pass"),
    ("patterns", "pw-dw5 s2-pw odd map"): ("dw_taps", "pad"),
    ("patterns", "pw-dw3 s2-pw even map"): ("pad",),
    ("patterns", "pw-pw-pw residual of two candidates"): ("res",),
    ("patterns", "six stages residual from buffer 3"): ("res", "dw_taps"),
    ("patterns", "eight stages"): ("res", "lo_pass"),
    ("channels", "couts 72 and 40 two K slices"): ("cout", "lo_pass"),
    ("channels", "pw 40 into a 48-deep buffer"): ("cout",),
    ("io", "three outputs pairs"): ("lo_pass", "dw_taps"),
    ("product", "pw-pw two outputs at 8x16"): ("cout", "lo_pass"),
    ("tail", "tail 24-32-16"): ("shuf", "lo_pass"),
    ("tail", "tail 64-96-16 pair in"): ("shuf", "cout"),
}
# lo_pass in the REAL run: the lo fragments carry 2^-11 of each weight; an fp16 output hides that, a pair output and the fp32 map do not
REAL_LO_PASS = {("io", "three outputs pairs"), ("product", "pw-pw two outputs at 8x16"), ("tail", "tail 24-32-16")}


def _spec(group, name):
    return next(sp for sp in CC.GROUPS[group]() if sp.name == name)


def test_every_mutation_is_applied():
    for m in CC.MUTATIONS:
        assert any(m in ms for ms in MUTATED.values()), m


@pytest.mark.parametrize("group,name", sorted(MUTATED))
def test_mutations_fail_the_checks(built_lib, group, name):
    sp = _spec(group, name)
    assert H.run_case(CC.case(sp), H.run_emulator) is not None          # (unmutated: passes)
    for m in MUTATED[(group, name)]:
        modes = ("exact", "real") if m in CC.REAL_MUST_FAIL or (m == "lo_pass" and (group, name) in REAL_LO_PASS) else ("exact",)
        for mode in modes:
            mutated = CC.case(sp, mutate=m, modes=(mode,))          # (a mutation that does not apply to the case raises ValueError here)
            with pytest.raises(AssertionError):
                H.run_case(mutated, H.run_emulator)
                print(f"{name}: mutation {m} passed the {mode} run")


# ---- 4. reach ---------------------------------------------------------------------------------------------------------------------------
def test_cases_reach_every_tile_kernel_and_product_pattern(built_lib):
    tiles, forms, lasts, pairs, small, large, ragged, loops = set(), set(), set(), set(), 0, 0, 0, 0
    for group in CC.GROUPS:
        for sp in CC.GROUPS[group]():
            b = CC.build(sp, "exact")
            tiles.add(sp.tile)
            forms.add(H.chain_form(b.rec)[0])
            lasts.add(b.note["last"])
            pairs.add((b.note["pattern"], sp.tile))
            small += b.note["vecs"] < 256
            large += b.note["vecs"] > 512
            ragged += b.note["vecs"] % 256 != 0
            loops += 9 <= b.note["ntiles"] <= 15
    assert tiles == set(chains.CHAIN_TILES), set(chains.CHAIN_TILES) - tiles
    assert forms == {"generic", "pw2"} and lasts == {"pw", "dw"}, (forms, lasts)
    assert small and large and ragged and loops >= 2, (small, large, ragged, loops)
    product = set()
    for what, r, blob in product_chains():
        stages, _w, tile, _b = decode_chain(blob, r)
        product.add((_pattern(stages), tile))
    assert product <= pairs, ("no case for", sorted(product - pairs))
    # the tiles no product chain reaches (at these sizes) are reached by the cases alone
    assert {t for _p, t in product} < set(chains.CHAIN_TILES)
