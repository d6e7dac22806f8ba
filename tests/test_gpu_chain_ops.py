"""The chain kernels ALONE (csrc/chain.hip: chain_kernel, chain_pw2_kernel): a one-record OP_CHAIN plan (tests/op_harness.py: chain_op,
chains.chain_plan / chain_pack — the compiler's own static planner and packer —, ref_chain) against a plain fp64 reference of the whole
chain, at the smallest shapes that reach each tile, stage pattern, channel padding, epilogue, output form and turn of the persistent
tile loop (tests/chain_cases.py).  Two runs per case:

    exact   dyadic inputs and sparse dyadic weights whose every partial sum is exact in fp32 and whose every LDS intermediate is exactly
            a hi + lo pair: got == float16(ref64) / the hi, lo split of ref64 / float32(ref64) BIT FOR BIT
    real    seeded normal inputs, non-zero biases, nonlinear activations, under op_harness.ratio, unchanged:
            fp16 output: ulp16 + 8 e32      fp32 map: 16 ulp32 + 8 e32      pair output: 2^-20 |ref64| + 2^-24 + 8 e32
            e32 = |ref_chain in float32 - ref_chain in float64|

Each case forces its tile and asserts the form it was written for (tile, buffer kinds, blocks per CU, kernel, tile count against the
device's CU count where the case is about the persistent loop).  A head tail runs with P_CH_PW2 = 1 and 0 on the same blob: the two maps
must be the same bits.  tests/test_chain_records.py runs the same cases on the CPU emulator, rebuilds every chain record of the fast
detectors through the same helpers byte for byte, proves that six mutations fail these checks, and that the cases reach every tile, both
kernels and every (stage pattern, tile) pair of the product programs.

Worst error / bound of the real run per group, measured on MI355X (the emulator's figure beside it; 0.5 = half an fp16 step, a correctly
rounded result; the exact runs are bit-identical on both):

    group (tests/chain_cases.py GROUPS)                                                        cases   MI355X   emulator
    tiles       all nine CHAIN_TILES on pw -> dw3 -> pw with tails, maps below a tile, 1 x 1      13     0.499     0.499
    patterns    pw-pw, dw-pw, pw-dw, residuals, six and eight stages, k 3 / 5, s 1 / 2            16     0.499     0.499
    product     the fast detectors' (stage pattern, tile) pairs, their outputs and residuals       8     0.498     0.498
    channels    Cp > C for both stage types, cout % 32 in {8, 16, 24}, two K slices, 8 channels    7     0.497     0.497
    epilogues   every ACT_* on both stage types, post affine, relu after a residual, S_MASK         9     0.499     0.499
    io          pair / wider inputs, batch 3, one to three outputs plain and pair, view widths     11     0.498     0.498
    persistent  9, 13, 15 tiles on 8 blocks; 832 tiles (> 3 per CU); one block per CU, 272 tiles    5     0.499     0.499
    tail        pw -> pw + pixel shuffle, c0 8 / 24 / 64 / 72, both kernels on one blob             9     0.102     0.061
    batch       an image alone and as image 2 of 3: the same bits                                   3     0.498     0.498
    refused     nine malformed records: the negative code, no launch                                9       -         -

Every case passes on MI355X and on the emulator: this suite found no wrong index and no wrong arithmetic in chain.hip, chains.py or the
emulator's _op14 — but one difference between the two: a stored output whose view is WIDER than the stage wrote zeros behind the stage's
channels on the emulator and nothing on the GPU; the emulator now stores what the kernel stores ("output view wider than cout").
The fp16 outputs sit at the 0.5 of their one rounding.  What measures the arithmetic are the outputs that carry more bits: the pair outputs
reach 0.067 ("one pair output") and 0.150 ("three outputs pairs") of 2^-20 |ref| + 2^-24 + 8 e32 on the GPU (emulator 0.049 and 0.082), the
fp32 map of the head tail 0.102 of 16 ulp32 + 8 e32 (emulator 0.061; chain_pw2_kernel and chain_kernel give the same bits).  The GPU's
figures are the larger ones: the emulator evaluates a 1x1 stage in float64 on the summed hi + lo operands, the kernel accumulates in fp32
and leaves the product W_lo x_lo out of its three MFMA passes.

The hi + lo rounding of the LDS intermediates fits inside the rule as it stands: over all cases e32 is 8e-8 .. 3.2e-6 and e_pair — the same
chain in float64 with every channel-minor intermediate passed through the hi + lo split — 0 (no such intermediate) .. 3.8e-7 (largest: "pw-dw5-pw-pw at 4x16",
e_pair 3.8e-7 beside e32 8.3e-7; the eight-stage chain 1.5e-7 beside 2.5e-7).  No case needs the 8 (e32 + e_pair) form; Spec.e_pair stays
unset everywhere.

The whole file: 10 tests (81 cases, 186 launches, 9 refusals), 2.8 s on one MI355X; the slowest test, the persistent group, 0.2 s.
"""
import pytest

import chain_cases as CC
import op_harness as H

pytestmark = pytest.mark.gpu


def _runner(ctx):
    return lambda ops, blob, tensors, widths, ws_bytes: H.run_gpu(ctx, ops, blob, tensors, widths, ws_bytes)


@pytest.mark.parametrize("group", sorted(CC.GROUPS))
def test_chain_kernel_matches_fp64_reference(ctx, group):
    n_cu = ctx.torch.cuda.get_device_properties(ctx.tdev).multi_processor_count
    worst, n, failed = 0.0, 0, []
    for sp in CC.GROUPS[group]():
        case = CC.case(sp)
        grid, tiles = H.chain_grid(case.runs[0].ops, n_cu)
        if sp.tiles_cu:
            assert tiles > sp.tiles_cu * n_cu, (sp.name, tiles, "tiles do not exceed", sp.tiles_cu, "x", n_cu, "CUs")
        if sp.tiles_cu or (sp.tiles and sp.tiles[0] > 8):
            assert grid < tiles, (sp.name, "every block has one tile:", grid, "blocks,", tiles, "tiles")
        try:
            r = H.run_case(case, _runner(ctx))
        except AssertionError as e:             # (every case of the group runs: the list says which paths are wrong, and by how much)
            failed.append(f"{sp.name}: {e}")
            continue
        assert r is not None, sp.name
        print(f"  {sp.name} [{H.chain_form(case.runs[0].ops)[0]}, {tiles} tiles]: {r:.3f}")
        worst, n = max(worst, r), n + 1
    print(f"{group}: {n} cases, worst error / bound {worst:.3f}")
    assert not failed, "\n".join(failed)
    assert n > 0


@pytest.mark.parametrize("group", sorted(CC.REFUSED))
def test_malformed_chain_records_are_refused(ctx, group):
    """Each record is well-formed but for one property; host code refuses it before any kernel starts (vse_plan_create, the top of
    launch_chain): the code the library must answer."""
    for name, rc, case in CC.REFUSED[group]():
        assert H.run_case(case, _runner(ctx)) is None
        assert case.note["rc"] == rc, (name, case.note, rc)
        print(f"{name}: rc={case.note['rc']}")
