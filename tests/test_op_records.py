"""CPU: the one-record cases of tests/op_cases.py on the emulator (oracle/ir_emul.py) against the same fp64 references under the same
bound as the GPU run (tests/test_gpu_ops.py) — the emulator is the reference of every "kernel leg" of the suite and is checked here op
by op — and the hand-built records against what the compiler emits for the same geometry."""
import numpy as np
import pytest

import op_cases
import op_harness as H
from oracle import net_ref
from vse_amd import compiler, ir


@pytest.mark.parametrize("group", sorted(op_cases.GROUPS))
def test_emulator_matches_fp64_reference(group):
    worst, n = 0.0, 0
    for case in op_cases.GROUPS[group]():
        r = H.run_case(case, H.run_emulator)
        assert r is not None, case.name
        worst, n = max(worst, r), n + 1
    print(f"{group}: {n} cases, worst error / bound {worst:.3f}")
    assert n > 0


@pytest.mark.parametrize("group", sorted(op_cases.REFUSED))
def test_refused_records_build(group):
    """The records the library must refuse (GPU test) are well-formed: only the one property named by the case is out of range."""
    for case in op_cases.REFUSED[group]():
        assert case.refused and len(case.runs) == 1 and case.runs[0].ops.dtype == ir.OP_DT


# ---- the hand-built records against the compiler's ------------------------------------------------------------------------------
def _same_record(theirs, mine, what):
    for fld in ("kind", "flags", "p", "f"):
        assert np.array_equal(theirs[fld], mine[0][fld]), (what, fld, theirs[fld], mine[0][fld])


def _program(mid, n, h, w, ragged, desc_w=None):
    desc, wts = desc_w or net_ref.get_weights(mid)
    return desc, compiler.compile_model(desc, wts, n, h, w, ragged=ragged)


def _desc_op(desc, typ, out_slot, name):
    hits = [o for o in desc["ops"] if o["type"] == typ and o["out"][out_slot][0] == name]
    assert len(hits) == 1, (typ, name)
    return hits[0]


def _wl(r):
    return int(r["p"][ir.P_WLIN]), int(r["p"][ir.P_WLOUT])


def _narrow_lstm(hidden):
    """V2_ch_rec with its two bidirectional LSTM layers cut down to `hidden` units (the first units of every gate, and the rows of the
    matrices that read them): no shipped model has an LSTM the scalar kernel serves."""
    desc, wts = net_ref.get_weights("V2_ch_rec")
    desc = dict(desc, ops=[dict(o, attrs=dict(o["attrs"], hidden_size=hidden)) if o["type"] == "rnn" else o for o in desc["ops"]])
    wts = dict(wts)
    rows = np.concatenate([np.arange(g * 256, g * 256 + hidden) for g in range(4)])
    units = np.concatenate([np.arange(hidden), 256 + np.arange(hidden)])
    for c in range(4):
        w_ih = wts[f"lstm_cell_{c}.w_0"][rows]
        wts[f"lstm_cell_{c}.w_0"] = w_ih if c < 2 else w_ih[:, units]
        wts[f"lstm_cell_{c}.w_1"] = wts[f"lstm_cell_{c}.w_1"][rows][:, :hidden]
        for b in ("b_0", "b_1"):
            wts[f"lstm_cell_{c}.{b}"] = wts[f"lstm_cell_{c}.{b}"][rows]
    wts["ctc_fc_w_attr"] = wts["ctc_fc_w_attr"][units]
    return desc, wts


@pytest.mark.parametrize("ragged", [False, True])
def test_records_match_the_compiler(ragged):
    """kind, flags, p[] and f[] of what op_harness builds = what the compiler emits for the same geometry, so the hand-built records
    cannot drift away from the product's (the geometry comes from the model descriptor, the views and offsets from the record)."""
    seen = set()
    # ---- V3_korean_rec_fast: depthwise convs, layer norm, global average pool, soft-max (3690 classes); V2_ch_rec: pools, MFMA LSTM
    for mid, shape in (("V3_korean_rec_fast", (2, 48, 96)), ("V2_ch_rec", (2, 32, 64))):
        desc, prog = _program(mid, *shape, ragged)
        dws = [o for o in desc["ops"] if o["type"] == "depthwise_conv2d"]
        recs = [r for r in prog.ops if int(r["kind"]) == ir.OP_DWCONV]
        # every depthwise conv of the graph is one OP_DWCONV or rides in a fused conv; the stand-alone ones keep the graph's order
        geoms = []
        for o in dws:
            wshape = net_ref.get_weights(mid)[1][o["in"]["Filter"][0]].shape
            geoms.append(((wshape[2], wshape[3]), tuple(o["attrs"]["strides"]), tuple(o["attrs"]["paddings"][:2])))
        gi = 0
        for r in recs:
            have = (tuple(int(v) for v in r["p"][0:2]), tuple(int(v) for v in r["p"][2:4]), tuple(int(v) for v in r["p"][4:6]))
            while gi < len(geoms) and geoms[gi] != have:
                gi += 1
            assert gi < len(geoms), (mid, "an OP_DWCONV whose geometry no depthwise_conv2d of the graph has, in order", have)
            k, s, pad = geoms[gi]
            gi += 1
            gate = r["in1"] if int(r["flags"]) & ir.F_GATE else None
            mine = H.dwconv_op(r["in0"], r["out"], k, s, pad, int(r["w_off"]), int(r["b_off"]), act=int(r["p"][ir.P_ACT]),
                               act_a=r["f"][ir.FS_ACT_A], act_b=r["f"][ir.FS_ACT_B], post_a=r["f"][ir.FS_POST_A], post_b=r["f"][ir.FS_POST_B],
                               gate=gate, gate_res=bool(int(r["flags"]) & ir.F_RES), lo_in=int(r["p"][ir.P_LO_RES]),
                               lo_out=int(r["p"][ir.P_LO_OUT]), hilo=bool(int(r["flags"]) & ir.F_HILO), wl=_wl(r))
            _same_record(r, mine, (mid, "dwconv"))
            seen.add(("dwconv", H.dwconv_form(r)[0]))
        for i, r in enumerate(prog.ops):
            kind, name = int(r["kind"]), prog.names[i]
            if kind == ir.OP_POOL:
                a = _desc_op(desc, "pool2d", "Out", name)["attrs"]
                pads = a["paddings"]
                mine = H.pool_op(r["in0"], r["out"], a["ksize"], a["strides"], (pads[0], pads[1]) if len(pads) == 2 else (pads[0], pads[2]),
                                 a["pooling_type"] == "max", a.get("ceil_mode", False), a.get("exclusive", True), wl=_wl(r))
                _same_record(r, mine, (mid, name))
                seen.add(("pool", H.pool_form(r)))
            elif kind == ir.OP_GAP:
                a = _desc_op(desc, "pool2d", "Out", name)["attrs"]
                assert a.get("adaptive") or a.get("global_pooling")
                _same_record(r, H.gap_op(r["in0"], r["in2"], r["out"], wl=_wl(r)), (mid, name))
                assert int(r["in2"]["esize"]) == 4 and (not ragged or int(r["in2"]["h"]) == int(r["in0"]["h"]))
                seen.add(("gap", ragged))
            elif kind == ir.OP_LAYERNORM:
                a = _desc_op(desc, "layer_norm", "Y", name)["attrs"]
                _same_record(r, H.layernorm_op(r["in0"], r["out"], a["epsilon"], int(r["w_off"]), wl=_wl(r)), (mid, name))
                seen.add("layernorm")
            elif kind == ir.OP_SOFTMAX:
                ncls = next(o["c"] for o in prog.outputs if o["kind"] == "probs")
                _same_record(r, H.softmax_op(r["in0"], r["out"], r["out2"], ncls, wl=_wl(r)), (mid, name))
                seen.add(("softmax",) + H.softmax_form(r))
            elif kind == ir.OP_LSTM:
                a = next(o for o in desc["ops"] if o["type"] == "rnn")["attrs"]
                assert a["is_bidirec"] and a["hidden_size"] == 256
                _same_record(r, H.lstm_op([r["in0"], r["in1"]], r["out"], 256, 2, int(r["w_off"]), True, wl=_wl(r)), (mid, name))
                seen.add(("lstm", H.lstm_form(r)))
    # ---- the scalar LSTM: the same graph with 48 hidden units
    desc, prog = _program(None, 2, 32, 64, ragged, desc_w=_narrow_lstm(48))
    recs = [r for r in prog.ops if int(r["kind"]) == ir.OP_LSTM]
    assert len(recs) == 4                                   # two layers x two directions, one launch each
    for j, r in enumerate(recs):
        _same_record(r, H.lstm_op(r["in0"], r["out"], 48, j % 2, int(r["w_off"]), False, wl=_wl(r)), ("scalar lstm", j))
        # one half of the layer's [B,1,T,2H] output: the reverse direction 48 channels (96 bytes) behind the forward one
        assert int(r["out"]["ld"]) == 96 and int(r["out"]["off"]) - int(recs[j - j % 2]["out"]["off"]) == (j % 2) * 96
        seen.add(("lstm", H.lstm_form(r)))
    want = {("dwconv", "col"), ("dwconv", "row"), ("pool", "max"), ("gap", ragged), "layernorm", ("lstm", "mfma"), ("lstm", "scalar")}
    assert want <= seen and any(s[0] == "softmax" for s in seen if isinstance(s, tuple)), seen
