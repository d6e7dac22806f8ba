"""bench.py's multi-rank control flow before the driver's 8-GPU run meets it: two ranks launched exactly like the driver does
(python -m torch.distributed.run, one process per rank), both on device 0 of this one-GPU box through the test hooks
VSE_DIST_BACKEND=gloo / VSE_BENCH_DEVICE=0 (bench.py main()).  What runs: process-group init, per-rank frame shards, the
barrier-bracketed timed region, the all_reduce(MAX) of the ranks' times, the ONE variable-length record gather
and the single JSON line of rank 0."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(cmd, env):
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_two_ranks_one_json_line(ctx, tmp_path):
    env = dict(os.environ, VSE_DIST_BACKEND="gloo", VSE_BENCH_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    flags = ["--steps", "2", "--warmup", "1", "--batch", "16", "--no-cpu-baseline", "--no-roofline", "--no-secondary", "--other-mode-steps", "0"]
    two = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                "--master-port", str(_free_port()), "bench.py", "--gpus", "2", "--dump-outputs", str(tmp_path / "two")] + flags, env)
    assert two["n_gpus"] == 2 and two["steps"] == 2 and two["warmup"] == 1 and two["scaling"] == "weak"
    assert two["config"]["records_gathered"] == 2 * 16 * 2            # ranks x frames per step x steps, gathered once
    assert two["config"]["frames_per_gpu_step"] == 16 and two["value"] > 0
    assert abs(two["value"] - 2 * 16 * 2 / (two["ms_per_step"] * 2 / 1e3)) < 0.02 * two["value"]      # whole-job frames / max time
    one = _run([sys.executable, "bench.py", "--gpus", "1", "--dump-outputs", str(tmp_path / "one")] + flags, dict(os.environ))
    assert one["n_gpus"] == 1 and one["config"]["records_gathered"] == 16 * 2
    assert one["config"]["boxes_last_step"] > 0
    # --dump-outputs: the last timed step of the whole job (rank 0's gathered records), frames in order
    for d, first, nf in ((tmp_path / "two", 2 * 16, 2 * 16), (tmp_path / "one", 16, 16)):
        got = {n: np.load(d / (n + ".npy")) for n in ("frame_numbers", "box_counts", "boxes", "scores", "text_codepoints")}
        assert got["frame_numbers"].tolist() == list(range(first, first + nf))
        nb = int(got["box_counts"].sum())
        assert nb > 0 and got["boxes"].shape == (nb, 4, 2) and got["scores"].shape == (nb,) and len(got["text_codepoints"]) == nb
    assert nb == one["config"]["boxes_last_step"]


def test_bench_one_rank_runs_every_collective_of_the_path_over_rccl(ctx):
    """no multi-GPU node is in reach, so RCCL's first contact would be the driver's 8-GPU run.  VSE_FORCE_DIST=1
    makes ONE rank initialise the process group with backend "nccl" (= RCCL on ROCm) and take the N > 1 branches: communicator init
    bound to the device, the mode vote (all_reduce on a device tensor + .item()), the probe gather, the barrier inside sync(), the
    all_reduce(MAX) of the ranks' times, the size all_gather and the ONE payload gather of the records (parallel.gather_records on
    device tensors) — each executes on an MI355X, on a world of one.  The 1 -> 8 curve stays unmeasured."""
    env = dict(os.environ, VSE_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("VSE_DIST_BACKEND", None)
    flags = ["--steps", "2", "--warmup", "1", "--batch", "16", "--no-cpu-baseline", "--no-roofline", "--no-secondary", "--other-mode-steps", "0"]
    one = _run([sys.executable, "bench.py", "--gpus", "1"] + flags, env)
    d = one["config"]["dist"]
    assert d["backend"] == "nccl" and d["world"] == 1 and d["forced_on_one_rank"] and d["collective_device"].startswith("cuda")
    c = d["collectives"]
    # vote 1 + time reductions 2 (warm-up block is untimed: one per timed() call) | probe 1 + payload per run_steps call 2 | sizes 2 | barriers 2 per timed()
    assert c["all_reduce"] >= 2 and c["gather"] >= 3 and c["all_gather"] >= 2 and c["barrier"] >= 2, c
    assert one["n_gpus"] == 1 and one["config"]["records_gathered"] == 16 * 2 and one["config"]["boxes_last_step"] > 0
    assert "gather" in one["config"]["gather"]


# share of exactly identical strings per recogniser on this path = the measured share minus a margin (tests/parity.py share_floor)
STRING_SHARE_FLOOR = {"V4_ch_rec": 0.8, "V4_ch_rec_fast": 0.2}      # measured (MI355X, round 6): 6/6 and 2/2; 3/10


@pytest.mark.parametrize("det_id,rec_id,H,W,nf", [("V4_ch_det", "V4_ch_rec", 1080, 1920, 4), ("V4_ch_det_fast", "V4_ch_rec_fast", 1080, 1920, 8),
                                                  ("V4_ch_det", "V4_ch_rec", 2160, 3840, 2)])
def test_bench_configuration_c2_against_the_oracle_in_one_piece(ctx, det_id, rec_id, H, W, nf):
    """The EXACT path bench.py times (BASELINE configs[1]; configs[0]'s models at the same frame size, the reference's default
    `fast` mode — bench.py --models fast, config.secondary.fast_mode_1080p; and configs[2]'s server pair on 4K frames —
    config.secondary.4k_batch32) against the CPU oracle, end to end on 4 x 1080p / 2 x 2160p frames:
    V4_ch_det map (engine vs oracle/net_ref) max-overlaid with bench.text_kernel_maps ON BOTH SIDES -> DB post-processing
    -> boxes (identical integers) -> perspective crops -> V4_ch_rec in the benchmarked ragged mode vs the oracle's
    rec_batches chunks (backend/tools/ocr.py:24-27,88-113; paddleocr TextSystem): every string reachable from the oracle's
    per-step distribution through near-ties only (oracle log-margin < tests/parity.py TOL tie = 1e-1), identical strings carry the oracle's
    confidence within TOL maxp_rel = 12 % relative (measured <= 1.9 %), different ones within conf_diff; the share of identical strings is printed (a random-weight head flips ~0.3-0.5 % of its steps)."""
    import numpy as np
    from parity import check_text
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from oracle import net_ref, pipeline_ref as P
    from vse_amd import pipeline, shim, synth
    from vse_amd import modelzoo
    det = modelzoo.get_model(det_id, seed=0)                          # bench.py's own stand-in detector (seeded, uncalibrated) ...
    det = (det[0], bench.empty_det_head(det[0], dict(det[1])))        # ... with its head pushed below the threshold, as bench.py does
    rec = net_ref.get_weights(rec_id)                                 # calibrated stand-in recogniser: a softmax that is not flat
    charset = shim.standin_charset("ch", shim._ncls(rec[0]))
    ref_charset = P.standin_charset(shim._ncls(rec[0]))
    frames, truth = synth.make_frames(nf, H, W, seed=100, return_truth=True)
    pipe = pipeline.OcrPipeline(ctx, det, rec, charset, rec_mode="ragged", bucket=256, batch_round=4, min_rec_group=8)
    mh, mw = pipeline.det_resize_shape(H, W, pipe.limit)
    overlay = bench.text_kernel_maps(truth, H, W, mh, mw, unclip_ratio=pipe.db["unclip_ratio"])
    dev = torch.from_numpy(frames).cuda()
    maps = pipe.det_maps(dev)
    torch.maximum(maps, torch.from_numpy(overlay).cuda(), out=maps)
    got_boxes = [pipeline.sorted_boxes(b[0]) for b in ctx.db_postprocess(maps, H, W, **pipe.db)]
    got_res = pipe.recognize(dev, got_boxes)
    maps_h = maps.cpu().numpy()
    nbox = nexact = 0
    for f in range(nf):
        x, _ = P.det_preprocess(frames[f])
        ref_map = np.maximum(net_ref.run_graph(det[0], det[1], x)[0].numpy()[0, 0], overlay[f])
        assert np.abs(maps_h[f] - ref_map).max() < 4e-2
        rb = P.sorted_boxes(P.db_postprocess(ref_map, H, W)[0])
        assert len(rb) == len(got_boxes[f]) > 0
        for a, b in zip(got_boxes[f], rb):
            assert np.array_equal(np.asarray(a), np.asarray(b)), (f, a, b)          # identical integers
        crops = [P.get_rotate_crop_image(frames[f], b) for b in rb]
        for idx, img_w in P.rec_batches(crops, 6):
            batch = np.stack([P.resize_norm_img(crops[i], img_w) for i in idx])
            probs = net_ref.run_graph(rec[0], rec[1], batch)[0].numpy()
            for k, i in enumerate(idx):
                ids, conf = P.ctc_greedy(probs[k])
                ref_text = P.decode_text(ids, ref_charset)
                text, score = got_res[f][i]
                nexact += check_text(rec_id, text, score, probs[k], ref_charset, ref_text, conf)
                nbox += 1
    print(f"{det_id} + {rec_id} @{H}p path vs oracle: {nbox} boxes identical, {nexact} / {nbox} strings identical (the rest reachable "
          f"through near-ties of the oracle's distribution, tests/parity.py)")
    from parity import CONF_DIFFS, share_floor
    print(f"reachable-but-different strings so far: {len(CONF_DIFFS)}, largest relative confidence difference {max(CONF_DIFFS, default=0.0):.3g}")
    assert nbox >= nf
    share_floor(nexact, nbox, STRING_SHARE_FLOOR[rec_id], (det_id, rec_id, H))
