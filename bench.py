#!/usr/bin/env python3
"""Headline benchmark: OCR frames/sec (DB detect + CTC recognise) on synthetic 1080p frames (BASELINE.json).

A "step" = one pass of the hot path over one batch of 64 device-resident 1080p frames per GPU:
  det pre-process -> V4/ch_det (server DB detector, 389.4 GFLOP/frame @544x960) -> DB post-process ->
  perspective crops of the text lines -> V4/ch_rec (server recogniser, SVTR neck + CTC) -> arg-max + CTC collapse
  -> text decode -> (N>1: one variable-length gather of the records to rank 0).

Weights: the reference checkout ships no weights for the V4 server models, so they are seeded random
stand-ins of the exact architectures ("data": "synthetic").  A random detector's probability map carries no
information about the frame, so INSIDE every step the map it produced is overlaid (one element-wise max on the
detector's stream) with a pre-rasterised map of the generator's text lines, shaped like a DB detector's output: a
shrunk text kernel per line with soft edges, 1-2 % of the pixels above the 0.3 threshold.  DB
post-processing (CCL, run records, host geometry, polygon scoring, unclip) then does its real work on every map,
and the recogniser's crops are cut from the boxes IT produced (`--boxes db`, the default; `--boxes gt` feeds the
generator's own boxes instead).  `--models fast-real` runs the one real-weight detector with no overlay at all.

Contract: python bench.py --gpus N --steps K --warmup W ; for N>1 launched by torch.distributed.run, one rank per
GPU.  Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times the K steps and prints the line; `--full` adds what
else the benchmark measures after the timed region (the other recogniser batching modes, the per-kernel roofline pass, the
secondary configurations and the CPU oracle baseline).  `--dump-outputs DIR` writes the last timed step's results (boxes,
recogniser scores and texts of every frame, rank 0's gathered records) as DIR/<name>.npy.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_PEAK_TFLOPS = 2500.0     # dense fp16/bf16 MFMA peak of the MI355X
HBM_PEAK_GBS = 8000.0


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64, help="frames per GPU per step")
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--models", default="server", choices=["server", "fast", "fast-real", "v2"],
                    help="server = V4_ch_det + V4_ch_rec (the headline); v2 = V2_ch_det + V2_ch_rec (ResNet + BiLSTM CRNN, 32-px crops)")
    ap.add_argument("--boxes", default="db", choices=["gt", "db"])
    ap.add_argument("--rec-mode", default="ragged", choices=["ragged", "bucketed", "reference"],
                    help="recogniser batching of the headline number (ragged = the reference's per-crop padded widths in shared "
                         "launches, bit-identical to `reference`); the other modes are timed beside it (`rec_modes` in the JSON line)")
    ap.add_argument("--other-mode-steps", type=int, default=4, help="timed steps of each non-headline rec mode (0 = skip)")
    ap.add_argument("--limit-side", type=int, default=960, help="det_limit_side_len (960 = the reference's default; 3840 = BASELINE "
                    "configs[2]'s stress form: a 4K frame becomes a 2176 x 3840 detector input)")
    ap.add_argument("--bucket", type=int, default=256, help="rec width bucket (px)")
    ap.add_argument("--batch-round", type=int, default=4)
    ap.add_argument("--min-rec-group", type=int, default=8,
                    help="rec width buckets with fewer crops absorb the next narrower bucket (0 = off); 8: the 4-crop 1280-px bucket of "
                         "the default workload joins the 1024-px one - 6 %% less GPU time in conv kernels at the same frames/s")
    ap.add_argument("--rec-streams", type=int, default=4, help="side streams of the recogniser's width groups (4: every group of a span in flight at once; server pair "
                    "2021 / 2003 vs 2010 / 2008 frames/s at 2 on one box = neutral, mobile pair 8.41-8.45 k vs 8.17-8.26 k)")
    ap.add_argument("--rec-span", type=int, default=2, help="streaming form, ragged mode: the crops of this many consecutive batches are "
                    "recognised together (results do not depend on the grouping; larger launches fill the chip on the recogniser's small maps)")
    ap.add_argument("--rec-graphs", action="store_true", help="every recogniser invocation (plan + CTC collapse, ~80 launches) as one HIP graph "
                    "captured against fixed buffers (needs --rec-streams > 1)")
    ap.add_argument("--ragged-floor", type=int, default=None, help="ragged grouping: crop-pixels below which a launch sequence stops getting faster")
    ap.add_argument("--ragged-launch-cost", type=int, default=None, help="ragged grouping: fixed cost of one launch sequence in crop-pixels")
    ap.add_argument("--no-det-chains", dest="det_chains", action="store_false", help="mobile detectors layer by layer (no OP_CHAIN / pair tensors)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-secondary", dest="secondary", action="store_false", help="skip config.secondary (4K batch 32, fast mode)")
    ap.add_argument("--secondary-steps", type=int, default=8)
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-overlap", action="store_true", help="finish batch k before the detector of batch k+1 starts")
    ap.add_argument("--no-host-pipeline", dest="host_pipeline", action="store_false",
                    help="read a span's recognition results back right behind its launches (rounds 1-5) instead of after the NEXT span's launches")
    ap.add_argument("--det-priority", type=int, default=0, help="HIP stream priority of the detector streams (-1 = high)")
    ap.add_argument("--rec-priority", type=int, default=-1, help="HIP stream priority of the recogniser side streams (-1 = high: the small recogniser kernels get CUs as they free up beside the detector of the next batch, +0.6 %)")
    ap.add_argument("--det-stream-mode", default="independent", choices=["own", "shared", "independent"],
                    help="detector batches in flight: own = one torch stream each (torch's round-robin pool: whether two of them share a "
                         "hardware queue is left to the runtime), shared = ONE stream for all of them (in order, back to back), independent = "
                         "streams verified to run concurrently with each other and with the main stream (engine.Context.side_streams)")
    ap.add_argument("--full", action="store_true", help="after the headline: the other rec modes (--other-mode-steps), the roofline pass, "
                    "config.secondary and the CPU baseline (each still switched off by its --no-* flag); a plain run times the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed step's boxes, scores and texts as DIR/<name>.npy")
    ap.add_argument("--det-depth", type=int, default=2, help="detector batches in flight ahead of the one being recognised (2: two detector launches fill each other's tails, +3.6 % over 1 on one box; 3: +1.6 %)")
    return ap.parse_args()


def empty_det_head(desc, weights, bias=-8.0):
    """Push the (random-weight) detector's output below the 0.3 bitmap threshold so that the DB post-process sees a
    sparse map, as it does on real subtitles, instead of coin-flip noise."""
    last_sig = [op for op in desc["ops"] if op["type"] == "sigmoid"][-1]
    prod = {o: op for op in desc["ops"] for outs in op["out"].values() for o in outs}
    op = prod[last_sig["in"]["X"][0]]
    assert op["type"] == "elementwise_add"
    b = op["in"]["Y"][0]
    weights[b] = np.full_like(weights[b], bias)
    return weights


def gt_quads(truth):
    out = []
    for tr in truth:
        qs = []
        for (x0, y0, x1, y1, _t) in tr:
            qs.append(np.array([[x0 - 4, y0 - 4], [x1 + 4, y0 - 4], [x1 + 4, y1 + 4], [x0 - 4, y1 + 4]], np.float32))
        out.append(qs)
    return out


def text_kernel_maps(truth, src_h, src_w, map_h, map_w, unclip_ratio=1.5, seed=7):
    """What a trained DB detector emits for the generator's text lines: per line a SHRUNK text kernel — inset by the distance d
    that post-processing grows back (d = kernel area * unclip_ratio / kernel perimeter, solved per line for the line's box
    + 4 px) — with probabilities near 1 inside, a soft ramp through the 0.3 threshold at the border and speckle on top, on
    a background of zeros.  -> float32 [n, map_h, map_w].  Used as an element-wise max overlay on the stand-in detector's map."""
    rng = np.random.default_rng(seed)
    out = np.zeros((len(truth), map_h, map_w), np.float32)
    sy, sx = map_h / float(src_h), map_w / float(src_w)
    yy, xx = np.mgrid[0:map_h, 0:map_w].astype(np.float32)
    for f, tr in enumerate(truth):
        for (x0, y0, x1, y1, _t) in tr:
            bx0, bx1, by0, by1 = (x0 - 4) * sx, (x1 + 4) * sx, (y0 - 4) * sy, (y1 + 4) * sy
            w, h = bx1 - bx0, by1 - by0
            lo_d, hi_d = 0.0, 0.5 * min(w, h)
            for _ in range(40):                                           # (w-2d)(h-2d) * unclip / (2 (w+h-4d)) = d
                d = 0.5 * (lo_d + hi_d)
                if (w - 2 * d) * (h - 2 * d) * unclip_ratio / (2 * (w + h - 4 * d)) > d:
                    lo_d = d
                else:
                    hi_d = d
            kx0, kx1, ky0, ky1 = bx0 + d, bx1 - d, by0 + d, by1 - d
            ya, yb = max(int(ky0) - 3, 0), min(int(ky1) + 4, map_h)
            xa, xb = max(int(kx0) - 3, 0), min(int(kx1) + 4, map_w)
            Y, X = yy[ya:yb, xa:xb], xx[ya:yb, xa:xb]
            # signed distance to the kernel rectangle (positive inside), 1.5-px ramp
            dist = np.minimum(np.minimum(X - kx0, kx1 - X), np.minimum(Y - ky0, ky1 - Y))
            p = np.clip(0.5 + dist / 1.5, 0.0, 1.0) * (0.86 + 0.12 * rng.random(dist.shape, dtype=np.float32))
            out[f, ya:yb, xa:xb] = np.maximum(out[f, ya:yb, xa:xb], p.astype(np.float32))
    return out


def cpu_baseline(args, frames, truth, det, rec, charset, overlay=None):
    """The oracle (CPU restatement, torch fp32, all host threads) on a bounded sample of the same workload."""
    import torch
    from oracle import net_ref, pipeline_ref as P
    nthreads = min(64, os.cpu_count() or 1)      # one socket's worth; more threads only slow torch-CPU convs down
    old_threads = torch.get_num_threads()
    torch.set_num_threads(nthreads)
    torch.set_flush_denormal(True)                # random stand-in weights can drive activations into denormals
    n = min(16, frames.shape[0])                  # bounded sample: stop after ~12 s of CPU work
    done = 0
    t0 = time.time()
    for f in range(n):
        if done and time.time() - t0 > 12:
            break
        done += 1
        x, _ = P.det_preprocess(frames[f])
        prob = net_ref.run_graph(det[0], det[1], x)[0].numpy()[0, 0]
        if overlay is not None:
            prob = np.maximum(prob, overlay[f])
        boxes, _scores = P.db_postprocess(prob, frames.shape[1], frames.shape[2])
        quads = P.sorted_boxes(boxes) if args.boxes == "db" else gt_quads([truth[f]])[0]
        crops = [P.get_rotate_crop_image(frames[f], q) for q in quads]
        for idx, img_w in P.rec_batches(crops, 6):
            batch = np.stack([P.resize_norm_img(crops[i], img_w) for i in idx])
            probs = net_ref.run_graph(rec[0], rec[1], batch)[0].numpy()
            for k in range(len(idx)):
                ids, _ = P.ctc_greedy(probs[k])
                P.decode_text(ids, charset)
    dt = time.time() - t0
    n = done
    torch.set_flush_denormal(False)
    torch.set_num_threads(old_threads)
    return {"value": round(n / dt, 4), "unit": "frames/s", "cores": nthreads, "kind": "port",
            "sample": f"{n} of the same synthetic {frames.shape[1]}p frames, batch 1 per frame like the reference, "
                      f"oracle/ (torch-CPU fp32 restatement; Paddle itself is not installable here)"}


def main():
    args = parse()
    # one process per GPU: cap this rank's host thread pools at cores / world BEFORE torch / OpenMP start them (8 ranks x all
    # cores otherwise); the host side of a step (DB geometry, grouping, decode) is single-threaded Python + numpy anyway
    from vse_amd import parallel as _parallel
    host_threads = _parallel.cap_host_threads()
    import torch
    if host_threads:
        torch.set_num_threads(host_threads)
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # test hooks (single-GPU boxes): VSE_DIST_BACKEND=gloo + VSE_BENCH_DEVICE=0 run several ranks on one device to
    # exercise the multi-rank control flow; the driver's launches use RCCL (backend "nccl"), one rank per GPU
    backend = os.environ.get("VSE_DIST_BACKEND", "nccl")
    if "VSE_BENCH_DEVICE" in os.environ:
        local = int(os.environ["VSE_BENCH_DEVICE"])
    # VSE_FORCE_DIST=1 on ONE rank: the process group is initialised anyway and every collective of the N > 1 path (mode vote
    # all_reduce, probe gather, barriers, all_reduce(MAX) of the times, size all_gather + payload gather) executes on a world of one
    # — how a one-GPU box runs RCCL communicator init and the device-tensor collectives the 8-GPU job takes (tests/test_gpu_bench.py)
    dist_on = world > 1 or os.environ.get("VSE_FORCE_DIST", "0") == "1"
    if dist_on and world == 1:
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            free_port = sk.getsockname()[1]
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(free_port))
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
    if dist_on:
        torch.cuda.set_device(local)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)
    from vse_amd import engine, modelzoo, parallel, pipeline, shim, synth

    t_start = time.time()

    def log(msg):
        if rank == 0:
            print(f"[bench +{time.time() - t_start:6.1f}s] {msg}", file=sys.stderr, flush=True)

    ctx = engine.Context(local)
    coll_dev = ctx.tdev if backend == "nccl" else "cpu"
    # gather vs all_gather for the record exchange: agreed by all ranks here, once, never inside the timed region (parallel.gather_mode)
    gmode = parallel.gather_mode(coll_dev)
    if dist_on and rank == 0:
        print(f"[bench] record exchange: {gmode} (agreed by all {world} ranks)", file=sys.stderr, flush=True)

    def sync():
        if dist_on:
            dist.barrier()
            parallel._count("barrier")
        torch.cuda.synchronize()

    # One workload = (model pair, frame size, frames per step): everything the timed region needs, built and resident before
    # it starts.  The headline is build(args...) below; `config.secondary` (north_star: "1080p AND 4K frame batches"; the
    # reference's default fast mode) times two more workloads with the same functions, a few steps each.
    args.dist_on, args.dist_backend = dist_on, backend
    W = build_workload(args, ctx, world, rank, coll_dev, sync, log, args.models, args.height, args.width, args.batch)
    pipe, det, rec, det_id, rec_id, lang = W.pipe, W.det, W.rec, W.det_id, W.rec_id, W.lang
    frames_np, truth, overlay_np, overlay, quads = W.frames_np, W.truth, W.overlay_np, W.overlay, W.quads
    timed, det_maps, stage2_recognise, span, depth = W.timed, W.det_maps, W.stage2_recognise, W.span, W.depth
    out, dt = timed(args.warmup, args.steps)
    log(f"timed region ({args.rec_mode} rec batching): {args.warmup} warmup + {args.steps} steps in {dt:.3f}s")
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, out, world * args.batch * (args.steps - 1))
        log(f"outputs of the last timed step written to {args.dump_outputs}")
    return finish(args, ctx, world, rank, W, out, dt, log, host_threads, build_secondary=lambda m, h, w_, b, **over: build_workload(
        args, ctx, world, rank, coll_dev, sync, log, m, h, w_, b, **over))


def build_workload(args, ctx, world, rank, coll_dev, sync, log, models, height, width, batch, **over):
    import types
    import torch
    import torch.distributed as dist
    from vse_amd import engine, modelzoo, parallel, pipeline, shim, synth
    args = argparse.Namespace(**dict(vars(args), models=models, height=height, width=width, batch=batch, **over))
    if args.models == "server":
        det_id, rec_id, lang = "V4_ch_det", "V4_ch_rec", "ch"
    elif args.models == "fast":
        det_id, rec_id, lang = "V4_ch_det_fast", "V4_ch_rec_fast", "ch"
    elif args.models == "v2":
        det_id, rec_id, lang = "V2_ch_det", "V2_ch_rec", "ch"
    else:
        det_id, rec_id, lang = "V3_ch_det_fast", "V4_en_rec_fast", "en"
    det = modelzoo.get_model(det_id, seed=0)
    rec = modelzoo.get_model(rec_id, seed=1)
    if not modelzoo.has_real_weights(det_id):
        det = (det[0], empty_det_head(det[0], det[1]))
    charset = shim.standin_charset(lang, shim._ncls(rec[0]))      # stand-in weights: index-faithful placeholder table
    pipe = pipeline.OcrPipeline(ctx, det, rec, charset, rec_mode=args.rec_mode, bucket=args.bucket,
                                batch_round=args.batch_round, min_rec_group=args.min_rec_group,
                                rec_h=32 if args.models == "v2" else 48, limit_side_len=args.limit_side,
                                det_chains=None if args.det_chains else False)

    pipe.rec_streams = args.rec_streams
    pipe.rec_graphs = args.rec_graphs
    if args.ragged_floor is not None:
        pipe.ragged_floor = args.ragged_floor
    if args.ragged_launch_cost is not None:
        pipe.ragged_launch_cost = args.ragged_launch_cost
    frames_np, truth = synth.make_frames(args.batch, args.height, args.width, seed=100 + rank, return_truth=True)
    frames = torch.from_numpy(frames_np).to(ctx.tdev)          # inputs resident in HBM before the timed region
    quads = gt_quads(truth)
    # stand-in detector weights: the text-kernel overlay of the generator's lines (see the module docstring), resident in HBM
    overlay_np, overlay = None, None
    if not modelzoo.has_real_weights(det_id):
        mh, mw = pipeline.det_resize_shape(args.height, args.width, pipe.limit)
        overlay_np = text_kernel_maps(truth, args.height, args.width, mh, mw, unclip_ratio=pipe.db["unclip_ratio"])
        overlay = torch.from_numpy(overlay_np).to(ctx.tdev)
    log(f"frames generated and uploaded ({frames_np.nbytes / 1e6:.0f} MB)"
        + (f"; text-kernel overlay: {100.0 * float((overlay_np > pipe.db['thresh']).mean()):.2f} % of map pixels above the threshold"
           if overlay_np is not None else ""))

    def det_maps(slot=0):
        maps = pipe.det_maps(frames, slot=slot)
        if overlay is not None:
            torch.maximum(maps, overlay, out=maps)      # bench scaffolding only (stand-in weights), on the detector's stream
        return maps

    def records(k, boxes, res):
        # frame numbers: step k of rank r covers frames [(k * world + r) * batch, ... + batch) of the job
        base = (k * world + rank) * args.batch
        return [(base + f, np.asarray(boxes[f], np.float32).reshape(-1, 4, 2), res[f]) for f in range(args.batch)]

    # Streaming form of the same work: the detector of batch k+1 (its own HIP stream and workspace slot) runs while batch k
    # goes through DB post-processing, the host-side box logic, the recogniser launches and the record gather — what a
    # whole-video extraction does with consecutive frame batches.  Every batch started inside the timed region is also
    # finished inside it (run_steps drains its last batch), so K steps = K complete det + rec passes.
    depth = max(1, args.det_depth)
    if args.det_stream_mode == "shared":
        det_streams = [torch.cuda.Stream(device=ctx.tdev, priority=args.det_priority)] * depth
    elif args.det_stream_mode == "independent":
        det_streams = ctx.side_streams(depth, priority=args.det_priority, role="det")
    else:
        det_streams = [torch.cuda.Stream(device=ctx.tdev, priority=args.det_priority) for _ in range(depth)]
    pipe.rec_stream_priority = args.rec_priority

    def stage1(k):
        st = det_streams[k % depth]
        with torch.cuda.stream(st):
            maps = det_maps(slot=k % (depth + 1))
            ev = torch.cuda.Event()
            ev.record(st)
        return maps, ev

    def stage2_boxes(handle):
        maps, ev, k = handle
        main = torch.cuda.current_stream(ctx.tdev)
        main.wait_event(ev)
        maps.record_stream(main)
        db = ctx.db_postprocess(maps, args.height, args.width, **pipe.db)
        return k, ([pipeline.sorted_boxes(b[0]) for b in db] if args.boxes == "db" else quads)

    def rec_launch(ready):
        """ready: [(step, boxes per frame)] of consecutive batches (every batch reads the same resident frames): their crops and
        recogniser sequences enqueued, nothing read back -> handle for rec_collect."""
        return list(ready), pipe.recognize_multi_launch([frames] * len(ready), [b for _, b in ready])

    def rec_collect(launched):
        ready, handle = launched
        out = []
        for (k, boxes), r in zip(ready, pipe.recognize_multi_collect(handle)):
            out += records(k, boxes, r)
        return out

    def stage2_recognise(ready):
        """launch + read-back in one piece (the profiling pass and the one-kernel-at-a-time form)."""
        return rec_collect(rec_launch(ready))

    span = max(1, args.rec_span) if args.rec_mode == "ragged" else 1

    def run_steps(n):
        """n complete det + rec passes over this rank's batch, then THE collective of the path: one variable-length gather of
        every rank's (frame, boxes, texts) records to rank 0 (north_star: "RCCL ... only for the final box/text gather")."""
        local = []
        if args.no_overlap:                   # one kernel at a time: same launches as the streamed form, nothing concurrent
            for k0 in range(0, n, span):
                ready = []
                for k in range(k0, min(n, k0 + span)):
                    db = ctx.db_postprocess(det_maps(), args.height, args.width, **pipe.db)
                    ready.append((k, [pipeline.sorted_boxes(b[0]) for b in db] if args.boxes == "db" else quads))
                local += stage2_recognise(ready)
        else:
            for st in det_streams:
                st.wait_stream(torch.cuda.current_stream(ctx.tdev))
            # software pipeline of the host side: the recognition of span s + 1 is LAUNCHED before the results of span s are read back,
            # so the host never waits behind launch chains it has just enqueued while the detector batches it has yet to enqueue wait
            # for it (every span launched inside the timed region is also collected inside it)
            queue, ready, launched = [], [], None
            need = span if pipe.rec_mode == "ragged" else 1

            def flush():
                nonlocal launched, ready
                nxt = rec_launch(ready)
                ready = []
                if not args.host_pipeline:
                    return rec_collect(nxt)
                got = rec_collect(launched) if launched is not None else []
                launched = nxt
                return got
            for k in range(n):
                queue.append(stage1(k) + (k,))
                if len(queue) > depth:
                    ready.append(stage2_boxes(queue.pop(0)))
                    if len(ready) >= need:
                        local += flush()
            while queue:
                ready.append(stage2_boxes(queue.pop(0)))
                if len(ready) >= need or not queue:
                    local += flush()
            if launched is not None:
                local += rec_collect(launched)
        return parallel.gather_records(local, device=coll_dev)

    def timed(warmup, steps):
        out = run_steps(warmup)
        sync()
        t0 = time.perf_counter()
        out = run_steps(steps)
        sync()
        dt = time.perf_counter() - t0
        if getattr(args, "dist_on", False):      # (tools that build a workload directly have no process group)
            tmax = torch.tensor([dt], dtype=torch.float64, device=coll_dev)
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            parallel._count("all_reduce")
            dt = float(tmax.item())
        return out, dt

    return types.SimpleNamespace(pipe=pipe, det=det, rec=rec, det_id=det_id, rec_id=rec_id, lang=lang, frames_np=frames_np, truth=truth,
                                 overlay_np=overlay_np, overlay=overlay, quads=quads, timed=timed, det_maps=det_maps,
                                 stage2_recognise=stage2_recognise, span=span, depth=depth, args=args, coll_dev=coll_dev)


def finish(args, ctx, world, rank, W, out, dt, log, host_threads, build_secondary):
    import torch
    import torch.distributed as dist
    from vse_amd import modelzoo, parallel, pipeline, shim
    pipe, det, rec, det_id, rec_id, lang = W.pipe, W.det, W.rec, W.det_id, W.rec_id, W.lang
    frames_np, truth, overlay_np, overlay, quads = W.frames_np, W.truth, W.overlay_np, W.overlay, W.quads
    timed, det_maps, stage2_recognise, span, depth = W.timed, W.det_maps, W.stage2_recognise, W.span, W.depth
    n_boxes = sum(len(r[1]) for r in out[-world * args.batch:]) if out is not None else 0
    # the other recogniser batching mode on the same workload, timed the same way (fewer steps: the reference grouping runs
    # one launch sequence per <= 6 crops of ONE frame and is launch-bound)
    rec_modes = {args.rec_mode: {"value": round(world * args.batch * args.steps / dt, 2), "ms_per_step": round(1e3 * dt / args.steps, 3),
                                 "steps": args.steps}}
    for other in ("ragged", "reference", "bucketed"):
        if other == args.rec_mode or args.other_mode_steps <= 0 or not args.full:
            continue
        pipe.rec_mode = other
        _o, dt2 = timed(1, args.other_mode_steps)
        pipe.rec_mode = args.rec_mode
        rec_modes[other] = {"value": round(world * args.batch * args.other_mode_steps / dt2, 2),
                            "ms_per_step": round(1e3 * dt2 / args.other_mode_steps, 3), "steps": args.other_mode_steps}
        log(f"{other} rec batching: {args.other_mode_steps} steps in {dt2:.3f}s")

    result = None
    if rank == 0:
        n_lines = sum(len(q) for q in quads)
        total_frames = world * args.batch * args.steps
        result = {
            "metric": f"OCR frames/sec (det+rec) @{args.height}p", "value": round(total_frames / dt, 2), "unit": "frames/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * dt / args.steps, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f16", "data": "synthetic",
            "config": {"workload": f"{args.batch}x{args.height}p frames/GPU/step, precise mode: {det_id} @{'x'.join(str(v) for v in pipeline.det_resize_shape(args.height, args.width, args.limit_side))} + "
                                   f"{rec_id}, {n_lines} text lines/batch, rec boxes={args.boxes}, rec batching="
                                   + {"bucketed": f"bucketed({args.bucket}px, min group {args.min_rec_group}): crops padded to their bucket, NOT "
                                                  "the reference's padding",
                                      "ragged": f"ragged({args.bucket}px groups, min group {args.min_rec_group}): every crop at the padded "
                                                "width of its reference chunk, crops of all frames share launches, results bit-identical "
                                                "to THIS ENGINE's run in the reference grouping (tests/test_gpu_pipeline.py; the C2 path vs "
                                                "the CPU oracle: tests/test_gpu_bench.py)",
                                      "reference": "reference (per frame, <= 6 crops per chunk, chunk padded to its widest crop)"}[args.rec_mode],
                       "det_map": ("detector output" if overlay is None else
                                   f"stand-in detector output (head bias -8) max-overlaid inside the step with the text-kernel map of the "
                                   f"generator's lines: {100.0 * float((overlay_np > pipe.db['thresh']).mean()):.2f} % of pixels > thresh"),
                       "boxes_last_step": n_boxes,
                       "rec_modes": rec_modes,
                       "streaming": "sequential batches" if args.no_overlap else
                                    f"detectors of the next {depth} batch(es) in flight (own HIP streams / workspace slots) while batch k is "
                                    "post-processed and recognised; all K batches start and finish inside the timed region",
                       "rec_span": f"crops of {span} consecutive batch(es) share the recogniser's launch sequences",
                       "frames_per_gpu_step": args.batch, "det_model": det_id, "rec_model": rec_id,
                       "weights": "real" if modelzoo.has_real_weights(det_id) else "seeded random (reference blobs missing)",
                       "gather": "one variable-length gather of all ranks' records to rank 0 at the end of the timed region"
                                 + (f" ({parallel.gather_mode(W.coll_dev)}, agreed by all ranks at start-up)" if args.dist_on else ""),
                       "host_threads_per_rank": host_threads if host_threads else "uncapped (1 rank)",
                       "records_gathered": len(out) if out is not None else 0},
        }
        if args.dist_on:
            # which collectives this rank issued so far (start-up vote + probe, the barriers and time reductions of every timed block,
            # the record exchange of every run_steps call); world 1 + VSE_FORCE_DIST=1 = the one-GPU rehearsal of the N > 1 path
            result["config"]["dist"] = {"backend": args.dist_backend, "world": world, "forced_on_one_rank": world == 1,
                                        "collective_device": str(W.coll_dev), "collectives": dict(parallel.COLLECTIVES)}
        if args.full and not args.no_roofline:
            def profile_pass():                                  # the work of `span` steps, sequential, every op timed
                ready = []
                for k in range(span):
                    maps = det_maps()
                    db = ctx.db_postprocess(maps, args.height, args.width, **pipe.db)
                    ready.append((k, [pipeline.sorted_boxes(b[0]) for b in db] if args.boxes == "db" else quads))
                stage2_recognise(ready)
            result["roofline"] = roofline(pipe, profile_pass, steps_per_call=span)     # rank 0 only: no collective
            log("roofline pass done")
        if (args.full and args.secondary and not args.no_roofline and world == 1 and args.models == "server" and args.height == 1080
                and args.limit_side == 960):                      # (the default headline only; the A/B tools pass --no-roofline)
            # the other single-GPU configurations north_star names, through the same functions, a few timed steps each (the headline
            # above is untouched: it was measured first): BASELINE configs[2]'s frame size (4K frames, batch 32; det_limit_side_len
            # stays the reference's 960, so the detector input is 544 x 960 and the crops come from 4K pixels), and the reference's
            # DEFAULT mode (backend/config.py:54 mode = fast -> V4/ch_det_fast + V4/ch_rec_fast, the mobile pair)
            sec = {}
            # (key, models, frame height, width, frames per step, overrides, timed steps per block, note)
            plan = (("4k_batch32", "server", 2160, 3840, 32, {}, args.secondary_steps, None),
                    # BASELINE configs[2] AS WRITTEN — "4K synthetic frames, LARGE DB detect + server CRNN, batch=32": det_limit_side_len = 3840,
                    # the detector input is 2176 x 3840 (16 x the work of the line above).  The reference never sets det_limit_side_len
                    # (backend/tools/ocr.py:91-113: 960 applies), so this is SURVEY 8(d) C3's "non-reference stress form".  One detector
                    # batch in flight ahead (two 64-GB workspace slots instead of three).
                    ("4k_batch32_limit3840", "server", 2160, 3840, 32, {"limit_side": 3840, "det_depth": 1}, max(2, args.secondary_steps // 4),
                     "non-reference stress form (SURVEY 8(d) C3): det_limit_side_len=3840, the reference's own call sites leave it at 960"),
                    ("fast_mode_1080p", "fast", 1080, 1920, 64, {"det_chains": True}, args.secondary_steps, None),
                    ("fast_mode_1080p_layerwise", "fast", 1080, 1920, 64, {"det_chains": False}, args.secondary_steps,
                     "development yardstick, NOT a parity-valid figure: the layer-by-layer mobile detector is below north_star's box IoU >= 0.99 "
                     "on 2-3 boxes per 400 (tests/test_gpu_pipeline.py); the product default is the line above"))
            for key, m, h, w_, b, over, nsteps, note in plan:
                try:
                    W2 = build_secondary(m, h, w_, b, **over)
                    # two timed blocks, both reported, the faster one is the figure.  The warm-up covers every detector workspace slot
                    # (step k runs in slot k % (depth + 1)) and two recogniser spans: a slot first touched inside a timed block costs an
                    # 8-GB allocation + zero fill there (round 5's driver line: 1569 / 1812 with a 2-step warm-up over 3 slots)
                    nwarm = max(4, W2.depth + 2)
                    _o2, dt2a = W2.timed(nwarm, nsteps)
                    _o2, dt2b = W2.timed(0, nsteps)
                    dt2 = min(dt2a, dt2b)
                    lim = over.get("limit_side", args.limit_side)
                    sec[key] = {"metric": f"OCR frames/sec (det+rec) @{h}p", "value": round(b * nsteps / dt2, 2), "unit": "frames/s",
                                "timed_blocks": [round(b * nsteps / dt2a, 2), round(b * nsteps / dt2b, 2)],
                                "ms_per_step": round(1e3 * dt2 / nsteps, 3), "steps": nsteps, "warmup": nwarm,
                                "workload": f"{b}x{h}p frames/step, {W2.det_id} @{'x'.join(str(v) for v in pipeline.det_resize_shape(h, w_, lim))} + {W2.rec_id}, "
                                            f"boxes from DB post-processing, ragged recognition",
                                "boxes_last_step": sum(len(r[1]) for r in _o2[-b:]),
                                "detector": ("fp16x2 weights, 1x1 / depthwise chains in LDS, hi + lo pair tensors (the default)" if over.get("det_chains", True) else
                                             "fp16x2 weights, layer by layer (det_chains=False)") if m == "fast" else "fp16"}
                    if note:
                        sec[key]["note"] = note
                    if key == "fast_mode_1080p_layerwise":
                        sec[key]["parity"] = "below north_star (IoU)"
                    if "limit_side" in over:
                        sec[key]["detector_convs"] = detector_convs_block(W2)      # this configuration's own roofline figure
                    log(f"secondary {key}: {sec[key]['value']} frames/s")
                    del W2, _o2
                    torch.cuda.empty_cache()
                except Exception as exc:      # the headline line must not die for a secondary figure
                    sec[key] = {"error": repr(exc)[:300]}
                    torch.cuda.empty_cache()
            result["config"]["secondary"] = sec
        if args.full and not args.no_cpu_baseline and world == 1:
            from oracle import pipeline_ref as P
            cs = P.standin_charset(shim._ncls(rec[0])) if lang != "en" else P.en_charset()
            result["cpu_baseline"] = cpu_baseline(args, frames_np, truth, det, rec, cs, overlay_np)
        print(json.dumps(result), flush=True)
    if args.dist_on:
        dist.barrier()
        dist.destroy_process_group()
        parallel.reset_gather_mode()
    return result


def dump_outputs(path, out, first_frame):
    """What a caller of the timed path receives for the last timed step (the gathered records of frames >= first_frame, in frame
    order) -> path/<name>.npy: frame_numbers [F], box_counts [F] (float64), boxes [B, 4, 2], scores [B] (float32) and
    text_codepoints [B, L] (float64, the recognised strings as Unicode code points, -1 past a string's end), boxes in frame order."""
    recs = sorted((r for r in out if r[0] >= first_frame), key=lambda r: r[0])
    boxes = [np.asarray(r[1], np.float32).reshape(-1, 4, 2) for r in recs]
    texts = [t for r in recs for t, _s in r[2]]
    codes = np.full((len(texts), max([1] + [len(t) for t in texts])), -1.0, np.float64)
    for i, t in enumerate(texts):
        codes[i, :len(t)] = [ord(c) for c in t]
    arrays = {"frame_numbers": np.array([r[0] for r in recs], np.float64),
              "box_counts": np.array([len(b) for b in boxes], np.float64),
              "boxes": np.concatenate(boxes) if boxes else np.zeros((0, 4, 2), np.float32),
              "scores": np.array([s for r in recs for _t, s in r[2]], np.float32),
              "text_codepoints": codes}
    assert len(arrays["scores"]) == len(arrays["boxes"]) == len(texts)
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)


def detector_convs_block(W):
    """The detector's conv ops of workload W alone, every op bracketed by HIP events on its launch stream (one sequential pass,
    the definition of `roofline.detector_convs`): algorithmic conv FLOPs / summed durations."""
    from vse_amd import ir
    pipe = W.pipe
    pipe.profile_sink = []
    try:
        W.det_maps()
        sink = pipe.profile_sink
    finally:
        pipe.profile_sink = None
    ms_sum = gmac = 0.0
    for ms, prog, _variants in sink:
        for k, r in enumerate(prog.ops):
            if int(r["kind"]) == ir.OP_CONV:
                ms_sum += float(ms[k])
                gmac += float(prog.op_gmacs[k])
    return {"tflops": round(2.0 * gmac / ms_sum, 1), "frac": round(2.0 * gmac / ms_sum / MFMA_PEAK_TFLOPS, 4), "ms_per_step": round(ms_sum, 3),
            "algorithmic_gflop_per_step": round(2.0 * gmac, 1), "bound": "mfma", "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s"}


def vendor_gemm_tflops(n=8192, reps=10):
    """The vendor GEMM's rate on this box (bench scaffolding, after the timed region): the practical ceiling of HIP-source matrix
    kernels on random operands — the chip clocks the matrix pipe to its power budget, well under the 2.4 GHz of the
    nominal peak `roofline.frac` is priced against."""
    import torch
    try:
        a = (torch.randn((n, n), device="cuda") * 0.1).half()
        b = (torch.randn((n, n), device="cuda") * 0.1).half()
        for _ in range(3):
            c = a @ b
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            c = a @ b
        e1.record()
        torch.cuda.synchronize()
        del a, b, c
        return round(2.0 * n ** 3 * reps / e0.elapsed_time(e1) / 1e9, 1)
    except Exception as exc:      # context only: never fail the bench line for it
        print(f"[bench] vendor GEMM probe failed: {exc}", file=sys.stderr)
        return None


def roofline(pipe, step, repeats=2, steps_per_call=1):
    """Dominant kernel = the conv_mfma_kernel instantiation with the largest total time over one whole step
    (detector + every recogniser launch).  Every op of every plan is bracketed by HIP events recorded on the stream
    the kernels are launched on (vse_plan_profile); achieved = algorithmic conv FLOPs routed to that kernel / its
    summed launch durations; avg_launch_us is directly comparable with rocprofv3 --stats' AverageNs for it.
    steps_per_call: `step` covers that many 64-frame steps (the streaming form recognises the crops of `--rec-span` consecutive
    batches together); every per-step figure is divided accordingly."""
    nsteps = repeats * steps_per_call
    from vse_amd import ir
    agg = {}
    det_conv = [0.0, 0.0]           # the detector's conv ops alone (north_star quotes its MFMA target on "detection convs")
    for _ in range(repeats):
        pipe.profile_sink = []
        step()
        for ms, prog, variants in pipe.profile_sink:
            is_det = bool(prog.outputs) and prog.outputs[0]["kind"] == "map"
            for k, r in enumerate(prog.ops):
                if int(r["kind"]) != ir.OP_CONV:
                    continue
                if is_det:
                    det_conv[0] += float(ms[k])
                    det_conv[1] += float(prog.op_gmacs[k])
                a = agg.setdefault(variants[k], [0.0, 0.0, 0, 0.0])
                a[0] += float(ms[k])
                a[1] += float(prog.op_gmacs[k])
                a[2] += 1
                # algorithmic HBM bytes of the op: every tensor it touches once (input, residual / second source, output) + its weights
                # (an fp16 hi + lo pair tensor — P_LO_OUT / P_LO_IN / P_LO_RES of the mobile detectors' box-exact mode — is two tensors)
                pair = {"out": 2.0 if int(r["p"][ir.P_LO_OUT]) else 1.0, "in0": 2.0 if int(r["p"][ir.P_LO_IN]) else 1.0,
                        "in1": 2.0 if int(r["p"][ir.P_LO_RES]) else 1.0}
                a[3] += sum(float(r[v]["n"]) * float(r[v]["h"]) * float(r[v]["w"]) * float(r[v]["c"]) * float(r[v]["esize"]) * pair.get(v, 1.0)
                            for v in ("in0", "in1", "in2", "out", "out2") if int(r[v]["n"]) > 0) \
                    + 2.0 * float(r["p"][ir.P_COUT]) * float(r["p"][ir.P_KTOT])
        pipe_last_sink = pipe.profile_sink
        pipe.profile_sink = None
    bn, (tms, gmac, cnt, _bytes) = max(agg.items(), key=lambda kv: kv[1][0])
    kname = bn
    achieved = 2.0 * gmac / tms          # GMAC/ms*2 = TFLOP/s
    # HBM bytes per launch of that kernel from the newest committed PMC summary that has it (separate rocprofv3 --pmc FETCH_SIZE /
    # WRITE_SIZE passes over this same command, tools/collect_profiles.sh; FETCH_SIZE doubled as the gfx950 guide prescribes)
    traffic, tsrc = None, None
    import glob
    for tpath in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic.json")), reverse=True):
        tj = json.load(open(tpath))
        if kname in tj.get("kernels", {}):
            traffic = tj["kernels"][kname]["hbm_bytes_per_launch"]
            tsrc = "profiles/" + os.path.basename(tpath)
            break
    all_ms = sum(v[0] for v in agg.values())
    assert all(len(v) == 4 for v in agg.values())
    # per-net totals of the last profiled step (diagnostics on stderr)
    per_net = {}
    for ms, prog, _v in pipe_last_sink:
        key = "det" if prog.outputs and prog.outputs[0]["kind"] == "map" else f"rec[{prog.in_shape[0]}x{prog.in_shape[2]}]"
        per_net[key] = per_net.get(key, 0.0) + float(ms.sum())
    rec_ms = sum(v for k, v in per_net.items() if k != "det") / steps_per_call
    print(f"[bench] per-net GPU ms (profiled pass over {steps_per_call} step(s)):", {k: round(v, 2) for k, v in per_net.items()},
          f"-> per step: det {per_net.get('det', 0.0) / steps_per_call:.2f}, rec {rec_ms:.2f}", file=sys.stderr)
    vendor = vendor_gemm_tflops()
    # the roofline that bounds the dominant kernel: the larger of flops / MFMA peak and algorithmic bytes / HBM peak (the server models'
    # 3x3 kernels: MFMA; the mobile pair of --models fast: HBM)
    hbm_bound = _bytes / (HBM_PEAK_GBS * 1e6) > 2.0 * gmac / MFMA_PEAK_TFLOPS
    head = {"bound": "hbm", "achieved": round(_bytes / tms / 1e6, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": round(_bytes / tms / 1e6 / HBM_PEAK_GBS, 4), "traffic": traffic, "mfma_tflops": round(achieved, 2),
            "algorithmic_bytes_per_launch": int(_bytes / cnt)} if hbm_bound else \
           {"bound": "mfma", "achieved": round(achieved, 2), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(achieved / MFMA_PEAK_TFLOPS, 4), "traffic": traffic}
    return {**head,
            # context for `frac` (not a replacement for it): what the vendor's GEMM reaches on this box, measured now
            "vendor_gemm_tflops": vendor, "vendor_gemm": "torch.matmul (hipBLASLt) fp16 8192^3, random operands, 10 launches",
            "frac_of_vendor_gemm": round(achieved / vendor, 3) if vendor else None,
            "traffic_source": f"{tsrc} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes)" if traffic else None,
            "kernel": kname, "launches_per_step": round(cnt / nsteps, 1),
            "avg_launch_us": round(1e3 * tms / cnt, 2),
            "algorithmic_gflop_per_launch": round(2 * gmac / cnt, 2),
            "share_of_conv_time": round(tms / all_ms, 3),
            "all_conv_tflops": round(2.0 * sum(v[1] for v in agg.values()) / all_ms, 2),
            "detector_convs": {"tflops": round(2.0 * det_conv[1] / det_conv[0], 1), "frac": round(2.0 * det_conv[1] / det_conv[0] / MFMA_PEAK_TFLOPS, 4),
                               "ms_per_step": round(det_conv[0] / nsteps, 3)} if det_conv[0] > 0 else None,
            "conv_ms_per_step": round(all_ms / nsteps, 3),
            # the other conv kernel instantiations by share of conv time (same definition of `achieved` for each)
            # per instantiation: the roofline that BOUNDS it = the larger of (flops / MFMA peak) and (algorithmic bytes / HBM peak): the
            # 1x1 aggregation convs on the 256 x 256 tile move ~200 FLOP per byte, under the ridge of 310 -> they are priced against HBM
            "kernels": [dict({"kernel": v, "share": round(t / all_ms, 3), "launches_per_step": round(c / nsteps, 1),
                              "achieved": round(2.0 * g / t, 1), "frac": round(2.0 * g / t / MFMA_PEAK_TFLOPS, 3),
                              "hbm_gbs": round(b / t / 1e6, 1), "hbm_frac": round(b / t / 1e6 / HBM_PEAK_GBS, 3)},
                             bound=("hbm" if b / (HBM_PEAK_GBS * 1e6) > 2.0 * g / MFMA_PEAK_TFLOPS else "mfma"))
                        for v, (t, g, c, b) in sorted(agg.items(), key=lambda kv: -kv[1][0])[:6]]}


if __name__ == "__main__":
    main()
