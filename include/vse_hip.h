/* libvse_hip.so — C ABI of the MI355X-native subtitle-OCR hot path (DB text detection + CTC recognition).
 *
 * The reference (eritpchy/video-subtitle-extractor v2.2.0) has no FFI for this path: its operator
 * interface is a set of Python callables that end in third-party paddleocr / Paddle Inference.  Each entry
 * point below names the reference call site whose work it replaces (file:line under /root/reference).
 * The Python binding a maintainer adds is in INTEGRATION.md (ctypes; it is what vse_amd/engine.py does).
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success or a negative VSE_E_*
 * code and never throws; vse_last_error() returns a thread-local message.  All device work is enqueued on
 * the hipStream_t passed in (as void*) and is asynchronous with respect to the host unless stated.
 * The caller owns every activation / input / output buffer (e.g. torch allocator); the library owns only
 * the uploaded weights.  One vse_ctx per (process, device); calls on one ctx are not thread-safe.
 */
#ifndef VSE_HIP_H
#define VSE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSE_OK 0
#define VSE_E_INVAL (-1)
#define VSE_E_HIP (-2)
#define VSE_E_UNSUPPORTED (-3)
#define VSE_E_NOMEM (-4)

typedef struct vse_ctx vse_ctx;
typedef struct vse_plan vse_plan;

/* A strided NHWC tensor view inside one of the arenas (see ir.py VIEW_DT; 40 bytes, packed). */
#pragma pack(push, 1)
typedef struct vse_view {
    int64_t off;    /* byte offset of element (0,0,0,0) in its arena */
    int32_t arena;  /* 0 workspace, 1 weights, 2+k external pointer k (0 = input, 1.. = outputs) */
    int32_t n, h, w;
    int32_t c;      /* physical channel span */
    int32_t ld;     /* elements between consecutive pixels */
    int32_t esize;  /* 2 = fp16, 4 = fp32/int32 */
    int32_t pad;
} vse_view;

/* One fused kernel launch of the engine program (see ir.py OP_DT). */
typedef struct vse_op {
    int32_t kind;
    int32_t flags;
    int32_t p[22];
    float f[8];
    vse_view in0, in1, in2, out, out2;
    int64_t w_off, b_off, aux_off;
} vse_op;
#pragma pack(pop)

/* ---- context ------------------------------------------------------------------------------------ */
/* Replaces: paddle predictor creation inside paddleocr TextDetector/TextRecognizer.__init__, reached from
 * backend/tools/subtitle_detect.py:22 and backend/tools/ocr.py:91 (PaddleOCR(...)). */
int vse_init(int device_id, vse_ctx** ctx);
void vse_destroy(vse_ctx* ctx);
const char* vse_last_error(void);
size_t vse_sizeof_op(void);
size_t vse_sizeof_view(void);
int vse_abi_version(void);

/* ---- network programs ----------------------------------------------------------------------------- */
/* Upload (or replace) the packed weight blob of one model; returns a weights handle id >= 0.
 * Replaces: loading inference.pdiparams (backend/tools/paddle_model_config.py:100-106 + Paddle loader). */
int vse_weights_upload(vse_ctx* ctx, const void* host_blob, size_t nbytes);
int vse_weights_free(vse_ctx* ctx, int weights_id);

/* Create an executable plan from `n_ops` vse_op records compiled for one static input shape. */
int vse_plan_create(vse_ctx* ctx, int weights_id, const vse_op* ops, int n_ops, size_t ws_bytes, vse_plan** plan);
void vse_plan_destroy(vse_plan* plan);

/* Run the network: `ws` is a device workspace of >= ws_bytes, ext[0] the fp16 NHWC(8) input, ext[1..] the
 * output buffers.  The caller zero-fills `ws` ONCE before its first use with a plan (channel-padding lanes that no kernel
 * writes are read against zero weights and must hold finite values) and gives every run that may be in flight at the same
 * time its own workspace; a plan keeps no state between runs.  Replaces the Paddle predictor.run() inside paddleocr predict_det.py / predict_rec.py,
 * i.e. the device work behind backend/tools/subtitle_detect.py:25 and backend/tools/ocr.py:27. */
int vse_plan_run(vse_plan* plan, void* ws, void* const* ext, int n_ext, void* stream);

/* Ragged recogniser batches.  The reference recognises the crops of ONE frame in chunks of rec_batch_num (6,
 * backend/config.py:58 -> backend/tools/ocr.py:99), every chunk zero-padded to its own widest crop; what a crop's logits are
 * depends on that padded width (conv borders, SVTR attention span), not on its neighbours.  A plan compiled for ragged batches
 * takes a batch whose tensor is `Wmax` wide and a device table d_widths[level][n] (int32; level 0 = the padded width sample
 * n would have had in its reference chunk, further levels = that width behind each stride / pooling step, computed by the
 * compiler's Program.width_table): every kernel treats x >= width as outside the image, so sample n receives bit for bit the
 * values a batch of exactly its width yields — crops of many frames share one launch sequence.  vse_plan_run refuses such a plan. */
int vse_plan_run_ragged(vse_plan* plan, void* ws, void* const* ext, int n_ext, const int32_t* d_widths, void* stream);
/* Number of width levels a ragged plan expects in d_widths (0 for an ordinary plan). */
int vse_plan_width_levels(vse_plan* plan);

/* A detector plan compiled with the pre-processing fused into its stem conv (compiler fuse_preprocess: F_U8SRC) takes the uint8
 * BGR frames themselves as ext[0]; their geometry (what vse_det_preprocess gets as arguments) is set here before vse_plan_run /
 * vse_plan_profile, and by vse_det_forward.  Host-side state of the plan: set + run from one thread.  Replaces paddleocr
 * DetResizeForTest + NormalizeImage + ToCHWImage (App. C.1) behind backend/tools/subtitle_detect.py:25, without the pass. */
int vse_plan_set_source(vse_plan* plan, int src_h, int src_w, int64_t pitch, int64_t frame_stride);
/* 1 when the plan takes uint8 frames (above), 0 when it takes the fp16 input of vse_det_preprocess. */
int vse_plan_takes_frames(vse_plan* plan);

/* ---- model-level calls ------------------------------------------------------------------------------------
 * One call per network invocation, composed of the entry points of this header over a compiled plan.
 * vse_det_forward = vse_det_preprocess + vse_plan_run: uint8 BGR frames -> DB probability maps d_prob fp32 [n, dst_h, dst_w]
 * (what paddleocr TextDetector computes before its post-processing, behind backend/tools/subtitle_detect.py:25).  d_in_f16 is
 * caller-owned scratch [n, dst_h, dst_w, 8] fp16 (may be NULL for a plan that takes the frames, vse_plan_takes_frames); raw_input
 * != 0 for a plan compiled with the normalisation in its stem.
 * vse_rec_forward = vse_plan_run(_ragged) + vse_ctc_collapse(_ragged): recogniser input fp16 [b, h, w, 8] (vse_rec_preprocess)
 * -> arg-max / max-probability pairs d_idx_maxp [b, t, 2] and the CTC-collapsed class ids, lengths and mean confidences (what
 * paddleocr TextRecognizer computes behind backend/tools/ocr.py:27).  d_widths / out_level: the ragged plan's width table and
 * the level of its output sequence (NULL / 0 for an ordinary plan). */
int vse_det_forward(vse_ctx* ctx, vse_plan* det_plan, void* ws, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch,
                    int64_t frame_stride, int dst_h, int dst_w, int raw_input, void* d_in_f16, float* d_prob, void* stream);
int vse_rec_forward(vse_ctx* ctx, vse_plan* rec_plan, void* ws, const void* d_rec_in_f16, const int32_t* d_widths, int out_level,
                    void* d_idx_maxp, int b, int t, int32_t* d_out_idx, int32_t* d_out_len, float* d_out_conf, void* stream);

/* vse_rec_forward captured as ONE HIP graph against fixed buffers (input, width table, workspace, outputs stay at these addresses;
 * the caller refills input and width table before every vse_graph_launch on the same stream).  `stream` must not be the default
 * stream.  Replaces ~80 kernel launches per recogniser invocation by one graph launch (backend/tools/ocr.py:27 -> TextRecognizer). */
typedef struct vse_graph vse_graph;
int vse_rec_graph_create(vse_ctx* ctx, vse_plan* rec_plan, void* ws, const void* d_rec_in_f16, const int32_t* d_widths, int out_level,
                         void* d_idx_maxp, int b, int t, int32_t* d_out_idx, int32_t* d_out_len, float* d_out_conf, void* stream,
                         vse_graph** graph);
int vse_graph_launch(vse_graph* graph, void* stream);
void vse_graph_destroy(vse_graph* graph);

/* Per-op timing of one run with HIP events on `stream` (synchronises); ms[n_ops] filled.  d_widths as for
 * vse_plan_run_ragged (NULL for an ordinary plan).  Where the plan runs a 3x3 conv and the max-pool record behind it as one
 * kernel (conv_c3pool_kernel), the launch's time is the conv record's and the pool record reports exactly 0. */
int vse_plan_profile(vse_plan* plan, void* ws, void* const* ext, int n_ext, const int32_t* d_widths, void* stream, float* ms);

/* Which kernel instantiation a record launches, as the name rocprofv3 reports ("conv_c3_kernel<4, 2>",
 * "conv_gemm_kernel<256, 256, 4, 4, 64, 2, 0>", "dwconv_kernel" ...): lets bench.py attribute the time vse_plan_profile
 * measures to the kernels of the committed rocprof summaries.  Needs no plan, context or GPU; a conv record the library
 * would refuse reads "(refused: <code>)".  The string is thread-local and valid until the next call.  A record is named on
 * its own: a conv that a plan fuses with the pool behind it (see vse_plan_profile) is named as the unfused conv here. */
const char* vse_op_kernel_name(const vse_op* op);

/* ---- det pre-processing ----------------------------------------------------------------------------- */
/* uint8 BGR frames [n, src_h, src_w, 3] (row pitch `pitch` bytes, frame stride `frame_stride` bytes) ->
 * bilinear resize to [dst_h, dst_w] with OpenCV's fixed-point INTER_LINEAR arithmetic -> (x/255-mean)/std ->
 * fp16 NHWC with 8 physical channels (3 real).  Replaces paddleocr DetResizeForTest + NormalizeImage +
 * ToCHWImage behind backend/tools/subtitle_detect.py:25.
 * mean3 == std3 == NULL: RAW mode — channels 0..2 hold the resized uint8 values themselves (exact in fp16) and channel 3
 * the constant 1; a detector plan compiled with the normalisation folded into its stem conv (compiler input_norm) takes
 * this input and computes on exactly the reference's normalised values instead of their fp16 roundings. */
int vse_det_preprocess(vse_ctx* ctx, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch,
                       int64_t frame_stride, void* d_out_f16, int dst_h, int dst_w, const float* mean3,
                       const float* std3, void* stream);

/* ---- DB post-processing (device part) ----------------------------------------------------------------- */
/* prob map fp32 [n,h,w] -> connected components (8-connectivity) of (prob > thresh) with, per component,
 * pixel count, bounding box and per-row x-extents (the rows' extreme pixels are a superset of the convex
 * hull vertices).  Host finishing (hull, min-area rect, score, unclip: csrc/db_geometry.h) happens inside
 * vse_db_postprocess() below.
 * Replaces cv2.findContours / minAreaRect / fillPoly+mean inside paddleocr DBPostProcess (App. C.2). */
typedef struct vse_db_params {
    double box_thresh;     /* 0.6: compared with the box score as Python floats (doubles) in the reference */
    double unclip_ratio;   /* 1.5: distance = area * unclip_ratio / perimeter is double arithmetic in the reference */
    float thresh;          /* 0.3: compared with the float32 map in float32 */
    int max_candidates;    /* 1000 */
    int min_size;          /* 3 */
} vse_db_params;

typedef struct vse_box {
    float pts[4][2];   /* tl, tr, br, bl in source-frame pixels */
    float score;
    int frame;
} vse_box;

/* Workspace size (bytes) for n maps of h x w. */
size_t vse_db_workspace_bytes(int n, int h, int w);
/* Full DB post-process for a batch of maps: device CCL + device scoring + host geometry.
 * boxes[max_boxes] is host memory; *n_boxes receives the count.  Synchronises `stream`.
 * src_h/src_w: original frame size the boxes are scaled to. */
int vse_db_postprocess(vse_ctx* ctx, const float* d_prob, int n, int h, int w, int src_h, int src_w,
                       const vse_db_params* prm, void* d_ws, size_t ws_bytes, vse_box* boxes, int max_boxes,
                       int* n_boxes, void* stream);

/* ---- rec pre-processing ------------------------------------------------------------------------------- */
/* One perspective crop per box from the ORIGINAL uint8 BGR frames (bicubic, replicate border, 90-degree
 * rotation when h/w >= 1.5), then bilinear resize to height `rec_h`, (x/255-0.5)/0.5, zero right-pad to
 * `rec_w`, written as fp16 NHWC(8) rows of a [n_boxes, rec_h, rec_w, 8] batch.
 * Replaces paddleocr get_rotate_crop_image + resize_norm_img (App. C.4-C.5) behind backend/tools/ocr.py:27. */
typedef struct vse_crop {
    float quad[4][2];   /* source quad (tl,tr,br,bl) in frame pixels */
    int frame;          /* which frame of the batch */
    int crop_w, crop_h; /* integer size of the rectified crop before the 48-high resize */
    int resized_w;      /* width after resize to rec_h (<= rec_w) */
    int rotate;         /* 1: rotate 90 (np.rot90) before resize */
} vse_crop;

/* `crops` is a HOST array (the box list comes from the host-side DB geometry); the library solves the four
 * point homographies in double and uploads them.  d_scratch holds the rectified uint8 crops. */
int vse_rec_preprocess(vse_ctx* ctx, const void* d_bgr, int n_frames, int src_h, int src_w, int64_t pitch,
                       int64_t frame_stride, const vse_crop* crops, int n_crops, void* d_out_f16, int rec_h,
                       int rec_w, void* d_scratch, size_t scratch_bytes, void* stream);
size_t vse_rec_preprocess_scratch_bytes(int n_crops, int max_crop_w, int max_crop_h);

/* ---- CTC greedy collapse --------------------------------------------------------------------------------- */
/* idx_maxp: int32/fp32 pairs [b, t, 2] from the softmax head.  Keeps t where idx[t] != idx[t-1] and idx != 0
 * (wavefront ballot scan), writes kept class ids compacted per row, their count and the mean kept prob.
 * Replaces paddleocr CTCLabelDecode (App. C.6) behind backend/tools/ocr.py:27. */
int vse_ctc_collapse(vse_ctx* ctx, const void* d_idx_maxp, int b, int t, int32_t* d_out_idx, int32_t* d_out_len,
                     float* d_out_conf, void* stream);
/* The same over a ragged batch: d_tlen[b] (device int32) = sequence length of each row (the last level's row of the width
 * table handed to vse_plan_run_ragged); time steps at or behind it are not decoded.  d_tlen == NULL = vse_ctc_collapse. */
int vse_ctc_collapse_ragged(vse_ctx* ctx, const void* d_idx_maxp, int b, int t, const int32_t* d_tlen, int32_t* d_out_idx,
                            int32_t* d_out_len, float* d_out_conf, void* stream);

/* ---- CTC posterior fusion over the frames of one subtitle ------------------------------------------------------------------ */
/* Replaces: nothing the reference computes itself; the role is VideoSubFinder's (the closed binary run by backend/main.py:378-505),
 * which reads each subtitle from all of its frames, where the reference's own loop recognises ONE frame per subtitle
 * (backend/tools/ocr.py:27) and a recognition error on that frame is final.  A subtitle stands still, so the same quad cut from K
 * frames of its interval gives K crops of one geometry, the same number of time steps and the same alignment: the recogniser's
 * per-step class probabilities are averaged before the arg-max and the result decodes with vse_ctc_collapse_ragged like any other
 * row (vse_amd.pipeline.OcrPipeline.recognize_fused).  What that gains on real footage is not measured here (no real clips, stand-in
 * recogniser weights).
 * d_probs: [b, t] rows of ncls fp32 probabilities, the `probs` output of a recogniser plan; row (r, s) starts (r * t + s) * row_stride
 * floats behind d_probs, row_stride >= ncls.  d_group (device, [g + 1]): ascending row offsets, group j = rows d_group[j] ..
 * d_group[j + 1] - 1.  d_tlen (device, [g]) = the sequence length of each group, or NULL = t for every group.  For group j with member
 * rows r0 < r1 < .. < r(K-1), 1 <= K <= 64, and every step s < tlen[j], all in float32, every operation rounded on its own:
 *   acc[c] = p[r0][s][c], then acc[c] = acc[c] + p[rk][s][c] for k = 1 .. K - 1 in that order;
 *   m[c] = acc[c] / (float)K                                     (a correctly rounded divide; no fused multiply-add anywhere)
 *   idx = the smallest c whose m[c] is the largest, maxp = m[idx];
 * d_idx_maxp[j][s] = {idx, maxp} as int32 / fp32 pairs [g, t, 2], the layout vse_ctc_collapse_ragged takes.  Steps s >= tlen[j] get
 * {0, 0.0f}, and what their probability rows hold is never read.  K = 1 copies a row's arg-max and its probability.
 * One launch on `stream`, no allocation, no device sync.  The library cannot check a device table: the kernel clamps every member row
 * into 0 .. b - 1, K into 1 .. 64 and tlen into 0 .. t, so a wrong table gives wrong text and never an out-of-range access.  No
 * alignment beyond the floats' own is required; steps whose member rows all start on a 16-byte boundary take 16-byte loads.
 * Returns VSE_E_INVAL, and launches nothing, for a NULL pointer other than d_tlen, b, t, ncls or g < 1, row_stride < ncls,
 * ncls > 2^30, or g * t >= 2^24 (one 256-thread block per group and step). */
int vse_ctc_fuse(vse_ctx* ctx, const float* d_probs, int b, int t, int ncls, int64_t row_stride /* floats between (row, step) rows, >= ncls */,
                 const int32_t* d_group /* device, [g + 1], ascending row offsets, group j = rows d_group[j] .. d_group[j+1] - 1 */, int g,
                 const int32_t* d_tlen /* device, [g], or NULL = t for every group */, void* d_idx_maxp /* [g, t, 2] int32 / fp32 pairs */, void* stream);

/* ---- subtitle-change frame selector ----------------------------------------------------------------------------------- */
/* Replaces: VideoSubFinder's frame search (the closed binary run by backend/main.py:378-505, extract_frame_by_vsf), which looks at
 * every frame of the subtitle area and reports where each subtitle starts and stops.  Here the device part: per frame, the
 * luma edge mask of the area and how much of it changed against the previous frame; the host turns the counts into
 * intervals (vse_amd.frame_select.ChangeFrameSelector).
 * Size in bytes of the caller-owned state that carries the previous frame's mask from one call to the next, for an area of
 * area_h x area_w pixels (0 when the area is smaller than 3 x 3).  A fresh state is zero-filled. */
size_t vse_frame_change_state_bytes(int area_h, int area_w);
/* uint8 BGR frames [n, src_h, src_w, 3] (row pitch `pitch` bytes, frame stride `frame_stride` bytes) and the area
 * [y0, y1) x [x0, x1) (at least 3 x 3, inside the frame) -> d_counts int32 [n, 3] = edges, appeared, vanished per frame:
 *   Y = (29 B + 150 G + 77 R + 128) >> 8;
 *   edge pixel = interior pixel of the area (y0 < y < y1 - 1, x0 < x < x1 - 1) with
 *                max(|Y[y][x+1] - Y[y][x-1]|, |Y[y+1][x] - Y[y-1][x]|) >= edge_thresh;
 *   edges = |E|, appeared = |E and not E'|, vanished = |E' and not E|, E' = the previous frame's edge pixels.
 * Only pixels of the area are read (a caller may pass the area's rows alone).  d_state (vse_frame_change_state_bytes of this
 * area, 8-byte aligned) holds the last frame's mask after the call; the first frame of the next call is compared with it, so
 * batches of any size give the counts of one batch.  With `reset`, or on a fresh state, E' is empty for the first frame.
 * Returns VSE_E_INVAL, without touching the device, for a degenerate or out-of-frame area. */
int vse_frame_change(vse_ctx* ctx, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride,
                     int y0, int y1, int x0, int x1, int edge_thresh, void* d_state, int reset,
                     int32_t* d_counts /* [n,3]: edges, appeared, vanished */, void* stream);
/* Replaces: nothing in the reference; it serves the selectors above and below, which recognise each subtitle on ONE frame of its
 * interval: a score by which the host picks that frame (vse_amd.frame_select.sharpest_rep) instead of taking the middle one, which in
 * compressed video may as well be a coarse, half-faded or flashed frame.  Area, Y, interior and the edge pixels E of a frame exactly as
 * for vse_frame_change; E' = the previous frame's edge pixels, empty on a fresh state or with `reset`.  Per frame:
 *   g(p) = max(|Y[y][x+1] - Y[y][x-1]|, |Y[y+1][x] - Y[y-1][x]|)           (0..255; p is in E when g(p) >= edge_thresh)
 *   K = E and E'     the edge pixels that were edge pixels one frame earlier: a subtitle's edges stand still, most of a moving
 *                    background's do not
 *   kept = |K|,  focus = the sum of g(p) over p in K.
 * What it gains in recognition on real footage is not measured (no real clips).  Known limit: edges of a static background count in
 * every frame alike, and on a busy static shot the score also rewards the background's sharpness.
 * d_state has the size and the meaning of vse_frame_change's (vse_frame_change_state_bytes; the last frame's mask): frames fed in
 * batches of any sizes give the rows of one call, and a state written by vse_frame_change may be continued here and the other way
 * round.  Every element of d_focus is written.  One launch on `stream` behind the clearing of d_focus, no allocation, no device sync;
 * the sums are integers and do not depend on the order of the blocks.  Returns VSE_E_INVAL, and launches nothing, for what
 * vse_frame_change refuses, n < 1, or an interior of more than 2^23 pixels (focus <= 255 * 2^23 < 2^31; a 4K frame fits). */
int vse_frame_focus(vse_ctx* ctx, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride,
                    int y0, int y1, int x0, int x1, int edge_thresh, void* d_state, int reset,
                    int32_t* d_focus /* [n,2]: kept, focus */, void* stream);

/* ---- subtitle-area locator --------------------------------------------------------------------------------------------- */
/* Replaces: the rectangle a person draws in the reference's GUI (config.subtitleSelectionAreas, backend/config.py:49), which
 * SubtitleExtractor.run needs before it can take either frame-accurate path (backend/main.py:137-147).  Not an algorithm of the
 * reference but that role: a subtitle is strong luma edges that hold still for a while and then change all at once, a logo never
 * changes, a scene changes all the time.  Here the device part: vse_frame_change's edge mask over a whole region, counted per CELL,
 * with the interval automaton of vse_amd.frame_select.change_intervals run per cell on the device; the host turns the few integers
 * per cell into a rectangle (vse_amd.area_locator.locate_area).
 * Region [y0, y1) x [x0, x1) of area_h x area_w pixels, at least 3 x 3; E = the edge pixels of its interior exactly as defined for
 * vse_frame_change.  Cell (j, i) = interior rows 8 j .. 8 j + 7 and interior columns 64 i .. 64 i + 63 (cut off at the interior's
 * end); gy = ceil((area_h - 2) / 8) by gx = ceil((area_w - 2) / 64) cells.  Per cell and frame t, over the cell's pixels:
 *   e[t] = |E|, a[t] = |E and not E'|, v[t] = |E' and not E|                  (E' = the previous frame's edge pixels)
 *   present[t] = e[t] >= min_edges
 *   ratio cut before t: present[t-1] and present[t] and e[t-1] + a[t] > 0 and (a[t] + v[t]) ratio_den >= ratio_num (e[t-1] + a[t])
 *   a run = a maximal stretch of present frames without a ratio cut inside; when a run of L frames closes (a frame that is not
 *   present, a ratio cut, or `flush`) and min_frames <= L <= max_frames: covered += L, runs += 1
 *   present = number of present frames, cuts = number of ratio cuts.
 * vse_frame_cells_dims: gy and gx of a region; VSE_E_INVAL below 3 x 3. */
int vse_frame_cells_dims(int area_h, int area_w, int* gy, int* gx);
/* Size in bytes of the caller-owned state (8-byte aligned) that carries each cell's last mask (e[t-1] is its population count) and
 * the length of its open run from one call to the next; 0 below 3 x 3.  A fresh state is zero-filled. */
size_t vse_frame_cells_state_bytes(int area_h, int area_w);
/* n >= 0 uint8 BGR frames [n, src_h, src_w, 3] (pitch and frame stride as for vse_frame_change; only the region's pixels are read)
 * -> d_totals int32 [gy, gx, 4] = covered, runs, present, cuts per cell, accumulated across calls: the call continues from d_state
 * and from what d_totals holds, so a clip fed in batches of any size gives the totals of one call.  `reset` starts a clip: state and
 * totals count from zero and E' is empty for the first frame.  `flush` closes the open runs after the last frame of the call (runs
 * still open count nowhere until then); n == 0 with `flush` does only that.  d_cell_counts, when not NULL, receives int32
 * [n, gy, gx, 3] = e, a, v per frame and cell; summed over the cells they are vse_frame_change's counts of the same area.
 * One launch on `stream`, no allocation, no device sync; a block owns its cell for all frames of the call and alone writes the
 * cell's state, totals and counts.  Returns VSE_E_INVAL, without touching the device, for a degenerate or out-of-frame region,
 * n < 0, ratio_num < 1, ratio_den outside 1..1024, or not 1 <= min_frames <= max_frames. */
int vse_frame_cells(vse_ctx* ctx, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride,
                    int y0, int y1, int x0, int x1, int edge_thresh,
                    int min_edges, int ratio_num, int ratio_den, int min_frames, int max_frames,
                    void* d_state, int reset, int flush,
                    int32_t* d_totals      /* [gy,gx,4]: covered, runs, present, cuts; accumulated across calls */,
                    int32_t* d_cell_counts /* nullable: [n,gy,gx,3] edges, appeared, vanished per frame and cell */,
                    void* stream);

/* ---- edge-threshold calibration ---------------------------------------------------------------------------------------- */
/* Replaces: nothing in the reference, which has no edge threshold; it serves the selectors and the locator above, whose constant
 * edge_thresh = 128 describes white text with a black outline and finds nothing on yellow, shadowed, unoutlined or washed-out
 * subtitles.  vse_frame_cells for nt thresholds (1 <= nt <= 8, ascending, distinct, each 1..255; a host array) in ONE pass over the
 * frames: every pixel's bytes are read and its luma and gradient computed once per frame, and only the comparison, the cells' mask
 * words, counts and automata are kept per threshold.  The host picks a threshold from the totals
 * (vse_amd.area_locator.pick_edge_thresh).
 * d_totals int32 [nt, gy, gx, 4]: d_totals[k] holds exactly the integers vse_frame_cells with edge_thresh = thresholds[k] leaves in
 * its d_totals for the same frames, call sequence, `reset` and `flush` (batches of any sizes give the totals of one call; n == 0 with
 * `flush` only closes the open runs).  There is no per-frame output.  d_state: vse_frame_cells_multi_state_bytes(area_h, area_w, nt)
 * bytes, 8-byte aligned, zero-filled when fresh: nt times vse_frame_cells' state, threshold k's slice laid out as that one (0 for a
 * region below 3 x 3 or nt outside 1..8).  A state belongs to one region size and one nt; the same thresholds go to every call of a clip.
 * One launch on `stream`, no allocation, no device sync; a block owns its cell for all frames of the call and alone writes the cell's
 * state and totals, for all thresholds.  Returns VSE_E_INVAL, without touching the device, for everything vse_frame_cells refuses,
 * nt outside 1..8, thresholds NULL, not strictly ascending, or one outside 1..255. */
size_t vse_frame_cells_multi_state_bytes(int area_h, int area_w, int nt);
int vse_frame_cells_multi(vse_ctx* ctx, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride,
                          int y0, int y1, int x0, int x1, const int* thresholds /* host, [nt] */, int nt,
                          int min_edges, int ratio_num, int ratio_den, int min_frames, int max_frames,
                          void* d_state, int reset, int flush,
                          int32_t* d_totals /* [nt,gy,gx,4]: covered, runs, present, cuts; accumulated across calls */,
                          void* stream);
/* Replaces: nothing in the reference; it serves a selector that has to choose its edge threshold while the frames go by (a pipe, which
 * cannot be read twice: vse_amd.frame_select.CalibratingChangeSelector).  vse_frame_cells_multi with one more output.  The cells tile
 * the interior of the region, 8 x 64 interior pixels each, and their edge pixels are vse_frame_change's, so a frame's (e, a, v) summed
 * over all cells at thresholds[q] are vse_frame_change's counts of that frame on the same rectangle at edge_thresh = thresholds[q]:
 *   d_totals and d_state: bit for bit what vse_frame_cells_multi leaves for the same calls; the state is that entry's
 *     (vse_frame_cells_multi_state_bytes(area_h, area_w, nt)) and may pass between the two entries in the middle of a clip.
 *   d_counts int32 [n, nt, 3]: d_counts[f][q] = edges, appeared, vanished, integer for integer what vse_frame_change writes for frame f
 *     at edge_thresh = thresholds[q] on the area [y0, y1) x [x0, x1), fed in the same batches from the same start; `reset` or a fresh
 *     state means an empty previous mask in both.  Every element is written; n == 0 writes none (d_counts may then be NULL).
 * One launch on `stream` behind the clearing of d_counts, no allocation, no device sync; the sums are integers and do not depend on the
 * order of the blocks.  Returns VSE_E_INVAL, without touching the device, for everything vse_frame_cells_multi refuses or d_counts
 * NULL with n > 0. */
int vse_frame_cells_counts(vse_ctx* ctx, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride,
                           int y0, int y1, int x0, int x1, const int* thresholds /* host, [nt] */, int nt,
                           int min_edges, int ratio_num, int ratio_den, int min_frames, int max_frames,
                           void* d_state, int reset, int flush,
                           int32_t* d_totals /* [nt,gy,gx,4], as vse_frame_cells_multi */,
                           int32_t* d_counts /* [n,nt,3]: edges, appeared, vanished of the WHOLE area at thresholds[q] */, void* stream);
/* Slice q (0 <= q < nt) of such a state, of a region of area_h x area_w pixels -> d_change_state, a vse_frame_change state of the same
 * area (vse_frame_change_state_bytes(area_h, area_w) bytes, 8-byte aligned): the cells' last mask words laid out as that entry keeps
 * them, every word written, the flag set.  After it vse_frame_change or vse_frame_focus at edge_thresh = thresholds[q] on the following
 * frames give the rows that an uninterrupted run of theirs from the clip's start gives.  The cells' state is only read.  One small
 * launch on `stream`, no allocation, no device sync.  Returns VSE_E_INVAL, and launches nothing, for an area below 3 x 3, nt outside
 * 1..8, q outside 0..nt - 1, a NULL or misaligned pointer. */
int vse_frame_cells_export_state(vse_ctx* ctx, const void* d_cells_state, int area_h, int area_w, int nt, int q, void* d_change_state,
                                 void* stream);
/* Replaces: nothing in the reference; it serves a selector that has to FIND its area while the frames go by (a pipe, which cannot be
 * read twice: vse_amd.frame_select.LocatingChangeSelector).  The counts of vse_frame_change on a rectangle that is not known yet cannot
 * be summed from the cells (the located rectangle's interior lies one row and one column off the cell grid), but the edge MASK of a
 * pixel depends on its four neighbours and the threshold only, so the locator's pass keeps its mask words, one bit per pixel and
 * threshold, and vse_frame_masks_replay counts any rectangle out of them once the area is decided.
 * vse_frame_masks_bytes: the bytes of a mask buffer of `cap` frame slots for a region of area_h x area_w pixels at nt thresholds,
 *   cap * nt * gy * gx * 64 (gy, gx: vse_frame_cells_dims); 0 for an area below 3 x 3, nt outside 1..8 or cap < 1.
 * vse_frame_cells_masks: vse_frame_cells_multi with one more output.  Arguments, checks, d_state (vse_frame_cells_multi_state_bytes;
 *   it may pass between the two entries in the middle of a clip) and d_totals are that entry's, bit for bit.  d_masks: the caller's
 *   buffer of `cap` slots, 8-byte aligned; frame i of the call lands in slot slot0 + i (no wrap).  Layout, cell-major, in 64-bit words:
 *     slot f, threshold q, cell (cy, cx), row k of the cell -> word (((f * nt + q) * gy + cy) * gx + cx) * 8 + k;
 *     bit b of that word = region-interior pixel (8 cy + k, 64 cx + b) is an edge pixel of that frame at thresholds[q] (the interior
 *     pixel (iy, ix) is region pixel (1 + iy, 1 + ix)); zero beyond the interior, in rows and in columns.
 *   Every word of the slots slot0 .. slot0 + n - 1 is written and no other; n == 0 writes none (d_masks may then be NULL).  One launch
 *   on `stream`, no allocation, no device sync.  Returns VSE_E_INVAL, without touching the device, for everything
 *   vse_frame_cells_multi refuses, d_masks NULL or misaligned with n > 0, cap < 1, slot0 < 0 or slot0 + n > cap.
 * vse_frame_masks_replay: slots [f0, f1) of such a buffer at threshold index q, and a rectangle [ry0, ry1) x [rx0, rx1) in REGION
 *   coordinates (at least 3 x 3, inside the region) ->
 *     d_counts int32 [f1 - f0, 3]: edges, appeared, vanished, integer for integer what vse_frame_change writes for those frames at
 *       edge_thresh = thresholds[q] on that rectangle of the frames, fed from frame f0 on;
 *     d_change_state: a vse_frame_change state of the rectangle (vse_frame_change_state_bytes(ry1 - ry0, rx1 - rx0) bytes, 8-byte
 *       aligned) holding the mask of slot f1 - 1 as that entry keeps it, every word written, the flag set: vse_frame_change or
 *       vse_frame_focus on the following frames then give the rows of an uninterrupted run.
 *   reset != 0: the mask before frame f0 is empty; reset == 0: it is slot f0 - 1's (f0 >= 1), so a long window can be replayed in
 *   pieces.  The buffer is only read: slots f0 - 1 (without reset) .. f1 - 1, and only words of cells the rectangle touches.  d_counts
 *   is cleared on `stream` ahead of the kernel (one launch per 65535 frames), whose integer sums do not depend on the order of the
 *   blocks; no allocation, no device sync.  Returns VSE_E_INVAL, launching nothing, for an area or rectangle below 3 x 3, a rectangle
 *   outside the region, nt outside 1..8, q outside 0..nt - 1, f0 < 0, f1 <= f0, f1 > cap, reset == 0 with f0 == 0, a NULL or
 *   misaligned pointer. */
size_t vse_frame_masks_bytes(int area_h, int area_w, int nt, int cap);
int vse_frame_cells_masks(vse_ctx* ctx, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride,
                          int y0, int y1, int x0, int x1, const int* thresholds /* host, [nt] */, int nt,
                          int min_edges, int ratio_num, int ratio_den, int min_frames, int max_frames,
                          void* d_state, int reset, int flush,
                          int32_t* d_totals /* [nt,gy,gx,4], as vse_frame_cells_multi */,
                          void* d_masks /* cap slots of vse_frame_masks_bytes(y1 - y0, x1 - x0, nt, 1) bytes */, int cap, int slot0,
                          void* stream);
int vse_frame_masks_replay(vse_ctx* ctx, const void* d_masks, int area_h, int area_w, int nt, int cap, int q, int f0, int f1,
                           int ry0, int ry1, int rx0, int rx1, int reset,
                           int32_t* d_counts /* [f1 - f0, 3] */, void* d_change_state, void* stream);

/* ---- held-edge frame selector ------------------------------------------------------------------------------------------- */
/* Replaces: the same frame search of VideoSubFinder as vse_frame_change (backend/main.py:378-505, extract_frame_by_vsf), for
 * footage whose background moves behind the subtitle.  vse_frame_change compares every edge pixel of the area with the frame
 * before, so a textured background that pans makes every frame a cut and no subtitle is found.  A subtitle's edges hold still for
 * many frames and a moving background's do not, so here only HELD edges are counted; the host runs the unchanged interval automaton
 * on the counts (vse_amd.frame_select.HoldFrameSelector).  Not VideoSubFinder's algorithm; `hold` and the behaviour on real footage
 * are not measured here (no real clips).  Known limit: background edges that stay on one pixel for `hold` frames still count (a
 * static busy shot, a pan along an edge's own direction).  While the background moves they only add intervals between subtitles,
 * which cost OCR calls; once it stands still for as long as subtitles come and go they sit in the denominator of the host's cut ratio
 * and in neither numerator, and a subtitle that vanishes or is replaced over more static edges than its own is merged with its
 * neighbour and lost: vse_frame_hold_bounded below is for that footage.
 * Frames of a clip are numbered 1..T; E_t = the edge pixels of the area's interior in frame t exactly as defined for
 * vse_frame_change.  H_u, the held mask of frame u: pixel p is in H_u when p is in E_u and the maximal run of consecutive frames
 * containing u in which p is an edge pixel is at least `hold` frames long; runs are cut off at frame 1 and, once `flush` is given,
 * at the clip's last frame.  H_0 is empty.  The row of frame u is |H_u|, |H_u \ H_{u-1}|, |H_{u-1} \ H_u|.  hold == 1 gives
 * vse_frame_change's counts.
 * Size in bytes of the caller-owned state (8-byte aligned) that carries the open runs and the last counted mask from one call to the
 * next; 0 below 3 x 3 or for hold outside 1..32.  A fresh state is zero-filled; its layout is the library's. */
size_t vse_frame_hold_state_bytes(int area_h, int area_w, int hold);
/* n >= 0 uint8 BGR frames [n, src_h, src_w, 3] (pitch and frame stride as for vse_frame_change; only the area's pixels are read, so a
 * caller may pass the area's rows alone), the next frames of a clip of which `fed` frames went to earlier calls; fed == 0 starts a
 * clip and the state's content is then ignored.  H_u needs the frames up to u + hold - 1, so the call writes, from row 0 of d_counts
 * on, the rows of the frames max(0, fed - hold + 1) + 1 .. max(0, fed + n - hold + 1), and with `flush` (the clip ends with this
 * call) up to fed + n; d_counts has room for n + hold - 1 rows.  n == 0 with `flush` only drains the pending rows.  A clip fed in
 * batches of any sizes gives the rows of one call.  One launch sequence on `stream`, no allocation, no device sync; a block owns its
 * 8 x 64 interior pixels for all frames of the call and alone reads and writes their state.  Returns VSE_E_INVAL, without touching
 * the device, for a degenerate or out-of-frame area, hold outside 1..32, n < 0, fed < 0 or a NULL state. */
int vse_frame_hold(vse_ctx* ctx, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride,
                   int y0, int y1, int x0, int x1, int edge_thresh, int hold, void* d_state, int64_t fed, int flush,
                   int32_t* d_counts /* [n + hold - 1, 3]: held edges, appeared, vanished */, void* stream);

/* ---- held-edge frame selector with bounded runs ------------------------------------------------------------------------- */
/* Replaces: nothing in the reference; vse_frame_hold for footage whose background also stands still.  A subtitle's edges hold for at
 * least `hold` frames and at most some seconds; a channel logo's, a watermark's and a long static shot's hold far longer.  With E_t and
 * the maximal runs of consecutive edge frames per pixel as defined for vse_frame_hold (cut off at frame 1 and, once `flush` is given,
 * at the clip's last frame), B_u, the bounded mask of frame u: pixel p is in B_u when p is in E_u and the run containing u is L frames
 * long with hold <= L <= max_hold.  B_0 is empty.  The row of frame u is |B_u|, |B_u \ B_{u-1}|, |B_{u-1} \ B_u|; max_hold >= the
 * clip's length gives vse_frame_hold's rows.  Membership is per whole run: a run that grows beyond max_hold leaves every frame it
 * covered, so a row is final only once max_hold further frames have been seen.  Known limits: a subtitle shown for more than max_hold
 * frames disappears with the rest; a static shot shorter than max_hold still dilutes the host's cut ratio as before; pixels that
 * flicker around the threshold on a static background make short runs that count and can add intervals in the gaps (OCR calls, no
 * subtitle lost).  max_hold and the behaviour on real footage are not measured here (no real clips).
 * Size in bytes of the caller-owned state (8-byte aligned): one run length per pixel, and the rows still pending, max_hold + 64 of
 * them; 0 below 3 x 3 or for max_hold outside 1..4000.  A state belongs to one area size and one max_hold; its layout is the
 * library's. */
size_t vse_frame_hold_bounded_state_bytes(int area_h, int area_w, int max_hold);
/* Frames, area, `fed`, `flush` and state as for vse_frame_hold: n >= 0 frames, the next of a clip of which `fed` went to earlier calls;
 * fed == 0 starts a clip and the state's content is then ignored.  The call writes, from row 0 of d_counts on, the rows of the frames
 * max(0, fed - max_hold) + 1 .. max(0, fed + n - max_hold), and with `flush` (the clip ends with this call) up to fed + n; d_counts has
 * room for n + max_hold rows.  n == 0 with `flush` only drains the pending rows.  A clip fed in batches of any sizes, smaller or
 * larger than max_hold, gives the rows of one call.  Launches on `stream` only (per 64 frames the walk over the tiles and one wave
 * that finishes the rows), no allocation, no device sync; a block owns its 8 x 64 interior pixels and alone reads and writes their run
 * lengths, and the pending rows are integer atomics, so the order of the blocks cannot change them.  Returns VSE_E_INVAL, without
 * touching the device, for everything vse_frame_hold refuses, max_hold < hold or max_hold > 4000. */
int vse_frame_hold_bounded(vse_ctx* ctx, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride,
                           int y0, int y1, int x0, int x1, int edge_thresh, int hold, int max_hold, void* d_state, int64_t fed,
                           int flush, int32_t* d_counts /* [n + max_hold, 3]: bounded edges, appeared, vanished */, void* stream);

/* ---- locator and calibration on held edges ------------------------------------------------------------------------------ */
/* Replaces: nothing in the reference; it serves vse_frame_hold's footage.  vse_frame_cells and vse_frame_cells_multi run the cell
 * automaton on vse_frame_change's edge masks, and behind a subtitle whose textured background moves every frame is a cut in every
 * cell: no area, no threshold.  Here the same cells, automaton and thresholds on HELD masks.  For each of nt thresholds (as for
 * vse_frame_cells_multi: 1 <= nt <= 8, ascending, distinct, each 1..255; a host array) H_u is vse_frame_hold's held mask of frame u
 * at that threshold and `hold` (1..32), and per cell of 8 x 64 interior pixels (vse_frame_cells' cells) and frame u
 *   e = |H_u|,  a = |H_u \ H_{u-1}|,  v = |H_{u-1} \ H_u|
 * go in frame order to vse_frame_cells' unchanged automaton, which leaves covered, runs, present, cuts in d_totals [nt, gy, gx, 4].
 * hold == 1 gives vse_frame_cells_multi's totals, integer for integer.  How the rule does on real footage is not measured here (no
 * real clips).  Known limit: texture that holds still on a pixel for `hold` frames counts as held; at low thresholds fine, fast
 * texture does (see EXPERIMENTS.md).
 * Size in bytes of the caller-owned state (8-byte aligned, zero-filled when fresh, layout the library's: per threshold
 * vse_frame_hold's pixel state and each cell's open run); 0 below 3 x 3, for nt outside 1..8 or hold outside 1..32.  A state belongs
 * to one region size, nt and hold. */
size_t vse_frame_cells_hold_state_bytes(int area_h, int area_w, int nt, int hold);
/* n >= 0 frames as for vse_frame_hold, the next frames of a clip of which `fed` went to earlier calls; fed == 0 starts a clip: the
 * state's content is ignored and the totals count from zero.  After a call without `flush` the totals cover the frames 1 ..
 * max(0, fed + n - hold + 1), whose held masks are complete, with the last run left open; with `flush` (the clip ends with this call)
 * they cover all fed + n frames and the open runs are closed.  n == 0 with `flush` only drains and closes.  Batches of any sizes give
 * the totals of one call; the same thresholds, hold and rule go to every call of a clip.  d_cell_counts (nullable) receives, per
 * threshold, e, a, v per cell for the frames whose rows this call completes, numbered from row 0 as vse_frame_hold numbers its rows
 * (n + hold - 1 rows of room per threshold; rows the call does not complete are left alone); summed over the cells they are
 * vse_frame_hold's rows.  One launch on `stream`, no allocation, no device sync; a block owns its cell for all frames of the call
 * and alone reads and writes the cell's state, totals and counts, for all thresholds.  Returns VSE_E_INVAL, without touching the
 * device, for everything vse_frame_cells_multi refuses, hold outside 1..32, fed < 0, or n + hold - 1 beyond INT32_MAX. */
int vse_frame_cells_hold(vse_ctx* ctx, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride,
                         int y0, int y1, int x0, int x1, const int* thresholds /* host, [nt] */, int nt, int hold,
                         int min_edges, int ratio_num, int ratio_den, int min_frames, int max_frames,
                         void* d_state, int64_t fed, int flush,
                         int32_t* d_totals /* [nt,gy,gx,4]: covered, runs, present, cuts; accumulated across calls */,
                         int32_t* d_cell_counts /* nullable: [nt, n + hold - 1, gy, gx, 3] */, void* stream);
/* Replaces: nothing in the reference; it serves the hold selector when it has to FIND its area while the frames go by (a pipe, which
 * cannot be read twice: vse_amd.frame_select.LocatingHoldSelector), as vse_frame_cells_masks / vse_frame_masks_replay serve the change
 * selector.  The held mask of a rectangle is a walk along the frames over its pixels' EDGE bits, and an edge bit depends on the pixel's
 * four neighbours and the threshold only, so the held locator's pass keeps the edge words it builds anyway, and once the area is decided
 * a second kernel walks the rectangle's pixels through them.
 * vse_frame_cells_hold_masks: vse_frame_cells_hold with one more output.  Arguments, checks, d_state
 *   (vse_frame_cells_hold_state_bytes; it may pass between the two entries in the middle of a clip), d_totals and d_cell_counts are
 *   that entry's, bit for bit.  d_masks, cap and slot0 are vse_frame_cells_masks': frame i of the call lands in slot slot0 + i of a
 *   buffer of vse_frame_masks_bytes, in that entry's layout, and what is kept are the edge words E_t, not the held ones: a call writes,
 *   bit for bit, the words vse_frame_cells_masks writes for the same frames, region and thresholds.  Only frames get a slot: the steps
 *   of a flush get none, n == 0 writes none (d_masks may then be NULL), and no slot beside slot0 .. slot0 + n - 1 is touched.  One
 *   launch on `stream`, no allocation, no device sync.  Returns VSE_E_INVAL, without touching the device, for everything
 *   vse_frame_cells_hold refuses, d_masks NULL or misaligned with n > 0, cap < 1, slot0 < 0 or slot0 + n > cap.
 * vse_frame_masks_replay_hold: vse_frame_hold with the kept words in place of frames.  Slots [f0, f1) of such a buffer at threshold
 *   index q on the rectangle [ry0, ry1) x [rx0, rx1) in REGION coordinates (at least 3 x 3, inside the region) are the next f1 - f0
 *   frames of a clip of which `fed` went to earlier calls ->
 *     d_counts int32 [f1 - f0 + hold - 1, 3]: from row 0 on the rows vse_frame_hold writes for those frames, integer for integer: that
 *       entry on that rectangle of the frames at edge_thresh = thresholds[q] with the same hold, fed and flush;
 *     d_hold_state: a vse_frame_hold state of the rectangle (vse_frame_hold_state_bytes(ry1 - ry0, rx1 - rx0, hold) bytes, 8-byte
 *       aligned), read unless fed == 0 and left such that vse_frame_hold on the following frames gives the rows of an uninterrupted run.
 *   A window replayed in pieces, with fed advancing, gives the rows of one call; fed == 0 ignores the state's content; f1 == f0 with
 *   `flush` only drains the pending rows.  The buffer is only read, and only words of cells the rectangle touches.  d_counts is cleared
 *   on `stream` ahead of the one kernel, whose integer sums do not depend on the order of the blocks; a block owns 8 x 64 interior
 *   pixels of the rectangle for all slots of the call and alone reads and writes their state; no allocation, no device sync.  Returns
 *   VSE_E_INVAL, launching nothing, for an area or rectangle below 3 x 3, a rectangle outside the region, nt outside 1..8, q outside
 *   0..nt - 1, f0 < 0, f1 < f0, f1 > cap, f1 == f0 without flush, hold outside 1..32, fed < 0, a NULL or misaligned pointer. */
int vse_frame_cells_hold_masks(vse_ctx* ctx, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride,
                               int y0, int y1, int x0, int x1, const int* thresholds /* host, [nt] */, int nt, int hold,
                               int min_edges, int ratio_num, int ratio_den, int min_frames, int max_frames,
                               void* d_state, int64_t fed, int flush,
                               int32_t* d_totals /* [nt,gy,gx,4], as vse_frame_cells_hold */,
                               int32_t* d_cell_counts /* nullable: [nt, n + hold - 1, gy, gx, 3] */,
                               void* d_masks /* cap slots of vse_frame_masks_bytes(y1 - y0, x1 - x0, nt, 1) bytes */, int cap, int slot0,
                               void* stream);
int vse_frame_masks_replay_hold(vse_ctx* ctx, const void* d_masks, int area_h, int area_w, int nt, int cap, int q, int f0, int f1,
                                int ry0, int ry1, int rx0, int rx1, int hold, void* d_hold_state, int64_t fed, int flush,
                                int32_t* d_counts /* [f1 - f0 + hold - 1, 3]: held edges, appeared, vanished */, void* stream);

/* ---- locator and calibration on bounded runs ---------------------------------------------------------------------------- */
/* Replaces: nothing in the reference; it serves vse_frame_hold_bounded's footage.  Behind a subtitle whose busy background stands
 * still, vse_frame_cells_hold's cells keep their static edges in every frame: the cells of the subtitle itself are present throughout
 * (the host's logo rule scores them 0) and elsewhere the static edges dilute every cut ratio.  Here the same cells, automaton and
 * thresholds on BOUNDED masks.  For each of nt thresholds (as for vse_frame_cells_multi) B_u is vse_frame_hold_bounded's bounded mask
 * of frame u at that threshold, `hold` (1..32) and `max_hold` (hold..4000), and per cell of 8 x 64 interior pixels (vse_frame_cells'
 * cells) and frame u
 *   e = |B_u|,  a = |B_u \ B_{u-1}|,  v = |B_{u-1} \ B_u|
 * go in frame order to vse_frame_cells' unchanged automaton, which leaves covered, runs, present, cuts in d_totals [nt, gy, gx, 4].
 * max_hold >= the clip's length gives vse_frame_cells_hold's totals, integer for integer.  Known limits, with vse_frame_hold_bounded's:
 * a gap between two subtitles shorter than max_hold lets the background runs under the text count (the text cuts them to a length in
 * range), which adds edges to the cells in the gap; a subtitle shown for more than max_hold frames vanishes from its cells; max_hold
 * and the behaviour on real footage are not measured here (no real clips).
 * Size in bytes of the caller-owned state (8-byte aligned, layout the library's): with ih = area_h - 2, iw = area_w - 2, words =
 * ceil(iw / 64) and cells = ceil(ih / 8) * words it is, rounded up to 8,
 *   nt * ih * words * 128                 one uint16 run length per pixel and threshold, as vse_frame_hold lays its pixels out
 * + nt * cells * (max_hold + 64) * 4      the pending rows of every cell and threshold, one uint32 per row: a | v << 16 (a cell has
 *                                         512 pixels, so neither count passes 512)
 * + nt * cells * 8                        |B| of the cell's last finished row, and its open run
 * (whole-frame 1080p, nt 8, max_hold 360: 33 MB + 55 MB); 0 below 3 x 3, for nt outside 1..8 or max_hold outside 1..4000.  A state
 * belongs to one region size, nt and max_hold. */
size_t vse_frame_cells_hold_bounded_state_bytes(int area_h, int area_w, int nt, int max_hold);
/* Frames, `fed`, `flush` and the lag as for vse_frame_hold_bounded: a row is final once max_hold further frames have been seen.
 * fed == 0 starts a clip: the state's content is ignored and the totals count from zero.  After a call without `flush` the totals
 * cover the frames 1 .. max(0, fed + n - max_hold) with the last run left open; with `flush` (the clip ends with this call) they cover
 * all fed + n frames and the open runs are closed.  n == 0 with `flush` only drains and closes.  Batches of any sizes, smaller or
 * larger than max_hold, give the totals of one call; the same thresholds, hold, max_hold and rule go to every call of a clip.
 * d_cell_counts (nullable) receives, per threshold, e, a, v per cell for the frames whose rows this call completes, numbered from row
 * 0 as vse_frame_hold_bounded numbers its rows (n + max_hold rows of room per threshold; rows the call does not complete are left
 * alone); summed over the cells they are vse_frame_hold_bounded's rows.  One kernel launch on `stream` (before a clip's first, a
 * clear of the pending rows on the same stream), no allocation, no device sync; a block owns its cell for all frames of the call and
 * alone reads and writes the cell's state, totals and counts, for all thresholds.  Returns VSE_E_INVAL, without touching the device,
 * for everything vse_frame_cells_hold refuses, max_hold < hold, max_hold > 4000, or n + max_hold beyond INT32_MAX. */
int vse_frame_cells_hold_bounded(vse_ctx* ctx, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride,
                                 int y0, int y1, int x0, int x1, const int* thresholds /* host, [nt] */, int nt, int hold, int max_hold,
                                 int min_edges, int ratio_num, int ratio_den, int min_frames, int max_frames,
                                 void* d_state, int64_t fed, int flush,
                                 int32_t* d_totals /* [nt,gy,gx,4]: covered, runs, present, cuts; accumulated across calls */,
                                 int32_t* d_cell_counts /* nullable: [nt, n + max_hold, gy, gx, 3] */, void* stream);
/* Replaces: nothing in the reference; it serves the hold selector with bounded runs when it has to FIND its area while the frames go by
 * (a pipe: vse_amd.frame_select.LocatingBoundedHoldSelector), as vse_frame_cells_hold_masks / vse_frame_masks_replay_hold serve the
 * unbounded one.  A bounded mask is a walk along the frames over a pixel's EDGE bits, so the bounded locator's pass keeps the edge words
 * it builds anyway, and once the area is decided a second kernel walks the rectangle's pixels through them.
 * vse_frame_cells_hold_bounded_masks: vse_frame_cells_hold_bounded with one more output.  Arguments, checks, d_state
 *   (vse_frame_cells_hold_bounded_state_bytes; it may pass between the two entries in the middle of a clip), d_totals and d_cell_counts
 *   are that entry's, bit for bit.  d_masks, cap and slot0 are vse_frame_cells_masks': frame i of the call lands in slot slot0 + i of a
 *   buffer of vse_frame_masks_bytes, in that entry's layout; what is kept are the edge words E_t: a call writes, bit for bit, the words
 *   vse_frame_cells_masks writes for the same frames, region and thresholds.  Only frames get a slot: the flush step gets none, n == 0
 *   writes none (d_masks may then be NULL), and no slot beside slot0 .. slot0 + n - 1 is touched.  One kernel launch on `stream`, no
 *   allocation, no device sync.  Returns VSE_E_INVAL, without touching the device, for everything vse_frame_cells_hold_bounded refuses,
 *   d_masks NULL or misaligned with n > 0, cap < 1, slot0 < 0 or slot0 + n > cap.
 * vse_frame_masks_replay_hold_bounded: vse_frame_hold_bounded with the kept words in place of frames.  Slots [f0, f1) of such a buffer
 *   at threshold index q on the rectangle [ry0, ry1) x [rx0, rx1) in REGION coordinates (at least 3 x 3, inside the region) are the
 *   next f1 - f0 frames of a clip of which `fed` went to earlier calls ->
 *     d_counts int32 [f1 - f0 + max_hold, 3]: from row 0 on the rows vse_frame_hold_bounded writes for those frames, integer for
 *       integer: that entry on that rectangle of the frames at edge_thresh = thresholds[q] with the same hold, max_hold, fed and flush;
 *     d_bounded_state: a vse_frame_hold_bounded state of the rectangle (vse_frame_hold_bounded_state_bytes(ry1 - ry0, rx1 - rx0,
 *       max_hold) bytes, 8-byte aligned), read unless fed == 0 and left byte for byte as that entry leaves it, so that
 *       vse_frame_hold_bounded on the following frames gives the rows of an uninterrupted run.
 *   A window replayed in pieces, with fed advancing, gives the rows of one call; f1 == f0 with `flush` only drains the pending rows.
 *   The buffer is only read, and only words of cells the rectangle touches.  Launches as vse_frame_hold_bounded (per 64 slots the walk
 *   over the rectangle's tiles and one wave that finishes the rows), integer atomics and single-owner stores only; no allocation, no
 *   device sync.  Returns VSE_E_INVAL, launching nothing, for everything vse_frame_masks_replay_hold refuses, max_hold < hold or
 *   max_hold > 4000. */
int vse_frame_cells_hold_bounded_masks(vse_ctx* ctx, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride,
                                       int y0, int y1, int x0, int x1, const int* thresholds /* host, [nt] */, int nt, int hold,
                                       int max_hold, int min_edges, int ratio_num, int ratio_den, int min_frames, int max_frames,
                                       void* d_state, int64_t fed, int flush,
                                       int32_t* d_totals /* [nt,gy,gx,4], as vse_frame_cells_hold_bounded */,
                                       int32_t* d_cell_counts /* nullable: [nt, n + max_hold, gy, gx, 3] */,
                                       void* d_masks /* cap slots of vse_frame_masks_bytes(y1 - y0, x1 - x0, nt, 1) bytes */, int cap,
                                       int slot0, void* stream);
int vse_frame_masks_replay_hold_bounded(vse_ctx* ctx, const void* d_masks, int area_h, int area_w, int nt, int cap, int q, int f0, int f1,
                                        int ry0, int ry1, int rx0, int rx1, int hold, int max_hold, void* d_bounded_state, int64_t fed,
                                        int flush, int32_t* d_counts /* [f1 - f0 + max_hold, 3]: bounded edges, appeared, vanished */,
                                        void* stream);

/* ---- interval composite ------------------------------------------------------------------------------------------------- */
/* Replaces: the picture VideoSubFinder hands to OCR for each subtitle it finds (the RGBImages the reference reads back at
 * backend/main.py:378-505), which that closed binary builds from all frames of the subtitle, not from one of them.  Not its
 * algorithm but the same idea: a subtitle stands still while the picture behind it moves, so a per-byte reduction over the frames of
 * one interval of vse_frame_change keeps the text and flattens the background (vse_amd.frame_select.IntervalCompositor).  Whether
 * that helps recognition on real footage is not measured here.  For every byte b of the area [y0, y1) x [x0, x1) x 3, over all
 * frames accumulated since the last `reset`:
 *   mn[b] = min, mx[b] = max, sm[b] = sum as uint32.
 * Size in bytes of the caller-owned state (16-byte aligned) that holds mn, mx and sm of an area of area_h x area_w pixels: 6 bytes
 * per byte of the area's rows, each row padded to a multiple of 16 bytes; 0 for an empty area.  Its layout is the library's. */
size_t vse_interval_state_bytes(int area_h, int area_w);
/* 1 <= n <= 65535 uint8 BGR frames [n, src_h, src_w, 3] (row pitch `pitch` bytes, frame stride `frame_stride` bytes) folded into
 * d_state.  With `reset` the call starts from its own first frame and the state needs no particular content beforehand; without it
 * the call continues the state, so an interval fed in batches of any size gives the state of one call.  Only the area's pixels are
 * used, so a caller may pass the area's rows alone (where a row of the area does not start or end on a 4-byte boundary, the aligned
 * 4 bytes around that end are fetched whole).  No alignment of frames, pitch or stride is required; a 16-byte aligned area start
 * (base + 3 x0), pitch and frame stride take 16-byte loads.  One launch on `stream`, no allocation, no device sync.
 * Returns VSE_E_INVAL, without touching the device, for an empty or out-of-frame area, n outside 1..65535, pitch < 3 src_w,
 * frame_stride < (src_h - 1) pitch + 3 src_w when n > 1, or a state that is not 16-byte aligned. */
int vse_interval_accumulate(vse_ctx* ctx, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride,
                            int y0, int y1, int x0, int x1, void* d_state, int reset, void* stream);
/* d_state -> d_out uint8 [area_h, area_w, 3] with row pitch `out_pitch` bytes (exactly the 3 area_w bytes of each row are written):
 *   mode 0: mn;  mode 1: mx;  mode 2: the mean, halves rounded up: (2 sm + frames) / (2 frames) in integer division.
 * `frames` is the caller's count of the frames accumulated since the last reset, 1..4194304 (2^22): within it 2 sm + frames
 * <= 2 * 255 * 2^22 + 2^22 < 2^32.  One launch on `stream`, no allocation, no device sync.
 * Returns VSE_E_INVAL, leaving the output untouched, for an empty area, any other mode or count, or out_pitch < 3 area_w. */
int vse_interval_composite(vse_ctx* ctx, const void* d_state, int area_h, int area_w, int frames, int mode /* 0 min, 1 max, 2 mean */,
                           void* d_out, int64_t out_pitch, void* stream);
/* The per-byte order statistic over time, the robust form of mn / mx above: for every byte b of the area [y0, y1) x [x0, x1) x 3 of
 * 1 <= n <= VSE_INTERVAL_RANK_MAX uint8 BGR frames [n, src_h, src_w, 3] (row pitch `pitch` bytes, frame stride `frame_stride` bytes),
 * the n values frame[f][b] sorted ascending, element `rank` (0-based: 0 is the minimum, n - 1 the maximum, (n - 1) / 2 the lower
 * median) -> d_out uint8 [area_h, area_w, 3] with row pitch `out_pitch` bytes (exactly the 3 area_w bytes of each row are written).
 * The temporal median of a subtitle that stands still over a picture that moves is the subtitle's own value at text pixels whatever
 * its colour, and a minority of outlier frames (a flash, a cut one frame late) cannot move it
 * (vse_amd.frame_select.IntervalQuantile, which hands it a few evenly spaced samples of an interval: exact over those samples, an
 * estimate of the interval's quantile when it has more frames).  Whether that helps recognition on real footage is not measured here.
 * Stateless; the frames are read only, and only the area's pixels are used, as vse_interval_accumulate uses them (where a row of the
 * area does not start or end on a 4-byte boundary, the aligned 4 bytes around that end are fetched whole).  No alignment is
 * required; a 4-byte aligned area start (base + 3 x0), pitch and frame stride take one aligned load per frame.  One launch on
 * `stream`, no allocation, no device sync, no atomics.
 * Returns VSE_E_INVAL, without touching the device, for everything vse_interval_accumulate refuses about frames, pitch, stride and
 * area, n outside 1..VSE_INTERVAL_RANK_MAX, rank outside 0..n - 1, a NULL d_out, or out_pitch < 3 area_w. */
#define VSE_INTERVAL_RANK_MAX 63
int vse_interval_rank(vse_ctx* ctx, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride,
                      int y0, int y1, int x0, int x1, int rank, void* d_out, int64_t out_pitch, void* stream);
/* Replaces: the second pass over the clip that vse_interval_accumulate / vse_interval_composite need (the reference has none: its
 * closed binary makes its pictures while it reads the film once, backend/main.py:378-505).  The same mn / mx / sm and the same three
 * modes, made in the selector's own pass (vse_amd.frame_select.StreamingCompositor): one call folds any number of SEGMENTS of
 * consecutive frames, writes the composite of every segment that ends a subtitle, and parks the frames whose fate is still open in
 * a small ring on the device, so a sequential source (a pipe) needs no second look at frames already gone.
 * Frames carry absolute 1-based numbers.  The n >= 0 frames of a call are frames fed + 1 .. fed + n (with n = 0, d_bgr may be
 * NULL).  The state holds the accumulators of vse_interval_state_bytes and behind them `cap` ring slots of one area band each (rows
 * padded to 16 bytes); frame f lives in slot f % cap.  A segment may read a batch frame, or a ring frame f <= fed with f > fed - cap
 * that an earlier call stored and no later store has replaced: the caller keeps that book, the library checks only the numbers.
 * After ALL segment reads of the call, the batch frames f >= store_from are written to their slots (area bytes only), so a segment
 * sees the ring as earlier calls left it even where this call's stores replace what it reads.
 * Segments ascend and are disjoint.  flags: 1 = CONTINUE, start from the state's accumulators (what an earlier call's last segment
 * left there) instead of from `first` alone: only the first segment may; 2 = EMIT, write the composite of the segment (mode 0 mn,
 * 1 mx, 2 the mean (2 sm + frames) / (2 frames) with `frames` = all frames folded into this picture, earlier calls included,
 * 1..4194304) to patch `out`: d_out + out * out_stride, rows `out_pitch` bytes apart, exactly the 3 area_w bytes of each row.  Only
 * the last segment may lack EMIT: its mn / mx / sm are then left in the accumulators for a later CONTINUE; after a call whose last
 * segment EMITs their content is unspecified.  Nothing advances implicitly: the same batch may be passed again with the same fed
 * and n (more segments than the maximum); stores are idempotent.
 * Loads as vse_interval_accumulate's (16-byte ones where area start, pitch and frame stride allow, the aligned dwords around the
 * area's bytes otherwise); ring slots are always 16-byte aligned.  At most one launch on `stream`, no allocation, no device sync,
 * no atomics.
 * Returns VSE_E_INVAL, without touching the device, for everything vse_interval_accumulate refuses about frames, pitch, stride and
 * area (a NULL d_bgr only for n > 0; n outside 0..65535), cap < 1, fed negative or above 2^62 (fed + n must not overflow), nseg outside 0..VSE_INTERVAL_STREAM_MAX_SEGS, a segment with
 * first > last or first < 1, out of order, or with a frame outside (fed - cap, fed + n], CONTINUE on a segment other than the first, a segment
 * without EMIT that is not the last, unknown flag bits, mode outside 0..2, with an EMIT: a NULL d_out, a negative `out`, out_pitch
 * < 3 area_w, and with mode 2 `frames` outside 1..4194304; or a state that is not 16-byte aligned. */
typedef struct {
    int64_t first, last;   /* absolute 1-based frame numbers, inclusive, first <= last */
    int32_t flags;         /* VSE_INTERVAL_SEG_CONTINUE | VSE_INTERVAL_SEG_EMIT */
    int32_t frames;        /* EMIT with mode 2: the frames folded into this picture, earlier calls included */
    int32_t out;           /* EMIT: the patch written */
} vse_interval_seg;
#define VSE_INTERVAL_SEG_CONTINUE 1
#define VSE_INTERVAL_SEG_EMIT 2
#define VSE_INTERVAL_STREAM_MAX_SEGS 32
/* vse_interval_state_bytes(area_h, area_w) + cap ring slots of area_h rows padded to 16 bytes; 0 for an empty area or cap < 1. */
size_t vse_interval_stream_state_bytes(int area_h, int area_w, int cap);
int vse_interval_stream(vse_ctx* ctx, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride,
                        int y0, int y1, int x0, int x1, void* d_state, int cap, int64_t fed,
                        const vse_interval_seg* segs /* host, [nseg] */, int nseg, int64_t store_from, int mode /* 0 min, 1 max, 2 mean */,
                        void* d_out, int64_t out_pitch, int64_t out_stride, void* stream);
/* vse_interval_rank on frames that wait in the ring of a vse_interval_stream state, so a subtitle's quantile picture
 * (vse_amd.frame_select.StreamingQuantile) is made in the selector's own pass, without a second look at frames already gone: a call
 * of vse_interval_stream with nseg = 0 and store_from = fed + 1 parks a whole batch, and once a subtitle's end is known its samples
 * are ranked where they lie.  d_state: a state of vse_interval_stream_state_bytes(area_h, area_w, cap); only its ring is read, and
 * neither the accumulators nor the ring are written.  `fed`: the frames of the clip stored so far, as the next vse_interval_stream
 * call would be told.  For each of the 0 <= ngroups <= VSE_INTERVAL_RING_MAX_GROUPS groups and every byte b of the area: the n
 * values ring[frames[k] % cap][b] sorted ascending, element `rank` -> patch `out`: d_out + out * out_stride, rows `out_pitch` bytes
 * apart, exactly the 3 area_w bytes of each row: the bytes vse_interval_rank gives for the same frames laid out contiguously.
 * Every named frame must lie in (fed - cap, fed] and be one that an earlier call stored and no later store has replaced: the caller
 * keeps that book, the library checks only the numbers.  Patches of one call must not overlap.
 * Slot rows are 16-byte aligned, so every load is one aligned dword.  One launch on `stream` for all groups (none for ngroups = 0,
 * which returns VSE_OK), no allocation, no device sync, no atomics; the groups travel as kernel arguments.
 * Returns VSE_E_INVAL, without touching the device, for a NULL context, state or d_out, a state that is not 16-byte aligned, an area
 * that vse_interval_stream_state_bytes sizes as 0, cap < 1, fed negative or above 2^62, ngroups outside
 * 0..VSE_INTERVAL_RING_MAX_GROUPS, n outside 1..VSE_INTERVAL_RANK_MAX, rank outside 0..n - 1, frames that do not ascend strictly or
 * lie outside (fed - cap, fed] (or below 1), a negative `out`, or out_pitch < 3 area_w. */
#define VSE_INTERVAL_RING_MAX_GROUPS 8
typedef struct {
    int32_t n;        /* 1..VSE_INTERVAL_RANK_MAX samples */
    int32_t rank;     /* 0..n-1 */
    int32_t out;      /* patch written: d_out + out * out_stride */
    int64_t frames[VSE_INTERVAL_RANK_MAX];   /* absolute 1-based frame numbers, strictly ascending */
} vse_interval_ring_group;
int vse_interval_ring_rank(vse_ctx* ctx, const void* d_state, int area_h, int area_w, int cap, int64_t fed,
                           const vse_interval_ring_group* groups /* host, [ngroups] */, int ngroups,
                           void* d_out, int64_t out_pitch, int64_t out_stride, void* stream);

/* ---- timeline sync: audio template search ----------------------------------------------------------------------------- */
/* Replaces: Sushi's WavStream.find_substream (backend/sushi/wav.py:179-189), cv2.matchTemplate(TM_SQDIFF_NORMED) of one group's
 * source audio against a window of the destination audio.  Both streams are uint8.  A query takes the pattern
 * p = src[src_off, src_off + m) and the window w = dst[dst_off, dst_off + win_len), n = win_len - m + 1 offsets; for every k < n:
 *   X_k = sum p[i] w[k+i], S_k = sum w[k+i]^2, P = sum p[i]^2                 (exact integers)
 *   num = (double) max(S_k - 2 X_k + P, 0), den = sqrt((double) S_k) * sqrt((double) P)
 *   v_k = (float)(num / den) if num < den, else 1.0f (so den == 0 gives 1)
 * and the result is the first k of the smallest v_k with v_k itself.  cv2 computes the same value with a float32 DFT cross term
 * and a meanStdDev template norm, so its last bits and its argmin on near-ties can differ. */
typedef struct {
    int64_t src_off, m, dst_off, win_len;
} vse_audio_query;
typedef struct {
    int32_t index;
    float value;
} vse_audio_match_result;
/* Workspace bytes vse_audio_match needs for these nq queries (0 when one of them is invalid). */
size_t vse_audio_match_workspace_bytes(const vse_audio_query* queries, int nq);
/* 1 <= nq <= 3 host-side queries -> d_out[nq] (device, 8-byte aligned), in two launches on `stream`, with no device sync and no
 * allocation.  d_ws: at least vse_audio_match_workspace_bytes of these queries, 256-byte aligned.  Returns VSE_E_INVAL, and
 * launches nothing, when m < 1, a window is shorter than its pattern, a range lies outside its stream, nq is not in 1..3 or
 * the workspace is too small. */
int vse_audio_match(vse_ctx* ctx, const uint8_t* d_src, int64_t src_len, const uint8_t* d_dst, int64_t dst_len,
                    const vse_audio_query* queries, int nq, void* d_ws, size_t ws_bytes, vse_audio_match_result* d_out, void* stream);

/* ---- timeline sync: WAV PCM -> uint8 search stream ------------------------------------------------------------------------ */
/* Replaces: Sushi's WavStream.__init__ and what it calls (backend/sushi/wav.py:17-165): the WAV is read one second at a time,
 * downmixed, resampled to the search rate by nearest index, padded with 10 s of the FILE's rate on each side, clipped to 3 x the
 * medians of its non-negative and non-positive samples and scaled to 0..255.  Here the int16 PCM goes to the device as it is and
 * the uint8 stream of vse_audio_match is built there, byte for byte the host's (vse_amd.timeline_sync.AudioStream).  Input: F =
 * `frames` frames of C = `channels` interleaved int16 values at R = `rate` Hz; S = `sample_rate` <= R is the search rate.
 *   ratio = S / (double)R, sample_count = ceil(F / (double)R * S), P = 10 R (counted at the file's rate: Sushi's quirk),
 *   L = 20 R + sample_count, K = ceil(F / R) chunks of one second;
 *   chunk k has n_k = min(R, F - k R) frames and gives new_k = rint(n_k * ratio) samples (the product in double, ties to even) at
 *     at_k = P + k S; every full chunk gives S;
 *   a sample is the exact integer s = the sum over the channels of its frame's int16 values; sample j of chunk k takes frame j
 *     when S == R, else frame min((int64)floor((double)j * scale_k), n_k - 1), scale_k = 1.0 / ((double)new_k / (double)n_k),
 *     all in double (cv2.resize's INTER_NEAREST index rule);
 *   the chunk lengths can sum to one short of sample_count: that element is 0;
 *   data[0:P] = data[P], data[L-P:L] = data[L-P-1] (which can be that zero);
 *   f(s) = (float)s for C == 1, else (float)s / (float)C, a correctly rounded float32 divide; f is monotone;
 *   hi = 3 m({s >= 0}), lo = 3 m({s <= 0}) over all L elements (zeros count in both sets), m of a set of n elements in ascending
 *     order: f(element n / 2) for odd n, else (f(element n / 2 - 1) + f(element n / 2)) rounded to float32, then / 2; the
 *     product with 3 rounded to float32;
 *   out[i] = (uint8)(((min(max(f(s_i), lo), hi) - lo) / (hi - lo)) * 255.0f + 0.5f): four float32 operations, each rounded on
 *     its own (no fused multiply-add, hi - lo rounded once), the conversion truncates.
 * The medians are exact order statistics: one counting pass into 65535 C + 1 uint32 bins and one scan over the bins.
 * vse_audio_stream_length: L.  vse_audio_stream_workspace_bytes: the bytes of the caller-owned workspace (the int32 samples and
 * the bins; 256-byte aligned, no particular content beforehand).  Both return 0 for what feed and finish refuse: channels
 * outside 1..8, rate < sample_rate, frames < 1, L > 2^31 - 1. */
typedef struct {
    uint32_t lo_bits, hi_bits;       /* lo and hi as float32 bits (a quiet NaN for an empty set) */
    uint32_t count_ge0, count_le0;   /* sizes of the two sets */
    int32_t status;                  /* 0 ok; 1: a set is empty or hi - lo == 0 (the host's "silence"), the stream is not written */
    int32_t reserved[3];
} vse_audio_stream_result;
int64_t vse_audio_stream_length(int64_t frames, int channels, int rate, int sample_rate);
size_t vse_audio_stream_workspace_bytes(int64_t frames, int channels, int rate, int sample_rate);
/* One piece of the file's PCM -> the int32 samples of its chunks in the workspace: d_pcm (device, 2-byte aligned) holds
 * piece_frames frames that start at second `first_second` of the file.  A piece is a whole number of seconds; only the piece that
 * ends the file may end in its partial second.  Pieces may come in any order of calls on one stream, each chunk exactly once, so a
 * long file goes through two staging buffers.  The workspace keeps nothing else between calls: it needs no begin or reset and
 * serves the next file as it is.  One launch on `stream`, no allocation, no device sync; a 4-byte aligned piece of an even channel
 * count takes 4-byte loads, and on the copy path (S == R) of mono / stereo a piece whose groups of four frames are 8- / 16-byte
 * aligned takes one load per group.
 * Returns VSE_E_INVAL, and launches nothing, for the arguments above, a workspace that is too small or not 256-byte aligned, a
 * piece that is empty, outside the file, or not whole seconds and not the file's end, and, when S != R, a last chunk with
 * new_k == 0 (the host's "too few to resample"). */
int vse_audio_stream_feed(vse_ctx* ctx, const int16_t* d_pcm, int64_t piece_frames, int64_t first_second, int64_t frames, int channels,
                          int rate, int sample_rate, void* d_ws, size_t ws_bytes, void* stream);
/* After every chunk was fed on `stream` (or before it in stream order): counts, selects lo and hi, writes the result record
 * d_result (device, 4-byte aligned) and, when its status is 0, the L bytes of d_out (device, any alignment; a 16-byte aligned
 * one takes whole 16-byte stores).  A clear of the bins and three launches on `stream`, no allocation, no device sync.
 * Returns VSE_E_INVAL, and launches nothing, for what vse_audio_stream_feed refuses of the same arguments. */
int vse_audio_stream_finish(vse_ctx* ctx, int64_t frames, int channels, int rate, int sample_rate, void* d_ws, size_t ws_bytes,
                            uint8_t* d_out, vse_audio_stream_result* d_result, void* stream);

/* ---- timeline sync: scene cuts for keyframe snapping ------------------------------------------------------------------- */
/* Replaces: the keyframes Sushi makes by piping the video through ffmpeg (scale=640:360) into SCXvid, an XviD first pass whose
 * I-frame decisions mark the scene cuts (backend/sushi/demux.py:113-135).  Not XviD's algorithm but the same role: per frame, how
 * many 16 x 16 macroblocks of a small luma plane the previous frame cannot predict within a search range; the host turns the
 * counts into keyframes (vse_amd.keyframes.SceneCutDetector).  All integer arithmetic:
 *   Y = (29 B + 150 G + 77 R + 128) >> 8;
 *   plane A[y][x] = (sum of the scale x scale luma box at (y scale, x scale) + scale scale / 2) / (scale scale), of
 *     ah = src_h / scale rows and aw = src_w / scale columns (source rows / columns beyond ah scale / aw scale are not read);
 *   macroblocks: bh = ah / 16 by bw = aw / 16 (plane rows / columns beyond them belong to no block but are reference pixels);
 *   inter_b = min over (dy, dx) in [-search, search]^2 of sum |A_t[16 by + y][16 bx + x] - P[16 by + dy + y][16 bx + dx + x]|,
 *     P = the plane of frame t - 1, over the vectors whose displaced block lies wholly inside the plane;
 *   m_b = (sum A_t + 128) >> 8, intra_b = sum |A_t - m_b|; block b is changed iff 2 inter_b > intra_b + bias;
 *   d_counts[t] = (changed blocks, sum_b inter_b, sum_b intra_b); a frame without a predecessor gives (bh bw, 0, sum_b intra_b).
 * d_state (vse_scene_change_state_bytes, 8-byte aligned, fresh = zero-filled) holds a flag and the last frame's plane after the
 * call, and the first frame of the next call is compared with it: batches of any size give the counts of one batch.  With
 * `reset`, or on a fresh state, the first frame has no predecessor.  d_ws (vse_scene_change_workspace_bytes, 4-byte aligned)
 * holds the planes of the call.  Three launches on `stream`, no allocation, no device sync.
 * Returns VSE_E_INVAL, and launches nothing, when scale is not in 1..8, search not in 0..8, bias not in 0..65535, ah or aw < 16,
 * aw ah > 2^23 (the int32 sums stay exact below it), n is not in 1..65535 or the workspace is too small.
 * The two size functions return 0 for a frame size and scale the call would refuse. */
size_t vse_scene_change_state_bytes(int src_h, int src_w, int scale);
size_t vse_scene_change_workspace_bytes(int n, int src_h, int src_w, int scale);
int vse_scene_change(vse_ctx* ctx, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride, int scale,
                     int search, int bias, void* d_state, int reset, void* d_ws, size_t ws_bytes,
                     int32_t* d_counts /* [n,3]: changed blocks, sum inter, sum intra */, void* stream);

/* ---- frame ingest: YUV 4:2:0 -> BGR ------------------------------------------------------------------------------------------ */
/* Replaces: the colour conversion inside the reference's decoder, cv2.VideoCapture.read() (backend/main.py:228-376 sequentially,
 * backend/tools/subtitle_ocr.py:173-204 by seeking), where FFmpeg's swscale turns the codec's yuv420p pictures into the BGR frame
 * the callers get.  Here the decoder's 4:2:0 bytes are uploaded as they are (1.5 instead of 3 bytes per pixel) and converted on
 * the device.  BT.601 limited range, nearest chroma (no interpolation, siting ignored), the fixed-point constants of
 * cv2.cvtColor(COLOR_YUV2BGR_I420 / _NV12); swscale's chroma up-sampling filter differs, so these are not swscale's bits.
 * All arithmetic int32, >> arithmetic, clip8(x) = min(max(x, 0), 255):
 *   Y = luma[r][x], U and V from chroma row (r + row_parity) >> 1 and column x >> 1;
 *   c = max(Y - 16, 0) * 1220542, u = U - 128, v = V - 128;
 *   B = clip8((c + 2116026 u + 2^19) >> 20), G = clip8((c - 409993 u - 852492 v + 2^19) >> 20), R = clip8((c + 1673527 v + 2^19) >> 20).
 * A packed (sub-)frame: h luma rows of w bytes, then ch = (h + row_parity + 1) >> 1 chroma rows of cw = (w + 1) >> 1 samples:
 * layout 0 (I420) a U plane then a V plane, each ch x cw bytes; layout 1 (NV12) one plane of ch rows of 2 cw bytes, U then V.
 * row_parity = 1 describes a band of rows that starts on an odd luma row of its frame (its first luma row is the SECOND row of
 * its first chroma row), so a host can upload any band of rows without touching the rest of the frame.
 * vse_yuv420_frame_bytes: that packed size; 0 for arguments vse_yuv420_to_bgr would refuse. */
size_t vse_yuv420_frame_bytes(int h, int w, int row_parity);
/* n packed frames at d_yuv, yuv_frame_stride bytes apart -> uint8 BGR [n, h, w, 3] at d_bgr (row pitch `pitch` bytes, frame stride
 * bgr_frame_stride bytes).  One launch on `stream`, no allocation, no device sync; writes exactly the w * 3 bytes of each of the
 * h rows of each frame (padding between rows and frames is never written).  No alignment is required; 16-byte aligned bases,
 * pitch and strides with w % 16 == 0, even h and row_parity 0 take the 16-byte load / store kernel.
 * Returns VSE_E_INVAL, and launches nothing, when h, w or n < 1, h * w > 2^31 - 1, layout or row_parity is not 0 | 1,
 * pitch < 3 w, yuv_frame_stride < vse_yuv420_frame_bytes or bgr_frame_stride < (h - 1) pitch + 3 w. */
int vse_yuv420_to_bgr(vse_ctx* ctx, const void* d_yuv, int n, int h, int w, int layout /* 0 = I420, 1 = NV12 */,
                      int row_parity /* 0 | 1 */, int64_t yuv_frame_stride, void* d_bgr, int64_t pitch, int64_t bgr_frame_stride,
                      void* stream);
/* vse_yuv420_to_bgr with the colour matrix chosen: matrix 0 = BT.601 (the call above: the same launcher, the same bytes), 1 = BT.709
 * limited range, what HD encodes normally carry.  The same c, rounding term, shift, clip8, chroma sampling, layouts and kernels:
 *   B = clip8((c + 2215014 u + 2^19) >> 20), G = clip8((c - 223607 u - 558796 v + 2^19) >> 20), R = clip8((c + 1879825 v + 2^19) >> 20),
 * the factors round(k 2^20) of 2 (1 - Kb) 255/224, 2 Kb (1 - Kb) / Kg 255/224, 2 Kr (1 - Kr) / Kg 255/224 and 2 (1 - Kr) 255/224 with
 * Kr = 0.2126, Kb = 0.0722, Kg = 1 - Kr - Kb.  Luma-only pictures (U = V = 128) come out identical under both matrices.
 * Returns VSE_E_INVAL, and launches nothing, for what vse_yuv420_to_bgr refuses and for a matrix that is not 0 | 1. */
int vse_yuv_to_bgr_matrix(vse_ctx* ctx, const void* d_yuv, int n, int h, int w, int layout /* 0 = I420, 1 = NV12 */,
                          int row_parity /* 0 | 1 */, int64_t yuv_frame_stride, void* d_bgr, int64_t pitch, int64_t bgr_frame_stride,
                          int matrix /* 0 = BT.601, 1 = BT.709 */, void* stream);

/* ---- frame ingest: any planar / semi-planar YUV -> BGR --------------------------------------------------------------------------- */
/* What else a decoder hands out, converted by the same kind of integers, so that nothing is converted on the host in front of the pipe:
 * 10-bit (HEVC Main10, Hi10P) and deeper, 4:2:2, 4:4:4, grey, full range (phone video, screen recordings, yuvj420p), BT.2020, and P010,
 * the surface of a hardware decoder.  A format is plain integers:
 *   sub_x, sub_y   log2 chroma subsampling: 0, 0 (4:4:4) | 1, 0 (4:2:2) | 1, 1 (4:2:0)
 *   chroma         0 none (grey; sub_x = sub_y = 0) | 1 planar, U then V | 2 interleaved U V (semi-planar; 4:2:0 only: NV12, P010)
 *   depth          8..16; depth 8 has 1-byte samples, 9..16 2-byte little-endian ones
 *   msb            0: the value in the low bits, a word above 2^depth - 1 is clamped to it (yuv420p10le, Y4M); 1: in the high bits,
 *                  value = word >> (16 - depth) (P010 / P012 / P016); 0 at depth 8
 *   matrix         0 BT.601 | 1 BT.709 | 2 BT.2020 non-constant luminance;   full_range 0 | 1
 * With s = depth - 8, U and V of chroma row (r + row_parity) >> sub_y and column x >> sub_x (nearest, no interpolation), int32, >>
 * arithmetic:
 *   limited: c = max(Y - (16 << s), 0) * KY_s;   full: c = Y * (2^20 >> s);   u = U - (128 << s), v = V - (128 << s) (grey: u = v = 0)
 *   B = clip8((c + BU_s u + 2^19) >> 20), G = clip8((c + GU_s u + GV_s v + 2^19) >> 20), R = clip8((c + RV_s v + 2^19) >> 20)
 *   K_s = sign(K_0) * ((|K_0| + ((1 << s) >> 1)) >> s)
 * K_0 (KY; BU, GU, GV, RV): limited BT.601 and BT.709 the numbers of the two entries above (at s = 0 this is their formula, bit for
 * bit), limited BT.2020 1220542; 2245811, -196426, -682019, 1760217 (BT.709's derivation with Kr = 0.2627, Kb = 0.0593); full range
 * round(k 2^20) of 2 (1 - Kb), -2 Kb (1 - Kb) / Kg, -2 Kr (1 - Kr) / Kg, 2 (1 - Kr), without 255/224: BT.601 1858077, -360853, -748826,
 * 1470104; BT.709 1945738, -196424, -490864, 1651297; BT.2020 1972791, -172546, -599107, 1546230.
 * NO transfer function is applied here: PQ / HLG material comes out flat (dim, low contrast); its text and edges remain.
 * vse_yuv_to_bgr_tonemap below is the conversion for such material.
 * A packed (sub-)frame of luma rows [y0, y1): h = y1 - y0 rows of w samples, then chroma rows y0 >> sub_y .. ((y1 - 1) >> sub_y) + 1,
 * that is ch = ((h - 1 + row_parity) >> sub_y) + 1 rows of cw = (w + sub_x) >> sub_x samples per plane (planar: U plane, V plane;
 * semi-planar: one plane of rows of 2 cw samples), row_parity = y0 & sub_y.  For 8-bit 4:2:0 this is vse_yuv420_to_bgr's.
 * vse_yuv_frame_bytes: that packed size in bytes; 0 for arguments vse_yuv_to_bgr_format would refuse. */
size_t vse_yuv_frame_bytes(int h, int w, int sub_x, int sub_y, int chroma, int depth, int row_parity);
/* n packed frames at d_yuv, yuv_frame_stride bytes apart -> uint8 BGR [n, h, w, 3] at d_bgr, as vse_yuv420_to_bgr: one launch on
 * `stream`, no allocation, no device sync, exactly the w * 3 bytes of each row written.  8-bit 4:2:0 limited BT.601 / BT.709 runs
 * vse_yuv_to_bgr_matrix's kernels and gives its bytes.  2-byte 4:2:0, planar or semi-planar, takes a 16-byte load / store kernel
 * under vse_yuv420_to_bgr's conditions (16-byte aligned bases, pitch and strides, w % 16 == 0, even h, row_parity 0); everything else
 * a kernel without conditions, except that 2-byte samples need a 2-byte aligned d_yuv and yuv_frame_stride.
 * Returns VSE_E_INVAL, with the values in vse_last_error, and launches nothing, for a format outside the table above, h, w or n < 1,
 * h * w > 2^31 - 1, row_parity outside 0..sub_y, that misalignment, pitch < 3 w, yuv_frame_stride < vse_yuv_frame_bytes or
 * bgr_frame_stride < (h - 1) pitch + 3 w. */
int vse_yuv_to_bgr_format(vse_ctx* ctx, const void* d_yuv, int n, int h, int w, int sub_x, int sub_y, int chroma, int depth, int msb,
                          int matrix, int full_range, int row_parity, int64_t yuv_frame_stride, void* d_bgr, int64_t pitch,
                          int64_t bgr_frame_stride, void* stream);

/* ---- frame ingest: HDR (PQ / HLG) YUV -> SDR BGR ----------------------------------------------------------------------------------- */
/* UHD Blu-ray and streaming masters are PQ (SMPTE ST 2084), UHD broadcast is HLG (BT.2100), both normally 10-bit BT.2020: converted by
 * vse_yuv_to_bgr_format they come out flat and desaturated.  This is that conversion with a transfer function, a tone curve and a gamut
 * change behind it, all of them DATA: the device applies two tables and nine integers that the host builds (vse_amd.ingest.ToneMap) and
 * knows nothing of PQ, HLG or curves, so its bytes are defined by exact integers like every other conversion here.
 * The format table, shift, 2^depth - 1, the offsets, KY_s .. RV_s, the chroma sampling (nearest), row_parity and the packed layout are
 * vse_yuv_to_bgr_format's.  All arithmetic int32, >> arithmetic, clip(lo, hi, x) = min(max(x, lo), hi):
 *   u = U - (128 << s), v = V - (128 << s)  (grey: u = v = 0);   c = max(Y - yoff, 0) * KY_s + 2^15
 *   E_B = clip(0, 4095, (c + BU_s u) >> 16), E_G = clip(0, 4095, (c + GU_s u + GV_s v) >> 16), E_R = clip(0, 4095, (c + RV_s v) >> 16)
 *                                                 the R'G'B' code at 12 bits: vse_yuv_to_bgr_format's sums, nominal peak 4080 = 255 << 4
 *   L_k = A[E_k]                                  A: uint16[4096], linear light behind the tone curve, 65535 = SDR white
 *   P_r = clip(0, 65535, (M[r][0] L_R + M[r][1] L_G + M[r][2] L_B + 2^13) >> 14)       r = R, G, B;  M: int32[3][3], Q14, linear light
 *   out_r = T[P_r < 4096 ? P_r : 3840 + (P_r >> 4)]
 *                                                 T: uint8[7936], the output gamma: every P below 4096 (its steep foot), every 16th above
 * and the bytes are stored B, G, R.  The positive entries of each row of M sum to at most 32767 and the negative ones to at least -32768:
 * then every partial sum lies within [-32768 * 65535, 32767 * 65535 + 2^13] and int32 is exact.
 * vse_yuv_tonemap_table_bytes: 4096 * 2 + 7936 = 16128, the table as the device takes it: A (little-endian uint16), then T. */
size_t vse_yuv_tonemap_table_bytes(void);
/* vse_yuv_to_bgr_format with the arithmetic above: one launch on `stream`, no allocation, no device sync, exactly the w * 3 bytes of each
 * row written.  d_table: the 16128 bytes on the device, 16-byte aligned, read by the launch (keep them until it has run); gamut: M, nine
 * integers on the host, row-major, rows R G B over columns R G B, read before the call returns.  Every block copies the table into LDS
 * once and gathers from there.  2-byte 4:2:0, planar or semi-planar, takes the 16-byte load / store kernel under vse_yuv420_to_bgr's
 * conditions, everything else (8-bit 4:2:0 included) the kernel without conditions.
 * Returns VSE_E_INVAL, with the values in vse_last_error, and launches nothing, for everything vse_yuv_to_bgr_format refuses, a NULL
 * d_table or one that is not 16-byte aligned, a NULL gamut, and a gamut row outside the bounds above. */
int vse_yuv_to_bgr_tonemap(vse_ctx* ctx, const void* d_yuv, int n, int h, int w, int sub_x, int sub_y, int chroma, int depth, int msb,
                           int matrix, int full_range, int row_parity, int64_t yuv_frame_stride, void* d_bgr, int64_t pitch,
                           int64_t bgr_frame_stride, const void* d_table /* device, 16-byte aligned */,
                           const int32_t* gamut /* host, 9 integers, row-major, rows R G B over columns R G B */, void* stream);

/* ---- frame ingest: interlaced YUV -> progressive YUV ------------------------------------------------------------------------------ */
/* DVDs, 576i / 480i captures and 1080i broadcasts carry two fields of different times woven into one picture.  This turns n packed
 * pictures of any format of vse_yuv_to_bgr_format's table into progressive pictures of the same format and layout
 * (vse_yuv_frame_bytes(h, w, ..., row_parity 0)), which the conversions above then take unchanged.  Motion-adaptive: what did not change
 * since the previous picture is woven (a subtitle keeps its full vertical resolution), what did is interpolated from the first field.
 * The rule is applied to every plane on its own (Y, U, V, or the interleaved UV plane; the samples as stored words, no clamp), up and
 * down a column only; row 0 of every plane is a top-field row.  For a plane of R rows, C the picture, P the previous picture:
 *   out[y] = C[y]                        where y & 1 == keep (keep: the parity of the rows of the field first in time; top field first:
 *                                        0), and for every y when R == 1
 *   otherwise moved[x] = d_prev is NULL, or mode == 1, or |C[r][x] - P[r][x]| > T for any r of {y - 1, y, y + 1} inside [0, R)
 *             a = C[y - 1] if y >= 1 else C[y + 1];   b = C[y + 1] if y + 1 < R else C[y - 1]
 *             out[y][x] = moved[x] ? (a[x] + b[x] + 1) >> 1 : C[y][x]
 *   T = thresh << (depth - 8), and << (16 - depth) more when msb = 1: thresh is in 8-bit levels.
 * Picture f is at d_yuv + f yuv_frame_stride, its previous picture at d_prev + f prev_frame_stride, its result at d_out + f
 * out_frame_stride: a run of consecutive frames passes d_prev = d_yuv - yuv_frame_stride and the same stride (the picture in front of
 * the run must then be there), scattered frames are laid out as (previous, current) pairs with both strides doubled.  d_prev NULL: no
 * frame has a previous picture, every frame is interpolated throughout.  One output frame per input frame.
 * One launch on `stream`, no allocation, no device sync, exactly the packed bytes of each picture written.  A kernel of 16-byte loads and
 * stores runs when every plane's base and row bytes and all frame strides are 16-byte aligned; otherwise one without conditions, except
 * that 2-byte samples need 2-byte aligned bases and strides.
 * Returns VSE_E_INVAL, with the values in vse_last_error, and launches nothing, for a format outside the table, keep or mode outside
 * 0 | 1, thresh outside 0..255, n, h or w < 1, h * w > 2^31 - 1, a frame stride below the packed size (prev_frame_stride only with
 * d_prev), 2-byte samples at an odd base or stride, or d_out equal to d_yuv or d_prev (the pictures must not overlap the output). */
int vse_yuv_deinterlace(vse_ctx* ctx, const void* d_yuv, const void* d_prev /* NULL: no frame has a previous picture */, int n, int h, int w,
                        int sub_x, int sub_y, int chroma, int depth, int msb, int keep /* 0 | 1 */, int mode /* 0 adaptive | 1 interpolate */,
                        int thresh /* 8-bit levels, 0..255 */, int64_t yuv_frame_stride, int64_t prev_frame_stride, void* d_out,
                        int64_t out_frame_stride, void* stream);

/* ---- frame ingest: film carried in interlaced video -> the film's pictures (field matching) ----------------------------------------- */
/* Much interlaced material is progressive film whose fields were dealt into interlaced frames: 3:2 pulldown (NTSC DVDs, 480i, 1080i60),
 * or fields shifted by one (mostly PAL).  Every picture of the film is still in the stream, whole; its second field merely sits in the
 * neighbouring frame.  This call weaves each frame's fields with the partner that combs least and so gives the film's pictures back
 * byte for byte, without a per-sample threshold; a frame that combs with every partner is video and gets vse_yuv_deinterlace's adaptive
 * rule.  One output frame per input frame (the duplicate of a pulldown cycle stays in), no lookahead, no cadence, one choice per frame.
 * Layouts, formats and `keep` are vse_yuv_deinterlace's.  Per frame, C the picture, P the previous one, R luma rows, w columns:
 *   candidates   each a whole picture; every plane follows the same choice, row by row of that plane (row 0 of a plane is a top-field row)
 *     choice 0  c    every row from C
 *     choice 1  p1   rows of parity keep from C, the other rows from P     (the frame's first field with the previous frame's second)
 *     choice 2  p2   rows of parity keep from P, the other rows from C     (the frame's second field with the previous frame's first)
 *   comb count   on the luma plane of a candidate W alone, the samples as stored words: for every row 1 <= y <= R - 2 and every column
 *                d1 = W[y] - W[y - 1], d2 = W[y] - W[y + 1];  combed iff (d1 > T and d2 > T) or (d1 < -T and d2 < -T)   (strict)
 *                T = comb_thresh << (depth - 8), and << (16 - depth) more when msb = 1.  The count is the number of combed samples;
 *                R < 3 counts 0 for every candidate.  |d| < 2^16 and T <= 255 << 8: int32 is exact; a count is at most 2^31 - 1.
 *   choice       the smallest count; ties go to c, then p1, then p2.  d_prev NULL: only c exists.
 *   fallback     when comb_limit >= 0 and best * 1000 > comb_limit * w * (R - 2), in 64 bits (best: the chosen candidate's count), the frame
 *                is video: choice 3, and its output is exactly what vse_yuv_deinterlace makes of it in mode adaptive with the same keep
 *                and `thresh` (d_prev NULL: every sample interpolated).  comb_limit < 0 never falls back.  (R = 1 makes the right side
 *                negative: choice 3, whose output is C, as choice 0's.)
 * comb_thresh 10 and comb_limit 20 per mille are the host's defaults; both are conventions and guesses, nothing is measured on real
 * footage.  The counts are taken over the luma rows of the picture handed in: a caller that hands in a band of rows gets the band's choice.
 * d_stats: uint32[n][4] on the device: the counts of c, p1 and p2 (0 for p1 and p2 with d_prev NULL) and the choice 0..3.
 * Everything is enqueued on `stream`: the call zeroes d_stats itself, a count kernel reads the luma of C and P once (16-byte columns where
 * the luma base, row bytes and the input strides are 16-byte aligned, 4 samples otherwise) and adds per-wave integer sums into d_stats
 * with atomics, and a weave kernel, which derives the choice from the counts in every block, writes the pictures; each plane on its own
 * takes 16-byte moves where its base and row bytes and all strides are 16-byte aligned (the 720-byte luma rows of a DVD do, its
 * 360-byte chroma rows do not), dwords or single samples otherwise.  No allocation, no device sync; exactly the packed bytes of each
 * picture and the 16 n bytes of d_stats are written; the inputs are only read.
 * Returns VSE_E_INVAL, with the values in vse_last_error, and launches nothing, for everything vse_yuv_deinterlace refuses (it has no
 * mode), a NULL d_stats or one that is not 4-byte aligned, comb_thresh outside 0..255, comb_limit above 1000, and a d_stats that overlaps
 * the pictures (from the first byte of the first to the last byte of the last picture of d_yuv, d_prev or d_out). */
int vse_yuv_field_match(vse_ctx* ctx, const void* d_yuv, const void* d_prev /* NULL: no frame has a previous picture */, int n, int h, int w,
                        int sub_x, int sub_y, int chroma, int depth, int msb, int keep /* 0 | 1 */, int comb_thresh /* 8-bit levels, 0..255 */,
                        int comb_limit /* per mille, < 0: never fall back */, int thresh /* the fallback's, 8-bit levels, 0..255 */,
                        int64_t yuv_frame_stride, int64_t prev_frame_stride, void* d_out, int64_t out_frame_stride,
                        void* d_stats /* device, uint32[n][4]: count c, p1, p2, choice 0..3 */, void* stream);

/* ---- frame ingest: anamorphic YUV -> square pixels (horizontal resample) ---------------------------------------------------------------- */
/* DVDs, HDV, DVCPRO HD and much 1080i broadcast store pixels that are not square: 720 columns shown as 854 (sample aspect ratio 32:27),
 * 1048 (16:11) or 640 (8:9), 1440 shown as 1920 (4:3).  This turns n packed pictures of any format of vse_yuv_to_bgr_format's table into
 * packed pictures of the same format and height whose rows are w_out columns long, every plane resampled along its rows; it stands behind
 * vse_yuv_deinterlace / vse_yuv_field_match (combing is a property of stored columns) and in front of the conversions, which take any
 * width.  Rows do not interact: a band of rows gives exactly the whole picture's rows.
 * The filter is DATA: the device knows tables, nothing of bicubic or Lanczos (vse_amd.ingest.Resample builds them).  A table for a plane
 * of P output columns and K taps (K even, 2..16) is left[P] (int32) followed by coef[P][K] (int16), P (4 + 2 K) bytes, 16-byte aligned.
 * For a plane of pw stored columns, every row and every output column x, int32, >> arithmetic:
 *   acc = sum over k < K of coef[x][k] * S[clamp(left[x] + k, 0, pw - 1)]
 *   out = clip(0, 2^depth - 1, (acc + 8192) >> 14)
 * S is the stored sample as a value: the word itself, or with msb = 1 the word >> (16 - depth), and the result is then stored
 * << (16 - depth).  Luma takes the luma table (w_in -> w_out columns), every chroma plane the chroma table (cw_in -> cw_out, cw = (w +
 * sub_x) >> sub_x); a semi-planar UV plane is a plane of cw columns of two components: entry x is applied to U at 2 (left + k) and to V
 * at 2 (left + k) + 1.  Grey has no chroma table.  The host guarantees sum over k of |coef[x][k]| <= 32767 for every x (ingest.Resample
 * and the Python binding check it; this call cannot read the device tables) and |left| <= 2^30: with 16-bit samples every partial sum
 * then stays below 2^31.  The table whose every row is one tap of 16384 at left[x] = x gives the input back (valid samples).
 * vse_yuv_resample_table_bytes: P (4 + 2 K) for `columns` = P and `taps` = K; 0 for columns < 1 or taps odd or outside 2..16. */
size_t vse_yuv_resample_table_bytes(int columns, int taps);
/* Picture f at d_yuv + f yuv_frame_stride (vse_yuv_frame_bytes(h, w_in, ..., row_parity) bytes) -> d_out + f out_frame_stride
 * (vse_yuv_frame_bytes(h, w_out, ...) bytes).  One launch on `stream`, no allocation, no device sync, no LDS; exactly the packed bytes of
 * each output picture are written, the inputs and the tables are only read (keep the tables until the launch has run).  A lane owns four
 * output samples of a strip of 8 rows with their table entries in registers and loads every source sample on its own, by its clamped
 * index, in both forms (no wide loads, no staging).  The forms differ in the store alone: where both pictures' bases, every plane's
 * row bytes and the frame strides are 16-byte aligned the four samples always go out as one 4-byte store (8-byte for 2-byte samples);
 * otherwise as a dword where they exist and lie 4-byte aligned and sample by sample where not; 2-byte samples need 2-byte aligned
 * bases and strides.
 * Returns VSE_E_INVAL, with the values in vse_last_error, and launches nothing, for a format outside the table, n, h, w_in or w_out < 1,
 * h * max(w_in, w_out) > 2^31 - 1, row_parity outside 0..sub_y, taps odd or outside 2..16 (taps_c only where the format has chroma), a NULL
 * or misaligned d_table_y, a NULL or misaligned d_table_c where the format has chroma, a frame stride below the packed size, 2-byte samples
 * at an odd base or stride, and a d_out whose pictures (first byte of the first to last byte of the last) overlap the input pictures or a table. */
int vse_yuv_resample(vse_ctx* ctx, const void* d_yuv, int n, int h, int w_in, int w_out, int sub_x, int sub_y, int chroma, int depth, int msb,
                     int row_parity, const void* d_table_y /* device, 16-byte aligned */, int taps_y,
                     const void* d_table_c /* device, 16-byte aligned; NULL for grey */, int taps_c, int64_t yuv_frame_stride, void* d_out,
                     int64_t out_frame_stride, void* stream);

/* ---- frame ingest: UHD and other oversized YUV -> fewer rows (vertical scale) ------------------------------------------------------------ */
/* The vertical counterpart of vse_yuv_resample: n packed pictures of any format of vse_yuv_to_bgr_format's table, h_in rows high, become
 * packed pictures of the same format and width that are h_out rows high, every plane filtered down (or up) its columns.  The order of the
 * ingest line is vertical, then horizontal (vse_yuv_resample), then the conversion, each pass rounding to the stored depth; the integers
 * depend on that order.  The device knows tables, not filters (vse_amd.ingest.VScale builds them).  A table for a plane of Q output rows
 * and K taps (K even, 2..16) is top[Q] (int32) followed by coef[Q][K] (int16, Q14): the layout of the horizontal table, so
 * vse_yuv_resample_table_bytes(Q, K) is its size; 16-byte aligned.  For a plane of ph stored rows, every column x and every output row y,
 * int32, >> arithmetic:
 *   acc = sum over k < K of coef[y][k] * S[clamp(top[y] + k, 0, ph - 1)][x]
 *   out = clip(0, 2^depth - 1, (acc + 8192) >> 14)
 * S the stored word, or with msb = 1 the word >> (16 - depth), the result then stored << (16 - depth).  Luma takes the luma table (h_in ->
 * h_out rows), every chroma plane the chroma table (ch_in -> ch_out, ch = (h + sub_y) >> sub_y); an interleaved UV plane is a plane of
 * 2 cw samples per row.  Grey has no chroma table.  The host guarantees sum over k of |coef[y][k]| <= 32767 for every y and |top| <= 2^30
 * (the Python binding checks both; this call cannot read the device tables).
 * ROW BANDS.  Input picture f, at d_yuv + f yuv_frame_stride, is the packed band of stored luma rows [s0, s1) of a picture of h_in rows:
 * row parity s0 & sub_y, chroma rows s0 >> sub_y .. ((s1 - 1) >> sub_y) + 1, vse_yuv_frame_bytes(s1 - s0, w, ..., s0 & sub_y) bytes.  The
 * output, at d_out + f out_frame_stride, is the packed band of output rows [y0, y1) of a picture of h_out rows: parity y0 & sub_y, chroma
 * rows y0 >> sub_y .. ((y1 - 1) >> sub_y) + 1.  Both tables are indexed in whole-picture rows.  A source row index is clamped to the
 * picture as above and then to the band handed in, so every load lies inside its input whatever the table says.  With a band that holds
 * every source row that rows [y0, y1) read with a coefficient other than zero, in every plane, the second clamp changes nothing: such a
 * band gives exactly the whole picture's rows, unconditionally.  This call cannot read the tables; the Python binding, which has them,
 * refuses a band that does not cover that support.
 * One launch on `stream`, no allocation, no device sync, no LDS; exactly the packed bytes of each output picture are written, the inputs
 * and the tables are only read (keep the tables until the launch has run).  A lane owns a run of one plane row and a wave makes one
 * output row at a time; top[y], the coefficients and the clamped source rows are the same in every lane of a wave.  Where both bases, both frame
 * strides and every plane's row bytes and plane offsets in both bands are 16-byte aligned the run is 16 bytes, loaded once per tap and
 * stored once; otherwise it is four samples, loaded and stored as dwords where they exist and lie aligned and sample by sample where not
 * (2-byte samples need 2-byte aligned bases and strides).
 * Returns VSE_E_INVAL, with the values in vse_last_error, and launches nothing, for a format outside the table, n, w, h_in or h_out < 1,
 * h_in * w or h_out * w > 2^31 - 1, a band that is empty or not inside its picture, taps odd or outside 2..16 (taps_c only where the
 * format has chroma), a NULL or misaligned d_table_y, a NULL or misaligned d_table_c where the format has chroma, a frame stride below
 * the packed size, 2-byte samples at an odd base or stride, and a d_out whose pictures (first byte of the first to last byte of the
 * last) overlap the input pictures or a table. */
int vse_yuv_vscale(vse_ctx* ctx, const void* d_yuv, int n, int w, int h_in, int h_out, int s0, int s1, int y0, int y1, int sub_x, int sub_y,
                   int chroma, int depth, int msb, const void* d_table_y /* device, 16-byte aligned */, int taps_y,
                   const void* d_table_c /* device, 16-byte aligned; NULL for grey */, int taps_c, int64_t yuv_frame_stride, void* d_out,
                   int64_t out_frame_stride, void* stream);

/* ---- colour key of the selectors' band (coloured subtitles) --------------------------------------------------------------------------- */
/* uint8 BGR frames [n, src_h, src_w, 3] (row pitch `pitch` bytes, frame stride `frame_stride` bytes) and the area [y0, y1) x [x0, x1)
 * (not empty, inside the frame; 1 x 1 is allowed) -> the same area of d_out, in the input's coordinates: pixel (y, x) of frame f is at
 * d_out + f out_frame_stride + y out_pitch + 3 x, so one `area` addresses both sides.  Exact integers:
 *   d = max(|B - key_b|, |G - key_g|, |R - key_r|);   K = max(0, 255 - ((d * slope) >> 8));   out pixel = (K, K, K)
 * The selectors' luma of (K, K, K) is K itself (29 + 150 + 77 = 256), so vse_frame_change and every other entry point that builds an edge
 * mask runs on the keyed frames unchanged: its gradient is K's.  The device knows integers, not tolerances: slope = ceil(255 * 256 / tol)
 * gives K = 255 at d = 0 and K = 0 from d = tol on (vse_amd.frame_select.ColourKey).
 * One launch on `stream`, no allocation, no device sync, no LDS.  Every pixel of the area is written.  The call may widen the columns to
 * 16-pixel boundaries inside [0, src_w) of the same rows, and what it writes there is the key of the pixel there; it reads and writes
 * nothing in rows outside [y0, y1), nothing beyond 3 * src_w bytes of a row and nothing outside the n frames, so a caller may pass the
 * area's rows alone, as with vse_frame_change.  The input is only read.  Where both bases, both pitches and (n > 1) both frame strides
 * are 16-byte aligned a lane owns 16 pixels (three 16-byte loads, three 16-byte stores); otherwise a lane owns one pixel of the area and
 * moves it byte by byte, at any alignment.  n == 0 is VSE_OK without a launch.
 * Returns VSE_E_INVAL, with the values in vse_last_error, and touches nothing on the device, for an empty or out-of-frame area, a key
 * component outside 0..255, slope outside 256..65280, a pitch below 3 * src_w on either side, n < 0, (n > 1) a frame stride below a
 * frame's bytes on either side, a NULL pointer with n > 0, and input and output byte ranges (rows [y0, y1) of the first frame to the
 * last frame) that overlap. */
int vse_colour_key(vse_ctx* ctx, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0,
                   int x1, int key_b, int key_g, int key_r, int slope, void* d_out, int64_t out_pitch, int64_t out_frame_stride,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VSE_HIP_H */
