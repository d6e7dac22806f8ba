// C-ABI runtime: context, weight arenas, plan creation and the op dispatch loop (see include/vse_hip.h).
#include <stdlib.h>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "conv_common.h"

static thread_local std::string g_err;
static void set_err(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}
void vse_set_error(const char* msg) { g_err = msg ? msg : ""; }
#define HIP_TRY(expr)                                                                  \
    do {                                                                               \
        hipError_t e_ = (expr);                                                        \
        if (e_ != hipSuccess) {                                                        \
            set_err("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return VSE_E_HIP;                                                          \
        }                                                                              \
    } while (0)

struct vse_ctx {
    int device;
    std::vector<void*> weights;       // device blobs
    std::vector<size_t> weight_bytes;
    void* zero_page;                  // 4 KiB of zeros (gather target for nothing yet; keeps pointers valid)
};

struct vse_plan {
    vse_ctx* ctx;
    int weights_id;
    std::vector<vse_op> ops;
    std::vector<ConvKernel> pooled;   // per op: family CK_C3POOL = this conv runs with the max-pool record behind it as one kernel (conv_pool_select)
    std::vector<ConvGap> gapped;      // per op: fused = this 1x1 conv sums the partials of the global-average pool record behind it (conv_gap_select)
    std::vector<int> scale_add;       // per op: != 0 = this OP_SCALE runs with the add record behind it as one pass (scale_add_select)
    size_t ws_bytes;
    int max_ext;
    int n_levels;                     // ragged plans: width levels referenced by the ops (0 = not a ragged plan)
    int batch;                        // images per run (n of the first op's input)
    bool u8_source;                   // an op pre-processes the uint8 frames itself (F_U8SRC): ext[0] = frames, geometry below
    int src_h, src_w;
    long src_pitch, src_fstride;
};

int vse_ctc_fuse_launch(const float* d_probs, int b, int t, int ncls, int64_t row_stride, const int32_t* d_group, int g, const int32_t* d_tlen,
                        void* d_idx_maxp, void* stream);                                                               // prepost.hip
int vse_frame_change_launch(const void* d_bgr, int n, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0, int x1, int edge_thresh,
                            void* d_state, int reset, int32_t* d_counts, void* stream);     // frame_change.hip
int vse_frame_focus_launch(const void* d_bgr, int n, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0, int x1, int edge_thresh,
                           void* d_state, int reset, int32_t* d_focus, void* stream);      // frame_change.hip
int vse_frame_cells_state_words();                                                                                     // frame_change.hip
int vse_frame_cells_launch(const void* d_bgr, int n, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0, int x1, int edge_thresh,
                           const CellRule& rule, void* d_state, int reset, int flush, int32_t* d_totals, int32_t* d_cell_counts,
                           void* stream);                                                                               // frame_change.hip
int vse_frame_cells_multi_max();                                                                                       // frame_change.hip
int vse_frame_cells_multi_launch(const void* d_bgr, int n, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0, int x1,
                                 const int* thresholds, int nt, const CellRule& rule, void* d_state, int reset, int flush,
                                 int32_t* d_totals, void* stream);                                                      // frame_change.hip
int vse_frame_cells_counts_launch(const void* d_bgr, int n, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0, int x1,
                                  const int* thresholds, int nt, const CellRule& rule, void* d_state, int reset, int flush,
                                  int32_t* d_totals, int32_t* d_counts, void* stream);                                  // frame_change.hip
int vse_frame_cells_export_launch(const void* d_cells_state, int area_h, int area_w, int q, void* d_change_state, void* stream);   // frame_change.hip
int vse_frame_cells_masks_launch(const void* d_bgr, int n, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0, int x1,
                                 const int* thresholds, int nt, const CellRule& rule, void* d_state, int reset, int flush,
                                 int32_t* d_totals, void* d_masks, int slot0, void* stream);                            // frame_change.hip
int vse_frame_masks_replay_launch(const void* d_masks, int area_h, int area_w, int nt, int q, int f0, int f1, int ry0, int ry1, int rx0,
                                  int rx1, int reset, int32_t* d_counts, void* d_change_state, void* stream);   // frame_change.hip
size_t vse_frame_hold_word_bytes();                                                                                    // frame_change.hip
int vse_frame_hold_launch(const void* d_bgr, int n, int steps, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0, int x1,
                          int edge_thresh, int hold, int skip, void* d_state, int fresh, int32_t* d_counts, void* stream);   // frame_change.hip
size_t vse_frame_hold_bounded_bytes(int ih, int iw, int max_hold);                                                       // frame_change.hip
int vse_frame_hold_bounded_launch(const void* d_bgr, int n, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0, int x1, int edge_thresh,
                                  int hold, int max_hold, void* d_state, int64_t fed, int flush, int32_t* d_counts, void* stream);
size_t vse_frame_cells_hold_bytes(int ih, int iw, int nt);                                                               // frame_change.hip
int vse_frame_cells_hold_launch(const void* d_bgr, int n, int steps, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0, int x1,
                                const int* thresholds, int nt, int hold, int skip, const CellRule& rule, void* d_state, int fresh, int flush,
                                int32_t* d_totals, int32_t* d_cell_counts, int count_rows, void* stream);               // frame_change.hip
int vse_frame_cells_hold_masks_launch(const void* d_bgr, int n, int steps, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0, int x1,
                                      const int* thresholds, int nt, int hold, int skip, const CellRule& rule, void* d_state, int fresh,
                                      int flush, int32_t* d_totals, int32_t* d_cell_counts, int count_rows, void* d_masks, int slot0,
                                      void* stream);                                                                    // frame_change.hip
int vse_frame_masks_replay_hold_launch(const void* d_masks, int area_h, int area_w, int nt, int q, int f0, int n, int steps, int ry0, int ry1,
                                       int rx0, int rx1, int hold, int skip, void* d_state, int fresh, int32_t* d_counts,
                                       void* stream);                                                                   // frame_change.hip
size_t vse_frame_cells_hold_bounded_bytes(int ih, int iw, int nt, int max_hold);                                        // frame_change.hip
int vse_frame_cells_hold_bounded_launch(const void* d_bgr, int n, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0, int x1,
                                        const int* thresholds, int nt, int hold, int max_hold, const CellRule& rule, void* d_state,
                                        int64_t fed, int flush, int32_t* d_totals, int32_t* d_cell_counts, int count_rows,
                                        void* stream);                                                                 // frame_change.hip
int vse_frame_cells_hold_bounded_masks_launch(const void* d_bgr, int n, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0, int x1,
                                              const int* thresholds, int nt, int hold, int max_hold, const CellRule& rule, void* d_state,
                                              int64_t fed, int flush, int32_t* d_totals, int32_t* d_cell_counts, int count_rows, void* d_masks,
                                              int slot0, void* stream);                                                // frame_change.hip
int vse_frame_masks_replay_hold_bounded_launch(const void* d_masks, int area_h, int area_w, int nt, int q, int f0, int n, int ry0, int ry1,
                                               int rx0, int rx1, int hold, int max_hold, void* d_state, int64_t fed, int flush,
                                               int32_t* d_counts, void* stream);                                       // frame_change.hip
int vse_scene_change_plane_pitch(int aw);                                                                              // scene_cut.hip
int vse_scene_change_launch(const void* d_bgr, int n, int64_t pitch, int64_t frame_stride, int scale, int ah, int aw, int search, int bias,
                            void* d_state, int reset, void* d_ws, int32_t* d_counts, void* stream);
size_t vse_audio_match_ws(const long* m, const long* n, int nq);                                                       // audio_match.hip
int vse_audio_match_launch(const uint8_t* const* pat, const uint8_t* const* win, const long* m, const long* n, int nq, void* d_ws,
                           unsigned long long* d_out, void* stream);

extern "C" {

const char* vse_last_error(void) { return g_err.c_str(); }
size_t vse_sizeof_op(void) { return sizeof(vse_op); }
size_t vse_sizeof_view(void) { return sizeof(vse_view); }
int vse_abi_version(void) { return 4; }

int vse_init(int device_id, vse_ctx** out) {
    if (!out) return VSE_E_INVAL;
    int count = 0;
    HIP_TRY(hipGetDeviceCount(&count));
    if (device_id < 0 || device_id >= count) {
        set_err("device %d not present (%d visible)", device_id, count);
        return VSE_E_INVAL;
    }
    HIP_TRY(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_id));
    if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos) {
        set_err("libvse_hip is built for gfx950 (MI355X) only; device %d is %s", device_id, prop.gcnArchName);
        return VSE_E_UNSUPPORTED;
    }
    vse_ctx* c = new vse_ctx();
    c->device = device_id;
    c->zero_page = nullptr;
    if (hipMalloc(&c->zero_page, 4096) != hipSuccess || hipMemset(c->zero_page, 0, 4096) != hipSuccess) {
        set_err("vse_init: cannot allocate the zero page on device %d: %s", device_id, hipGetErrorString(hipGetLastError()));
        if (c->zero_page) (void)hipFree(c->zero_page);
        delete c;
        return VSE_E_HIP;
    }
    *out = c;
    return VSE_OK;
}

void vse_destroy(vse_ctx* c) {
    if (!c) return;
    for (void* w : c->weights)
        if (w) (void)hipFree(w);
    if (c->zero_page) (void)hipFree(c->zero_page);
    delete c;
}

int vse_weights_upload(vse_ctx* c, const void* host_blob, size_t nbytes) {
    if (!c || !host_blob || !nbytes) return VSE_E_INVAL;
    HIP_TRY(hipSetDevice(c->device));
    void* d = nullptr;
    HIP_TRY(hipMalloc(&d, nbytes + 256));
    HIP_TRY(hipMemcpy(d, host_blob, nbytes, hipMemcpyHostToDevice));
    c->weights.push_back(d);
    c->weight_bytes.push_back(nbytes);
    return (int)c->weights.size() - 1;
}

int vse_weights_free(vse_ctx* c, int id) {
    if (!c || id < 0 || id >= (int)c->weights.size()) return VSE_E_INVAL;
    if (c->weights[id]) (void)hipFree(c->weights[id]);
    c->weights[id] = nullptr;
    return VSE_OK;
}

int vse_plan_create(vse_ctx* c, int weights_id, const vse_op* ops, int n_ops, size_t ws_bytes, vse_plan** out) {
    if (!c || !ops || n_ops <= 0 || !out) return VSE_E_INVAL;
    if (weights_id < 0 || weights_id >= (int)c->weights.size() || !c->weights[weights_id]) {
        set_err("bad weights id %d", weights_id);
        return VSE_E_INVAL;
    }
    vse_plan* p = new vse_plan();
    p->ctx = c;
    p->weights_id = weights_id;
    p->ops.assign(ops, ops + n_ops);
    p->ws_bytes = ws_bytes;
    p->max_ext = -1;
    p->n_levels = 0;
    p->batch = ops[0].in0.n;
    p->u8_source = false;
    p->src_h = p->src_w = 0;
    p->src_pitch = p->src_fstride = 0;
    const size_t wbytes = c->weight_bytes[weights_id];
    for (int i = 0; i < n_ops; ++i) {
        const vse_op& o = ops[i];
        if (o.kind < OP_CONV || o.kind > OP_CHAIN) {
            set_err("op %d: unknown kind %d", i, o.kind);
            delete p;
            return VSE_E_INVAL;
        }
        if (o.p[P_WLIN] < 0 || o.p[P_WLOUT] < 0) {
            set_err("op %d: negative width level", i);
            delete p;
            return VSE_E_INVAL;
        }
        p->n_levels = std::max(p->n_levels, std::max(o.p[P_WLIN], o.p[P_WLOUT]));
        if (o.kind == OP_CONV && (o.flags & F_U8SRC)) {
            if (!(o.flags & F_STEM) || o.in0.arena != 2) {
                set_err("op %d: F_U8SRC is for a stem conv that reads the plan input", i);
                delete p;
                return VSE_E_INVAL;
            }
            p->u8_source = true;
        }
        const vse_view* vs[5] = {&o.in0, &o.in1, &o.in2, &o.out, &o.out2};
        for (const vse_view* v : vs) {
            if (v->n == 0) continue;
            if (v->arena >= 2) p->max_ext = std::max(p->max_ext, v->arena - 2);
            if (v->arena == 0) {
                const size_t end = (size_t)v->off + ((size_t)v->n * v->h * v->w - 1) * v->ld * v->esize + (size_t)v->c * v->esize;
                if (end > ws_bytes) {
                    set_err("op %d: view exceeds workspace (%zu > %zu)", i, end, ws_bytes);
                    delete p;
                    return VSE_E_INVAL;
                }
            }
        }
        if ((size_t)o.w_off > wbytes || (size_t)o.b_off > wbytes) {
            set_err("op %d: weight offset out of range", i);
            delete p;
            return VSE_E_INVAL;
        }
        if (o.kind == OP_CHAIN) {
            // the chain kernels read their descriptor from the weight blob: check, once, that the record and the blob describe the
            // same chain (header: magic, stages, buffers, LDS image bytes / offset / total; compiler.py emit_chain) and that the
            // descriptor + LDS image lie inside the blob — a stale or foreign blob must fail here, not inside a kernel
            int hdr[16];
            const size_t words = 16 + (size_t)std::max(o.p[4], 0) * 16 + (size_t)std::max(o.p[3], 0) * 28;
            if ((size_t)o.w_off + words * 4 > wbytes || (o.w_off & 3) ||
                hipMemcpy(hdr, reinterpret_cast<const char*>(c->weights[weights_id]) + o.w_off, sizeof hdr, hipMemcpyDeviceToHost) != hipSuccess) {
                set_err("op %d: chain descriptor out of the weight blob", i);
                delete p;
                return VSE_E_INVAL;
            }
            if (hdr[0] != 0x43484e31 || hdr[1] != o.p[3] || hdr[2] != o.p[4] || hdr[5] != o.p[2] || hdr[3] < 0 || hdr[4] < 0 ||
                (size_t)o.w_off + (size_t)hdr[4] + (size_t)hdr[3] > wbytes) {
                set_err("op %d: chain descriptor does not match its record (magic %#x, stages %d / %d, buffers %d / %d, LDS %d / %d)", i, hdr[0],
                        hdr[1], o.p[3], hdr[2], o.p[4], hdr[5], o.p[2]);
                delete p;
                return VSE_E_INVAL;
            }
        }
    }
    // conv + max-pool pairs that run as one kernel: decided here, once, from the records (ragged plans stay as they are)
    p->pooled.assign(n_ops, ConvKernel{CK_NONE, VSE_OK, {0, 0, 0}});
    for (int i = 0; i + 1 < n_ops && !p->n_levels; ++i) p->pooled[i] = conv_pool_select(ops, n_ops, i);
    // 1x1 conv + global-average pool pairs whose partial sums the conv takes itself (not in ragged plans: their pools sum row by row),
    // and gate multiply + residual add pairs that run as one pass (ragged plans too): decided here as well
    p->gapped.assign(n_ops, ConvGap{0, 0, 0, 0, 0, 0, 0});
    p->scale_add.assign(n_ops, 0);
    for (int i = 0; i + 1 < n_ops; ++i) {
        if (!p->n_levels) {
            const ConvGap g = conv_gap_select(ops, n_ops, i);
            if (g.fused && g.part_off >= 0 && (size_t)(g.part_off + g.part_bytes) <= ws_bytes) p->gapped[i] = g;
        }
        p->scale_add[i] = scale_add_select(ops, n_ops, i);
    }
    *out = p;
    return VSE_OK;
}

void vse_plan_destroy(vse_plan* p) { delete p; }

static inline TView resolve(const vse_view& v, char* ws, char* wts, void* const* ext) {
    TView t;
    t.ptr = nullptr;
    t.n = v.n; t.h = v.h; t.w = v.w; t.c = v.c; t.ld = v.ld; t.esize = v.esize;
    if (v.n == 0) return t;
    char* base = v.arena == 0 ? ws : (v.arena == 1 ? wts : reinterpret_cast<char*>(ext[v.arena - 2]));
    t.ptr = base + v.off;
    return t;
}

static int run_op(vse_plan* p, int i, char* ws, void* const* ext, const int32_t* wtab, hipStream_t st, const SrcGeom& src) {
    const vse_op& o = p->ops[i];
    // ragged plans: widths[level][n]
    const int* wl_in = (wtab && o.p[P_WLIN]) ? wtab + (size_t)(o.p[P_WLIN] - 1) * p->batch : nullptr;
    const int* wl_out = (wtab && o.p[P_WLOUT]) ? wtab + (size_t)(o.p[P_WLOUT] - 1) * p->batch : nullptr;
    char* wts = reinterpret_cast<char*>(p->ctx->weights[p->weights_id]);
    const TView in0 = resolve(o.in0, ws, wts, ext), in1 = resolve(o.in1, ws, wts, ext),
                in2 = resolve(o.in2, ws, wts, ext), out = resolve(o.out, ws, wts, ext),
                out2 = resolve(o.out2, ws, wts, ext);
    int rc;
    if (i > 0 && p->pooled[i - 1].family == CK_C3POOL) return VSE_OK;      // this pool ran inside the conv in front of it
    if (i > 0 && p->scale_add[i - 1]) return VSE_OK;                       // this add ran with the gate multiply in front of it
    if (i > 0 && p->gapped[i - 1].fused) {
        // the conv in front of this pool left the partial sums: the finish pass alone
        const ConvGap& g = p->gapped[i - 1];
        rc = launch_gap_finish(reinterpret_cast<const float*>(ws + g.part_off), in0, out, o.in2.h, g.slots, st);
    } else if (p->gapped[i].fused) {
        const ConvGap& g = p->gapped[i];
        float* part = reinterpret_cast<float*>(ws + g.part_off);
        // two tiles add into one slot: the slots start from zero (otherwise every slot that is read is overwritten)
        if (g.atomic && hipMemsetAsync(part, 0, (size_t)g.part_bytes, st) != hipSuccess) rc = VSE_E_HIP;
        else rc = launch_conv_gap(o, g, in0, out, wts, reinterpret_cast<const half_t*>(p->ctx->zero_page), part, p->ops[i + 1].in2.h, st);
    } else if (p->scale_add[i]) {
        const vse_op& b = p->ops[i + 1];
        rc = launch_scale_add(in0, in1, resolve(p->scale_add[i] == 1 ? b.in1 : b.in0, ws, wts, ext), resolve(b.out, ws, wts, ext), b.p[2], st);
    } else if (p->pooled[i].family == CK_C3POOL) {
        const TView pool_out = resolve(p->ops[i + 1].out, ws, wts, ext);
        rc = launch_conv_pool(o, p->pooled[i], in0, pool_out, wts, reinterpret_cast<const half_t*>(p->ctx->zero_page), st);
    } else if (o.kind == OP_CONV) {
        const uint8_t* u8src = (o.flags & F_U8SRC) ? reinterpret_cast<const uint8_t*>(ext[0]) : nullptr;
        rc = launch_conv(o, in0, in1, in2, out, out2, wts, reinterpret_cast<const half_t*>(p->ctx->zero_page), wl_out, u8src, src, st);
    } else if (o.kind == OP_CHAIN) {
        rc = launch_chain(o, in0, out, out2, in2, wts, st);
    } else {
        rc = launch_simple_op(o, in0, in1, in2, out, out2, wts, wl_in, wl_out, st);
    }
    if (rc != VSE_OK) set_err("op %d (kind %d) failed to launch: rc=%d (%s)", i, o.kind, rc, hipGetErrorString(hipGetLastError()));
    return rc;
}

static int check_run(vse_plan* p, void* ws, void* const* ext, int n_ext, const int32_t* d_widths, const char* who) {
    if (!p || !ext || n_ext <= p->max_ext) {
        set_err("%s: need %d external pointers", who, p ? p->max_ext + 1 : 0);
        return VSE_E_INVAL;
    }
    if (!ws && p->ws_bytes) return VSE_E_INVAL;
    if (p->n_levels && !d_widths) {
        set_err("%s: the plan was compiled for ragged batches (%d width levels): run it with a width table", who, p->n_levels);
        return VSE_E_INVAL;
    }
    if (!p->n_levels && d_widths) {
        set_err("%s: width table given to a plan that was not compiled for ragged batches", who);
        return VSE_E_INVAL;
    }
    if (p->u8_source && (p->src_h <= 0 || p->src_w <= 0)) {
        set_err("%s: the plan pre-processes the uint8 frames in its stem: call vse_plan_set_source (or vse_det_forward) first", who);
        return VSE_E_INVAL;
    }
    return VSE_OK;
}

int vse_plan_set_source(vse_plan* p, int src_h, int src_w, int64_t pitch, int64_t frame_stride) {
    if (!p || src_h <= 0 || src_w <= 0 || pitch < (int64_t)src_w * 3 || frame_stride < 0) return VSE_E_INVAL;
    if (!p->u8_source) {
        set_err("vse_plan_set_source: the plan takes a pre-processed fp16 input, not uint8 frames");
        return VSE_E_INVAL;
    }
    p->src_h = src_h; p->src_w = src_w; p->src_pitch = pitch; p->src_fstride = frame_stride;
    return VSE_OK;
}
int vse_plan_takes_frames(vse_plan* p) { return p ? (p->u8_source ? 1 : 0) : VSE_E_INVAL; }

int vse_plan_run(vse_plan* p, void* ws, void* const* ext, int n_ext, void* stream) {
    return vse_plan_run_ragged(p, ws, ext, n_ext, nullptr, stream);
}

// the frame geometry travels with the RUN (a by-value copy taken here), never read from the plan while ops are being launched:
// the same plan may serve callers with different source sizes (vse_det_forward hands over its own arguments)
static int run_all(vse_plan* p, void* ws, void* const* ext, const int32_t* d_widths, void* stream, const SrcGeom src) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    for (int i = 0; i < (int)p->ops.size(); ++i) {
        const int rc = run_op(p, i, reinterpret_cast<char*>(ws), ext, d_widths, st, src);
        if (rc != VSE_OK) return rc;
    }
    return VSE_OK;
}

int vse_plan_run_ragged(vse_plan* p, void* ws, void* const* ext, int n_ext, const int32_t* d_widths, void* stream) {
    int rc = check_run(p, ws, ext, n_ext, d_widths, "vse_plan_run");
    if (rc != VSE_OK) return rc;
    return run_all(p, ws, ext, d_widths, stream, SrcGeom{p->src_h, p->src_w, p->src_pitch, p->src_fstride});
}

int vse_plan_width_levels(vse_plan* p) { return p ? p->n_levels : VSE_E_INVAL; }

// ---- model-level calls: one call per network invocation over a compiled plan ---------------------------------
int vse_det_forward(vse_ctx* c, vse_plan* det_plan, void* ws, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch,
                    int64_t frame_stride, int dst_h, int dst_w, int raw_input, void* d_in_f16, float* d_prob, void* stream) {
    if (!c || !det_plan || !d_bgr || !d_prob) return VSE_E_INVAL;
    if (det_plan->batch != n || det_plan->ops[0].in0.h != dst_h || det_plan->ops[0].in0.w != dst_w) {
        set_err("vse_det_forward: the plan was compiled for %d x %d x %d, called with %d x %d x %d", det_plan->batch,
                det_plan->ops[0].in0.h, det_plan->ops[0].in0.w, n, dst_h, dst_w);
        return VSE_E_INVAL;
    }
    if (det_plan->u8_source) {
        // the plan's stem resizes the frames itself: no pre-processing pass, no fp16 input tensor; the geometry of THIS call's
        // frames goes to the kernels directly (nothing is stored on the shared plan)
        if (src_h <= 0 || src_w <= 0 || pitch < (int64_t)src_w * 3 || frame_stride < 0 || (!ws && det_plan->ws_bytes)) return VSE_E_INVAL;
        if (det_plan->max_ext > 1 || det_plan->n_levels) {
            set_err("vse_det_forward: not a one-map detector plan");
            return VSE_E_INVAL;
        }
        void* ext[2] = {const_cast<void*>(d_bgr), d_prob};
        return run_all(det_plan, ws, ext, nullptr, stream, SrcGeom{src_h, src_w, (long)pitch, (long)frame_stride});
    }
    if (!d_in_f16) return VSE_E_INVAL;
    static const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};      // paddleocr NormalizeImage (DB detectors)
    int rc = vse_det_preprocess(c, d_bgr, n, src_h, src_w, pitch, frame_stride, d_in_f16, dst_h, dst_w, raw_input ? nullptr : mean,
                                raw_input ? nullptr : sd, stream);
    if (rc != VSE_OK) return rc;
    void* ext[2] = {d_in_f16, d_prob};
    return vse_plan_run(det_plan, ws, ext, 2, stream);
}

int vse_rec_forward(vse_ctx* c, vse_plan* rec_plan, void* ws, const void* d_rec_in_f16, const int32_t* d_widths, int out_level,
                    void* d_idx_maxp, int b, int t, int32_t* d_out_idx, int32_t* d_out_len, float* d_out_conf, void* stream) {
    if (!c || !rec_plan || !d_rec_in_f16 || !d_idx_maxp) return VSE_E_INVAL;
    if (rec_plan->batch != b || rec_plan->max_ext != 1) {
        set_err("vse_rec_forward: the plan takes %d crops and %d external buffers (compile it with want_probs=False)", rec_plan->batch,
                rec_plan->max_ext + 1);
        return VSE_E_INVAL;
    }
    if (d_widths && (out_level < 0 || out_level >= rec_plan->n_levels)) return VSE_E_INVAL;
    void* ext[2] = {const_cast<void*>(d_rec_in_f16), d_idx_maxp};
    int rc = vse_plan_run_ragged(rec_plan, ws, ext, 2, d_widths, stream);
    if (rc != VSE_OK) return rc;
    return vse_ctc_collapse_ragged(c, d_idx_maxp, b, t, d_widths ? d_widths + (size_t)out_level * b : nullptr, d_out_idx, d_out_len,
                                   d_out_conf, stream);
}

// ---- a recogniser invocation as ONE HIP graph ---------------------------------------------------------------------------------
// ~80 launches of a recogniser plan + the CTC collapse, captured once against FIXED buffers (the caller keeps input, width table,
// workspace and outputs at the same addresses and refills them) and replayed with a single hipGraphLaunch.
struct vse_graph {
    hipGraph_t graph;
    hipGraphExec_t exec;
};

int vse_rec_graph_create(vse_ctx* c, vse_plan* rec_plan, void* ws, const void* d_rec_in_f16, const int32_t* d_widths, int out_level,
                         void* d_idx_maxp, int b, int t, int32_t* d_out_idx, int32_t* d_out_len, float* d_out_conf, void* stream,
                         vse_graph** out) {
    if (!out) return VSE_E_INVAL;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (!st) {
        set_err("vse_rec_graph_create: capture needs a non-default stream");
        return VSE_E_INVAL;
    }
    HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
    const int rc = vse_rec_forward(c, rec_plan, ws, d_rec_in_f16, d_widths, out_level, d_idx_maxp, b, t, d_out_idx, d_out_len, d_out_conf, stream);
    hipGraph_t g = nullptr;
    const hipError_t e = hipStreamEndCapture(st, &g);
    if (rc != VSE_OK) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
    }
    if (e != hipSuccess || !g) {
        set_err("hipStreamEndCapture failed: %s", hipGetErrorString(e));
        return VSE_E_HIP;
    }
    vse_graph* vg = new vse_graph{g, nullptr};
    const hipError_t e2 = hipGraphInstantiate(&vg->exec, g, nullptr, nullptr, 0);
    if (e2 != hipSuccess) {
        set_err("hipGraphInstantiate failed: %s", hipGetErrorString(e2));
        (void)hipGraphDestroy(g);
        delete vg;
        return VSE_E_HIP;
    }
    *out = vg;
    return VSE_OK;
}
int vse_graph_launch(vse_graph* g, void* stream) {
    if (!g || !g->exec) return VSE_E_INVAL;
    HIP_TRY(hipGraphLaunch(g->exec, reinterpret_cast<hipStream_t>(stream)));
    return VSE_OK;
}
void vse_graph_destroy(vse_graph* g) {
    if (!g) return;
    if (g->exec) (void)hipGraphExecDestroy(g->exec);
    if (g->graph) (void)hipGraphDestroy(g->graph);
    delete g;
}

// ---- CTC posterior fusion (prepost.hip) --------------------------------------------------------------------------------------
int vse_ctc_fuse(vse_ctx* c, const float* d_probs, int b, int t, int ncls, int64_t row_stride, const int32_t* d_group, int g,
                 const int32_t* d_tlen, void* d_idx_maxp, void* stream) {
    if (!c || !d_probs || !d_group || !d_idx_maxp || b < 1 || t < 1 || ncls < 1 || g < 1 || row_stride < ncls ||
        ncls > (1 << 30) || (int64_t)g * t >= (1 << 24) || (reinterpret_cast<uintptr_t>(d_probs) & 3)) {
        set_err("vse_ctc_fuse: bad arguments (b %d, t %d, ncls %d, g %d: all >= 1, ncls <= 2^30, g * t < 2^24; row stride %lld >= ncls; non-NULL "
                "4-byte aligned probabilities, group table and output)", b, t, ncls, g, (long long)row_stride);
        return VSE_E_INVAL;
    }
    const int rc = vse_ctc_fuse_launch(d_probs, b, t, ncls, row_stride, d_group, g, d_tlen, d_idx_maxp, stream);
    if (rc != VSE_OK) set_err("vse_ctc_fuse: launch failed: %s", hipGetErrorString(hipGetLastError()));
    return rc;
}

// ---- argument checks shared by the vse_frame_* entry points: each sets the error text in the name of `who` and returns false ------
// n frames of src_h x src_w pixels behind d_bgr (NULL only with n == 0, which min_n == 0 allows) and an 8-byte aligned state; `rest`:
// the entry point's other pointers and counts are in order
static bool check_frames(const char* who, bool rest, const void* d_bgr, int n, int min_n, int src_h, int src_w, int64_t pitch,
                         int64_t frame_stride, const void* d_state) {
    if (rest && d_state && (d_bgr || n <= 0) && n >= min_n && src_h > 0 && src_w > 0 && pitch >= (int64_t)src_w * 3 &&
        (n <= 1 || frame_stride >= (int64_t)(src_h - 1) * pitch + (int64_t)src_w * 3) && !(reinterpret_cast<uintptr_t>(d_state) & 7))
        return true;
    set_err("%s: bad arguments (n %d of at least %d, frame %d x %d, pitch %lld, frame stride %lld, state 8-byte aligned, no NULL pointer)",
            who, n, min_n, src_h, src_w, (long long)pitch, (long long)frame_stride);
    return false;
}

// the rectangle [y0, y1) x [x0, x1), which the messages call `noun`, has an interior and lies inside the frame
static bool check_area(const char* who, const char* noun, int y0, int y1, int x0, int x1, int src_h, int src_w) {
    if (y0 >= 0 && x0 >= 0 && y1 <= src_h && x1 <= src_w && y1 - y0 >= 3 && x1 - x0 >= 3) return true;
    set_err("%s: %s [%d, %d) x [%d, %d) is degenerate or outside the %d x %d frame", who, noun, y0, y1, x0, x1, src_h, src_w);
    return false;
}

// the per-cell interval rule of the locator
static bool check_rule(const char* who, int ratio_num, int ratio_den, int min_frames, int max_frames) {
    if (ratio_num >= 1 && ratio_den >= 1 && ratio_den <= 1024 && min_frames >= 1 && max_frames >= min_frames) return true;
    set_err("%s: ratio %d / %d (numerator >= 1, denominator 1..1024) or run length %d..%d (1 <= min <= max) out of range", who, ratio_num,
            ratio_den, min_frames, max_frames);
    return false;
}

// the edge thresholds of the entry points that take several: 1 .. vse_frame_cells_multi_max() of them, each 1..255, ascending
static bool check_thresholds(const char* who, const int* thresholds, int nt) {
    if (!thresholds || nt < 1 || nt > vse_frame_cells_multi_max()) {
        set_err("%s: %d thresholds (1..%d, not NULL)", who, nt, vse_frame_cells_multi_max());
        return false;
    }
    for (int q = 0; q < nt; ++q) {
        if (thresholds[q] < 1 || thresholds[q] > 255 || (q && thresholds[q] <= thresholds[q - 1])) {
            set_err("%s: threshold %d of %d is %d (each 1..255, ascending and distinct)", who, q, nt, thresholds[q]);
            return false;
        }
    }
    return true;
}

constexpr int FRAME_HOLD_BOUNDED_MAX = 4000;       // the per-pixel run length is a uint16 and the ring of pending rows stays small

// the frames an edge pixel must hold still, and with bounded runs the most it may
static bool check_hold(const char* who, int hold) {
    if (hold >= 1 && hold <= 32) return true;
    set_err("%s: hold %d outside 1..32", who, hold);
    return false;
}

static bool check_hold_bounded(const char* who, int hold, int max_hold) {
    if (hold >= 1 && hold <= 32 && max_hold >= hold && max_hold <= FRAME_HOLD_BOUNDED_MAX) return true;
    set_err("%s: hold %d outside 1..32, or max_hold %d outside hold..%d", who, hold, max_hold, FRAME_HOLD_BOUNDED_MAX);
    return false;
}

// the steps of a held-edge call and those of them that belong to no frame: the mask of a frame is known hold - 1 frames later, so a flush
// feeds that many frames without an edge, and the first hold - 1 steps of a clip come before frame 1
static int64_t hold_steps(int n, int hold, int64_t fed, int flush, int* skip) {
    *skip = fed >= hold - 1 ? 0 : (int)(hold - 1 - fed);
    return (int64_t)n + (flush ? hold - 1 : 0);
}

// the end of an entry point: rc of its launcher, with the error text set where the launch failed
static int launched(const char* who, int rc) {
    if (rc != VSE_OK) set_err("%s: launch failed: %s", who, hipGetErrorString(hipGetLastError()));
    return rc;
}

// ---- subtitle-change frame selector (frame_change.hip) ---------------------------------------------------------------------
size_t vse_frame_change_state_bytes(int area_h, int area_w) {
    if (area_h < 3 || area_w < 3) return 0;
    return 16 + (size_t)(area_h - 2) * (size_t)((area_w - 2 + 63) / 64) * 8;
}

int vse_frame_change(vse_ctx* c, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride, int y0, int y1,
                     int x0, int x1, int edge_thresh, void* d_state, int reset, int32_t* d_counts, void* stream) {
    if (!check_frames("vse_frame_change", c && d_counts, d_bgr, n, 1, src_h, src_w, pitch, frame_stride, d_state) ||
        !check_area("vse_frame_change", "area", y0, y1, x0, x1, src_h, src_w))
        return VSE_E_INVAL;
    return vse_frame_change_launch(d_bgr, n, pitch, frame_stride, y0, y1, x0, x1, edge_thresh, d_state, reset, d_counts, stream);
}

// ---- sharpness of the edges that stand still (frame_change.hip) ---------------------------------------------------------------
int vse_frame_focus(vse_ctx* c, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride, int y0, int y1,
                    int x0, int x1, int edge_thresh, void* d_state, int reset, int32_t* d_focus, void* stream) {
    if (!check_frames("vse_frame_focus", c && d_focus, d_bgr, n, 1, src_h, src_w, pitch, frame_stride, d_state) ||
        !check_area("vse_frame_focus", "area", y0, y1, x0, x1, src_h, src_w))
        return VSE_E_INVAL;
    if ((int64_t)(y1 - y0 - 2) * (x1 - x0 - 2) > ((int64_t)1 << 23)) {
        set_err("vse_frame_focus: the area's interior of %d x %d pixels exceeds 2^23, beyond which a frame's focus may not fit an int32",
                y1 - y0 - 2, x1 - x0 - 2);
        return VSE_E_INVAL;
    }
    return vse_frame_focus_launch(d_bgr, n, pitch, frame_stride, y0, y1, x0, x1, edge_thresh, d_state, reset, d_focus, stream);
}

// ---- subtitle-area locator (frame_change.hip) -------------------------------------------------------------------------------
int vse_frame_cells_dims(int area_h, int area_w, int* gy, int* gx) {
    if (area_h < 3 || area_w < 3 || !gy || !gx) return VSE_E_INVAL;
    *gy = (area_h - 2 + 7) / 8;
    *gx = (area_w - 2 + 63) / 64;
    return VSE_OK;
}

size_t vse_frame_cells_state_bytes(int area_h, int area_w) {
    int gy, gx;
    if (vse_frame_cells_dims(area_h, area_w, &gy, &gx) != VSE_OK) return 0;
    return (size_t)gy * gx * vse_frame_cells_state_words() * 8;
}

int vse_frame_cells(vse_ctx* c, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0,
                    int x1, int edge_thresh, int min_edges, int ratio_num, int ratio_den, int min_frames, int max_frames, void* d_state,
                    int reset, int flush, int32_t* d_totals, int32_t* d_cell_counts, void* stream) {
    if (!check_frames("vse_frame_cells", c && d_totals, d_bgr, n, 0, src_h, src_w, pitch, frame_stride, d_state) ||
        !check_area("vse_frame_cells", "region", y0, y1, x0, x1, src_h, src_w) ||
        !check_rule("vse_frame_cells", ratio_num, ratio_den, min_frames, max_frames))
        return VSE_E_INVAL;
    if (n == 0 && !reset && !flush) return VSE_OK;
    return launched("vse_frame_cells", vse_frame_cells_launch(d_bgr, n, pitch, frame_stride, y0, y1, x0, x1, edge_thresh,
                    {min_edges, ratio_num, ratio_den, min_frames, max_frames}, d_state, reset, flush, d_totals, d_cell_counts, stream));
}

// ---- edge-threshold calibration: the locator's cells at several thresholds in one pass (frame_change.hip) ---------------------------
size_t vse_frame_cells_multi_state_bytes(int area_h, int area_w, int nt) {
    if (nt < 1 || nt > vse_frame_cells_multi_max()) return 0;
    return (size_t)nt * vse_frame_cells_state_bytes(area_h, area_w);
}

int vse_frame_cells_multi(vse_ctx* c, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride, int y0, int y1,
                          int x0, int x1, const int* thresholds, int nt, int min_edges, int ratio_num, int ratio_den, int min_frames,
                          int max_frames, void* d_state, int reset, int flush, int32_t* d_totals, void* stream) {
    if (!check_frames("vse_frame_cells_multi", c && d_totals, d_bgr, n, 0, src_h, src_w, pitch, frame_stride, d_state) ||
        !check_area("vse_frame_cells_multi", "region", y0, y1, x0, x1, src_h, src_w) ||
        !check_rule("vse_frame_cells_multi", ratio_num, ratio_den, min_frames, max_frames))
        return VSE_E_INVAL;
    if (!check_thresholds("vse_frame_cells_multi", thresholds, nt)) return VSE_E_INVAL;
    if (n == 0 && !reset && !flush) return VSE_OK;
    return launched("vse_frame_cells_multi", vse_frame_cells_multi_launch(d_bgr, n, pitch, frame_stride, y0, y1, x0, x1, thresholds, nt,
                    {min_edges, ratio_num, ratio_den, min_frames, max_frames}, d_state, reset, flush, d_totals, stream));
}

// ---- calibration and selector counts in one pass (frame_change.hip) -------------------------------------------------------------------
int vse_frame_cells_counts(vse_ctx* c, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride, int y0, int y1,
                           int x0, int x1, const int* thresholds, int nt, int min_edges, int ratio_num, int ratio_den, int min_frames,
                           int max_frames, void* d_state, int reset, int flush, int32_t* d_totals, int32_t* d_counts, void* stream) {
    if (!check_frames("vse_frame_cells_counts", c && d_totals && (d_counts || n <= 0), d_bgr, n, 0, src_h, src_w, pitch, frame_stride,
                      d_state) ||
        !check_area("vse_frame_cells_counts", "region", y0, y1, x0, x1, src_h, src_w) ||
        !check_rule("vse_frame_cells_counts", ratio_num, ratio_den, min_frames, max_frames))
        return VSE_E_INVAL;
    if (!check_thresholds("vse_frame_cells_counts", thresholds, nt)) return VSE_E_INVAL;
    if (n == 0 && !reset && !flush) return VSE_OK;
    return launched("vse_frame_cells_counts", vse_frame_cells_counts_launch(d_bgr, n, pitch, frame_stride, y0, y1, x0, x1, thresholds, nt,
                    {min_edges, ratio_num, ratio_den, min_frames, max_frames}, d_state, reset, flush, d_totals, d_counts, stream));
}

int vse_frame_cells_export_state(vse_ctx* c, const void* d_cells_state, int area_h, int area_w, int nt, int q, void* d_change_state,
                                 void* stream) {
    if (!c || !d_cells_state || !d_change_state || area_h < 3 || area_w < 3 || nt < 1 || nt > vse_frame_cells_multi_max() || q < 0 ||
        q >= nt || ((reinterpret_cast<uintptr_t>(d_cells_state) | reinterpret_cast<uintptr_t>(d_change_state)) & 7)) {
        set_err("vse_frame_cells_export_state: bad arguments (area %d x %d of at least 3 x 3, slice %d of %d thresholds (1..%d), states "
                "8-byte aligned, no NULL pointer)", area_h, area_w, q, nt, vse_frame_cells_multi_max());
        return VSE_E_INVAL;
    }
    return launched("vse_frame_cells_export_state", vse_frame_cells_export_launch(d_cells_state, area_h, area_w, q, d_change_state, stream));
}

// ---- the locator's masks kept for a rectangle decided later (frame_change.hip) ------------------------------------------------------
size_t vse_frame_masks_bytes(int area_h, int area_w, int nt, int cap) {
    int gy, gx;
    if (nt < 1 || nt > vse_frame_cells_multi_max() || cap < 1 || vse_frame_cells_dims(area_h, area_w, &gy, &gx) != VSE_OK) return 0;
    return (size_t)cap * nt * gy * gx * 64;
}

int vse_frame_cells_masks(vse_ctx* c, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride, int y0, int y1,
                          int x0, int x1, const int* thresholds, int nt, int min_edges, int ratio_num, int ratio_den, int min_frames,
                          int max_frames, void* d_state, int reset, int flush, int32_t* d_totals, void* d_masks, int cap, int slot0,
                          void* stream) {
    if (!check_frames("vse_frame_cells_masks", c && d_totals && (d_masks || n <= 0) && !(reinterpret_cast<uintptr_t>(d_masks) & 7), d_bgr, n,
                      0, src_h, src_w, pitch, frame_stride, d_state) ||
        !check_area("vse_frame_cells_masks", "region", y0, y1, x0, x1, src_h, src_w) ||
        !check_rule("vse_frame_cells_masks", ratio_num, ratio_den, min_frames, max_frames))
        return VSE_E_INVAL;
    if (!check_thresholds("vse_frame_cells_masks", thresholds, nt)) return VSE_E_INVAL;
    if (cap < 1 || slot0 < 0 || (int64_t)slot0 + n > cap) {
        set_err("vse_frame_cells_masks: %d frames from slot %d on do not fit a mask buffer of %d slots (no wrap)", n, slot0, cap);
        return VSE_E_INVAL;
    }
    if (n == 0 && !reset && !flush) return VSE_OK;
    return launched("vse_frame_cells_masks", vse_frame_cells_masks_launch(d_bgr, n, pitch, frame_stride, y0, y1, x0, x1, thresholds, nt,
                    {min_edges, ratio_num, ratio_den, min_frames, max_frames}, d_state, reset, flush, d_totals, d_masks, slot0, stream));
}

int vse_frame_masks_replay(vse_ctx* c, const void* d_masks, int area_h, int area_w, int nt, int cap, int q, int f0, int f1, int ry0,
                           int ry1, int rx0, int rx1, int reset, int32_t* d_counts, void* d_change_state, void* stream) {
    if (!c || !d_masks || !d_counts || !d_change_state || area_h < 3 || area_w < 3 || nt < 1 || nt > vse_frame_cells_multi_max() || q < 0 ||
        q >= nt || ((reinterpret_cast<uintptr_t>(d_masks) | reinterpret_cast<uintptr_t>(d_change_state)) & 7) ||
        (reinterpret_cast<uintptr_t>(d_counts) & 3)) {
        set_err("vse_frame_masks_replay: bad arguments (region %d x %d of at least 3 x 3, threshold %d of %d (1..%d), masks and state 8-byte "
                "aligned, no NULL pointer)", area_h, area_w, q, nt, vse_frame_cells_multi_max());
        return VSE_E_INVAL;
    }
    if (f0 < 0 || f1 <= f0 || f1 > cap || (!reset && f0 == 0)) {
        set_err("vse_frame_masks_replay: slots [%d, %d) of a buffer of %d (0 <= f0 < f1 <= cap; without reset the mask before f0 is slot "
                "f0 - 1, so f0 >= 1)", f0, f1, cap);
        return VSE_E_INVAL;
    }
    if (ry0 < 0 || rx0 < 0 || ry1 > area_h || rx1 > area_w || ry1 - ry0 < 3 || rx1 - rx0 < 3) {
        set_err("vse_frame_masks_replay: rectangle [%d, %d) x [%d, %d) is degenerate or outside the %d x %d region", ry0, ry1, rx0, rx1,
                area_h, area_w);
        return VSE_E_INVAL;
    }
    return launched("vse_frame_masks_replay", vse_frame_masks_replay_launch(d_masks, area_h, area_w, nt, q, f0, f1, ry0, ry1, rx0, rx1, reset,
                    d_counts, d_change_state, stream));
}

// ---- held-edge frame selector (frame_change.hip) ------------------------------------------------------------------------------
size_t vse_frame_hold_state_bytes(int area_h, int area_w, int hold) {
    if (area_h < 3 || area_w < 3 || hold < 1 || hold > 32) return 0;
    return (size_t)(area_h - 2) * (size_t)((area_w - 2 + 63) / 64) * vse_frame_hold_word_bytes();
}

int vse_frame_hold(vse_ctx* c, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0,
                   int x1, int edge_thresh, int hold, void* d_state, int64_t fed, int flush, int32_t* d_counts, void* stream) {
    if (!check_frames("vse_frame_hold", c && fed >= 0, d_bgr, n, 0, src_h, src_w, pitch, frame_stride, d_state) ||
        !check_area("vse_frame_hold", "area", y0, y1, x0, x1, src_h, src_w))
        return VSE_E_INVAL;
    if (!check_hold("vse_frame_hold", hold)) return VSE_E_INVAL;
    int skip;
    const int64_t steps = hold_steps(n, hold, fed, flush, &skip);
    if (steps == 0) return VSE_OK;
    if (steps > INT32_MAX || (steps > skip && !d_counts)) {
        set_err("vse_frame_hold: %lld steps need d_counts and must fit an int", (long long)steps);
        return VSE_E_INVAL;
    }
    return launched("vse_frame_hold", vse_frame_hold_launch(d_bgr, n, (int)steps, pitch, frame_stride, y0, y1, x0, x1, edge_thresh, hold, skip,
                    d_state, fed == 0, d_counts, stream));
}

// ---- held-edge frame selector with bounded runs (frame_change.hip) -------------------------------------------------------------
size_t vse_frame_hold_bounded_state_bytes(int area_h, int area_w, int max_hold) {
    if (area_h < 3 || area_w < 3 || max_hold < 1 || max_hold > FRAME_HOLD_BOUNDED_MAX) return 0;
    return vse_frame_hold_bounded_bytes(area_h - 2, area_w - 2, max_hold);
}

int vse_frame_hold_bounded(vse_ctx* c, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride, int y0, int y1,
                           int x0, int x1, int edge_thresh, int hold, int max_hold, void* d_state, int64_t fed, int flush, int32_t* d_counts,
                           void* stream) {
    if (!check_frames("vse_frame_hold_bounded", c && fed >= 0, d_bgr, n, 0, src_h, src_w, pitch, frame_stride, d_state) ||
        !check_area("vse_frame_hold_bounded", "area", y0, y1, x0, x1, src_h, src_w))
        return VSE_E_INVAL;
    if (!check_hold_bounded("vse_frame_hold_bounded", hold, max_hold)) return VSE_E_INVAL;
    if (n == 0 && !flush) return VSE_OK;
    // the row of a frame is final max_hold frames later, or at the flush
    const int64_t rows = (flush ? fed + n : std::max<int64_t>(0, fed + n - max_hold)) - std::max<int64_t>(0, fed - max_hold);
    if (n == INT32_MAX || (rows > 0 && !d_counts)) {
        set_err("vse_frame_hold_bounded: %lld rows need d_counts, and n + 1 must fit an int", (long long)rows);
        return VSE_E_INVAL;
    }
    return launched("vse_frame_hold_bounded", vse_frame_hold_bounded_launch(d_bgr, n, pitch, frame_stride, y0, y1, x0, x1, edge_thresh, hold,
                    max_hold, d_state, fed, flush != 0, d_counts, stream));
}

// ---- locator and calibration on held edges (frame_change.hip) -------------------------------------------------------------------
size_t vse_frame_cells_hold_state_bytes(int area_h, int area_w, int nt, int hold) {
    if (area_h < 3 || area_w < 3 || nt < 1 || nt > vse_frame_cells_multi_max() || hold < 1 || hold > 32) return 0;
    return vse_frame_cells_hold_bytes(area_h - 2, area_w - 2, nt);
}

int vse_frame_cells_hold(vse_ctx* c, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride, int y0, int y1,
                         int x0, int x1, const int* thresholds, int nt, int hold, int min_edges, int ratio_num, int ratio_den,
                         int min_frames, int max_frames, void* d_state, int64_t fed, int flush, int32_t* d_totals,
                         int32_t* d_cell_counts, void* stream) {
    if (!check_frames("vse_frame_cells_hold", c && d_totals && fed >= 0, d_bgr, n, 0, src_h, src_w, pitch, frame_stride, d_state) ||
        !check_area("vse_frame_cells_hold", "region", y0, y1, x0, x1, src_h, src_w) ||
        !check_rule("vse_frame_cells_hold", ratio_num, ratio_den, min_frames, max_frames))
        return VSE_E_INVAL;
    if (!check_thresholds("vse_frame_cells_hold", thresholds, nt)) return VSE_E_INVAL;
    if (!check_hold("vse_frame_cells_hold", hold)) return VSE_E_INVAL;
    int skip;
    const int64_t steps = hold_steps(n, hold, fed, flush, &skip);
    if ((int64_t)n + hold - 1 > INT32_MAX) {
        set_err("vse_frame_cells_hold: %lld steps do not fit an int", (long long)n + hold - 1);
        return VSE_E_INVAL;
    }
    if (n == 0 && !flush) return VSE_OK;
    return launched("vse_frame_cells_hold", vse_frame_cells_hold_launch(d_bgr, n, (int)steps, pitch, frame_stride, y0, y1, x0, x1, thresholds, nt,
                    hold, skip, {min_edges, ratio_num, ratio_den, min_frames, max_frames}, d_state, fed == 0, flush != 0, d_totals, d_cell_counts,
                    n + hold - 1, stream));
}

// ---- the held locator's edge masks kept, and the held selector's rows out of them (frame_change.hip) ----------------------------------
int vse_frame_cells_hold_masks(vse_ctx* c, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride, int y0,
                               int y1, int x0, int x1, const int* thresholds, int nt, int hold, int min_edges, int ratio_num, int ratio_den,
                               int min_frames, int max_frames, void* d_state, int64_t fed, int flush, int32_t* d_totals,
                               int32_t* d_cell_counts, void* d_masks, int cap, int slot0, void* stream) {
    if (!check_frames("vse_frame_cells_hold_masks", c && d_totals && fed >= 0 && (d_masks || n <= 0) && !(reinterpret_cast<uintptr_t>(d_masks) & 7),
                      d_bgr, n, 0, src_h, src_w, pitch, frame_stride, d_state) ||
        !check_area("vse_frame_cells_hold_masks", "region", y0, y1, x0, x1, src_h, src_w) ||
        !check_rule("vse_frame_cells_hold_masks", ratio_num, ratio_den, min_frames, max_frames))
        return VSE_E_INVAL;
    if (!check_thresholds("vse_frame_cells_hold_masks", thresholds, nt)) return VSE_E_INVAL;
    if (!check_hold("vse_frame_cells_hold_masks", hold)) return VSE_E_INVAL;
    int skip;
    const int64_t steps = hold_steps(n, hold, fed, flush, &skip);
    if ((int64_t)n + hold - 1 > INT32_MAX) {
        set_err("vse_frame_cells_hold_masks: %lld steps do not fit an int", (long long)n + hold - 1);
        return VSE_E_INVAL;
    }
    if (cap < 1 || slot0 < 0 || (int64_t)slot0 + n > cap) {
        set_err("vse_frame_cells_hold_masks: %d frames from slot %d on do not fit a mask buffer of %d slots (no wrap)", n, slot0, cap);
        return VSE_E_INVAL;
    }
    if (n == 0 && !flush) return VSE_OK;
    return launched("vse_frame_cells_hold_masks", vse_frame_cells_hold_masks_launch(d_bgr, n, (int)steps, pitch, frame_stride, y0, y1, x0, x1,
                    thresholds, nt, hold, skip, {min_edges, ratio_num, ratio_den, min_frames, max_frames}, d_state, fed == 0, flush != 0,
                    d_totals, d_cell_counts, n + hold - 1, d_masks, slot0, stream));
}

// what vse_frame_masks_replay_hold and vse_frame_masks_replay_hold_bounded check alike: the buffer, the slots and the rectangle
static bool check_replay_hold(const char* who, vse_ctx* c, const void* d_masks, int area_h, int area_w, int nt, int cap, int q, int f0, int f1,
                              int ry0, int ry1, int rx0, int rx1, const void* d_hold_state, int64_t fed, int flush, const int32_t* d_counts) {
    if (!c || !d_masks || !d_hold_state || area_h < 3 || area_w < 3 || nt < 1 || nt > vse_frame_cells_multi_max() || q < 0 || q >= nt ||
        fed < 0 || ((reinterpret_cast<uintptr_t>(d_masks) | reinterpret_cast<uintptr_t>(d_hold_state)) & 7) ||
        (reinterpret_cast<uintptr_t>(d_counts) & 3)) {
        set_err("%s: bad arguments (region %d x %d of at least 3 x 3, threshold %d of %d (1..%d), fed %lld, masks and "
                "state 8-byte aligned, no NULL pointer)", who, area_h, area_w, q, nt, vse_frame_cells_multi_max(), (long long)fed);
        return false;
    }
    if (f0 < 0 || f1 < f0 || f1 > cap || (f1 == f0 && !flush)) {
        set_err("%s: slots [%d, %d) of a buffer of %d (0 <= f0 < f1 <= cap; f1 == f0 only with flush)", who, f0, f1, cap);
        return false;
    }
    if (ry0 < 0 || rx0 < 0 || ry1 > area_h || rx1 > area_w || ry1 - ry0 < 3 || rx1 - rx0 < 3) {
        set_err("%s: rectangle [%d, %d) x [%d, %d) is degenerate or outside the %d x %d region", who, ry0, ry1, rx0, rx1,
                area_h, area_w);
        return false;
    }
    return true;
}

int vse_frame_masks_replay_hold(vse_ctx* c, const void* d_masks, int area_h, int area_w, int nt, int cap, int q, int f0, int f1, int ry0,
                                int ry1, int rx0, int rx1, int hold, void* d_hold_state, int64_t fed, int flush, int32_t* d_counts,
                                void* stream) {
    if (!check_replay_hold("vse_frame_masks_replay_hold", c, d_masks, area_h, area_w, nt, cap, q, f0, f1, ry0, ry1, rx0, rx1, d_hold_state,
                           fed, flush, d_counts))
        return VSE_E_INVAL;
    if (!check_hold("vse_frame_masks_replay_hold", hold)) return VSE_E_INVAL;
    int skip;
    const int64_t steps = hold_steps(f1 - f0, hold, fed, flush, &skip);
    if (steps > INT32_MAX || (steps > skip && !d_counts)) {
        set_err("vse_frame_masks_replay_hold: %lld steps need d_counts and must fit an int", (long long)steps);
        return VSE_E_INVAL;
    }
    if (steps == 0) return VSE_OK;
    return launched("vse_frame_masks_replay_hold", vse_frame_masks_replay_hold_launch(d_masks, area_h, area_w, nt, q, f0, f1 - f0, (int)steps,
                    ry0, ry1, rx0, rx1, hold, skip, d_hold_state, fed == 0, d_counts, stream));
}

// ---- locator and calibration on bounded runs (frame_change.hip) -----------------------------------------------------------------
size_t vse_frame_cells_hold_bounded_state_bytes(int area_h, int area_w, int nt, int max_hold) {
    if (area_h < 3 || area_w < 3 || nt < 1 || nt > vse_frame_cells_multi_max() || max_hold < 1 || max_hold > FRAME_HOLD_BOUNDED_MAX) return 0;
    return vse_frame_cells_hold_bounded_bytes(area_h - 2, area_w - 2, nt, max_hold);
}

int vse_frame_cells_hold_bounded(vse_ctx* c, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride, int y0,
                                 int y1, int x0, int x1, const int* thresholds, int nt, int hold, int max_hold, int min_edges, int ratio_num,
                                 int ratio_den, int min_frames, int max_frames, void* d_state, int64_t fed, int flush, int32_t* d_totals,
                                 int32_t* d_cell_counts, void* stream) {
    if (!check_frames("vse_frame_cells_hold_bounded", c && d_totals && fed >= 0, d_bgr, n, 0, src_h, src_w, pitch, frame_stride, d_state) ||
        !check_area("vse_frame_cells_hold_bounded", "region", y0, y1, x0, x1, src_h, src_w) ||
        !check_rule("vse_frame_cells_hold_bounded", ratio_num, ratio_den, min_frames, max_frames))
        return VSE_E_INVAL;
    if (!check_thresholds("vse_frame_cells_hold_bounded", thresholds, nt)) return VSE_E_INVAL;
    if (!check_hold_bounded("vse_frame_cells_hold_bounded", hold, max_hold)) return VSE_E_INVAL;
    // as vse_frame_hold_bounded: the row of a frame is final max_hold frames later, or at the flush, which is one step of its own
    if ((int64_t)n + max_hold > INT32_MAX) {
        set_err("vse_frame_cells_hold_bounded: %lld rows do not fit an int", (long long)n + max_hold);
        return VSE_E_INVAL;
    }
    if (n == 0 && !flush) return VSE_OK;
    return launched("vse_frame_cells_hold_bounded", vse_frame_cells_hold_bounded_launch(d_bgr, n, pitch, frame_stride, y0, y1, x0, x1, thresholds,
                    nt, hold, max_hold, {min_edges, ratio_num, ratio_den, min_frames, max_frames}, d_state, fed, flush != 0, d_totals,
                    d_cell_counts, n + max_hold, stream));
}

// ---- the bounded locator's edge masks kept, and the bounded selector's rows out of them (frame_change.hip) ----------------------------
int vse_frame_cells_hold_bounded_masks(vse_ctx* c, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride,
                                       int y0, int y1, int x0, int x1, const int* thresholds, int nt, int hold, int max_hold, int min_edges,
                                       int ratio_num, int ratio_den, int min_frames, int max_frames, void* d_state, int64_t fed, int flush,
                                       int32_t* d_totals, int32_t* d_cell_counts, void* d_masks, int cap, int slot0, void* stream) {
    const char* who = "vse_frame_cells_hold_bounded_masks";
    if (!check_frames(who, c && d_totals && fed >= 0 && (d_masks || n <= 0) && !(reinterpret_cast<uintptr_t>(d_masks) & 7), d_bgr, n, 0, src_h,
                      src_w, pitch, frame_stride, d_state) ||
        !check_area(who, "region", y0, y1, x0, x1, src_h, src_w) || !check_rule(who, ratio_num, ratio_den, min_frames, max_frames))
        return VSE_E_INVAL;
    if (!check_thresholds(who, thresholds, nt)) return VSE_E_INVAL;
    if (!check_hold_bounded(who, hold, max_hold)) return VSE_E_INVAL;
    if ((int64_t)n + max_hold > INT32_MAX) {
        set_err("%s: %lld rows do not fit an int", who, (long long)n + max_hold);
        return VSE_E_INVAL;
    }
    if (cap < 1 || slot0 < 0 || (int64_t)slot0 + n > cap) {
        set_err("%s: %d frames from slot %d on do not fit a mask buffer of %d slots (no wrap)", who, n, slot0, cap);
        return VSE_E_INVAL;
    }
    if (n == 0 && !flush) return VSE_OK;
    return launched(who, vse_frame_cells_hold_bounded_masks_launch(d_bgr, n, pitch, frame_stride, y0, y1, x0, x1, thresholds, nt, hold, max_hold,
                    {min_edges, ratio_num, ratio_den, min_frames, max_frames}, d_state, fed, flush != 0, d_totals, d_cell_counts, n + max_hold,
                    d_masks, slot0, stream));
}

int vse_frame_masks_replay_hold_bounded(vse_ctx* c, const void* d_masks, int area_h, int area_w, int nt, int cap, int q, int f0, int f1, int ry0,
                                        int ry1, int rx0, int rx1, int hold, int max_hold, void* d_bounded_state, int64_t fed, int flush,
                                        int32_t* d_counts, void* stream) {
    const char* who = "vse_frame_masks_replay_hold_bounded";
    if (!check_replay_hold(who, c, d_masks, area_h, area_w, nt, cap, q, f0, f1, ry0, ry1, rx0, rx1, d_bounded_state, fed, flush, d_counts))
        return VSE_E_INVAL;
    if (!check_hold_bounded(who, hold, max_hold)) return VSE_E_INVAL;
    // as vse_frame_hold_bounded: the row of a frame is final max_hold frames later, or at the flush
    const int64_t n = f1 - f0;
    const int64_t rows = (flush ? fed + n : std::max<int64_t>(0, fed + n - max_hold)) - std::max<int64_t>(0, fed - max_hold);
    if (n == INT32_MAX || (rows > 0 && !d_counts)) {
        set_err("%s: %lld rows need d_counts, and the slots + 1 must fit an int", who, (long long)rows);
        return VSE_E_INVAL;
    }
    return launched(who, vse_frame_masks_replay_hold_bounded_launch(d_masks, area_h, area_w, nt, q, f0, (int)n, ry0, ry1, rx0, rx1, hold,
                    max_hold, d_bounded_state, fed, flush != 0, d_counts, stream));
}

// ---- timeline sync: scene cuts for keyframe snapping (scene_cut.hip) ---------------------------------------------------------
// -> plane size; false when scale is out of range, the plane holds no macroblock or aw * ah > 2^23 (the int32 sums stay exact)
static bool scene_plane_size(int src_h, int src_w, int scale, int* ah, int* aw) {
    if (scale < 1 || scale > 8 || src_h <= 0 || src_w <= 0) return false;
    *ah = src_h / scale;
    *aw = src_w / scale;
    return *ah >= 16 && *aw >= 16 && (int64_t)*ah * *aw <= (int64_t)1 << 23;
}

size_t vse_scene_change_state_bytes(int src_h, int src_w, int scale) {
    int ah, aw;
    if (!scene_plane_size(src_h, src_w, scale, &ah, &aw)) return 0;
    return 16 + (size_t)ah * vse_scene_change_plane_pitch(aw);
}

size_t vse_scene_change_workspace_bytes(int n, int src_h, int src_w, int scale) {
    int ah, aw;
    if (n <= 0 || !scene_plane_size(src_h, src_w, scale, &ah, &aw)) return 0;
    return (size_t)n * ah * vse_scene_change_plane_pitch(aw);
}

int vse_scene_change(vse_ctx* c, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride, int scale, int search,
                     int bias, void* d_state, int reset, void* d_ws, size_t ws_bytes, int32_t* d_counts, void* stream) {
    if (!c || !d_bgr || !d_state || !d_ws || !d_counts || n <= 0 || n > 65535 || src_h <= 0 || src_w <= 0 || pitch < (int64_t)src_w * 3 ||
        (n > 1 && frame_stride < (int64_t)(src_h - 1) * pitch + (int64_t)src_w * 3) || (reinterpret_cast<uintptr_t>(d_state) & 7) ||
        (reinterpret_cast<uintptr_t>(d_ws) & 3)) {
        set_err("vse_scene_change: bad arguments (n %d of 1..65535, frame %d x %d, pitch %lld, frame stride %lld, state 8-byte and workspace "
                "4-byte aligned)", n, src_h, src_w, (long long)pitch, (long long)frame_stride);
        return VSE_E_INVAL;
    }
    if (search < 0 || search > 8 || bias < 0 || bias > 65535) {
        set_err("vse_scene_change: search radius %d (0..8) or bias %d (0..65535) out of range", search, bias);
        return VSE_E_INVAL;
    }
    int ah, aw;
    if (!scene_plane_size(src_h, src_w, scale, &ah, &aw)) {
        set_err("vse_scene_change: scale %d (1..8) on a %d x %d frame: the plane must be at least 16 x 16 and at most 2^23 pixels", scale, src_h,
                src_w);
        return VSE_E_INVAL;
    }
    const size_t need = vse_scene_change_workspace_bytes(n, src_h, src_w, scale);
    if (ws_bytes < need) {
        set_err("vse_scene_change: workspace of %zu bytes, %zu needed", ws_bytes, need);
        return VSE_E_INVAL;
    }
    const int rc = vse_scene_change_launch(d_bgr, n, pitch, frame_stride, scale, ah, aw, search, bias, d_state, reset, d_ws, d_counts, stream);
    if (rc != VSE_OK) set_err("vse_scene_change: launch failed: %s", hipGetErrorString(hipGetLastError()));
    return rc;
}

// ---- timeline sync: audio template search (audio_match.hip) ------------------------------------------------------------------
static const char* audio_query_error(const vse_audio_query& q, int64_t src_len, int64_t dst_len) {
    if (q.m < 1) return "pattern length m < 1";
    if (q.win_len < q.m) return "window shorter than the pattern";
    if (q.src_off < 0 || q.src_off > src_len - q.m) return "pattern range outside the source stream";
    if (q.dst_off < 0 || q.dst_off > dst_len - q.win_len) return "window range outside the destination stream";
    if (q.win_len > INT32_MAX / 2) return "window longer than 2^30 bytes";
    return nullptr;
}

size_t vse_audio_match_workspace_bytes(const vse_audio_query* queries, int nq) {
    if (!queries || nq < 1 || nq > 3) return 0;
    long m[3], n[3];
    for (int i = 0; i < nq; ++i) {
        if (audio_query_error(queries[i], INT64_MAX / 2, INT64_MAX / 2)) return 0;
        m[i] = (long)queries[i].m;
        n[i] = (long)(queries[i].win_len - queries[i].m + 1);
    }
    return vse_audio_match_ws(m, n, nq);
}

int vse_audio_match(vse_ctx* c, const uint8_t* d_src, int64_t src_len, const uint8_t* d_dst, int64_t dst_len, const vse_audio_query* queries,
                    int nq, void* d_ws, size_t ws_bytes, vse_audio_match_result* d_out, void* stream) {
    if (!c || !d_src || !d_dst || !queries || !d_ws || !d_out || (reinterpret_cast<uintptr_t>(d_out) & 7) ||
        (reinterpret_cast<uintptr_t>(d_ws) & 255)) {
        set_err("vse_audio_match: null or misaligned pointer");
        return VSE_E_INVAL;
    }
    if (nq < 1 || nq > 3) {
        set_err("vse_audio_match: %d queries (1..3 per call)", nq);
        return VSE_E_INVAL;
    }
    const uint8_t* pat[3];
    const uint8_t* win[3];
    long m[3], n[3];
    for (int i = 0; i < nq; ++i) {
        const vse_audio_query& q = queries[i];
        if (const char* why = audio_query_error(q, src_len, dst_len)) {
            set_err("vse_audio_match: query %d (pattern %lld + %lld of %lld, window %lld + %lld of %lld): %s", i, (long long)q.src_off,
                    (long long)q.m, (long long)src_len, (long long)q.dst_off, (long long)q.win_len, (long long)dst_len, why);
            return VSE_E_INVAL;
        }
        pat[i] = d_src + q.src_off;
        win[i] = d_dst + q.dst_off;
        m[i] = (long)q.m;
        n[i] = (long)(q.win_len - q.m + 1);
    }
    const size_t need = vse_audio_match_ws(m, n, nq);
    if (ws_bytes < need) {
        set_err("vse_audio_match: workspace of %zu bytes, %zu needed", ws_bytes, need);
        return VSE_E_INVAL;
    }
    const int rc = vse_audio_match_launch(pat, win, m, n, nq, d_ws, reinterpret_cast<unsigned long long*>(d_out), stream);
    if (rc != VSE_OK) set_err("vse_audio_match: launch failed: %s", hipGetErrorString(hipGetLastError()));
    return rc;
}

// The kernel a record launches, spelled as rocprofv3 reports it (thread-local storage); no plan, context or GPU needed.
const char* vse_op_kernel_name(const vse_op* op) {
    static thread_local char buf[96];
    buf[0] = 0;
    if (!op) return buf;
    const vse_op& o = *op;
    static const char* simple[] = {"", "", "dwconv_kernel", "pool_kernel", "gap_kernel", "scale_kernel", "binary_kernel", "resize_kernel",
                                   "unary_kernel", "layernorm_kernel", "attn_kernel", "softmax_kernel", "lstm_kernel", "wscale_kernel", "chain_kernel"};
    if (o.kind != OP_CONV) {
        snprintf(buf, sizeof buf, "%s", (o.kind >= 2 && o.kind <= OP_CHAIN) ? simple[o.kind] : "?");
        return buf;
    }
    auto shape = [](const vse_view& v) { return TView{nullptr, v.n, v.h, v.w, v.c, v.ld, v.esize}; };
    const ConvParams p = conv_params(o, shape(o.in0), shape(o.in1), shape(o.in2), shape(o.out), shape(o.out2), nullptr, nullptr, nullptr, nullptr,
                                     SrcGeom{0, 0, 0, 0});
    conv_kernel_name(conv_select(p, o.p[P_KTOT]), buf, sizeof buf);
    return buf;
}

int vse_plan_profile(vse_plan* p, void* ws, void* const* ext, int n_ext, const int32_t* d_widths, void* stream, float* ms) {
    if (!ms) return VSE_E_INVAL;
    int rc0 = check_run(p, ws, ext, n_ext, d_widths, "vse_plan_profile");
    if (rc0 != VSE_OK) return rc0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int n = (int)p->ops.size();
    std::vector<hipEvent_t> ev(n + 1);
    for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
    HIP_TRY(hipEventRecord(ev[0], st));
    for (int i = 0; i < n; ++i) {
        int rc = run_op(p, i, reinterpret_cast<char*>(ws), ext, d_widths, st, SrcGeom{p->src_h, p->src_w, p->src_pitch, p->src_fstride});
        if (rc != VSE_OK) return rc;
        HIP_TRY(hipEventRecord(ev[i + 1], st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
    // a max-pool that ran inside the conv in front of it launched nothing: its time is the conv's, and it reports exactly 0
    for (int i = 1; i < n; ++i)
        if (p->pooled[i - 1].family == CK_C3POOL || p->scale_add[i - 1]) ms[i] = 0.f;      // (likewise an add that ran with its gate multiply)
    for (auto& e : ev) (void)hipEventDestroy(e);
    return VSE_OK;
}

}  // extern "C"
