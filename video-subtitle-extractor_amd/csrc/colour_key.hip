// Colour key of the selectors' band (vse_colour_key, include/vse_hip.h): every pixel of the area becomes (K, K, K) with
//   d = max(|B - key_b|, |G - key_g|, |R - key_r|),  K = max(0, 255 - ((d * slope) >> 8))          (d * slope <= 255 * 65280 < 2^24)
// so the luma the selectors take of it, (29 K + 150 K + 77 K + 128) >> 8, is K itself and every kernel of frame_change.hip runs on the
// keyed band unchanged.  The integers are the specification (tests/colour_key_ref.py restates them in numpy).
// HBM-bound byte work, 3 bytes read and 3 written per pixel, no LDS, no scratch, no atomics.  Two kernels:
//   fast     a lane owns the 16 pixels of one 16-pixel column group of a row: three 16-byte loads, three 16-byte stores.  Taken where
//            base, pitch and frame stride of both sides are 16-byte aligned; the area's columns are widened to the groups that hold
//            them, so x0 does not matter.  A group that the frame's right edge cuts short goes pixel by pixel.
//   general  a lane owns one pixel of the area, any size / pitch / stride / byte alignment: byte loads and byte stores.
// K is clamped BEFORE the shift, min(d * slope, 65535) >> 8 (the same value): see clip8 in yuv.hip for what hipcc made of
// shift-then-clamp on bytes that share a dword on this target.
#include <cstdio>

#include "common.h"

void vse_set_error(const char* msg);      // vse_runtime.hip

namespace {

constexpr int CK_THREADS = 256;

struct CkArgs {
    const uint8_t* src;
    uint8_t* dst;
    long pitch, fstride, opitch, ofstride;
    int n, src_w, y0, rows, x0, x1;
    int kb, kg, kr, slope;
};

__device__ __forceinline__ unsigned ck_key(unsigned b, unsigned g, unsigned r, const CkArgs& a) {
    const int db = abs((int)b - a.kb), dg = abs((int)g - a.kg), dr = abs((int)r - a.kr);
    const unsigned d = (unsigned)max(max(db, dg), dr);
    return 255u - (min((unsigned)__umul24(d, (unsigned)a.slope), 65535u) >> 8);
}

__device__ __forceinline__ unsigned ck_byte(const unsigned (&w)[12], int i) { return (w[i >> 2] >> (8 * (i & 3))) & 255u; }

// grid.x: the (row, group) pairs of one frame in chunks of CK_THREADS, grid.y: frames (strided when there are more than the grid holds)
__global__ __launch_bounds__(CK_THREADS) void colour_key_fast_kernel(CkArgs a, int g0, int groups) {
    const long item = (long)blockIdx.x * CK_THREADS + threadIdx.x;
    if (item >= (long)a.rows * groups) return;
    const int row = (int)(item / groups), px = (g0 + (int)(item - (long)row * groups)) * 16;
    const long off = (long)(a.y0 + row) * a.pitch + 3L * px, ooff = (long)(a.y0 + row) * a.opitch + 3L * px;
    for (int f = blockIdx.y; f < a.n; f += gridDim.y) {
        const uint8_t* s = a.src + f * a.fstride + off;
        uint8_t* o = a.dst + f * a.ofstride + ooff;
        if (px + 16 <= a.src_w) {
            unsigned w[12], k[16];
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const uint4 v = reinterpret_cast<const uint4*>(s)[q];
                w[4 * q] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int p = 0; p < 16; ++p) k[p] = ck_key(ck_byte(w, 3 * p), ck_byte(w, 3 * p + 1), ck_byte(w, 3 * p + 2), a);
#pragma unroll
            for (int q = 0; q < 3; ++q) {           // four pixels make three dwords: K0 K0 K0 K1 | K1 K1 K2 K2 | K2 K3 K3 K3
                unsigned d[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = 4 * q + e, p = 4 * (j / 3);
                    d[e] = j % 3 == 0 ? k[p] * 0x010101u | k[p + 1] << 24
                         : j % 3 == 1 ? k[p + 1] * 0x0101u | k[p + 2] * 0x01010000u
                                      : k[p + 2] | k[p + 3] * 0x01010100u;
                }
                reinterpret_cast<uint4*>(o)[q] = make_uint4(d[0], d[1], d[2], d[3]);
            }
        } else {
            for (int p = 0; p < a.src_w - px; ++p) {
                const uint8_t k = (uint8_t)ck_key(s[3 * p], s[3 * p + 1], s[3 * p + 2], a);
                o[3 * p] = o[3 * p + 1] = o[3 * p + 2] = k;
            }
        }
    }
}

// grid.x: the pixels of one frame's area in chunks of CK_THREADS, grid.y: frames
__global__ __launch_bounds__(CK_THREADS) void colour_key_general_kernel(CkArgs a) {
    const int aw = a.x1 - a.x0;
    const long item = (long)blockIdx.x * CK_THREADS + threadIdx.x;
    if (item >= (long)a.rows * aw) return;
    const int row = (int)(item / aw), x = a.x0 + (int)(item - (long)row * aw);
    const long off = (long)(a.y0 + row) * a.pitch + 3L * x, ooff = (long)(a.y0 + row) * a.opitch + 3L * x;
    for (int f = blockIdx.y; f < a.n; f += gridDim.y) {
        const uint8_t* s = a.src + f * a.fstride + off;
        uint8_t* o = a.dst + f * a.ofstride + ooff;
        const uint8_t k = (uint8_t)ck_key(s[0], s[1], s[2], a);
        o[0] = o[1] = o[2] = k;
    }
}

}  // namespace

extern "C" {

int vse_colour_key(vse_ctx* c, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0,
                   int x1, int key_b, int key_g, int key_r, int slope, void* d_out, int64_t out_pitch, int64_t out_frame_stride,
                   void* stream) {
    char msg[400];
    const int64_t row_bytes = (int64_t)src_w * 3;
    const bool frames_ok = c && n >= 0 && src_h > 0 && src_w > 0 && pitch >= row_bytes && out_pitch >= row_bytes &&
                           (n <= 1 || (frame_stride >= (int64_t)(src_h - 1) * pitch + row_bytes &&
                                       out_frame_stride >= (int64_t)(src_h - 1) * out_pitch + row_bytes)) &&
                           (n == 0 || (d_bgr && d_out));
    if (!frames_ok) {
        snprintf(msg, sizeof msg, "vse_colour_key: bad arguments (n %d of at least 0, frame %d x %d, pitch %lld and %lld of at least 3 * "
                 "src_w, frame stride %lld and %lld of at least a frame, no NULL pointer)", n, src_h, src_w, (long long)pitch,
                 (long long)out_pitch, (long long)frame_stride, (long long)out_frame_stride);
        vse_set_error(msg);
        return VSE_E_INVAL;
    }
    if (y0 < 0 || x0 < 0 || y1 > src_h || x1 > src_w || y1 <= y0 || x1 <= x0) {
        snprintf(msg, sizeof msg, "vse_colour_key: area [%d, %d) x [%d, %d) is empty or outside the %d x %d frame", y0, y1, x0, x1, src_h,
                 src_w);
        vse_set_error(msg);
        return VSE_E_INVAL;
    }
    if ((key_b | key_g | key_r) < 0 || key_b > 255 || key_g > 255 || key_r > 255 || slope < 256 || slope > 65280) {
        snprintf(msg, sizeof msg, "vse_colour_key: key (%d, %d, %d) outside 0..255, or slope %d outside 256..65280", key_b, key_g, key_r,
                 slope);
        vse_set_error(msg);
        return VSE_E_INVAL;
    }
    if (n == 0) return VSE_OK;
    // the bytes either side may touch: rows [y0, y1) of frames 0 .. n - 1, whole rows of 3 * src_w bytes
    const uintptr_t in0 = reinterpret_cast<uintptr_t>(d_bgr) + (uintptr_t)(y0 * pitch);
    const uintptr_t in1 = reinterpret_cast<uintptr_t>(d_bgr) + (uintptr_t)((n - 1) * frame_stride + (y1 - 1) * pitch + row_bytes);
    const uintptr_t out0 = reinterpret_cast<uintptr_t>(d_out) + (uintptr_t)(y0 * out_pitch);
    const uintptr_t out1 = reinterpret_cast<uintptr_t>(d_out) + (uintptr_t)((n - 1) * out_frame_stride + (y1 - 1) * out_pitch + row_bytes);
    if (in0 < out1 && out0 < in1) {
        vse_set_error("vse_colour_key: the input and output byte ranges overlap (the key is not taken in place)");
        return VSE_E_INVAL;
    }
    CkArgs a;
    a.src = static_cast<const uint8_t*>(d_bgr), a.dst = static_cast<uint8_t*>(d_out);
    a.pitch = pitch, a.fstride = frame_stride, a.opitch = out_pitch, a.ofstride = out_frame_stride;
    a.n = n, a.src_w = src_w, a.y0 = y0, a.rows = y1 - y0, a.x0 = x0, a.x1 = x1;
    a.kb = key_b, a.kg = key_g, a.kr = key_r, a.slope = slope;
    const bool fast = !((reinterpret_cast<uintptr_t>(d_bgr) | reinterpret_cast<uintptr_t>(d_out) | (uintptr_t)pitch | (uintptr_t)out_pitch |
                         (uintptr_t)(n > 1 ? frame_stride : 0) | (uintptr_t)(n > 1 ? out_frame_stride : 0)) & 15);
    const int g0 = x0 / 16, groups = (x1 + 15) / 16 - g0;
    const int64_t items = (int64_t)a.rows * (fast ? groups : x1 - x0);
    const int64_t blocks = (items + CK_THREADS - 1) / CK_THREADS;
    if (blocks > 0x7fffffffLL) {
        vse_set_error("vse_colour_key: the area has more than 2^39 pixels");
        return VSE_E_INVAL;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks, (unsigned)(n < 65535 ? n : 65535)), block(CK_THREADS);
    if (fast)
        hipLaunchKernelGGL(colour_key_fast_kernel, grid, block, 0, st, a, g0, groups);
    else
        hipLaunchKernelGGL(colour_key_general_kernel, grid, block, 0, st, a);
    if (hipGetLastError() != hipSuccess) {
        vse_set_error("vse_colour_key: launch failed");
        return VSE_E_HIP;
    }
    return VSE_OK;
}

}  // extern "C"
