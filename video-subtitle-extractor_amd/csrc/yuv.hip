// YUV 4:2:0 -> BGR (vse_yuv420_to_bgr, include/vse_hip.h): what a decoder hands out (planar I420, semi-planar NV12, 1.5 bytes per pixel)
// becomes the uint8 BGR frames every other entry point takes, on the device, so the host stores, packs and uploads half the bytes.
// BT.601 limited range, nearest chroma; the integers are the specification (tests/yuv_ref.py restates them in numpy, bit for bit):
//   c = max(Y - 16, 0) * 1220542, u = U - 128, v = V - 128                      (U, V of chroma row (r + row_parity) >> 1, column x >> 1)
//   B = clip8((c + 2116026 u + 2^19) >> 20), G = clip8((c - 409993 u - 852492 v + 2^19) >> 20), R = clip8((c + 1673527 v + 2^19) >> 20)
// |sum| <= 560 969 128: int32 is exact.  Every factor fits 24 bits, so the products are the full-rate 24-bit multiplies.
// vse_yuv_to_bgr_matrix picks the matrix: 0 is the above, 1 is BT.709 limited range (what HD encodes normally carry), the same c, rounding
// term, shift and clip8 with the chroma factors 2215014 (B), -223607 u - 558796 v (G), 1879825 (R) = round(k * 2^20) of 2 (1 - Kb) 255/224,
// 2 Kb (1 - Kb) / Kg 255/224, 2 Kr (1 - Kr) / Kg 255/224, 2 (1 - Kr) 255/224 with Kr = 0.2126, Kb = 0.0722 (tests/yuv709_ref.py restates
// them).  Each is below 2^23 and |sum| <= 573 540 604, so the same int32 / 24-bit argument holds.  The matrix is a template parameter of
// both kernels: the factors stay literals.
// HBM-bound byte work, 1.5 bytes read and 3 written per pixel.  Two kernels:
//   fast     a lane owns 16 pixels x 2 rows: two 16-byte luma loads, 8 + 8 bytes of U and V (I420) or 16 bytes of UV (NV12), six 16-byte
//            stores; the chroma terms are computed once for both rows.  Needs w % 16 == 0, even h, row_parity 0, and 16-byte aligned
//            bases, pitch and frame strides.
//   general  a lane owns 4 pixels of one row, any size / pitch / parity / byte alignment: dword stores where the row is 4-byte aligned
//            and the 4 pixels exist, byte stores otherwise.
//
// vse_yuv_to_bgr_format (include/vse_hip.h) widens this to what else a decoder hands out: 4:4:4 / 4:2:2 / 4:2:0 / grey, 8 to 16 bits (1-byte
// samples at depth 8, 2-byte little-endian ones above, the value in the low bits or, P010-style, in the high bits), planar or semi-planar,
// BT.601 / BT.709 / BT.2020 (non-constant luminance), limited or full range.  No transfer function is applied.  With s = depth - 8:
//   Y, U, V = min(word >> shift, 2^depth - 1)           (shift = 16 - depth for high-bit words, else 0)
//   c = max(Y - yoff, 0) * KY_s, u = U - (128 << s), v = V - (128 << s)   (yoff = 16 << s, limited; 0 and KY_0 = 2^20, full; grey: u = v = 0)
//   B = clip8((c + BU_s u + 2^19) >> 20), G = clip8((c + GU_s u + GV_s v + 2^19) >> 20), R = clip8((c + RV_s v + 2^19) >> 20)
//   K_s = sign(K_0) ((|K_0| + ((1 << s) >> 1)) >> s)
// K_0: limited BT.601 / BT.709 the literals above; limited BT.2020 the same derivation with Kr = 0.2627, Kb = 0.0593: 2245811 (B), -196426 u
// - 682019 v (G), 1760217 (R); full range round(k * 2^20) of 2 (1 - Kb), 2 Kb (1 - Kb) / Kg, 2 Kr (1 - Kr) / Kg, 2 (1 - Kr), no 255/224:
// BT.601 1858077, -360853, -748826, 1470104; BT.709 1945738, -196424, -490864, 1651297; BT.2020 1972791, -172546, -599107, 1546230.
// int32: Y - yoff < 2^depth and KY_s <= (KY_0 >> s) + 1, so c < 2^8 KY_0 + 2^16 <= 312 524 288; |u|, |v| <= 2^(depth - 1) and |K_s| <=
// (|K_0| >> s) + 1, so a chroma product is at most 2^7 |K_0| + 2^15 and the largest sum, limited BT.2020's B, stays below 312 524 288 +
// 287 496 576 + 2^19 = 600 545 152 (G's two products together are smaller: at most 2^7 (409993 + 852492) + 2^16, BT.601's); every operand
// fits 24 signed bits (samples 17, |K_s| < 2^23), so the products are the 24-bit multiplies.  shift, 2^depth - 1, the two offsets and the
// five factors are kernel arguments (wave-uniform); the kernels are templated on what changes the loads alone, the sample width and the
// chroma arrangement:
//   fast     2-byte 4:2:0, planar (yuv420p10le ...) or semi-planar (P010 ...): the shape of the 8-bit one, a lane owns 16 pixels x 2 rows:
//            four 16-byte luma loads, two 16-byte chroma loads, six 16-byte stores, the chroma terms once for both rows.  Same conditions.
//   general  any format: a lane owns 4 pixels of one row; 2-byte formats need 2-byte aligned bases and strides.
// 8-bit 4:2:0 limited BT.601 / BT.709 goes to the two 8-bit kernels above and gives their bytes.
//
// vse_yuv_to_bgr_tonemap (include/vse_hip.h) is the same two kernels with another end (ToneOut below in place of PlainOut): the sums are
// shifted by 16 to 12-bit codes, which go through a linearising / tone-mapping table, a 3 x 3 gamut matrix and an output gamma table
// (tests/tonemap_ref.py restates the integers).  The tables are staged into LDS once per block, so its launches cap the grid (TONE_MAX_BLOCKS).
//
// vse_yuv_deinterlace (include/vse_hip.h) stands in front of all of them for interlaced pictures: packed pictures of any format above
// become progressive pictures of the same format, which the conversions then take unchanged.  Motion-adaptive, per plane (Y, U, V or the
// interleaved UV plane, the samples as stored words), up and down a column only; tests/deinterlace_ref.py restates it in int64:
//   out[y] = C[y]                                                             rows of the first field (y & 1 == keep), and a one-row plane
//   moved  = no previous picture, or mode interpolate, or |C[r] - P[r]| > T for a row r of {y - 1, y, y + 1} inside the plane
//   out[y] = moved ? (a + b + 1) >> 1 : C[y],  a = C[y - 1] (C[y + 1] on row 0), b = C[y + 1] (C[y - 1] on the last row)
// T = thresh << (depth - 8), and << (16 - depth) more for high-bit words: at most 255 << 8, and |C - P| < 2^16, so int32 is exact.
// What stood still (a subtitle) keeps its full vertical resolution; what moved loses the second field.  HBM-bound byte work without
// LDS, three packed pictures of traffic per frame (read C, read P, write), templated on the sample width alone:
//   fast     a lane owns one 16-byte column of a plane and walks down a strip of 8 rows, carrying the row above and the row below with
//            their `moved` masks in registers: every row of C and P is loaded once per strip, plus the strip's two halo rows.  The
//            arithmetic is on whole dwords: the rounded mean is (a | b) - (((a ^ b) >> 1) & 0x7f7f7f7f) (0x7fff7fff for 2-byte
//            samples) and the choice a mask.  Needs every plane's base and row bytes and all frame strides 16-byte aligned.
//   general  the same walk on 4 samples, any width and byte alignment (2-byte samples: 2-byte aligned): the aligned dwords that hold them,
//            shifted into place, sample by sample at the end of a row; dword stores where they are aligned, else sample by sample.
//
// vse_yuv_field_match (include/vse_hip.h) stands in the deinterlacer's place for film carried in interlaced video (3:2 pulldown, fields
// shifted by one): every picture of the film is still in the stream, its second field in the neighbouring frame.  Per frame three whole
// pictures are candidates: the frame as stored (c), its first field with the previous frame's second (p1), its second field with the
// previous frame's first (p2); the one whose luma combs least is copied out, and a frame whose best candidate still combs in more than
// comb_limit per mille of its samples is video and gets the adaptive rule above (tests/field_match_ref.py restates it in int64).  Three
// enqueues on the stream, no LDS, no scratch: a memset of the stats, then
//   count    luma only, read once: the deinterlacer's walk (16-byte columns, or 4 samples where the luma rows are not 16-byte aligned)
//            with rows y - 1, y, y + 1 of both pictures in registers and three comb tests per row (C alone; C between P's rows; P
//            between C's rows, the last two booked to p1 or p2 by the row's parity); per-lane integer counts, a wave reduction by
//            shuffles, one integer atomic per wave and candidate into the frame's stats.
//   weave    every block reads its frame's three counts and derives the choice (uniform over the frame; one thread stores it); choices
//            0 to 2 copy each row of each plane from C or P, choice 3 runs the deinterlacer's strip walk (deint_strip16 /
//            deint_strip_quad, shared with its kernels).  The planes whose base and row bytes are 16-byte aligned go through one launch
//            of 16-byte moves, the others (the 360-byte chroma rows of a DVD under its 720-byte luma rows) through one of quads.
//
// vse_yuv_resample (include/vse_hip.h) stands behind those two and in front of the conversions for anamorphic pictures (DVD, HDV: pixels
// that are not square): packed pictures of w_in columns become packed pictures of w_out columns of the same format and height, every plane
// resampled along its rows.  The device knows tables, not filters (ingest.Resample builds them; tests/resample_ref.py restates the integers
// in int64): per plane left[P] (int32) and coef[P][K] (int16, Q14), K even and 2..16, and for a plane of pw stored columns
//   acc = sum over k < K of coef[x][k] * S[clamp(left[x] + k, 0, pw - 1)],   out = clip(0, 2^depth - 1, (acc + 8192) >> 14)
// S the stored word, or word >> (16 - depth) for high-bit words (the result is stored << (16 - depth)); an interleaved UV plane is a plane
// of cw columns of two components that share the chroma table.  The host keeps sum |coef[x]| <= 32767, so with 16-bit samples every partial
// sum stays below 2^31; coefficients and samples fit 24 signed bits, so the products are the 24-bit multiplies.  One launch, no LDS, no
// scratch, no atomics: a lane owns four output samples of a plane (four columns, or two U V pairs) and walks down a strip of 8 rows
// with its columns' left and coefficients in registers (the table is read once per lane, not once per row); every source sample is a load
// of its own by its clamped index, which the vector cache serves (neighbouring lanes read neighbouring samples).  Templated on the sample
// width, planar / interleaved chroma, and an upper bound on the tap pairs (1, 2, 3, 4 or 8: the unrolled form keeps the coefficients in
// registers), in two forms that differ in the store alone (the loads are per sample in both; nothing is loaded wide or staged):
//   fast     every plane's base and row bytes and all strides 16-byte aligned: the four samples are always one 4-byte store (8-byte for
//            2-byte samples), without a test
//   general  any width and byte alignment (2-byte samples: 2-byte aligned): a dword where the four samples exist and lie aligned, sample
//            by sample otherwise (the 854-byte rows of a 16:9 NTSC DVD alternate between the two)
//
// vse_yuv_vscale (include/vse_hip.h) stands in front of that for UHD and other oversized progressive pictures: packed pictures of h_in
// rows become packed pictures of h_out rows of the same format and width, every plane filtered down its columns by a table of the same
// layout (top[Q], coef[Q][K]; ingest.VScale builds them, tests/vscale_ref.py restates the integers).  Input and output are row bands of
// their pictures (stored luma rows [s0, s1) in, output rows [y0, y1) out, chroma rows by the packing's rule), the tables are indexed in
// whole-picture rows, and a source row is clamped to the picture and then to the band, so no table can make a load leave the input.
// This pass coalesces by itself: a lane owns a run of a plane row, a wave makes one output row at a time, K row loads and one store per
// output row; the output row is the same in all lanes of a wave, so top, the coefficients and the clamped rows are scalar.  Templated
// on the sample width and a bound on the tap pairs (1, 2, 3, 4, 6, 8), in two forms:
//   fast     bases, frame strides and every plane's row bytes and offsets in both bands 16-byte aligned: the run is 16 bytes, one
//            load per tap and one store
//   general  any width, pitch and byte alignment: the run is four samples through load_quad / store_quad
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <type_traits>

#include "common.h"
#include "yuv_planes.h"

void vse_set_error(const char* msg);      // vse_runtime.hip

namespace {

constexpr int YUV_I420 = 0, YUV_NV12 = 1;
constexpr int BT601 = 0, BT709 = 1;
constexpr int FAST_THREADS = 256, FAST_MAX_BLOCKS = 2048;
constexpr int GEN_LANES = 64, GEN_ROWS = 4;        // block of the general kernel: 64 pixel groups x 4 rows

struct ChromaTerms {
    int b, g, r;      // the chroma part of each channel's sum, rounding constant included
};

template <int MATRIX>
__device__ __forceinline__ ChromaTerms chroma_terms(int U, int V) {
    constexpr int BU = MATRIX == BT709 ? 2215014 : 2116026, GU = MATRIX == BT709 ? -223607 : -409993;
    constexpr int GV = MATRIX == BT709 ? -558796 : -852492, RV = MATRIX == BT709 ? 1879825 : 1673527;
    const int u = U - 128, v = V - 128;
    ChromaTerms t;
    t.b = __mul24(u, BU) + (1 << 19);
    t.g = __mul24(u, GU) + __mul24(v, GV) + (1 << 19);
    t.r = __mul24(v, RV) + (1 << 19);
    return t;
}

// clip8(x >> 20), clamped BEFORE the shift (the same value: floor, then 0..255).  Shift-then-clamp is folded by hipcc into gfx950's
// v_ashr_pk_u8_i32 wherever two neighbouring bytes of a dword come from it, and those bytes differed from the integers above on the
// device (the G of a quad's third pixel read 127 for 124 at Y, U, V = 254, 255, 255) while the unfused ones were right.
__device__ __forceinline__ unsigned clip8(int x) { return (unsigned)min(max(x, 0), (255 << 20) | 0xfffff) >> 20; }

// 4 pixels (luma bytes of `yw`, low byte first; chroma terms t0 for pixels 0-1, t1 for pixels 2-3) -> 12 bytes B G R B G R ...
__device__ __forceinline__ void bgr4(unsigned yw, const ChromaTerms& t0, const ChromaTerms& t1, unsigned& d0, unsigned& d1, unsigned& d2) {
    unsigned b[4], g[4], r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int y = (int)((yw >> (8 * k)) & 255u);
        const int c = __mul24(max(y - 16, 0), 1220542);
        const ChromaTerms& t = k < 2 ? t0 : t1;
        b[k] = clip8(c + t.b);
        g[k] = clip8(c + t.g);
        r[k] = clip8(c + t.r);
    }
    d0 = b[0] | (g[0] << 8) | (r[0] << 16) | (b[1] << 24);
    d1 = g[1] | (r[1] << 8) | (b[2] << 16) | (g[2] << 24);
    d2 = r[2] | (b[3] << 8) | (g[3] << 16) | (r[3] << 24);
}

// 16 pixels of one row -> 48 bytes as three 16-byte stores
__device__ __forceinline__ void row16(const uint4& y, const ChromaTerms (&t)[8], uint8_t* dst) {
    const unsigned yw[4] = {y.x, y.y, y.z, y.w};
    unsigned o[12];
#pragma unroll
    for (int q = 0; q < 4; ++q) bgr4(yw[q], t[2 * q], t[2 * q + 1], o[3 * q], o[3 * q + 1], o[3 * q + 2]);
    uint4* d = reinterpret_cast<uint4*>(dst);
    d[0] = make_uint4(o[0], o[1], o[2], o[3]);
    d[1] = make_uint4(o[4], o[5], o[6], o[7]);
    d[2] = make_uint4(o[8], o[9], o[10], o[11]);
}

// Work item i of a frame = (row pair i / cgs, 16-pixel column group i % cgs); consecutive lanes take consecutive column groups, so
// a wave's luma loads are contiguous and its stores cover contiguous 3 KiB runs of two output rows.  blockIdx.y strides the frames.
template <int LAYOUT, int MATRIX>
__global__ __launch_bounds__(FAST_THREADS) void yuv420_fast_kernel(const uint8_t* __restrict__ src, int n, int h, int w, long sstride,
                                                                   uint8_t* __restrict__ dst, long pitch, long dstride) {
    const unsigned cgs = (unsigned)w >> 4, items = ((unsigned)h >> 1) * cgs;
    const long plane = (long)h * w, cw = w >> 1;
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const uint8_t* s = src + (long)f * sstride;
        uint8_t* d = dst + (long)f * dstride;
        for (unsigned i = blockIdx.x * FAST_THREADS + threadIdx.x; i < items; i += gridDim.x * FAST_THREADS) {
            const unsigned rp = i / cgs, cg = i - rp * cgs;
            const uint8_t* yp = s + (long)(2 * rp) * w + 16 * cg;
            const uint4 y0 = *reinterpret_cast<const uint4*>(yp);
            const uint4 y1 = *reinterpret_cast<const uint4*>(yp + w);
            ChromaTerms t[8];
            if (LAYOUT == YUV_I420) {
                const uint8_t* up = s + plane + (long)rp * cw + 8 * cg;
                const uint2 u = *reinterpret_cast<const uint2*>(up);
                const uint2 v = *reinterpret_cast<const uint2*>(up + (plane >> 2));
                const unsigned uw[2] = {u.x, u.y}, vw[2] = {v.x, v.y};
#pragma unroll
                for (int k = 0; k < 8; ++k) t[k] = chroma_terms<MATRIX>((int)((uw[k >> 2] >> (8 * (k & 3))) & 255u), (int)((vw[k >> 2] >> (8 * (k & 3))) & 255u));
            } else {
                const uint4 uv = *reinterpret_cast<const uint4*>(s + plane + (long)rp * w + 16 * cg);
                const unsigned q[4] = {uv.x, uv.y, uv.z, uv.w};
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const unsigned p = q[k >> 1] >> (16 * (k & 1));
                    t[k] = chroma_terms<MATRIX>((int)(p & 255u), (int)((p >> 8) & 255u));
                }
            }
            uint8_t* o = d + (long)(2 * rp) * pitch + 48 * cg;
            row16(y0, t, o);
            row16(y1, t, o + pitch);
        }
    }
}

// Lane (threadIdx.x, threadIdx.y) = pixels 4 xg .. 4 xg + 3 of one row; blockIdx.y strides the rows, blockIdx.z the frames.
template <int LAYOUT, int MATRIX>
__global__ __launch_bounds__(GEN_LANES * GEN_ROWS) void yuv420_general_kernel(const uint8_t* __restrict__ src, int n, int h, int w, int parity,
                                                                              long sstride, uint8_t* __restrict__ dst, long pitch, long dstride) {
    const int x = 4 * (int)(blockIdx.x * GEN_LANES + threadIdx.x);
    if (x >= w) return;
    const int npx = min(4, w - x);
    const long plane = (long)h * w, cw = (w + 1) >> 1, ch = (h + parity + 1) >> 1;
    const int c0 = x >> 1, c1 = npx > 2 ? c0 + 1 : c0;         // chroma columns of pixels 0-1 and 2-3 (the second only if pixel 2 exists)
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        const uint8_t* s = src + (long)f * sstride;
        uint8_t* d = dst + (long)f * dstride;
        for (int r = blockIdx.y * GEN_ROWS + threadIdx.y; r < h; r += gridDim.y * GEN_ROWS) {
            const uint8_t* yp = s + (long)r * w + x;
            unsigned yw = 0;
            if (npx == 4 && (reinterpret_cast<uintptr_t>(yp) & 3) == 0) {
                yw = *reinterpret_cast<const unsigned*>(yp);
            } else {
                for (int k = 0; k < npx; ++k) yw |= (unsigned)yp[k] << (8 * k);
            }
            const long cr = (r + parity) >> 1;
            ChromaTerms t0, t1;
            if (LAYOUT == YUV_I420) {
                const uint8_t* up = s + plane + cr * cw;
                const uint8_t* vp = up + ch * cw;
                t0 = chroma_terms<MATRIX>(up[c0], vp[c0]);
                t1 = chroma_terms<MATRIX>(up[c1], vp[c1]);
            } else {
                const uint8_t* uv = s + plane + cr * 2 * cw;
                t0 = chroma_terms<MATRIX>(uv[2 * c0], uv[2 * c0 + 1]);
                t1 = chroma_terms<MATRIX>(uv[2 * c1], uv[2 * c1 + 1]);
            }
            unsigned o[3];
            bgr4(yw, t0, t1, o[0], o[1], o[2]);
            uint8_t* op = d + (long)r * pitch + 3 * (long)x;
            if (npx == 4 && (reinterpret_cast<uintptr_t>(op) & 3) == 0) {
                unsigned* o4 = reinterpret_cast<unsigned*>(op);
                o4[0] = o[0];
                o4[1] = o[1];
                o4[2] = o[2];
            } else {
                for (int k = 0; k < 3 * npx; ++k) op[k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
            }
        }
    }
}

// ---- any format (vse_yuv_to_bgr_format) -----------------------------------------------------------------------------------------
struct YuvParams {
    int shift, maxv;              // sample = min(word >> shift, maxv)
    int yoff, coff;               // 16 << s (0: full range), 128 << s
    int ky, bu, gu, gv, rv;       // K_s
};

__device__ __forceinline__ int sample_of(unsigned word, const YuvParams& p) { return min((int)(word >> p.shift), p.maxv); }

__device__ __forceinline__ int luma_term(int Y, const YuvParams& p) { return __mul24(max(Y - p.yoff, 0), p.ky); }

// `half` is the rounding constant of the shift that follows: 2^19 in front of >> 20, 2^15 in front of the tone-mapped route's >> 16
__device__ __forceinline__ ChromaTerms chroma_terms(int U, int V, const YuvParams& p, int half = 1 << 19) {
    const int u = U - p.coff, v = V - p.coff;
    ChromaTerms t;
    t.b = __mul24(u, p.bu) + half;
    t.g = __mul24(u, p.gu) + __mul24(v, p.gv) + half;
    t.r = __mul24(v, p.rv) + half;
    return t;
}

// What becomes of a pixel's three sums (luma term + chroma term, rounding constant included) is a policy of the two kernels below.
// PlainOut: the bytes of vse_yuv_to_bgr_format.
struct PlainOut {
    struct Args {};
    static constexpr bool TONE = false;
    static constexpr int HALF = 1 << 19;
    static __device__ __forceinline__ PlainOut begin(const Args&, int, int) { return PlainOut(); }
    __device__ __forceinline__ void operator()(int c, const ChromaTerms& t, unsigned& b, unsigned& g, unsigned& r) const {
        b = clip8(c + t.b);
        g = clip8(c + t.g);
        r = clip8(c + t.r);
    }
};

// ToneOut: vse_yuv_to_bgr_tonemap.  The sums shifted by 16 are 12-bit codes E; L = A[E] is linear light, P = clip16((M L + 2^13) >> 14) the
// gamut-mapped light, T[P < 4096 ? P : 3840 + (P >> 4)] the byte.  The kernel knows two tables and nine integers, nothing of PQ or HLG.
// int32: a row of M has positive entries that sum to at most 32767 and negative ones that sum to at least -32768 (checked on the host)
// and L <= 65535, so every partial sum lies in [-32768 * 65535, 32767 * 65535 + 2^13], inside int32; |M| <= 2^15 and L < 2^16 fit 24
// signed bits, so the products are the 24-bit multiplies.  Both clips are made before their shift, as clip8's is.
// The tables live in LDS, A then T as the host stores them (uint16[4096], uint8[7936]: 16 128 bytes): six gathers per pixel with
// data-dependent addresses.  They are left packed: a bank is a dword, so neighbouring codes (2 of A, 4 of T) share one, and lanes of a
// wave hold neighbouring pixels, whose codes in real pictures are close: equal dwords are one broadcast, near ones fall into
// different banks.  Widening A to a dword per entry would spread the same codes over 32 banks no better and double the staging.
constexpr int TONE_A = 4096, TONE_T = 7936, TONE_BYTES = 2 * TONE_A + TONE_T, TONE_VECS = TONE_BYTES / 16;
static_assert(TONE_BYTES % 16 == 0, "the table is staged by 16-byte loads");

struct ToneOut {
    struct Args {
        const uint4* table;      // device, 16-byte aligned: A then T
        int m[9];                // rows R, G, B over columns R, G, B, Q14
    };
    static constexpr bool TONE = true;
    static constexpr int HALF = 1 << 15;
    const uint16_t* A;
    const uint8_t* T;
    int m[9];

    // every thread of the block calls this once, before anything else: the block's copy of the table
    static __device__ __forceinline__ ToneOut begin(const Args& a, int tid, int threads) {
        __shared__ uint4 lds[TONE_VECS];
        for (int i = tid; i < TONE_VECS; i += threads) lds[i] = a.table[i];
        __syncthreads();
        ToneOut o;
        o.A = reinterpret_cast<const uint16_t*>(lds);
        o.T = reinterpret_cast<const uint8_t*>(lds) + 2 * TONE_A;
#pragma unroll
        for (int k = 0; k < 9; ++k) o.m[k] = a.m[k];
        return o;
    }
    __device__ __forceinline__ int light(int sum) const { return A[min(max(sum, 0), (4095 << 16) | 0xffff) >> 16]; }
    __device__ __forceinline__ unsigned byte_of(const int* row, int lr, int lg, int lb) const {
        const int s = __mul24(row[0], lr) + __mul24(row[1], lg) + __mul24(row[2], lb) + (1 << 13);
        const int p = min(max(s, 0), (65535 << 14) | 0x3fff) >> 14;
        return T[p < 4096 ? p : 3840 + (p >> 4)];
    }
    __device__ __forceinline__ void operator()(int c, const ChromaTerms& t, unsigned& b, unsigned& g, unsigned& r) const {
        const int lb = light(c + t.b), lg = light(c + t.g), lr = light(c + t.r);
        r = byte_of(m, lr, lg, lb);
        g = byte_of(m + 3, lr, lg, lb);
        b = byte_of(m + 6, lr, lg, lb);
    }
};

// 4 pixels (luma terms c, chroma terms t) -> 12 bytes B G R B G R ...
template <class OUT>
__device__ __forceinline__ void pack4(const int (&c)[4], const ChromaTerms (&t)[4], const OUT& out, unsigned& d0, unsigned& d1, unsigned& d2) {
    unsigned b[4], g[4], r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) out(c[k], t[k], b[k], g[k], r[k]);
    d0 = b[0] | (g[0] << 8) | (r[0] << 16) | (b[1] << 24);
    d1 = g[1] | (r[1] << 8) | (b[2] << 16) | (g[2] << 24);
    d2 = r[2] | (b[3] << 8) | (g[3] << 16) | (r[3] << 24);
}

// 16 pixels of one row of 2-byte samples (ya: pixels 0-7, yb: pixels 8-15; t[k]: pixels 2 k, 2 k + 1) -> 48 bytes as three 16-byte stores
template <class OUT>
__device__ __forceinline__ void row16_wide(const uint4& ya, const uint4& yb, const ChromaTerms (&t)[8], const YuvParams& p, const OUT& out,
                                           uint8_t* dst) {
    const unsigned yw[8] = {ya.x, ya.y, ya.z, ya.w, yb.x, yb.y, yb.z, yb.w};
    unsigned o[12];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int c[4] = {luma_term(sample_of(yw[2 * q] & 0xffffu, p), p), luma_term(sample_of(yw[2 * q] >> 16, p), p),
                          luma_term(sample_of(yw[2 * q + 1] & 0xffffu, p), p), luma_term(sample_of(yw[2 * q + 1] >> 16, p), p)};
        const ChromaTerms tq[4] = {t[2 * q], t[2 * q], t[2 * q + 1], t[2 * q + 1]};
        pack4(c, tq, out, o[3 * q], o[3 * q + 1], o[3 * q + 2]);
    }
    uint4* d = reinterpret_cast<uint4*>(dst);
    d[0] = make_uint4(o[0], o[1], o[2], o[3]);
    d[1] = make_uint4(o[4], o[5], o[6], o[7]);
    d[2] = make_uint4(o[8], o[9], o[10], o[11]);
}

// yuv420_fast_kernel for 2-byte samples: the same work items and strides; sstride, the planes and the rows are counted in bytes.
// With ToneOut the launcher caps the grid, so that a block stages the table once and then walks several items and frames.
template <int CHROMA, class OUT>
__global__ __launch_bounds__(FAST_THREADS) void yuv420_wide_fast_kernel(const uint8_t* __restrict__ src, int n, int h, int w, long sstride,
                                                                        uint8_t* __restrict__ dst, long pitch, long dstride, YuvParams p,
                                                                        typename OUT::Args oa) {
    const OUT out = OUT::begin(oa, threadIdx.x, FAST_THREADS);
    const unsigned cgs = (unsigned)w >> 4, items = ((unsigned)h >> 1) * cgs;
    const long lrow = 2L * w, plane = (long)h * lrow;              // bytes of a luma row (= of a semi-planar chroma row) and of the luma plane
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const uint8_t* s = src + (long)f * sstride;
        uint8_t* d = dst + (long)f * dstride;
        for (unsigned i = blockIdx.x * FAST_THREADS + threadIdx.x; i < items; i += gridDim.x * FAST_THREADS) {
            const unsigned rp = i / cgs, cg = i - rp * cgs;
            const uint8_t* yp = s + (long)(2 * rp) * lrow + 32 * cg;
            const uint4 y0a = *reinterpret_cast<const uint4*>(yp), y0b = *reinterpret_cast<const uint4*>(yp + 16);
            const uint4 y1a = *reinterpret_cast<const uint4*>(yp + lrow), y1b = *reinterpret_cast<const uint4*>(yp + lrow + 16);
            ChromaTerms t[8];
            if (CHROMA == CHROMA_PLANAR) {
                const uint8_t* up = s + plane + (long)rp * w + 16 * cg;          // a chroma row is w / 2 samples = w bytes
                const uint4 u = *reinterpret_cast<const uint4*>(up);
                const uint4 v = *reinterpret_cast<const uint4*>(up + (plane >> 2));
                const unsigned uw[4] = {u.x, u.y, u.z, u.w}, vw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    t[k] = chroma_terms(sample_of((uw[k >> 1] >> (16 * (k & 1))) & 0xffffu, p), sample_of((vw[k >> 1] >> (16 * (k & 1))) & 0xffffu, p), p,
                                         OUT::HALF);
            } else {
                const uint8_t* cp = s + plane + (long)rp * lrow + 32 * cg;
                const uint4 a = *reinterpret_cast<const uint4*>(cp), b = *reinterpret_cast<const uint4*>(cp + 16);
                const unsigned q[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
                for (int k = 0; k < 8; ++k) t[k] = chroma_terms(sample_of(q[k] & 0xffffu, p), sample_of(q[k] >> 16, p), p, OUT::HALF);
            }
            uint8_t* o = d + (long)(2 * rp) * pitch + 48 * cg;
            row16_wide(y0a, y0b, t, p, out, o);
            row16_wide(y1a, y1b, t, p, out, o + pitch);
        }
    }
}

// yuv420_general_kernel for any format: S is the sample type, the planes are counted in samples.  Chroma column (x + k) >> sub_x, chroma
// row (r + parity) >> sub_y; with sub_x = 1 pixels 0-1 and 2-3 share their terms (x is a multiple of 4).
template <typename S, int CHROMA, class OUT>
__global__ __launch_bounds__(GEN_LANES * GEN_ROWS) void yuv_general_kernel(const S* __restrict__ src, int n, int h, int w, int sub_x, int sub_y,
                                                                           int parity, long sstride, uint8_t* __restrict__ dst, long pitch,
                                                                           long dstride, YuvParams p, typename OUT::Args oa) {
    const OUT out = OUT::begin(oa, (int)(threadIdx.y * GEN_LANES + threadIdx.x), GEN_LANES * GEN_ROWS);      // (before any lane leaves)
    const int x = 4 * (int)(blockIdx.x * GEN_LANES + threadIdx.x);
    if (x >= w) return;
    const int npx = min(4, w - x);
    const long plane = (long)h * w, cw = (w + sub_x) >> sub_x, ch = ((h - 1 + parity) >> sub_y) + 1;
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        const S* s = src + (long)f * sstride;
        uint8_t* d = dst + (long)f * dstride;
        for (int r = blockIdx.y * GEN_ROWS + threadIdx.y; r < h; r += gridDim.y * GEN_ROWS) {
            const S* yp = s + (long)r * w + x;
            int c[4] = {0, 0, 0, 0};
            if (npx == 4 && (reinterpret_cast<uintptr_t>(yp) & (4 * sizeof(S) - 1)) == 0) {
                if (sizeof(S) == 1) {
                    const unsigned yw = *reinterpret_cast<const unsigned*>(yp);
#pragma unroll
                    for (int k = 0; k < 4; ++k) c[k] = luma_term(sample_of((yw >> (8 * k)) & 255u, p), p);
                } else {
                    const uint2 yw = *reinterpret_cast<const uint2*>(yp);
                    c[0] = luma_term(sample_of(yw.x & 0xffffu, p), p);
                    c[1] = luma_term(sample_of(yw.x >> 16, p), p);
                    c[2] = luma_term(sample_of(yw.y & 0xffffu, p), p);
                    c[3] = luma_term(sample_of(yw.y >> 16, p), p);
                }
            } else {
                for (int k = 0; k < npx; ++k) c[k] = luma_term(sample_of(yp[k], p), p);
            }
            ChromaTerms t[4];
            if (CHROMA == CHROMA_NONE) {
                t[0] = t[1] = t[2] = t[3] = chroma_terms(p.coff, p.coff, p, OUT::HALF);
            } else {
                const long cr = (r + parity) >> sub_y;
                const S* up = s + plane + cr * cw * (CHROMA == CHROMA_SEMI ? 2 : 1);
                const long vo = CHROMA == CHROMA_SEMI ? 1 : ch * cw;      // V behind U: the next sample, or the next plane
                const int cs = CHROMA == CHROMA_SEMI ? 2 : 1;
                const auto terms_of = [&](int k) {
                    const int cx = (min(x + k, w - 1) >> sub_x) * cs;      // (a pixel past the row's end takes the last sample: it is not stored)
                    return chroma_terms(sample_of(up[cx], p), sample_of(up[cx + vo], p), p, OUT::HALF);
                };
                t[0] = terms_of(0);
                t[2] = terms_of(2);
                if (sub_x) {
                    t[1] = t[0];
                    t[3] = t[2];
                } else {
                    t[1] = terms_of(1);
                    t[3] = terms_of(3);
                }
            }
            unsigned o[3];
            pack4(c, t, out, o[0], o[1], o[2]);
            uint8_t* op = d + (long)r * pitch + 3 * (long)x;
            if (npx == 4 && (reinterpret_cast<uintptr_t>(op) & 3) == 0) {
                unsigned* o4 = reinterpret_cast<unsigned*>(op);
                o4[0] = o[0];
                o4[1] = o[1];
                o4[2] = o[2];
            } else {
                for (int k = 0; k < 3 * npx; ++k) op[k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
            }
        }
    }
}

// ---- deinterlace (vse_yuv_deinterlace) ---------------------------------------------------------------------------------------------
constexpr int DEINT_STRIP = 8;        // rows a lane of the fast kernel walks down

// The planes of one packed picture.  off and row are in bytes for the fast kernel and in samples for the general one; first[p] is the
// fast kernel's work item at which plane p begins (items behind the last plane: the total).  Read with constant indices only, so the
// struct stays in scalar registers.
struct DeintPlanes {
    int count;
    int rows[3];
    long off[3], row[3];
    unsigned first[4];
};

// per sample of a dword: all ones where |c - p| > T
template <typename S>
__device__ __forceinline__ unsigned moved_word(unsigned c, unsigned p, int T) {
    constexpr int BITS = 8 * sizeof(S), PER = 4 / sizeof(S);
    constexpr unsigned ONES = (1u << BITS) - 1u;
    unsigned m = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int d = (int)((c >> (BITS * k)) & ONES) - (int)((p >> (BITS * k)) & ONES);
        m |= (d > T || -d > T) ? ONES << (BITS * k) : 0u;
    }
    return m;
}

// (a + b + 1) >> 1 of every sample of a dword
template <typename S>
__device__ __forceinline__ unsigned mean_word(unsigned a, unsigned b) {
    return (a | b) - (((a ^ b) >> 1) & (sizeof(S) == 1 ? 0x7f7f7f7fu : 0x7fff7fffu));
}

// Rows [y0, y1) of one 16-byte column of a plane of `rows` rows of rb bytes (s, q, d: the picture, its previous picture and the output,
// at the column's first byte; adaptive false: q is not read, every sample moved), by the rule: the walk of the fast kernel, shared with the field
// matcher's fallback (field_weave_fast_kernel).
template <typename S>
__device__ __forceinline__ void deint_strip16(const uint8_t* __restrict__ s, const uint8_t* __restrict__ q, uint8_t* __restrict__ d, long rb,
                                              int rows, int y0, int y1, int keep, int T, bool adaptive) {
    const auto load = [&](int y, uint4& c, uint4& m) {
        c = *reinterpret_cast<const uint4*>(s + (long)y * rb);
        if (adaptive) {
            const uint4 p = *reinterpret_cast<const uint4*>(q + (long)y * rb);
            m = make_uint4(moved_word<S>(c.x, p.x, T), moved_word<S>(c.y, p.y, T), moved_word<S>(c.z, p.z, T), moved_word<S>(c.w, p.w, T));
        } else {
            m = make_uint4(~0u, ~0u, ~0u, ~0u);
        }
    };
    uint4 ca, ma, cc, mc, cb, mb;                 // the row above, the row itself, the row below, each with its mask
    load(y0, cc, mc);
    ca = cc;
    ma = make_uint4(0u, 0u, 0u, 0u);
    if (y0 > 0) load(y0 - 1, ca, ma);
    for (int y = y0; y < y1; ++y) {
        cb = cc;
        mb = make_uint4(0u, 0u, 0u, 0u);
        const bool below = y + 1 < rows;
        if (below) load(y + 1, cb, mb);
        uint4 o = cc;
        if ((y & 1) != keep && rows > 1) {
            const uint4 a = y > 0 ? ca : cb, b = below ? cb : ca;
            const uint4 m = make_uint4(ma.x | mc.x | mb.x, ma.y | mc.y | mb.y, ma.z | mc.z | mb.z, ma.w | mc.w | mb.w);
            o.x = (mean_word<S>(a.x, b.x) & m.x) | (cc.x & ~m.x);
            o.y = (mean_word<S>(a.y, b.y) & m.y) | (cc.y & ~m.y);
            o.z = (mean_word<S>(a.z, b.z) & m.z) | (cc.z & ~m.z);
            o.w = (mean_word<S>(a.w, b.w) & m.w) | (cc.w & ~m.w);
        }
        *reinterpret_cast<uint4*>(d + (long)y * rb) = o;
        ca = cc;
        ma = mc;
        cc = cb;
        mc = mb;
    }
}

// Work item i of the planes `pl` -> its plane's rows and row bytes, its strip's rows [y0, y1) and the byte offset of its 16-byte column
// in the picture.  Item = (plane, strip of DEINT_STRIP rows, 16-byte column), columns fastest: consecutive lanes take consecutive columns,
// so a wave's loads and stores of a row are contiguous.
struct DeintItem {
    long base, rb;
    int rows, y0, y1;
};

__device__ __forceinline__ DeintItem deint_item(const DeintPlanes& pl, unsigned i) {
    const bool p1 = i >= pl.first[1], p2 = i >= pl.first[2];
    const unsigned j = i - (p2 ? pl.first[2] : p1 ? pl.first[1] : 0u);
    DeintItem it;
    it.rb = p2 ? pl.row[2] : p1 ? pl.row[1] : pl.row[0];
    it.rows = p2 ? pl.rows[2] : p1 ? pl.rows[1] : pl.rows[0];
    const unsigned cols = (unsigned)(it.rb >> 4), strip = j / cols, col = j - strip * cols;
    it.base = (p2 ? pl.off[2] : p1 ? pl.off[1] : pl.off[0]) + 16L * col;
    it.y0 = (int)strip * DEINT_STRIP;
    it.y1 = min(it.y0 + DEINT_STRIP, it.rows);
    return it;
}

// blockIdx.x strides the work items of a picture (deint_item), blockIdx.y the frames.  prev == nullptr: every sample moved.
template <typename S>
__global__ __launch_bounds__(FAST_THREADS) void deinterlace_fast_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ prev, int n,
                                                                        long sstride, long pstride, uint8_t* __restrict__ dst, long dstride,
                                                                        DeintPlanes pl, int keep, int T) {
    const bool adaptive = prev != nullptr;
    const unsigned items = pl.first[3];
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const uint8_t* s = src + (long)f * sstride;
        const uint8_t* q = adaptive ? prev + (long)f * pstride : nullptr;
        uint8_t* d = dst + (long)f * dstride;
        for (unsigned i = blockIdx.x * FAST_THREADS + threadIdx.x; i < items; i += gridDim.x * FAST_THREADS) {
            const DeintItem it = deint_item(pl, i);
            deint_strip16<S>(s + it.base, q + it.base, d + it.base, it.rb, it.rows, it.y0, it.y1, keep, T, adaptive);
        }
    }
}

// 4 samples at p, of which ns exist, as dwords (low sample first).  All four: the aligned dwords they lie in, shifted into place (a
// dword that holds one of the samples lies in the picture's buffer as far as the memory system cares, and the inputs are only read);
// fewer (the end of a row): sample by sample.
template <typename S>
struct Quad {
    unsigned v[sizeof(S) == 1 ? 1 : 2];
};

template <typename S>
__device__ __forceinline__ Quad<S> load_quad(const S* p, int ns) {
    constexpr int PER = 4 / sizeof(S), BITS = 8 * sizeof(S), DW = sizeof(S) == 1 ? 1 : 2;
    Quad<S> q;
    if (ns == 4) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        const unsigned m = (unsigned)(a & 3);
        const unsigned* w = reinterpret_cast<const unsigned*>(a - m);
        if (m == 0) {
#pragma unroll
            for (int k = 0; k < DW; ++k) q.v[k] = w[k];
        } else {
            unsigned d[DW + 1];
#pragma unroll
            for (int k = 0; k <= DW; ++k) d[k] = w[k];
#pragma unroll
            for (int k = 0; k < DW; ++k) q.v[k] = (unsigned)((((unsigned long long)d[k + 1] << 32) | d[k]) >> (8 * m));
        }
    } else {
#pragma unroll
        for (int k = 0; k < DW; ++k) q.v[k] = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < ns) q.v[k / PER] |= (unsigned)p[k] << (BITS * (k % PER));
    }
    return q;
}

// dword stores where p is 4-byte aligned and all four samples exist, sample by sample otherwise: no byte outside them is written
template <typename S>
__device__ __forceinline__ void store_quad(S* p, const Quad<S>& q, int ns) {
    constexpr int PER = 4 / sizeof(S), BITS = 8 * sizeof(S), DW = sizeof(S) == 1 ? 1 : 2;
    if (ns == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
#pragma unroll
        for (int k = 0; k < DW; ++k) reinterpret_cast<unsigned*>(p)[k] = q.v[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < ns) p[k] = (S)(q.v[k / PER] >> (BITS * (k % PER)));
    }
}

// deint_strip16 on quads: rows [y0, y1) of ns samples of a plane of `rows` rows of rl samples (s, q, d at the quad's first sample)
template <typename S>
__device__ __forceinline__ void deint_strip_quad(const S* __restrict__ s, const S* __restrict__ q, S* __restrict__ d, long rl, int rows, int ns,
                                                 int y0, int y1, int keep, int T, bool adaptive) {
    constexpr int DW = sizeof(S) == 1 ? 1 : 2;
    const auto load = [&](int y, Quad<S>& c, Quad<S>& m) {
        c = load_quad(s + (long)y * rl, ns);
        if (adaptive) {
            const Quad<S> pq = load_quad(q + (long)y * rl, ns);
#pragma unroll
            for (int k = 0; k < DW; ++k) m.v[k] = moved_word<S>(c.v[k], pq.v[k], T);
        } else {
#pragma unroll
            for (int k = 0; k < DW; ++k) m.v[k] = ~0u;
        }
    };
    Quad<S> ca, ma, cc, mc, cb, mb;           // the row above, the row itself, the row below, each with its mask
    load(y0, cc, mc);
    ca = cc;
#pragma unroll
    for (int k = 0; k < DW; ++k) ma.v[k] = 0u;
    if (y0 > 0) load(y0 - 1, ca, ma);
    for (int y = y0; y < y1; ++y) {
        cb = cc;
#pragma unroll
        for (int k = 0; k < DW; ++k) mb.v[k] = 0u;
        const bool below = y + 1 < rows;
        if (below) load(y + 1, cb, mb);
        Quad<S> o = cc;
        if ((y & 1) != keep && rows > 1) {
            const Quad<S> a = y > 0 ? ca : cb, b = below ? cb : ca;
#pragma unroll
            for (int k = 0; k < DW; ++k) {
                const unsigned m = ma.v[k] | mc.v[k] | mb.v[k];
                o.v[k] = (mean_word<S>(a.v[k], b.v[k]) & m) | (cc.v[k] & ~m);
            }
        }
        store_quad(d + (long)y * rl, o, ns);
        ca = cc;
        ma = mc;
        cc = cb;
        mc = mb;
    }
}

// The fast kernel's walk on quads: lane (threadIdx.x, threadIdx.y) = samples 4 xg .. 4 xg + 3 of a strip of DEINT_STRIP rows of each plane;
// blockIdx.y strides the strips, blockIdx.z the frames.  Strides, offsets and rows are counted in samples.
template <typename S>
__global__ __launch_bounds__(GEN_LANES * GEN_ROWS) void deinterlace_general_kernel(const S* __restrict__ src, const S* __restrict__ prev, int n,
                                                                                   long sstride, long pstride, S* __restrict__ dst, long dstride,
                                                                                   DeintPlanes pl, int keep, int T) {
    const long x = 4L * (blockIdx.x * GEN_LANES + threadIdx.x);
    const bool adaptive = prev != nullptr;
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            if (p >= pl.count || x >= pl.row[p]) continue;
            const long rl = pl.row[p];
            const int rows = pl.rows[p], ns = (int)min(4L, rl - x);
            const S* s = src + (long)f * sstride + pl.off[p] + x;
            const S* q = adaptive ? prev + (long)f * pstride + pl.off[p] + x : nullptr;
            S* d = dst + (long)f * dstride + pl.off[p] + x;
            for (int y0 = (blockIdx.y * GEN_ROWS + threadIdx.y) * DEINT_STRIP; y0 < rows; y0 += gridDim.y * GEN_ROWS * DEINT_STRIP)
                deint_strip_quad<S>(s, q, d, rl, rows, ns, y0, min(y0 + DEINT_STRIP, rows), keep, T, adaptive);
        }
    }
}

// ---- field matching (vse_yuv_field_match) ------------------------------------------------------------------------------------------
// The comb test of include/vse_hip.h on every sample of a dword: m the row in the middle, a and b the rows above and below -> how many
// samples stand out of both neighbours by more than T, the same way.
template <typename S>
__device__ __forceinline__ unsigned comb_word(unsigned m, unsigned a, unsigned b, int T) {
    constexpr int BITS = 8 * sizeof(S), PER = 4 / sizeof(S);
    constexpr unsigned ONES = (1u << BITS) - 1u;
    unsigned count = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int v = (int)((m >> (BITS * k)) & ONES);
        const int d1 = v - (int)((a >> (BITS * k)) & ONES), d2 = v - (int)((b >> (BITS * k)) & ONES);
        count += (min(d1, d2) > T || max(d1, d2) < -T) ? 1u : 0u;
    }
    return count;
}

template <typename S>
__device__ __forceinline__ unsigned comb16(const uint4& m, const uint4& a, const uint4& b, int T) {
    return comb_word<S>(m.x, a.x, b.x, T) + comb_word<S>(m.y, a.y, b.y, T) + comb_word<S>(m.z, a.z, b.z, T) + comb_word<S>(m.w, a.w, b.w, T);
}

// A wave's sums of the three counts -> one atomic per candidate into the frame's stats, from lane 0 (zeros add nothing and are skipped:
// the call has zeroed the stats).  `lane`: the thread's index in its wave.
__device__ __forceinline__ void add_counts(unsigned* stats, unsigned lane, unsigned c, unsigned p1, unsigned p2) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        c += __shfl_down(c, off, 64);
        p1 += __shfl_down(p1, off, 64);
        p2 += __shfl_down(p2, off, 64);
    }
    if (lane == 0) {
        if (c) atomicAdd(stats + 0, c);
        if (p1) atomicAdd(stats + 1, p1);
        if (p2) atomicAdd(stats + 2, p2);
    }
}

// The count over luma: item i of a frame = (strip of DEINT_STRIP rows, 16-byte column), columns fastest; a lane walks down its strip with
// rows y - 1, y, y + 1 of the picture and of the previous one in registers and makes three tests per row: the picture alone (c), the
// picture's row between the previous picture's (p1 on a row of parity keep, else p2), the previous picture's row between the picture's
// (p2 on a row of parity keep, else p1).  Rows 0 and rows - 1 have one neighbour and are not tested.  prev == nullptr: c alone.
template <typename S>
__global__ __launch_bounds__(FAST_THREADS) void field_count_fast_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ prev, int n,
                                                                        long sstride, long pstride, int rows, long rb, int keep, int T,
                                                                        unsigned* __restrict__ stats) {
    const bool pair = prev != nullptr;
    const unsigned cols = (unsigned)(rb >> 4), items = cols * (unsigned)((rows + DEINT_STRIP - 1) / DEINT_STRIP);
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const uint8_t* s = src + (long)f * sstride;
        const uint8_t* q = pair ? prev + (long)f * pstride : nullptr;
        unsigned nc = 0, n1 = 0, n2 = 0;
        for (unsigned i = blockIdx.x * FAST_THREADS + threadIdx.x; i < items; i += gridDim.x * FAST_THREADS) {
            const unsigned strip = i / cols, col = i - strip * cols;
            const int y0 = max((int)strip * DEINT_STRIP, 1), y1 = min((int)strip * DEINT_STRIP + DEINT_STRIP, rows - 1);
            if (y0 >= y1) continue;
            const long base = 16L * col;
            const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
            uint4 ca = *reinterpret_cast<const uint4*>(s + base + (long)(y0 - 1) * rb), cc = *reinterpret_cast<const uint4*>(s + base + (long)y0 * rb);
            uint4 pa = zero, pc = zero, cb, pb = zero;
            if (pair) {
                pa = *reinterpret_cast<const uint4*>(q + base + (long)(y0 - 1) * rb);
                pc = *reinterpret_cast<const uint4*>(q + base + (long)y0 * rb);
            }
            for (int y = y0; y < y1; ++y) {
                cb = *reinterpret_cast<const uint4*>(s + base + (long)(y + 1) * rb);
                nc += comb16<S>(cc, ca, cb, T);
                if (pair) {
                    pb = *reinterpret_cast<const uint4*>(q + base + (long)(y + 1) * rb);
                    const unsigned cur_mid = comb16<S>(cc, pa, pb, T), prev_mid = comb16<S>(pc, ca, cb, T);
                    const bool first = (y & 1) == keep;
                    n1 += first ? cur_mid : prev_mid;
                    n2 += first ? prev_mid : cur_mid;
                }
                ca = cc;
                cc = cb;
                pa = pc;
                pc = pb;
            }
        }
        add_counts(stats + 4L * f, threadIdx.x & 63u, nc, n1, n2);
    }
}

// The same count on quads (any width and byte alignment): lane (threadIdx.x, threadIdx.y) = 4 samples of strips of DEINT_STRIP rows;
// blockIdx.y strides the strips, blockIdx.z the frames; a block's row of 64 lanes is one wave.  Strides and rows are counted in samples.
// Samples behind the end of a row are zero in every row (load_quad) and never comb.
template <typename S>
__global__ __launch_bounds__(GEN_LANES * GEN_ROWS) void field_count_general_kernel(const S* __restrict__ src, const S* __restrict__ prev, int n,
                                                                                   long sstride, long pstride, int rows, long rl, int keep, int T,
                                                                                   unsigned* __restrict__ stats) {
    constexpr int DW = sizeof(S) == 1 ? 1 : 2;
    const long x = 4L * (blockIdx.x * GEN_LANES + threadIdx.x);
    const bool pair = prev != nullptr;
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        unsigned nc = 0, n1 = 0, n2 = 0;
        if (x < rl) {
            const int ns = (int)min(4L, rl - x);
            const S* s = src + (long)f * sstride + x;
            const S* q = pair ? prev + (long)f * pstride + x : nullptr;
            for (int t0 = (blockIdx.y * GEN_ROWS + threadIdx.y) * DEINT_STRIP; t0 < rows; t0 += gridDim.y * GEN_ROWS * DEINT_STRIP) {
                const int y0 = max(t0, 1), y1 = min(t0 + DEINT_STRIP, rows - 1);
                if (y0 >= y1) continue;
                Quad<S> ca = load_quad(s + (long)(y0 - 1) * rl, ns), cc = load_quad(s + (long)y0 * rl, ns), cb, pa = {}, pc = {}, pb = {};
                if (pair) {
                    pa = load_quad(q + (long)(y0 - 1) * rl, ns);
                    pc = load_quad(q + (long)y0 * rl, ns);
                }
                for (int y = y0; y < y1; ++y) {
                    cb = load_quad(s + (long)(y + 1) * rl, ns);
                    if (pair) pb = load_quad(q + (long)(y + 1) * rl, ns);
                    unsigned cur_mid = 0, prev_mid = 0;
#pragma unroll
                    for (int k = 0; k < DW; ++k) {
                        nc += comb_word<S>(cc.v[k], ca.v[k], cb.v[k], T);
                        if (pair) {
                            cur_mid += comb_word<S>(cc.v[k], pa.v[k], pb.v[k], T);
                            prev_mid += comb_word<S>(pc.v[k], ca.v[k], cb.v[k], T);
                        }
                    }
                    const bool first = (y & 1) == keep;
                    n1 += first ? cur_mid : prev_mid;
                    n2 += first ? prev_mid : cur_mid;
                    ca = cc;
                    cc = cb;
                    pa = pc;
                    pc = pb;
                }
            }
        }
        add_counts(stats + 4L * f, threadIdx.x, nc, n1, n2);
    }
}

// What the weave kernels need beside the pictures: the fallback's bound (limit_on: comb_limit >= 0; bound = comb_limit * w * (R - 2)),
// and whether this launch stores the choice (one of the launches of a call does: the one that holds the luma plane).
struct MatchRule {
    long bound;
    int limit_on, store;
};

// The choice of include/vse_hip.h from a frame's three counts (wave-uniform: every lane reads the same three words).
__device__ __forceinline__ int field_choice(const unsigned* stats, bool pair, const MatchRule& rule) {
    const unsigned c = stats[0], p1 = stats[1], p2 = stats[2];
    unsigned best = c;
    int choice = 0;
    if (pair && p1 < best) {
        best = p1;
        choice = 1;
    }
    if (pair && p2 < best) {
        best = p2;
        choice = 2;
    }
    return rule.limit_on && (long)best * 1000L > rule.bound ? 3 : choice;
}

// Whether row y of a plane comes from the picture (else from the previous one) under choice 0, 1 or 2
__device__ __forceinline__ bool row_from_picture(int choice, int y, int keep) { return choice == 0 || ((y & 1) == keep) == (choice == 1); }

// The weave of the planes `pl` (the ones whose base, row bytes and strides are 16-byte aligned; deint_item's work items): choice 0 to 2
// copies each row from the picture or the previous one, choice 3 is the deinterlacer's adaptive rule.
template <typename S>
__global__ __launch_bounds__(FAST_THREADS) void field_weave_fast_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ prev, int n,
                                                                        long sstride, long pstride, uint8_t* __restrict__ dst, long dstride,
                                                                        DeintPlanes pl, int keep, int T, unsigned* stats, MatchRule rule) {
    const bool pair = prev != nullptr;
    const unsigned items = pl.first[3];
    for (int f = blockIdx.y; f < n; f += gridDim.y) {
        const uint8_t* s = src + (long)f * sstride;
        const uint8_t* q = pair ? prev + (long)f * pstride : nullptr;
        uint8_t* d = dst + (long)f * dstride;
        const int choice = field_choice(stats + 4L * f, pair, rule);
        if (rule.store && blockIdx.x == 0 && threadIdx.x == 0) stats[4L * f + 3] = (unsigned)choice;
        for (unsigned i = blockIdx.x * FAST_THREADS + threadIdx.x; i < items; i += gridDim.x * FAST_THREADS) {
            const DeintItem it = deint_item(pl, i);
            if (choice == 3) {
                deint_strip16<S>(s + it.base, q + it.base, d + it.base, it.rb, it.rows, it.y0, it.y1, keep, T, pair);
            } else {
                for (int y = it.y0; y < it.y1; ++y) {
                    const uint8_t* from = row_from_picture(choice, y, keep) ? s : q;
                    *reinterpret_cast<uint4*>(d + it.base + (long)y * it.rb) = *reinterpret_cast<const uint4*>(from + it.base + (long)y * it.rb);
                }
            }
        }
    }
}

// The weave of the other planes, on quads: dword moves where a quad's four samples exist and lie 4-byte aligned, else sample by sample.
template <typename S>
__global__ __launch_bounds__(GEN_LANES * GEN_ROWS) void field_weave_general_kernel(const S* __restrict__ src, const S* __restrict__ prev, int n,
                                                                                   long sstride, long pstride, S* __restrict__ dst, long dstride,
                                                                                   DeintPlanes pl, int keep, int T, unsigned* stats, MatchRule rule) {
    const long x = 4L * (blockIdx.x * GEN_LANES + threadIdx.x);
    const bool pair = prev != nullptr;
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        const int choice = field_choice(stats + 4L * f, pair, rule);
        if (rule.store && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0) stats[4L * f + 3] = (unsigned)choice;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            if (p >= pl.count || x >= pl.row[p]) continue;
            const long rl = pl.row[p];
            const int rows = pl.rows[p], ns = (int)min(4L, rl - x);
            const S* s = src + (long)f * sstride + pl.off[p] + x;
            const S* q = pair ? prev + (long)f * pstride + pl.off[p] + x : nullptr;
            S* d = dst + (long)f * dstride + pl.off[p] + x;
            for (int y0 = (blockIdx.y * GEN_ROWS + threadIdx.y) * DEINT_STRIP; y0 < rows; y0 += gridDim.y * GEN_ROWS * DEINT_STRIP) {
                const int y1 = min(y0 + DEINT_STRIP, rows);
                if (choice == 3) {
                    deint_strip_quad<S>(s, q, d, rl, rows, ns, y0, y1, keep, T, pair);
                } else {
                    for (int y = y0; y < y1; ++y)
                        store_quad(d + (long)y * rl, load_quad((row_from_picture(choice, y, keep) ? s : q) + (long)y * rl, ns), ns);
                }
            }
        }
    }
}

// ---- horizontal resample (vse_yuv_resample) ---------------------------------------------------------------------------------------------
constexpr int RES_STRIP = 8;           // rows a lane walks down with its columns' table entries in registers
constexpr int RES_MAX_TAPS = 16;

// The planes of the packed input and output pictures, in samples.  pin / pout: stored and output columns per component (an interleaved UV
// row has 2 pin samples in and 2 pout out); left / coef: the plane's table on the device (coef rows of `taps` int16, read as dwords: taps
// is even).  Read with constant indices only, so the struct stays in scalar registers.
struct ResPlanes {
    int count;
    int rows[3], pin[3], pout[3], taps[3];
    long off_in[3], off_out[3];
    const int* left[3];
    const unsigned* coef[3];
};

// One plane for one lane.  The lane owns output samples [4 g, 4 g + 4) of every row: COLS = 4 columns of a planar row, or 2 columns (U V U V)
// of an interleaved one.  Their `left` and coefficients (two int16 per dword, TP dwords per column: TP is the instantiation's bound on tap
// pairs, so that the loops unroll without a test, every index is a constant, nothing goes to scratch and a row's loads are all in flight
// together; a pair at or past `taps` is zero, and zero times a sample that exists adds nothing) are loaded once and kept over all frames
// and strips of the lane.  A source sample is loaded by its clamped index, so every read lies inside its row whatever the table says; the sums are 24-bit multiplies (|coef| <= 2^15,
// sample < 2^16).  ALIGNED: every output quad exists whole and lies 4-sample aligned (the launcher has checked bases, row bytes and
// strides): one dword / two-dword store; otherwise store_quad decides per quad.
template <typename S, bool SEMI, bool ALIGNED, int TP>
__device__ __forceinline__ void resample_plane(const S* __restrict__ src, S* __restrict__ dst, int n, long sstride, long dstride, int rows, int pin,
                                               int pout, int taps, const int* __restrict__ left, const unsigned* __restrict__ coef, long g,
                                               int strip0, int strip_step, int f0, int f_step, int shift, int maxv) {
    constexpr int COLS = SEMI ? 2 : 4, COMPS = SEMI ? 2 : 1, PER = 4 / sizeof(S), BITS = 8 * sizeof(S);
    const long x0 = g * COLS;
    if (x0 >= pout) return;
    const int ncols = (int)min((long)COLS, pout - x0), ns = ncols * COMPS;
    int lf[COLS];
    unsigned cf[COLS][TP];
#pragma unroll
    for (int c = 0; c < COLS; ++c) {
        const long x = min(x0 + c, (long)pout - 1);           // (a column past the row's end repeats the last one: it is not stored)
        lf[c] = left[x];
#pragma unroll
        for (int j = 0; j < TP; ++j) cf[c][j] = 2 * j < taps ? coef[x * (taps >> 1) + j] : 0u;
    }
    const long rin = (long)pin * COMPS, rout = (long)pout * COMPS;
    const int top = (maxv << 14) | 0x3fff;
    for (int f = f0; f < n; f += f_step) {
        const S* s = src + (long)f * sstride;
        S* d = dst + (long)f * dstride + x0 * COMPS;
        for (int y0 = strip0; y0 < rows; y0 += strip_step) {
            const int y1 = min(y0 + RES_STRIP, rows);
#pragma unroll 1          // (one row's loads in flight per lane: unrolled rows cost registers, and with them the waves that hide the latency)
            for (int y = y0; y < y1; ++y) {
                const S* row = s + (long)y * rin;
                int acc[4] = {0, 0, 0, 0};
#pragma unroll
                for (int c = 0; c < COLS; ++c) {
                    // The clamped indices are made anew in every row (an add and a v_med3 per tap): hoisted out of the row loop they are
                    // 2 TP registers per column, which at 8 pairs spilled to scratch and at 2 already halved the waves per SIMD.
                    int l = lf[c];
                    asm volatile("" : "+v"(l));
#pragma unroll
                    for (int j = 0; j < TP; ++j) {
                        const int k0 = (int)(short)(cf[c][j] & 0xffffu), k1 = (int)cf[c][j] >> 16;
                        const int i0 = min(max(l + 2 * j, 0), pin - 1) * COMPS, i1 = min(max(l + 2 * j + 1, 0), pin - 1) * COMPS;
#pragma unroll
                        for (int e = 0; e < COMPS; ++e)
                            acc[c * COMPS + e] += __mul24(k0, (int)row[i0 + e] >> shift) + __mul24(k1, (int)row[i1 + e] >> shift);
                    }
                }
                Quad<S> q;
#pragma unroll
                for (int k = 0; k < (int)(sizeof(q.v) / sizeof(q.v[0])); ++k) q.v[k] = 0u;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned v = (unsigned)(min(max(acc[k] + 8192, 0), top) >> 14) << shift;          // (clamped before the shift, as clip8)
                    q.v[k / PER] |= v << (BITS * (k % PER));
                }
                S* o = d + (long)y * rout;
                if (ALIGNED) {
#pragma unroll
                    for (int k = 0; k < (int)(sizeof(q.v) / sizeof(q.v[0])); ++k) reinterpret_cast<unsigned*>(o)[k] = q.v[k];
                } else {
                    store_quad(o, q, ns);
                }
            }
        }
    }
}

// Lane (threadIdx.x, threadIdx.y) = output samples 4 g .. 4 g + 3 of strips of RES_STRIP rows of each plane; blockIdx.y strides the strips,
// blockIdx.z the frames.  Strides and offsets are counted in samples.  ALIGNED is the fast kernel, TP the bound on the tap pairs of
// both tables (see resample_plane).
template <typename S, bool SEMI, bool ALIGNED, int TP>
__global__ __launch_bounds__(GEN_LANES * GEN_ROWS) void resample_kernel(const S* __restrict__ src, int n, long sstride, S* __restrict__ dst,
                                                                        long dstride, ResPlanes pl, int shift, int maxv) {
    const long g = (long)blockIdx.x * GEN_LANES + threadIdx.x;
    const int strip0 = (int)(blockIdx.y * GEN_ROWS + threadIdx.y) * RES_STRIP, strip_step = (int)gridDim.y * GEN_ROWS * RES_STRIP;
    resample_plane<S, false, ALIGNED, TP>(src + pl.off_in[0], dst + pl.off_out[0], n, sstride, dstride, pl.rows[0], pl.pin[0], pl.pout[0], pl.taps[0],
                                      pl.left[0], pl.coef[0], g, strip0, strip_step, (int)blockIdx.z, (int)gridDim.z, shift, maxv);
#pragma unroll
    for (int p = 1; p < 3; ++p) {
        if (p >= pl.count) continue;
        resample_plane<S, SEMI, ALIGNED, TP>(src + pl.off_in[p], dst + pl.off_out[p], n, sstride, dstride, pl.rows[p], pl.pin[p], pl.pout[p],
                                         pl.taps[p], pl.left[p], pl.coef[p], g, strip0, strip_step, (int)blockIdx.z, (int)gridDim.z, shift, maxv);
    }
}

// ---- vertical scale (vse_yuv_vscale) ----------------------------------------------------------------------------------------------------
// The planes of the packed input and output bands, in samples.  rl: samples per row (an interleaved UV row has 2 cw); ph: the rows of the
// WHOLE input picture's plane, [b0, b1) the rows of it the input band holds, [o0, o1) the output rows to make, all in whole-picture rows
// of the plane; top / coef: the plane's table (coef rows of `taps` int16, read as dwords).  Read with constant indices only.
struct VsPlanes {
    int count;
    int rl[3], ph[3], b0[3], b1[3], o0[3], o1[3], taps[3];
    long off_in[3], off_out[3];
    const int* top[3];
    const unsigned* coef[3];
};

// One plane for one lane.  The lane owns samples [V g, V g + V) of every row: FAST, V is the 16 bytes of one load or store (the launcher
// has checked bases, row bytes and strides); otherwise 4 samples through load_quad / store_quad, which decide per quad.  A wave makes
// one output row at a time, rows row0, row0 + row_step, ... (strips of 2, 4 and 8 consecutive rows per wave measured up to 8, 40 and 92 %
// slower: EXPERIMENTS.md AG); the row is the same in all its lanes (row0 comes from readfirstlane), so top[r], the coefficient
// dwords and the clamped source rows are scalar; TP is the instantiation's bound on the tap pairs (a pair at or past `taps` is zero and
// reads a row that exists).  A source row is clamped to the picture and then to the band, so every load lies inside the input
// whatever the table says.
template <typename S, bool FAST, int TP>
__device__ __forceinline__ void vscale_plane(const S* __restrict__ src, S* __restrict__ dst, int n, long sstride, long dstride, int rl, int ph,
                                             int b0, int b1, int o0, int o1, int taps, const int* __restrict__ top,
                                             const unsigned* __restrict__ coef, long g, int row0, int row_step, int f0, int f_step, int shift,
                                             int maxv) {
    constexpr int V = FAST ? 16 / (int)sizeof(S) : 4, PER = 4 / (int)sizeof(S), BITS = 8 * (int)sizeof(S), DW = V / PER;
    constexpr unsigned ONES = (1u << BITS) - 1u;
    const long x0 = g * V;
    if (x0 >= rl) return;
    const int ns = (int)min((long)V, (long)rl - x0);
    const int rows = o1 - o0, hi = (maxv << 14) | 0x3fff;
    for (int f = f0; f < n; f += f_step) {
        const S* s = src + (long)f * sstride + x0;
        S* d = dst + (long)f * dstride + x0;
#pragma unroll 1
        for (int t = row0; t < rows; t += row_step) {
            const int r = o0 + t, tp = top[r];
            const unsigned* cr = coef + (long)r * (taps >> 1);
            int acc[V];
#pragma unroll
            for (int k = 0; k < V; ++k) acc[k] = 0;
#pragma unroll
            for (int j = 0; j < TP; ++j) {
                const unsigned c = 2 * j < taps ? cr[j] : 0u;
                const int kk[2] = {(int)(short)(c & 0xffffu), (int)c >> 16};
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const int i = min(max(min(max(tp + 2 * j + e, 0), ph - 1), b0), b1 - 1) - b0;
                    const S* p = s + (long)i * rl;
                    unsigned w[DW];
                    if constexpr (FAST) {
                        const uint4 v = *reinterpret_cast<const uint4*>(p);
                        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
                    } else {
                        const Quad<S> q = load_quad(p, ns);
#pragma unroll
                        for (int k = 0; k < DW; ++k) w[k] = q.v[k];
                    }
#pragma unroll
                    for (int k = 0; k < V; ++k) acc[k] += __mul24(kk[e], (int)((w[k / PER] >> (BITS * (k % PER))) & ONES) >> shift);
                }
            }
            unsigned o[DW];
#pragma unroll
            for (int k = 0; k < DW; ++k) o[k] = 0u;
#pragma unroll
            for (int k = 0; k < V; ++k)
                o[k / PER] |= ((unsigned)(min(max(acc[k] + 8192, 0), hi) >> 14) << shift) << (BITS * (k % PER));
            S* out = d + (long)t * rl;
            if constexpr (FAST) {
                *reinterpret_cast<uint4*>(out) = make_uint4(o[0], o[1], o[2], o[3]);
            } else {
                Quad<S> q;
#pragma unroll
                for (int k = 0; k < DW; ++k) q.v[k] = o[k];
                store_quad(out, q, ns);
            }
        }
    }
}

// Lane (threadIdx.x, threadIdx.y) = samples V g .. V g + V - 1 of output rows of each plane; a wave is one threadIdx.y (the block is
// GEN_LANES = 64 wide), blockIdx.y strides the rows, blockIdx.z the frames.  Strides and offsets are counted in samples.
template <typename S, bool FAST, int TP>
__global__ __launch_bounds__(GEN_LANES * GEN_ROWS) void vscale_kernel(const S* __restrict__ src, int n, long sstride, S* __restrict__ dst,
                                                                      long dstride, VsPlanes pl, int shift, int maxv) {
    const long g = (long)blockIdx.x * GEN_LANES + threadIdx.x;
    const int row0 = __builtin_amdgcn_readfirstlane((int)(blockIdx.y * GEN_ROWS + threadIdx.y)), row_step = (int)gridDim.y * GEN_ROWS;
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        if (p >= pl.count) continue;
        vscale_plane<S, FAST, TP>(src + pl.off_in[p], dst + pl.off_out[p], n, sstride, dstride, pl.rl[p], pl.ph[p], pl.b0[p], pl.b1[p], pl.o0[p],
                                  pl.o1[p], pl.taps[p], pl.top[p], pl.coef[p], g, row0, row_step, (int)blockIdx.z, (int)gridDim.z, shift, maxv);
    }
}

// ==== host: what the entry points below share ===============================================================================================
// ---- one copy of each argument check
int sample_bytes(int depth) { return depth > 8 ? 2 : 1; }
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool msb_ok(int msb, int ss) { return msb >= 0 && msb <= (ss == 2 ? 1 : 0); }
bool odd(const void* p, int64_t stride) { return (reinterpret_cast<uintptr_t>(p) & 1) || (stride & 1); }
bool holds(int64_t stride, size_t frame) { return stride >= (int64_t)frame; }
bool bgr_ok(int h, int w, int64_t pitch, int64_t bgr_frame_stride) {
    return pitch >= (int64_t)w * 3 && bgr_frame_stride >= (int64_t)(h - 1) * pitch + (int64_t)w * 3;
}
bool table_ok(const void* p, size_t bytes) { return bytes && p && aligned16(p); }
// the `bytes` at p (nullptr: nothing) do not meet [lo, hi)
bool apart(uintptr_t lo, uintptr_t hi, const void* p, uintptr_t bytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    return !p || hi <= a || a + bytes <= lo;
}

// what vse_yuv_deinterlace and vse_yuv_field_match both refuse: pictures, optional previous pictures and an output of the same packing
bool fields_call_ok(const vse_ctx* c, const void* d_yuv, const void* d_prev, const void* d_out, int n, size_t frame, int ss, int msb, int keep,
                    int thresh, int64_t yuv_frame_stride, int64_t prev_frame_stride, int64_t out_frame_stride) {
    return c && d_yuv && d_out && n >= 1 && frame && msb_ok(msb, ss) && keep >= 0 && keep <= 1 && thresh >= 0 && thresh <= 255 &&
           holds(yuv_frame_stride, frame) && holds(out_frame_stride, frame) && (!d_prev || holds(prev_frame_stride, frame)) && d_out != d_yuv &&
           d_out != d_prev &&
           !(ss == 2 && (odd(d_yuv, yuv_frame_stride) || odd(d_out, out_frame_stride) || (d_prev && odd(d_prev, prev_frame_stride))));
}

bool resample_table_ok(int columns, int taps) { return columns >= 1 && taps >= 2 && taps <= RES_MAX_TAPS && taps % 2 == 0; }

// what vse_yuv_resample and vse_yuv_vscale both refuse: pictures of frame_in bytes, an output of frame_out bytes, a luma table and, where
// the format has chroma, a chroma table (table_y, table_c: their bytes, 0 for a table that cannot be)
bool scaler_call_ok(const vse_ctx* c, const void* d_yuv, const void* d_out, int n, size_t frame_in, size_t frame_out, int ss, int msb,
                    const void* d_table_y, size_t table_y, const void* d_table_c, size_t table_c, bool has_chroma, int64_t yuv_frame_stride,
                    int64_t out_frame_stride) {
    if (!(c && d_yuv && d_out && n >= 1 && frame_in && frame_out && msb_ok(msb, ss) && table_ok(d_table_y, table_y) &&
          (!has_chroma || table_ok(d_table_c, table_c)) && holds(yuv_frame_stride, frame_in) && holds(out_frame_stride, frame_out) &&
          !(ss == 2 && (odd(d_yuv, yuv_frame_stride) || odd(d_out, out_frame_stride)))))
        return false;
    // the output lies apart from the input pictures (first byte of the first to last byte of the last) and from both tables
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(d_out), o1 = o0 + (uintptr_t)(n - 1) * (uintptr_t)out_frame_stride + frame_out;
    const auto clear = [&](const void* p, size_t bytes) { return !bytes || apart(o0, o1, p, bytes); };
    return clear(d_yuv, (size_t)(n - 1) * (size_t)yuv_frame_stride + frame_in) && clear(d_table_y, table_y) &&
           clear(has_chroma ? d_table_c : nullptr, table_c);
}

// ---- the refusal message: "<entry point>: bad arguments (n ..., " and what the caller adds, cut at `cap` bytes as one snprintf would
class Refusal {
    char text[1024];
    size_t cap, len;

  public:
    Refusal(size_t cap_, const char* who, int n) : cap(cap_), len(0) { add("%s: bad arguments (n %d, ", who, n); }
    __attribute__((format(printf, 2, 3))) Refusal& add(const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        const int more = vsnprintf(text + len, cap - len, fmt, ap);
        va_end(ap);
        len = std::min(len + (size_t)std::max(more, 0), cap - 1);
        return *this;
    }
    Refusal& picture(int h, int w) { return add("frame %d x %d of at most 2^31 - 1 pixels, ", h, w); }
    Refusal& format(int sub_x, int sub_y, int chroma, int depth, int msb) {
        return add("subsampling %d, %d of 0, 0 | 1, 0 | 1, 1, chroma %d of 0 (with subsampling 0, 0) | 1 | 2 (with subsampling 1, 1), depth %d of "
                   "8..16, msb %d of 0 | 1 (0 at depth 8), ", sub_x, sub_y, chroma, depth, msb);
    }
    // what vse_yuv_deinterlace's and vse_yuv_field_match's messages share
    Refusal& fields(int64_t yuv_frame_stride, int64_t prev_frame_stride, int64_t out_frame_stride, size_t frame, const void* d_yuv,
                    const void* d_prev, const void* d_out) {
        return add("frame strides %lld, %lld (previous pictures) and %lld (output) of at least %zu, bases %p, %p, %p and strides 2-byte aligned for "
                   "2-byte samples, the output none of the inputs", (long long)yuv_frame_stride, (long long)prev_frame_stride,
                   (long long)out_frame_stride, frame, d_yuv, d_prev, d_out);
    }
    // vse_yuv_resample's and vse_yuv_vscale's, to the end
    Refusal& scaler(int taps_y, int taps_c, const void* d_table_y, const void* d_table_c, int64_t yuv_frame_stride, size_t frame_in,
                    int64_t out_frame_stride, size_t frame_out, const void* d_yuv, const void* d_out) {
        return add("taps %d (luma) and %d (chroma) even and of 2..16, tables %p and %p 16-byte aligned (the chroma table only where the format has "
                   "chroma), frame strides %lld of at least %zu and %lld (output) of at least %zu, bases %p, %p and strides 2-byte aligned for "
                   "2-byte samples, the output apart from the pictures and the tables)", taps_y, taps_c, d_table_y, d_table_c,
                   (long long)yuv_frame_stride, frame_in, (long long)out_frame_stride, frame_out, d_yuv, d_out);
    }
    int send() {
        vse_set_error(text);
        return VSE_E_INVAL;
    }
};

// ---- the launches
// blocks of FAST_THREADS lanes that stride `items` work items per frame, blockIdx.y the frames
dim3 fast_grid(long items, int n) {
    return dim3((unsigned)std::min<long>((items + FAST_THREADS - 1) / FAST_THREADS, FAST_MAX_BLOCKS), (unsigned)std::min(n, 65535));
}

// blocks of GEN_LANES x GEN_ROWS lanes: one lane per group of a row, blockIdx.y strides the rows (or strips of rows), blockIdx.z the frames
dim3 general_grid(long groups, long rows, int n) {
    return dim3((unsigned)((groups + GEN_LANES - 1) / GEN_LANES), (unsigned)std::min<long>((rows + GEN_ROWS - 1) / GEN_ROWS, 65535),
                (unsigned)std::min(n, 65535));
}

int strips_of(int rows) { return (rows + DEINT_STRIP - 1) / DEINT_STRIP; }

// The pictures of a call as a kernel on samples S takes them: typed pointers, the frame strides in samples.
template <typename S>
struct Pictures {
    const S* src;
    const S* prev;
    S* dst;
    long sstride, pstride, dstride;
};

// f(Pictures<uint8_t>) or f(Pictures<uint16_t>) by the sample bytes ss; the strides come in bytes
template <class F>
void with_samples(int ss, const void* src, const void* prev, void* dst, int64_t sstride, int64_t pstride, int64_t dstride, F&& f) {
    if (ss == 1)
        f(Pictures<uint8_t>{reinterpret_cast<const uint8_t*>(src), reinterpret_cast<const uint8_t*>(prev), reinterpret_cast<uint8_t*>(dst), (long)sstride,
                            (long)pstride, (long)dstride});
    else
        f(Pictures<uint16_t>{reinterpret_cast<const uint16_t*>(src), reinterpret_cast<const uint16_t*>(prev), reinterpret_cast<uint16_t*>(dst),
                             (long)sstride / 2, (long)pstride / 2, (long)dstride / 2});
}

// the end of every entry point that launched: `failure` is its "<entry point>: launch failed"
int launched(const char* failure) {
    if (hipGetLastError() == hipSuccess) return VSE_OK;
    vse_set_error(failure);
    return VSE_E_HIP;
}

// ---- conversion (vse_yuv_to_bgr_format, vse_yuv_to_bgr_tonemap)
// {KY, BU, GU, GV, RV}_0 of [full_range][matrix]
constexpr int YUV_K0[2][3][5] = {{{1220542, 2116026, -409993, -852492, 1673527},
                                  {1220542, 2215014, -223607, -558796, 1879825},
                                  {1220542, 2245811, -196426, -682019, 1760217}},
                                 {{1 << 20, 1858077, -360853, -748826, 1470104},
                                  {1 << 20, 1945738, -196424, -490864, 1651297},
                                  {1 << 20, 1972791, -172546, -599107, 1546230}}};

int scaled_factor(int k0, int s) {
    const int m = ((k0 < 0 ? -k0 : k0) + ((1 << s) >> 1)) >> s;
    return k0 < 0 ? -m : m;
}

YuvParams yuv_params(int depth, int msb, int matrix, int full_range) {
    const int s = depth - 8;
    const int* k0 = YUV_K0[full_range][matrix];
    YuvParams p;
    p.shift = msb ? 16 - depth : 0;
    p.maxv = (1 << depth) - 1;
    p.yoff = full_range ? 0 : 16 << s;
    p.coff = 128 << s;
    p.ky = scaled_factor(k0[0], s);
    p.bu = scaled_factor(k0[1], s);
    p.gu = scaled_factor(k0[2], s);
    p.gv = scaled_factor(k0[3], s);
    p.rv = scaled_factor(k0[4], s);
    return p;
}

// Blocks of a tone-mapped launch: each stages the 16 128-byte table before its first pixel, so the grid is capped and blocks stride the
// work.  Measured on 64 x 1080p / 16 x 2160p P010 (us per frame, 16-byte kernel; general kernel): 512 4.5 / 17.7; 12.4 / 43.5, 1024 3.9 /
// 15.6; 8.6 / 29.5, 4096 3.4 / 14.1; 6.7 / 21.3, 8192 3.4 / 13.7; 5.6 / 20.8, 16384 3.4 / 13.7; 5.5 / 21.1: the copies cost less than idle
// CUs do, and past 8192 nothing is gained.
constexpr int TONE_MAX_BLOCKS = 8192;

// The launch of an accepted call.  PlainOut: one block per 256 work items, as ever.  ToneOut: at most about TONE_MAX_BLOCKS blocks in all,
// which stride the items, rows and frames.
template <class OUT>
void launch_format(const uint8_t* src, int n, int h, int w, int sub_x, int sub_y, int chroma, int ss, int row_parity, int64_t yuv_frame_stride,
                   uint8_t* dst, int64_t pitch, int64_t bgr_frame_stride, const YuvParams& p, const typename OUT::Args& oa, hipStream_t st) {
    constexpr bool tone = OUT::TONE;
    const bool fast = ss == 2 && sub_x == 1 && sub_y == 1 && chroma != CHROMA_NONE && w % 16 == 0 && h % 2 == 0 && row_parity == 0 &&
                      pitch % 16 == 0 && yuv_frame_stride % 16 == 0 && bgr_frame_stride % 16 == 0 && aligned16(src) && aligned16(dst);
    if (fast) {
        const long items = (long)(h / 2) * (w / 16);
        dim3 grid = fast_grid(items, n);
        if (tone) {
            const long gx = std::min<long>((items + FAST_THREADS - 1) / FAST_THREADS, TONE_MAX_BLOCKS);
            grid = dim3((unsigned)gx, (unsigned)std::min<long>(n, std::max<long>(TONE_MAX_BLOCKS / gx, 1)));
        }
        const auto kernel = chroma == CHROMA_PLANAR ? yuv420_wide_fast_kernel<CHROMA_PLANAR, OUT> : yuv420_wide_fast_kernel<CHROMA_SEMI, OUT>;
        hipLaunchKernelGGL(kernel, grid, dim3(FAST_THREADS), 0, st, src, n, h, w, (long)yuv_frame_stride, dst, (long)pitch, (long)bgr_frame_stride, p,
                           oa);
        return;
    }
    dim3 grid = general_grid(((long)w + 3) / 4, h, n);
    if (tone) {
        grid.y = std::min<long>(grid.y, std::max<long>(TONE_MAX_BLOCKS / grid.x, 1));
        grid.z = std::min<long>(grid.z, std::max<long>(TONE_MAX_BLOCKS / ((long)grid.x * grid.y), 1));
    }
    with_samples(ss, src, nullptr, nullptr, yuv_frame_stride, 0, 0, [&](auto pics) {
        using S = std::remove_cv_t<std::remove_pointer_t<decltype(pics.src)>>;
        const auto kernel = chroma == CHROMA_NONE ? yuv_general_kernel<S, CHROMA_NONE, OUT>
                          : chroma == CHROMA_PLANAR ? yuv_general_kernel<S, CHROMA_PLANAR, OUT> : yuv_general_kernel<S, CHROMA_SEMI, OUT>;
        hipLaunchKernelGGL(kernel, grid, dim3(GEN_LANES, GEN_ROWS), 0, st, pics.src, n, h, w, sub_x, sub_y, row_parity, pics.sstride, dst, (long)pitch,
                           (long)bgr_frame_stride, p, oa);
    });
}

// vse_yuv_to_bgr_format (OUT PlainOut; no table, no gamut) and vse_yuv_to_bgr_tonemap (OUT ToneOut): `who` and `cap` are the entry point's
// name and the bytes its message is cut at
template <class OUT>
int convert(const char* who, size_t cap, vse_ctx* c, const void* d_yuv, int n, int h, int w, int sub_x, int sub_y, int chroma, int depth, int msb,
            int matrix, int full_range, int row_parity, int64_t yuv_frame_stride, void* d_bgr, int64_t pitch, int64_t bgr_frame_stride,
            const void* d_table, const int32_t* gamut, void* stream) {
    const size_t frame = vse_yuv_frame_bytes(h, w, sub_x, sub_y, chroma, depth, row_parity);
    const int ss = sample_bytes(depth);
    bool ok = c && d_yuv && d_bgr && n >= 1 && frame && msb_ok(msb, ss) && matrix >= 0 && matrix <= 2 && full_range >= 0 && full_range <= 1 &&
              holds(yuv_frame_stride, frame) && bgr_ok(h, w, pitch, bgr_frame_stride) && !(ss == 2 && odd(d_yuv, yuv_frame_stride)) &&
              (!OUT::TONE || (table_ok(d_table, TONE_BYTES) && gamut));
    for (int r = 0; OUT::TONE && ok && r < 3; ++r) {
        long pos = 0, neg = 0;
        for (int k = 0; k < 3; ++k) (gamut[3 * r + k] > 0 ? pos : neg) += gamut[3 * r + k];
        ok = pos <= 32767 && neg >= -32768;
    }
    if (!ok) {
        Refusal r(cap, who, n);
        r.picture(h, w).format(sub_x, sub_y, chroma, depth, msb)
            .add("matrix %d of 0 | 1 | 2, full range %d of 0 | 1, row parity %d of 0..%d, packed frame stride %lld of at least %zu, pitch %lld, output "
                 "frame stride %lld, base %p and stride 2-byte aligned for 2-byte samples", matrix, full_range, row_parity, sub_y == 1 ? 1 : 0,
                 (long long)yuv_frame_stride, frame, (long long)pitch, (long long)bgr_frame_stride, d_yuv);
        int g[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int k = 0; gamut && k < 9; ++k) g[k] = gamut[k];
        if (OUT::TONE)
            r.add(", table %p 16-byte aligned, gamut %p [%d %d %d; %d %d %d; %d %d %d] with each row's positive entries summing to at most 32767 and "
                  "its negative ones to at least -32768", d_table, (const void*)gamut, g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8]);
        return r.add(")").send();
    }
    // what the 8-bit 4:2:0 kernels convert stays theirs
    if (!OUT::TONE && ss == 1 && sub_x == 1 && sub_y == 1 && chroma != CHROMA_NONE && !full_range && matrix <= BT709)
        return vse_yuv_to_bgr_matrix(c, d_yuv, n, h, w, chroma - 1, row_parity, yuv_frame_stride, d_bgr, pitch, bgr_frame_stride, matrix, stream);
    typename OUT::Args oa = {};
    if constexpr (OUT::TONE) {
        oa.table = reinterpret_cast<const uint4*>(d_table);
        for (int k = 0; k < 9; ++k) oa.m[k] = gamut[k];
    }
    launch_format<OUT>(reinterpret_cast<const uint8_t*>(d_yuv), n, h, w, sub_x, sub_y, chroma, ss, row_parity, yuv_frame_stride,
                       reinterpret_cast<uint8_t*>(d_bgr), pitch, bgr_frame_stride, yuv_params(depth, msb, matrix, full_range), oa,
                       reinterpret_cast<hipStream_t>(stream));
    return launched(OUT::TONE ? "vse_yuv_to_bgr_tonemap: launch failed" : "vse_yuv_to_bgr_format: launch failed");
}

// ---- deinterlace and field match: the kernels' planes from the picture's
// plane p of the picture joins pl, counted in samples (unit 1) or bytes (unit: the sample bytes)
void add_plane(DeintPlanes& pl, const YuvPlanes& pic, int p, int unit) {
    const int k = pl.count++;
    pl.rows[k] = pic.rows[p];
    pl.off[k] = pic.off[p] * unit;
    pl.row[k] = pic.row[p] * unit;
}

// the fast kernels' work items of planes counted in bytes: sets pl.first and returns the total
long deint_items(DeintPlanes& pl) {
    long items = 0;
    for (int p = 0; p < 3; ++p) {
        pl.first[p] = (unsigned)items;
        if (p < pl.count) items += (pl.row[p] / 16) * strips_of(pl.rows[p]);
    }
    pl.first[3] = (unsigned)items;
    return items;
}

// the general kernels' grid over planes counted in samples: the widest row and the tallest plane
dim3 deint_general_grid(const DeintPlanes& pl, int n) {
    long row = 0;
    int rows = 0;
    for (int p = 0; p < pl.count; ++p) {
        row = std::max(row, pl.row[p]);
        rows = std::max(rows, pl.rows[p]);
    }
    return general_grid((row + 3) / 4, strips_of(rows), n);
}

// ---- resample and vscale: the instantiation of an accepted call
// tap pairs 1, 2, 3, 4 (what bilinear, bicubic and Lanczos-3 need up to a reduction of 4 : 3) or 8
template <typename S, int TP>
auto resample_kernel_of(bool semi, bool fast) -> decltype(&resample_kernel<S, false, false, TP>) {
    return fast ? (semi ? resample_kernel<S, true, true, TP> : resample_kernel<S, false, true, TP>)
                : (semi ? resample_kernel<S, true, false, TP> : resample_kernel<S, false, false, TP>);
}

template <typename S>
void launch_resample(const Pictures<S>& pics, int n, const ResPlanes& pl, int shift, int maxv, bool semi, bool fast, int pairs, dim3 grid,
                     hipStream_t st) {
    const auto kernel = pairs <= 1 ? resample_kernel_of<S, 1>(semi, fast) : pairs == 2 ? resample_kernel_of<S, 2>(semi, fast)
                      : pairs == 3 ? resample_kernel_of<S, 3>(semi, fast) : pairs == 4 ? resample_kernel_of<S, 4>(semi, fast)
                      : resample_kernel_of<S, RES_MAX_TAPS / 2>(semi, fast);
    hipLaunchKernelGGL(kernel, grid, dim3(GEN_LANES, GEN_ROWS), 0, st, pics.src, n, pics.sstride, pics.dst, pics.dstride, pl, shift, maxv);
}

// tap pairs 1, 2, 3, 4, 6 (bilinear, bicubic and Lanczos-3 down to a reduction of 2 : 1) or 8
template <typename S>
void launch_vscale(const Pictures<S>& pics, int n, const VsPlanes& pl, int shift, int maxv, bool fast, int pairs, dim3 grid, hipStream_t st) {
#define VSE_VS(TP) (fast ? vscale_kernel<S, true, TP> : vscale_kernel<S, false, TP>)
    const auto kernel = pairs <= 1 ? VSE_VS(1) : pairs == 2 ? VSE_VS(2) : pairs == 3 ? VSE_VS(3) : pairs == 4 ? VSE_VS(4)
                      : pairs <= 6 ? VSE_VS(6) : VSE_VS(RES_MAX_TAPS / 2);
#undef VSE_VS
    hipLaunchKernelGGL(kernel, grid, dim3(GEN_LANES, GEN_ROWS), 0, st, pics.src, n, pics.sstride, pics.dst, pics.dstride, pl, shift, maxv);
}

// a plane's table on the device: `entries` int32 (left / top), then the coefficient rows as dwords
void set_table(const int*& first, const unsigned*& coef, const void* d_table, long entries) {
    const uint8_t* table = reinterpret_cast<const uint8_t*>(d_table);
    first = reinterpret_cast<const int*>(table);
    coef = reinterpret_cast<const unsigned*>(table + 4L * entries);
}

}  // namespace

extern "C" {

size_t vse_yuv420_frame_bytes(int h, int w, int row_parity) { return (size_t)yuv_planes(h, w, 1, 1, CHROMA_PLANAR, 8, row_parity).total; }

int vse_yuv_to_bgr_matrix(vse_ctx* c, const void* d_yuv, int n, int h, int w, int layout, int row_parity, int64_t yuv_frame_stride,
                          void* d_bgr, int64_t pitch, int64_t bgr_frame_stride, int matrix, void* stream) {
    const size_t frame = vse_yuv420_frame_bytes(h, w, row_parity);
    if (!c || !d_yuv || !d_bgr || n < 1 || !frame || (layout != YUV_I420 && layout != YUV_NV12) || (matrix != BT601 && matrix != BT709) ||
        !holds(yuv_frame_stride, frame) || !bgr_ok(h, w, pitch, bgr_frame_stride)) {
        return Refusal(360, "vse_yuv420_to_bgr", n).picture(h, w)
            .add("layout %d of 0 | 1, row parity %d of 0 | 1, packed frame stride %lld of at least %zu, pitch %lld, output frame stride %lld, matrix %d "
                 "of 0 | 1)", layout, row_parity, (long long)yuv_frame_stride, frame, (long long)pitch, (long long)bgr_frame_stride, matrix).send();
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint8_t* src = reinterpret_cast<const uint8_t*>(d_yuv);
    uint8_t* dst = reinterpret_cast<uint8_t*>(d_bgr);
    const bool fast = w % 16 == 0 && h % 2 == 0 && row_parity == 0 && pitch % 16 == 0 && yuv_frame_stride % 16 == 0 &&
                      bgr_frame_stride % 16 == 0 && aligned16(src) && aligned16(dst);
    const int which = 2 * matrix + layout;
    if (fast) {
        const auto kernel = which == 0 ? yuv420_fast_kernel<YUV_I420, BT601> : which == 1 ? yuv420_fast_kernel<YUV_NV12, BT601>
                          : which == 2 ? yuv420_fast_kernel<YUV_I420, BT709> : yuv420_fast_kernel<YUV_NV12, BT709>;
        hipLaunchKernelGGL(kernel, fast_grid((long)(h / 2) * (w / 16), n), dim3(FAST_THREADS), 0, st, src, n, h, w, (long)yuv_frame_stride, dst,
                           (long)pitch, (long)bgr_frame_stride);
    } else {
        const auto kernel = which == 0 ? yuv420_general_kernel<YUV_I420, BT601> : which == 1 ? yuv420_general_kernel<YUV_NV12, BT601>
                          : which == 2 ? yuv420_general_kernel<YUV_I420, BT709> : yuv420_general_kernel<YUV_NV12, BT709>;
        hipLaunchKernelGGL(kernel, general_grid(((long)w + 3) / 4, h, n), dim3(GEN_LANES, GEN_ROWS), 0, st, src, n, h, w, row_parity,
                           (long)yuv_frame_stride, dst, (long)pitch, (long)bgr_frame_stride);
    }
    return launched("vse_yuv420_to_bgr: launch failed");
}

int vse_yuv420_to_bgr(vse_ctx* c, const void* d_yuv, int n, int h, int w, int layout, int row_parity, int64_t yuv_frame_stride,
                      void* d_bgr, int64_t pitch, int64_t bgr_frame_stride, void* stream) {
    return vse_yuv_to_bgr_matrix(c, d_yuv, n, h, w, layout, row_parity, yuv_frame_stride, d_bgr, pitch, bgr_frame_stride, BT601, stream);
}

size_t vse_yuv_frame_bytes(int h, int w, int sub_x, int sub_y, int chroma, int depth, int row_parity) {
    return (size_t)yuv_planes(h, w, sub_x, sub_y, chroma, depth, row_parity).total * sample_bytes(depth);
}

int vse_yuv_to_bgr_format(vse_ctx* c, const void* d_yuv, int n, int h, int w, int sub_x, int sub_y, int chroma, int depth, int msb, int matrix,
                          int full_range, int row_parity, int64_t yuv_frame_stride, void* d_bgr, int64_t pitch, int64_t bgr_frame_stride,
                          void* stream) {
    return convert<PlainOut>("vse_yuv_to_bgr_format", 560, c, d_yuv, n, h, w, sub_x, sub_y, chroma, depth, msb, matrix, full_range, row_parity,
                             yuv_frame_stride, d_bgr, pitch, bgr_frame_stride, nullptr, nullptr, stream);
}

size_t vse_yuv_tonemap_table_bytes(void) { return TONE_BYTES; }

int vse_yuv_to_bgr_tonemap(vse_ctx* c, const void* d_yuv, int n, int h, int w, int sub_x, int sub_y, int chroma, int depth, int msb, int matrix,
                           int full_range, int row_parity, int64_t yuv_frame_stride, void* d_bgr, int64_t pitch, int64_t bgr_frame_stride,
                           const void* d_table, const int32_t* gamut, void* stream) {
    return convert<ToneOut>("vse_yuv_to_bgr_tonemap", 1024, c, d_yuv, n, h, w, sub_x, sub_y, chroma, depth, msb, matrix, full_range, row_parity,
                            yuv_frame_stride, d_bgr, pitch, bgr_frame_stride, d_table, gamut, stream);
}

int vse_yuv_deinterlace(vse_ctx* c, const void* d_yuv, const void* d_prev, int n, int h, int w, int sub_x, int sub_y, int chroma, int depth,
                        int msb, int keep, int mode, int thresh, int64_t yuv_frame_stride, int64_t prev_frame_stride, void* d_out,
                        int64_t out_frame_stride, void* stream) {
    const YuvPlanes pic = yuv_planes(h, w, sub_x, sub_y, chroma, depth, 0);
    const int ss = sample_bytes(depth);
    const size_t frame = (size_t)pic.total * ss;
    if (!fields_call_ok(c, d_yuv, d_prev, d_out, n, frame, ss, msb, keep, thresh, yuv_frame_stride, prev_frame_stride, out_frame_stride) || mode < 0 ||
        mode > 1) {
        return Refusal(560, "vse_yuv_deinterlace", n).picture(h, w).format(sub_x, sub_y, chroma, depth, msb)
            .add("keep %d of 0 | 1, mode %d of 0 | 1, thresh %d of 0..255, ", keep, mode, thresh)
            .fields(yuv_frame_stride, prev_frame_stride, out_frame_stride, frame, d_yuv, d_prev, d_out).add(")").send();
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const void* prev = mode == 0 ? d_prev : nullptr;       // interpolate: no picture is compared
    bool fast = aligned16(d_yuv) && aligned16(d_out) && yuv_frame_stride % 16 == 0 && out_frame_stride % 16 == 0 &&
                (!prev || (aligned16(prev) && prev_frame_stride % 16 == 0));
    for (int p = 0; p < pic.count; ++p) fast = fast && (pic.row[p] * ss) % 16 == 0;          // then every plane's offset is a multiple of 16 too
    const int T = thresh << (depth - 8 + (msb ? 16 - depth : 0));
    DeintPlanes pl = {};
    for (int p = 0; p < pic.count; ++p) add_plane(pl, pic, p, fast ? ss : 1);
    if (fast) {
        const dim3 grid = fast_grid(deint_items(pl), n);
        const auto kernel = ss == 1 ? deinterlace_fast_kernel<uint8_t> : deinterlace_fast_kernel<uint16_t>;
        hipLaunchKernelGGL(kernel, grid, dim3(FAST_THREADS), 0, st, reinterpret_cast<const uint8_t*>(d_yuv), reinterpret_cast<const uint8_t*>(prev), n,
                           (long)yuv_frame_stride, (long)prev_frame_stride, reinterpret_cast<uint8_t*>(d_out), (long)out_frame_stride, pl, keep, T);
    } else {
        with_samples(ss, d_yuv, prev, d_out, yuv_frame_stride, prev_frame_stride, out_frame_stride, [&](auto pics) {
            using S = std::remove_pointer_t<decltype(pics.dst)>;
            hipLaunchKernelGGL(deinterlace_general_kernel<S>, deint_general_grid(pl, n), dim3(GEN_LANES, GEN_ROWS), 0, st, pics.src, pics.prev, n,
                               pics.sstride, pics.pstride, pics.dst, pics.dstride, pl, keep, T);
        });
    }
    return launched("vse_yuv_deinterlace: launch failed");
}

int vse_yuv_field_match(vse_ctx* c, const void* d_yuv, const void* d_prev, int n, int h, int w, int sub_x, int sub_y, int chroma, int depth,
                        int msb, int keep, int comb_thresh, int comb_limit, int thresh, int64_t yuv_frame_stride, int64_t prev_frame_stride,
                        void* d_out, int64_t out_frame_stride, void* d_stats, void* stream) {
    const YuvPlanes pic = yuv_planes(h, w, sub_x, sub_y, chroma, depth, 0);
    const int ss = sample_bytes(depth);
    const size_t frame = (size_t)pic.total * ss;
    bool ok = fields_call_ok(c, d_yuv, d_prev, d_out, n, frame, ss, msb, keep, thresh, yuv_frame_stride, prev_frame_stride, out_frame_stride) &&
              d_stats && comb_thresh >= 0 && comb_thresh <= 255 && comb_limit <= 1000 && (reinterpret_cast<uintptr_t>(d_stats) & 3) == 0;
    if (ok) {
        // the stats lie apart from every picture: from the first byte of a run's first picture to the last byte of its last one
        const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_stats), s1 = s0 + 16 * (uintptr_t)n;
        const auto run = [&](int64_t stride) { return (uintptr_t)(n - 1) * (uintptr_t)stride + frame; };
        ok = apart(s0, s1, d_yuv, run(yuv_frame_stride)) && apart(s0, s1, d_prev, run(prev_frame_stride)) &&
             apart(s0, s1, d_out, run(out_frame_stride));
    }
    if (!ok) {
        return Refusal(720, "vse_yuv_field_match", n).picture(h, w).format(sub_x, sub_y, chroma, depth, msb)
            .add("keep %d of 0 | 1, comb_thresh %d of 0..255, comb_limit %d of at most 1000, thresh %d of 0..255, ", keep, comb_thresh, comb_limit, thresh)
            .fields(yuv_frame_stride, prev_frame_stride, out_frame_stride, frame, d_yuv, d_prev, d_out)
            .add(", stats %p 4-byte aligned and apart from the pictures)", d_stats).send();
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint8_t* src = reinterpret_cast<const uint8_t*>(d_yuv);
    const uint8_t* prev = reinterpret_cast<const uint8_t*>(d_prev);
    uint8_t* dst = reinterpret_cast<uint8_t*>(d_out);
    unsigned* stats = reinterpret_cast<unsigned*>(d_stats);
    const int up = depth - 8 + (msb ? 16 - depth : 0);
    const int comb_t = comb_thresh << up, T = thresh << up;
    if (hipMemsetAsync(d_stats, 0, 16 * (size_t)n, st) != hipSuccess) {
        vse_set_error("vse_yuv_field_match: clearing the stats failed");
        return VSE_E_HIP;
    }
    // ---- the count, over luma: 16-byte columns where the inputs allow them
    const bool in16 = aligned16(src) && yuv_frame_stride % 16 == 0 && (!prev || (aligned16(prev) && prev_frame_stride % 16 == 0));
    if (h >= 3) {
        if (in16 && ((long)w * ss) % 16 == 0) {
            const auto kernel = ss == 1 ? field_count_fast_kernel<uint8_t> : field_count_fast_kernel<uint16_t>;
            hipLaunchKernelGGL(kernel, fast_grid(((long)w * ss / 16) * strips_of(h), n), dim3(FAST_THREADS), 0, st, src, prev, n,
                               (long)yuv_frame_stride, (long)prev_frame_stride, h, (long)w * ss, keep, comb_t, stats);
        } else {
            with_samples(ss, d_yuv, d_prev, nullptr, yuv_frame_stride, prev_frame_stride, 0, [&](auto pics) {
                using S = std::remove_pointer_t<decltype(pics.dst)>;
                hipLaunchKernelGGL(field_count_general_kernel<S>, general_grid(((long)w + 3) / 4, strips_of(h), n), dim3(GEN_LANES, GEN_ROWS), 0, st,
                                   pics.src, pics.prev, n, pics.sstride, pics.pstride, h, (long)w, keep, comb_t, stats);
            });
        }
    }
    // ---- the weave: every plane on its own takes 16-byte moves where its base and row bytes allow them, quads otherwise
    const bool all16 = in16 && aligned16(dst) && out_frame_stride % 16 == 0;
    DeintPlanes fast = {}, gen = {};
    MatchRule fast_rule = {(long)comb_limit * w * ((long)h - 2), comb_limit >= 0 ? 1 : 0, 0}, gen_rule = fast_rule;
    for (int p = 0; p < pic.count; ++p) {
        const bool p16 = all16 && (pic.off[p] * ss) % 16 == 0 && (pic.row[p] * ss) % 16 == 0;
        add_plane(p16 ? fast : gen, pic, p, p16 ? ss : 1);
        if (p == 0) (p16 ? fast_rule : gen_rule).store = 1;
    }
    if (fast.count) {
        const dim3 grid = fast_grid(deint_items(fast), n);
        const auto kernel = ss == 1 ? field_weave_fast_kernel<uint8_t> : field_weave_fast_kernel<uint16_t>;
        hipLaunchKernelGGL(kernel, grid, dim3(FAST_THREADS), 0, st, src, prev, n, (long)yuv_frame_stride, (long)prev_frame_stride, dst,
                           (long)out_frame_stride, fast, keep, T, stats, fast_rule);
    }
    if (gen.count) {
        with_samples(ss, d_yuv, d_prev, d_out, yuv_frame_stride, prev_frame_stride, out_frame_stride, [&](auto pics) {
            using S = std::remove_pointer_t<decltype(pics.dst)>;
            hipLaunchKernelGGL(field_weave_general_kernel<S>, deint_general_grid(gen, n), dim3(GEN_LANES, GEN_ROWS), 0, st, pics.src, pics.prev, n,
                               pics.sstride, pics.pstride, pics.dst, pics.dstride, gen, keep, T, stats, gen_rule);
        });
    }
    return launched("vse_yuv_field_match: launch failed");
}

size_t vse_yuv_resample_table_bytes(int columns, int taps) {
    return resample_table_ok(columns, taps) ? (size_t)columns * (4 + 2 * (size_t)taps) : 0;
}

int vse_yuv_resample(vse_ctx* c, const void* d_yuv, int n, int h, int w_in, int w_out, int sub_x, int sub_y, int chroma, int depth, int msb,
                     int row_parity, const void* d_table_y, int taps_y, const void* d_table_c, int taps_c, int64_t yuv_frame_stride, void* d_out,
                     int64_t out_frame_stride, void* stream) {
    const YuvPlanes in = yuv_planes(h, w_in, sub_x, sub_y, chroma, depth, row_parity), out = yuv_planes(h, w_out, sub_x, sub_y, chroma, depth, row_parity);
    const int ss = sample_bytes(depth), comps = chroma == CHROMA_SEMI ? 2 : 1;
    const size_t frame_in = (size_t)in.total * ss, frame_out = (size_t)out.total * ss;
    const bool has_chroma = in.count > 1;
    const size_t table_y = frame_out ? vse_yuv_resample_table_bytes(w_out, taps_y) : 0;
    const size_t table_c = has_chroma && frame_out ? vse_yuv_resample_table_bytes((int)(out.row[1] / comps), taps_c) : 0;
    if (!scaler_call_ok(c, d_yuv, d_out, n, frame_in, frame_out, ss, msb, d_table_y, table_y, d_table_c, table_c, has_chroma, yuv_frame_stride,
                        out_frame_stride)) {
        return Refusal(900, "vse_yuv_resample", n).add("frame %d x %d -> %d columns, each of at most 2^31 - 1 pixels, ", h, w_in, w_out)
            .format(sub_x, sub_y, chroma, depth, msb).add("row parity %d of 0..%d, ", row_parity, sub_y == 1 ? 1 : 0)
            .scaler(taps_y, taps_c, d_table_y, d_table_c, yuv_frame_stride, frame_in, out_frame_stride, frame_out, d_yuv, d_out).send();
    }
    ResPlanes pl = {};
    pl.count = in.count;
    // the fast kernel: every output quad whole and on a 4-sample boundary
    bool fast = aligned16(d_yuv) && aligned16(d_out) && yuv_frame_stride % 16 == 0 && out_frame_stride % 16 == 0;
    for (int p = 0; p < pl.count; ++p) {
        const int cs = p ? comps : 1;
        pl.rows[p] = in.rows[p];
        pl.pin[p] = (int)(in.row[p] / cs);
        pl.pout[p] = (int)(out.row[p] / cs);
        pl.taps[p] = p ? taps_c : taps_y;
        pl.off_in[p] = in.off[p];
        pl.off_out[p] = out.off[p];
        set_table(pl.left[p], pl.coef[p], p ? d_table_c : d_table_y, pl.pout[p]);
        fast = fast && (in.row[p] * ss) % 16 == 0 && (out.row[p] * ss) % 16 == 0 && (in.off[p] * ss) % 16 == 0 && (out.off[p] * ss) % 16 == 0;
    }
    // (no chroma row has more quads than the luma row: 2 cw_out <= w_out + 1)
    const dim3 grid = general_grid(((long)w_out + 3) / 4, (h + RES_STRIP - 1) / RES_STRIP, n);
    const int shift = msb ? 16 - depth : 0, maxv = (1 << depth) - 1;
    const int pairs = std::max(taps_y, has_chroma ? taps_c : 0) / 2;
    with_samples(ss, d_yuv, nullptr, d_out, yuv_frame_stride, 0, out_frame_stride, [&](auto pics) {
        launch_resample(pics, n, pl, shift, maxv, chroma == CHROMA_SEMI, fast, pairs, grid, reinterpret_cast<hipStream_t>(stream));
    });
    return launched("vse_yuv_resample: launch failed");
}

int vse_yuv_vscale(vse_ctx* c, const void* d_yuv, int n, int w, int h_in, int h_out, int s0, int s1, int y0, int y1, int sub_x, int sub_y,
                   int chroma, int depth, int msb, const void* d_table_y, int taps_y, const void* d_table_c, int taps_c, int64_t yuv_frame_stride,
                   void* d_out, int64_t out_frame_stride, void* stream) {
    // the whole pictures bound the products of rows and columns; the bands are parts of them, pictures of their own by their first row's parity
    const YuvPlanes whole_in = yuv_planes(h_in, w, sub_x, sub_y, chroma, depth, 0), whole_out = yuv_planes(h_out, w, sub_x, sub_y, chroma, depth, 0);
    const bool bands = whole_in.count && whole_out.count && s0 >= 0 && s0 < s1 && s1 <= h_in && y0 >= 0 && y0 < y1 && y1 <= h_out;
    const YuvPlanes in = bands ? yuv_planes(s1 - s0, w, sub_x, sub_y, chroma, depth, s0 & sub_y) : YuvPlanes{};
    const YuvPlanes out = bands ? yuv_planes(y1 - y0, w, sub_x, sub_y, chroma, depth, y0 & sub_y) : YuvPlanes{};
    const int ss = sample_bytes(depth);
    const size_t frame_in = (size_t)in.total * ss, frame_out = (size_t)out.total * ss;
    const bool has_chroma = in.count > 1;
    const size_t table_y = frame_out ? vse_yuv_resample_table_bytes(h_out, taps_y) : 0;
    const size_t table_c = has_chroma && frame_out ? vse_yuv_resample_table_bytes(whole_out.rows[1], taps_c) : 0;
    if (!scaler_call_ok(c, d_yuv, d_out, n, frame_in, frame_out, ss, msb, d_table_y, table_y, d_table_c, table_c, has_chroma, yuv_frame_stride,
                        out_frame_stride)) {
        return Refusal(1000, "vse_yuv_vscale", n)
            .add("frames of %d columns and %d -> %d rows, each of at most 2^31 - 1 pixels, stored rows %d:%d and output rows %d:%d inside them and "
                 "not empty, ", w, h_in, h_out, s0, s1, y0, y1)
            .format(sub_x, sub_y, chroma, depth, msb)
            .scaler(taps_y, taps_c, d_table_y, d_table_c, yuv_frame_stride, frame_in, out_frame_stride, frame_out, d_yuv, d_out).send();
    }
    VsPlanes pl = {};
    pl.count = in.count;
    // the fast kernel: every plane's rows of both bands start on a 16-byte boundary and are whole 16-byte runs
    bool fast = aligned16(d_yuv) && aligned16(d_out) && yuv_frame_stride % 16 == 0 && out_frame_stride % 16 == 0;
    long widest = 0;
    for (int p = 0; p < pl.count; ++p) {
        const int sy = p ? sub_y : 0;
        pl.rl[p] = (int)in.row[p];
        pl.ph[p] = whole_in.rows[p];
        pl.b0[p] = s0 >> sy;
        pl.b1[p] = pl.b0[p] + in.rows[p];
        pl.o0[p] = y0 >> sy;
        pl.o1[p] = pl.o0[p] + out.rows[p];
        pl.taps[p] = p ? taps_c : taps_y;
        pl.off_in[p] = in.off[p];
        pl.off_out[p] = out.off[p];
        set_table(pl.top[p], pl.coef[p], p ? d_table_c : d_table_y, whole_out.rows[p]);
        fast = fast && (in.row[p] * ss) % 16 == 0 && (in.off[p] * ss) % 16 == 0 && (out.off[p] * ss) % 16 == 0;
        widest = std::max(widest, in.row[p]);
    }
    const long per = fast ? 16 / ss : 4;
    const dim3 grid = general_grid((widest + per - 1) / per, y1 - y0, n);          // (no chroma plane has more output rows than luma)
    const int shift = msb ? 16 - depth : 0, maxv = (1 << depth) - 1;
    const int pairs = std::max(taps_y, has_chroma ? taps_c : 0) / 2;
    with_samples(ss, d_yuv, nullptr, d_out, yuv_frame_stride, 0, out_frame_stride, [&](auto pics) {
        launch_vscale(pics, n, pl, shift, maxv, fast, pairs, grid, reinterpret_cast<hipStream_t>(stream));
    });
    return launched("vse_yuv_vscale: launch failed");
}

}  // extern "C"
