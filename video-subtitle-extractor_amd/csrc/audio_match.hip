// Audio template search for timeline sync (vse_audio_match, include/vse_hip.h): the normalised squared difference of a
// uint8 pattern p[0..m) against every offset k of a uint8 window w[0..n+m-1), and its first minimum.  The integers are the
// specification (tests/audio_match_ref.py restates them in numpy, bit for bit):
//   X_k = sum p[i] w[k+i],  S_k = sum w[k+i]^2,  P = sum p[i]^2                          (exact, int64)
//   num = (double) max(S_k - 2 X_k + P, 0),  den = sqrt((double) S_k) * sqrt((double) P)
//   v_k = (float)(num / den) if num < den else 1.0f;   result = (first argmin k, v_k)
//
// Launch 1 (audio_match_main) has two kinds of blocks:
//  * MFMA blocks: a tile of AM_TK offsets x one chunk of the K range.  The cross term runs on v_mfma_i32_16x16x64_i8 with the
//    bytes biased to s = x - 128 (x ^ 0x80 read as int8):  C[a][r] = sum_c A[a][c] B[c][r] with A[a][c] = s_p[c - a] (a banded
//    Toeplitz of the pattern, zero outside [0, m)) and B[c][r] = s_w[b + 16 r + c], so C[a][r] = sum_i s_p[i] s_w[b + 16 r + a + i]
//    is the biased cross term of offset b + 16 r + a.  c runs over [0, m + 15).  A and B take their K index from the same lane /
//    byte position, so the hardware's K order within an instruction does not matter.  A chunk holds at most 65536 K values, so
//    its int32 sums stay below 2^30; each chunk writes its own int32 partials, which the finalize adds as int64.
//  * segment blocks: sum x and sum x^2 of AM_SEG consecutive bytes of the pattern or the window (int64 out).
//  Block 0 also sets every query's result key to the largest value.
// Launch 2 (audio_match_finalize): a block owns AM_SEG offsets.  It gets P, sum p and the window sums at its first offset from
// the segment sums, runs S_k and sum w_k forward over its offsets by a block scan, adds the chunk partials, undoes the bias:
//   X_k = sum s_p s_w + 128 (sum p + sum w_k) - 16384 m
// and reduces (float bits << 32 | k) with a global 64-bit atomicMin: v >= 0, so the bits order like the value and the smallest
// key is the first smallest v.  In memory the key is the little-endian pair (int32 k, float32 v) of the result.
#include "common.h"

typedef int i32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int AM_THREADS = 256;                 // 4 waves
constexpr int AM_TILES = 4;                     // 256-offset MFMA tiles per wave
constexpr int AM_TK = 4 * AM_TILES * 256;       // offsets per MFMA block
constexpr int AM_SUB = 512;                     // K values staged in LDS at a time
constexpr int AM_MAXSUB = 65536 / AM_SUB;       // K values per chunk <= 65536: int32 partials stay exact
constexpr int AM_SEG = 2048;                    // bytes per segment sum = offsets per finalize block
constexpr int AM_WANT_BLOCKS = 2048;            // MFMA blocks a query asks for (8 per CU) before it stops splitting K

struct AmQuery {
    const uint8_t* pat;        // p[0..m)
    const uint8_t* win;        // w[0..len)
    int* part;                 // [chunks][tiles * AM_TK] int32 partial cross terms
    long long* seg;            // [segp + segw][2] sum, sum of squares
    int m, n, len;             // len = n + m - 1
    int tiles, chunks, spc;    // spc: AM_SUB steps per chunk
    int nsub, segp, segw;
    int begin1, begin2;        // first block of this query in launch 1 / launch 2
};

struct AmArgs {
    AmQuery q[3];
    unsigned long long* out;   // [nq] keys
    int nq;
};

__device__ __forceinline__ int am_query(const AmArgs& a, int bid, bool second) {
    int q = 0;
    for (int i = 1; i < a.nq; ++i)
        if (bid >= (second ? a.q[i].begin2 : a.q[i].begin1)) q = i;
    return q;
}

__device__ __forceinline__ unsigned biased(const uint8_t* p, long i, long lo, long hi) {
    return (i >= lo && i < hi) ? (unsigned)(p[i] ^ 0x80u) : 0u;
}

__device__ void mfma_block(const AmQuery& q, int lb) {
    __shared__ unsigned wlds[(AM_TK + AM_SUB) / 4];
    __shared__ unsigned plds[(AM_SUB + 32) / 4];
    const int tile = lb % q.tiles, chunk = lb / q.tiles;
    const int k0 = tile * AM_TK;
    const int c_begin = chunk * q.spc * AM_SUB, c_end = min(c_begin + q.spc * AM_SUB, q.nsub * AM_SUB);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = lane & 15, grp = lane >> 4;
    i32x4 acc[AM_TILES];
#pragma unroll
    for (int t = 0; t < AM_TILES; ++t) acc[t] = i32x4{0, 0, 0, 0};

    for (int cs = c_begin; cs < c_end; cs += AM_SUB) {
        __syncthreads();
        // window bytes k0 + cs + [0, AM_TK + AM_SUB), pattern bytes cs - 16 + [0, AM_SUB + 32); zero outside their arrays
        for (int d = threadIdx.x; d < (AM_TK + AM_SUB) / 4; d += AM_THREADS) {
            const long i = (long)k0 + cs + 4 * d;
            wlds[d] = biased(q.win, i, 0, q.len) | biased(q.win, i + 1, 0, q.len) << 8 | biased(q.win, i + 2, 0, q.len) << 16 |
                      biased(q.win, i + 3, 0, q.len) << 24;
        }
        for (int d = threadIdx.x; d < (AM_SUB + 32) / 4; d += AM_THREADS) {
            const long i = (long)cs - 16 + 4 * d;
            plds[d] = biased(q.pat, i, 0, q.m) | biased(q.pat, i + 1, 0, q.m) << 8 | biased(q.pat, i + 2, 0, q.m) << 16 |
                      biased(q.pat, i + 3, 0, q.m) << 24;
        }
        __syncthreads();
#pragma unroll 2
        for (int cc = 0; cc < AM_SUB; cc += 64) {
            // A: s_p[cs + cc + 16 grp + j - col], j = 0..15, at LDS byte 16 + cc + 16 grp - col (>= 1)
            const int pos = 16 + cc + 16 * grp - col;
            const int dw = pos >> 2, sh = pos & 3;
            unsigned d[5];
#pragma unroll
            for (int e = 0; e < 5; ++e) d[e] = plds[dw + e];
            i32x4 a;
#pragma unroll
            for (int e = 0; e < 4; ++e) a[e] = (int)__builtin_amdgcn_alignbyte(d[e + 1], d[e], sh);
#pragma unroll
            for (int t = 0; t < AM_TILES; ++t) {
                // B: s_w[k0 + cs + b + 16 col + cc + 16 grp + j], b = the tile's first offset in the block (16-byte aligned)
                const int wb = wave * (AM_TILES * 256) + t * 256 + 16 * col + cc + 16 * grp;
                const i32x4 b = *reinterpret_cast<const i32x4*>(&wlds[wb >> 2]);
                acc[t] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc[t], 0, 0, 0);
            }
        }
    }
    // D[a][r] in lane 16 (a / 4) + r, element a % 4: offsets b + 16 col + 4 grp + 0..3
    int* dst = q.part + (long)chunk * q.tiles * AM_TK + k0 + wave * (AM_TILES * 256) + 16 * col + 4 * grp;
#pragma unroll
    for (int t = 0; t < AM_TILES; ++t) *reinterpret_cast<i32x4*>(dst + t * 256) = acc[t];
}

template <typename T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ void seg_block(const AmQuery& q, int s) {
    __shared__ long long red[2][AM_THREADS / 64];
    const bool pat = s < q.segp;
    const uint8_t* src = pat ? q.pat : q.win;
    const int base = (pat ? s : s - q.segp) * AM_SEG;
    const int cnt = min(AM_SEG, (pat ? q.m : q.len) - base);
    int s1 = 0, s2 = 0;          // <= 2048 * 255^2 < 2^31
    for (int i = threadIdx.x; i < cnt; i += AM_THREADS) {
        const int x = src[base + i];
        s1 += x;
        s2 += x * x;
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = s1;
        red[1][threadIdx.x >> 6] = s2;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        long long t = 0;
        for (int w = 0; w < AM_THREADS / 64; ++w) t += red[threadIdx.x][w];
        q.seg[2 * s + threadIdx.x] = t;
    }
}

__global__ __launch_bounds__(AM_THREADS) void audio_match_main(AmArgs args) {
    const int bid = blockIdx.x;
    if (bid == 0 && (int)threadIdx.x < args.nq) args.out[threadIdx.x] = ~0ull;
    const int qi = am_query(args, bid, false);
    const AmQuery& q = args.q[qi];
    const int lb = bid - q.begin1;
    if (lb < q.tiles * q.chunks) mfma_block(q, lb);
    else seg_block(q, lb - q.tiles * q.chunks);
}

__global__ __launch_bounds__(AM_THREADS) void audio_match_finalize(AmArgs args) {
    constexpr int PER = AM_SEG / AM_THREADS;     // offsets per thread
    __shared__ long long red[6][AM_THREADS / 64];
    __shared__ long long base6[6];
    __shared__ int scan[2][AM_THREADS];
    __shared__ unsigned long long kmin[AM_THREADS / 64];
    const int qi = am_query(args, blockIdx.x, true);
    const AmQuery& q = args.q[qi];
    const int blk = blockIdx.x - q.begin2;
    const int k0 = blk * AM_SEG;                 // a segment boundary of the window
    const int m = q.m, n = q.n;
    const int e = k0 + m, je = e / AM_SEG;       // e <= len
    const long long* wseg = q.seg + 2 * q.segp;

    // P, sum p; window prefix sums at k0 and at k0 + m
    long long v[6] = {0, 0, 0, 0, 0, 0};
    for (int j = threadIdx.x; j < q.segp; j += AM_THREADS) {
        v[0] += q.seg[2 * j];
        v[1] += q.seg[2 * j + 1];
    }
    for (int j = threadIdx.x; j < je; j += AM_THREADS) {
        const long long a = wseg[2 * j], b = wseg[2 * j + 1];
        if (j < blk) {
            v[2] += a;
            v[3] += b;
        }
        v[4] += a;
        v[5] += b;
    }
#pragma unroll 8
    for (int i = je * AM_SEG + threadIdx.x; i < e; i += AM_THREADS) {
        const long long x = q.win[i];
        v[4] += x;
        v[5] += x * x;
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const long long t = wave_sum(v[r]);
        if ((threadIdx.x & 63) == 0) red[r][threadIdx.x >> 6] = t;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        long long t = 0;
        for (int w = 0; w < AM_THREADS / 64; ++w) t += red[threadIdx.x][w];
        base6[threadIdx.x] = t;
    }

    // this thread's offsets k0 + PER t + j; the step from k to k + 1 adds w[k + m] and drops w[k]
    const int kt = k0 + PER * threadIdx.x;
    int d1 = 0, d2 = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int k = kt + j;
        if (k + 1 < n) {
            const int xa = q.win[k + m], xd = q.win[k];
            d1 += xa - xd;
            d2 += xa * xa - xd * xd;
        }
    }
    scan[0][threadIdx.x] = d1;
    scan[1][threadIdx.x] = d2;
    __syncthreads();
    for (int o = 1; o < AM_THREADS; o <<= 1) {       // inclusive scan (block total < 2^31)
        const int a = threadIdx.x >= o ? scan[0][threadIdx.x - o] : 0, b = threadIdx.x >= o ? scan[1][threadIdx.x - o] : 0;
        __syncthreads();
        scan[0][threadIdx.x] += a;
        scan[1][threadIdx.x] += b;
        __syncthreads();
    }
    const long long P1 = base6[0], P2 = base6[1];
    long long w1 = base6[4] - base6[2] + (scan[0][threadIdx.x] - d1);
    long long w2 = base6[5] - base6[3] + (scan[1][threadIdx.x] - d2);

    long long xs[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) xs[j] = 0;
    if (kt < n) {
        const long stride = (long)q.tiles * AM_TK;
#pragma unroll 8
        for (int c = 0; c < q.chunks; ++c) {                 // unrolled: several chunks' loads in flight at once
            const i32x4* pp = reinterpret_cast<const i32x4*>(q.part + c * stride + kt);
#pragma unroll
            for (int h = 0; h < PER / 4; ++h) {
                const i32x4 t = pp[h];
#pragma unroll
                for (int e4 = 0; e4 < 4; ++e4) xs[4 * h + e4] += t[e4];
            }
        }
    }
    const double sp = sqrt((double)P2);
    unsigned long long best = ~0ull;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int k = kt + j;
        if (k < n) {
            const long long x = xs[j] + 128 * (P1 + w1) - 16384LL * m;
            const long long t = w2 - 2 * x + P2;
            const double num = (double)(t > 0 ? t : 0);
            const double den = sqrt((double)w2) * sp;
            const float val = num < den ? (float)(num / den) : 1.0f;
            const unsigned long long key = (unsigned long long)__float_as_uint(val) << 32 | (unsigned)k;
            best = key < best ? key : best;
            if (k + 1 < n) {
                const int xa = q.win[k + m], xd = q.win[k];
                w1 += xa - xd;
                w2 += xa * xa - xd * xd;
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(best, o);
        best = t < best ? t : best;
    }
    if ((threadIdx.x & 63) == 0) kmin[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < AM_THREADS / 64; ++w) best = kmin[w] < best ? kmin[w] : best;
        atomicMin(args.out + qi, best);
    }
}

// Block layout of one query (a pure function of m and n: the workspace size depends on nothing else).
void am_shape(long m, long n, AmQuery& q) {
    q.m = (int)m;
    q.n = (int)n;
    q.len = (int)(n + m - 1);
    q.tiles = (int)((n + AM_TK - 1) / AM_TK);
    q.nsub = (int)((m + 15 + AM_SUB - 1) / AM_SUB);
    int chunks = max((AM_WANT_BLOCKS + q.tiles - 1) / q.tiles, (q.nsub + AM_MAXSUB - 1) / AM_MAXSUB);
    chunks = min(chunks, q.nsub);
    q.spc = (q.nsub + chunks - 1) / chunks;
    q.chunks = (q.nsub + q.spc - 1) / q.spc;
    q.segp = (int)((m + AM_SEG - 1) / AM_SEG);
    q.segw = (int)((q.len + AM_SEG - 1) / AM_SEG);
}

size_t am_align(size_t x) { return (x + 255) & ~(size_t)255; }
size_t am_part_bytes(const AmQuery& q) { return am_align((size_t)q.chunks * q.tiles * AM_TK * 4); }
size_t am_seg_bytes(const AmQuery& q) { return am_align((size_t)(q.segp + q.segw) * 16); }

}  // namespace

// Workspace of one call: per query, its partials and segment sums (256-byte aligned pieces).
size_t vse_audio_match_ws(const long* m, const long* n, int nq) {
    size_t tot = 0;
    for (int i = 0; i < nq; ++i) {
        AmQuery q;
        am_shape(m[i], n[i], q);
        tot += am_part_bytes(q) + am_seg_bytes(q);
    }
    return tot;
}

// Arguments checked by the caller (vse_runtime.hip): 1 <= nq <= 3, ranges inside their streams, ws large enough.
int vse_audio_match_launch(const uint8_t* const* pat, const uint8_t* const* win, const long* m, const long* n, int nq, void* d_ws,
                           unsigned long long* d_out, void* stream) {
    AmArgs a = {};
    a.out = d_out;
    a.nq = nq;
    char* ws = static_cast<char*>(d_ws);
    int b1 = 0, b2 = 0;
    for (int i = 0; i < nq; ++i) {
        AmQuery& q = a.q[i];
        am_shape(m[i], n[i], q);
        q.pat = pat[i];
        q.win = win[i];
        q.part = reinterpret_cast<int*>(ws);
        ws += am_part_bytes(q);
        q.seg = reinterpret_cast<long long*>(ws);
        ws += am_seg_bytes(q);
        q.begin1 = b1;
        q.begin2 = b2;
        b1 += q.tiles * q.chunks + q.segp + q.segw;
        b2 += (q.n + AM_SEG - 1) / AM_SEG;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(audio_match_main, dim3(b1), dim3(AM_THREADS), 0, st, a);
    if (hipGetLastError() != hipSuccess) return VSE_E_HIP;
    hipLaunchKernelGGL(audio_match_finalize, dim3(b2), dim3(AM_THREADS), 0, st, a);
    return hipGetLastError() == hipSuccess ? VSE_OK : VSE_E_HIP;
}
