// Scene-cut finder, device part (vse_scene_change, include/vse_hip.h): per frame, how many 16x16 macroblocks of a box-filtered
// luma plane the previous frame cannot predict, the role SCXvid's XviD first pass plays for Sushi's keyframes.  The integers
// are the specification (tests/scene_cut_ref.py restates them in numpy, bit for bit):
//   Y = (29 B + 150 G + 77 R + 128) >> 8
//   A[y][x] = (sum of the s x s luma box at (y s, x s) + s s / 2) / (s s)             ah = H / s, aw = W / s
//   inter_b = min over (dy, dx) in [-R, R]^2, displaced block wholly inside the plane, of sum |A_t - P(+dy, +dx)|   (P = A_(t-1))
//   m_b = (sum A_t + 128) >> 8, intra_b = sum |A_t - m_b|, block b changed iff 2 inter_b > intra_b + bias
//   counts[t] = (changed blocks, sum inter_b, sum intra_b); without a predecessor (bh bw, 0, sum intra_b)
//
// Three launches per call, ordered by the stream:
//   scene_plane_kernel   streams the BGR bytes once (memory-bound) and writes the planes of the call to the caller's workspace;
//   scene_search_kernel  a block owns up to SC_GROUP horizontally adjacent macroblocks of one frame.  Each macroblock's reference window
//                        of (16 + 2R)^2 bytes of P sits in LDS (bytes outside the plane are zero and their vectors masked).  A lane owns
//                        one dy and four consecutive dx: per block row it reads five window dwords and issues four packed quad-SADs
//                        (v_qsad_pk_u16_u8: four SADs of four pixels at consecutive byte offsets; a block's SAD is at most
//                        256 * 255 = 65280, so the four 16-bit accumulators cannot overflow).  The window is staged as whole dwords of
//                        the plane rows (its left edge rounded down to one), and m_b and intra_b are summed with v_sad_u8 by the threads
//                        that stage the macroblock itself.  Minima meet in LDS; one thread adds the block's three sums to the frame's
//                        counts (integer sums: the totals do not depend on the order the blocks arrive in);
//   scene_state_kernel   copies the last plane into the caller's state and sets its flag (after the search has read the old one).
#include "common.h"

namespace {

constexpr int SC_MB = 16;          // macroblock edge on the plane
constexpr int SC_MAXR = 8;         // largest search radius
constexpr int SC_WROWS = SC_MB + 2 * SC_MAXR;      // window rows
constexpr int SC_WPITCH = 9;       // window row pitch in dwords: a lane reads dwords q .. q + 4, q <= 4; odd, so rows spread over the banks
constexpr int SC_GROUP = 8;        // most macroblocks per search block (3 at R = 8: 3 * 85 lanes of work for 256 threads)
constexpr int SC_THREADS = 256;

__device__ __forceinline__ int luma(const uint8_t* p) {
    return (29 * (int)p[0] + 150 * (int)p[1] + 77 * (int)p[2] + 128) >> 8;
}

// planes[t][y][x], row pitch ap bytes (a multiple of 4; the pad bytes are never read as pixels)
__global__ __launch_bounds__(SC_THREADS) void scene_plane_kernel(const uint8_t* __restrict__ src, long pitch, long fstride, int s, int ah, int aw,
                                                                 int ap, uint8_t* __restrict__ planes) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= aw || y >= ah) return;
    const uint8_t* p = src + (long)blockIdx.z * fstride + (long)y * s * pitch + (long)x * s * 3;
    int sum = 0;
    for (int j = 0; j < s; ++j, p += pitch)
        for (int i = 0; i < s; ++i) sum += luma(p + i * 3);
    const int ss = s * s;
    planes[((long)blockIdx.z * ah + y) * ap + x] = (uint8_t)((sum + ss / 2) / ss);
}

// grid: (ceil(bw / group), bh, n).  prev0: the plane before frame 0 (the state's), used when has_prev0.
__global__ __launch_bounds__(SC_THREADS) void scene_search_kernel(const uint8_t* __restrict__ planes, const uint8_t* __restrict__ prev0,
                                                                  const unsigned* flag, int reset, int ah, int aw, int ap, int bw, int R,
                                                                  int bias, int group, int* __restrict__ counts) {
    __shared__ unsigned win[SC_GROUP][SC_WROWS * SC_WPITCH];
    __shared__ unsigned cur[SC_GROUP][SC_MB * SC_MB / 4];
    __shared__ int best[SC_GROUP], intra[SC_GROUP];
    __shared__ unsigned total[SC_GROUP];
    const int tid = threadIdx.x, t = blockIdx.z, by = blockIdx.y, bx0 = blockIdx.x * group;
    const int ng = min(group, bw - bx0);
    const bool has_prev = t > 0 || (!reset && *flag != 0);
    const uint8_t* A = planes + (long)t * ah * ap;
    const uint8_t* P = t > 0 ? A - (long)ah * ap : prev0;
    const int wrows = SC_MB + 2 * R;
    const int o = (4 - (R & 3)) & 3;               // the window starts at column 16 bx - R - o: a whole dword of the plane row

    if (tid < SC_GROUP) {
        best[tid] = 0x7fffffff;
        intra[tid] = 0;
        total[tid] = 0u;
    }
    __syncthreads();
    for (int v = tid; v < ng * (SC_MB * SC_MB / 4); v += SC_THREADS) {
        const int g = v >> 6, y = (v >> 2) & 15, c = v & 3;
        const unsigned d = *reinterpret_cast<const unsigned*>(A + (long)(by * SC_MB + y) * ap + (bx0 + g) * SC_MB + c * 4);
        cur[g][y * 4 + c] = d;
        atomicAdd(&total[g], __builtin_amdgcn_sad_u8(d, 0u, 0u));
    }
    if (has_prev) {
        // dwords that lie outside the plane are zero; one that straddles aw holds pad bytes, which only masked vectors read
        const int per = wrows * SC_WPITCH;
        for (int v = tid; v < ng * per; v += SC_THREADS) {
            const int g = v / per, r = v - g * per, wy = r / SC_WPITCH, k = r - wy * SC_WPITCH;
            const int py = by * SC_MB - R + wy, px = (bx0 + g) * SC_MB - R - o + k * 4;
            const bool in = py >= 0 && py < ah && px >= 0 && px < ap;
            win[g][wy * SC_WPITCH + k] = in ? *reinterpret_cast<const unsigned*>(P + (long)py * ap + px) : 0u;
        }
    }
    __syncthreads();
    for (int v = tid; v < ng * (SC_MB * SC_MB / 4); v += SC_THREADS) {
        const int g = v >> 6;
        const unsigned m = ((total[g] + 128) >> 8) * 0x01010101u;
        atomicAdd(&intra[g], (int)__builtin_amdgcn_sad_u8(cur[g][v & 63], m, 0u));
    }

    const int nq = (2 * R + o + 4) / 4;            // quads of window columns per dy
    const int lanes = (2 * R + 1) * nq;            // search lanes of a macroblock
    for (int item = tid; has_prev && item < ng * lanes; item += SC_THREADS) {
        const int g = item / lanes, r = item - g * lanes;
        const unsigned* c = cur[g];
        const int iy = r / nq, q = r - iy * nq;
        const int y0 = by * SC_MB + iy - R;
        const unsigned* w = win[g] + iy * SC_WPITCH + q;
        unsigned long long acc = 0;
#pragma unroll 4
        for (int y = 0; y < SC_MB; ++y, w += SC_WPITCH) {
            const unsigned long long r0 = w[0], r1 = w[1], r2 = w[2], r3 = w[3], r4 = w[4];
            acc = __builtin_amdgcn_qsad_pk_u16_u8(r0 | (r1 << 32), c[y * 4 + 0], acc);
            acc = __builtin_amdgcn_qsad_pk_u16_u8(r1 | (r2 << 32), c[y * 4 + 1], acc);
            acc = __builtin_amdgcn_qsad_pk_u16_u8(r2 | (r3 << 32), c[y * 4 + 2], acc);
            acc = __builtin_amdgcn_qsad_pk_u16_u8(r3 | (r4 << 32), c[y * 4 + 3], acc);
        }
        int b = 0x7fffffff;
        if (y0 >= 0 && y0 + SC_MB <= ah) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int ox = q * 4 + i - o, x0 = (bx0 + g) * SC_MB + ox - R;          // ox = R + dx
                if (ox >= 0 && ox <= 2 * R && x0 >= 0 && x0 + SC_MB <= aw) b = min(b, (int)((acc >> (16 * i)) & 0xffffu));
            }
        }
        if (b != 0x7fffffff) atomicMin(&best[g], b);
    }
    __syncthreads();
    if (tid == 0) {
        int changed = 0, inter = 0, tra = 0;
        for (int g = 0; g < ng; ++g) {
            const int e = has_prev ? best[g] : 0;
            changed += (!has_prev || 2 * e > intra[g] + bias) ? 1 : 0;
            inter += e;
            tra += intra[g];
        }
        int* o = counts + (long)t * 3;
        if (changed) atomicAdd(o, changed);
        if (inter) atomicAdd(o + 1, inter);
        if (tra) atomicAdd(o + 2, tra);
    }
}

__global__ __launch_bounds__(SC_THREADS) void scene_state_kernel(const unsigned* __restrict__ last, int words, unsigned* __restrict__ state_plane,
                                                                 unsigned* flag) {
    const int v = blockIdx.x * SC_THREADS + threadIdx.x;
    if (v < words) state_plane[v] = last[v];
    if (v == 0) *flag = 1u;
}

}  // namespace

// Plane geometry shared with vse_runtime.hip: plane row pitch in bytes.
int vse_scene_change_plane_pitch(int aw) { return (aw + 3) & ~3; }

// Called by vse_scene_change (vse_runtime.hip) after it has checked the arguments.
int vse_scene_change_launch(const void* d_bgr, int n, int64_t pitch, int64_t frame_stride, int scale, int ah, int aw, int search, int bias,
                            void* d_state, int reset, void* d_ws, int32_t* d_counts, void* stream) {
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const int ap = vse_scene_change_plane_pitch(aw), bh = ah / SC_MB, bw = aw / SC_MB;
    const int lanes = (2 * search + 1) * ((2 * search + ((4 - (search & 3)) & 3) + 4) / 4);
    const int group = max(1, min(SC_GROUP, SC_THREADS / lanes));
    if (hipMemsetAsync(d_counts, 0, (size_t)n * 3 * sizeof(int32_t), st) != hipSuccess) return VSE_E_HIP;
    uint8_t* planes = reinterpret_cast<uint8_t*>(d_ws);
    unsigned* flag = reinterpret_cast<unsigned*>(d_state);
    uint8_t* state_plane = reinterpret_cast<uint8_t*>(d_state) + 16;
    hipLaunchKernelGGL(scene_plane_kernel, dim3((aw + 63) / 64, (ah + 3) / 4, n), dim3(SC_THREADS), 0, st,
                       reinterpret_cast<const uint8_t*>(d_bgr), (long)pitch, (long)frame_stride, scale, ah, aw, ap, planes);
    hipLaunchKernelGGL(scene_search_kernel, dim3((bw + group - 1) / group, bh, n), dim3(SC_THREADS), 0, st, planes, state_plane, flag, reset, ah,
                       aw, ap, bw, search, bias, group, reinterpret_cast<int*>(d_counts));
    const int words = ah * ap / 4;
    hipLaunchKernelGGL(scene_state_kernel, dim3((words + SC_THREADS - 1) / SC_THREADS), dim3(SC_THREADS), 0, st,
                       reinterpret_cast<const unsigned*>(planes + (size_t)(n - 1) * ah * ap), words, reinterpret_cast<unsigned*>(state_plane), flag);
    return hipGetLastError() == hipSuccess ? VSE_OK : VSE_E_HIP;
}
