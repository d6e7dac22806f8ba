// Subtitle-change frame selector, device part (vse_frame_change, include/vse_hip.h): per frame, the luma edge mask of the
// subtitle area and how much of it appeared / vanished against the previous frame.  The integers are the specification
// (tests/frame_change_ref.py restates them in numpy, bit for bit):
//   Y = (29 B + 150 G + 77 R + 128) >> 8
//   E = max(|Y[y][x+1] - Y[y][x-1]|, |Y[y+1][x] - Y[y-1][x]|) >= thresh   for the interior pixels of the area
//   edges = |E|, appeared = |E & ~E'|, vanished = |E' & ~E|               (E' = the previous frame's mask)
// Memory-bound byte work: one pass over the area rows of every frame, a few integers out per frame.
//
// Layout: a block owns one 64-column word of FC_ROWS interior rows (a tile) for ALL frames of the call.  Its waves compute the
// tile's mask words of different frames side by side (the frames are independent), a ballot of 64 consecutive columns being
// one packed word; the words of a chunk of frames meet in LDS, where one thread per frame compares each frame with the one
// before it.  The previous mask of the tile is read from the caller's state at the start and written back at the end by the
// same block: no block reads what another block writes, so a batch needs no second pass and no grid-wide ordering.
#include "common.h"

namespace {

constexpr int FC_ROWS = 8;     // interior rows of a tile (+2 halo rows; 16 rows hold 148 VGPRs and spill SGPRs)
constexpr int FC_WAVES = 8;    // waves per block: frames of a chunk in flight at once
constexpr int FC_CHUNK = 64;   // frames whose mask words are held in LDS at a time (4 KiB)

__device__ __forceinline__ int luma(const uint8_t* p) {
    return (29 * (int)p[0] + 150 * (int)p[1] + 77 * (int)p[2] + 128) >> 8;
}

// src points at row y0 of frame 0 (the kernel reads rows y0 .. y0 + ih + 1 and columns x0 .. x0 + iw + 1 only).
// words[iy * wpr + w]: packed mask of interior row iy, columns 64 w .. 64 w + 63; flag: nonzero once the words hold a mask.
__global__ __launch_bounds__(FC_WAVES * 64) void frame_change_kernel(const uint8_t* __restrict__ src, int n, long pitch, long fstride,
                                                                     int x0, int ih, int iw, int wpr, int thresh,
                                                                     unsigned long long* __restrict__ words, unsigned* flag, int reset,
                                                                     int* __restrict__ counts) {
    __shared__ unsigned long long msk[FC_CHUNK][FC_ROWS];
    __shared__ unsigned long long prv[FC_ROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int w = blockIdx.x, iy0 = blockIdx.y * FC_ROWS;
    const int rows = min(FC_ROWS, ih - iy0);
    const int ix = w * 64 + lane;              // interior column of this lane
    const bool inner = ix < iw;
    const bool own = ix <= iw;                 // the right border column is read too (the horizontal neighbour of the last one)
    const int x = x0 + 1 + ix;
    // a wave's horizontal neighbours come from the lanes beside it; lanes 0 and 63 read the column outside the word themselves
    const bool extra = inner && (lane == 0 || lane == 63);
    const int xe = lane == 0 ? x - 1 : x + 1;
    unsigned long long* st = words + (long)iy0 * wpr + w;
    // A flag set by another block of this launch leaves this block reading its own words of the previous call, which are
    // zero in a fresh (zero-filled) state: the same empty mask as an unset flag.
    const bool use_prev = !reset && *(volatile unsigned*)flag != 0;
    if (threadIdx.x < FC_ROWS) prv[threadIdx.x] = (use_prev && (int)threadIdx.x < rows) ? st[(long)threadIdx.x * wpr] : 0ull;

    for (int c0 = 0; c0 < n; c0 += FC_CHUNK) {
        const int cn = min(FC_CHUNK, n - c0);
        for (int tl = wave; tl < cn; tl += FC_WAVES) {
            const uint8_t* f = src + (long)(c0 + tl) * fstride + (long)iy0 * pitch;
            int yc[FC_ROWS + 2], ye[FC_ROWS];
#pragma unroll
            for (int k = 0; k < FC_ROWS + 2; ++k) yc[k] = (k < rows + 2 && own) ? luma(f + (long)k * pitch + x * 3) : 0;
#pragma unroll
            for (int k = 0; k < FC_ROWS; ++k) ye[k] = (k < rows && extra) ? luma(f + (long)(k + 1) * pitch + xe * 3) : 0;
#pragma unroll
            for (int k = 0; k < FC_ROWS; ++k) {
                unsigned long long b = 0;
                if (k < rows) {                // block-uniform
                    const int l = __shfl_up(yc[k + 1], 1), r = __shfl_down(yc[k + 1], 1);
                    const int left = lane == 0 ? ye[k] : l, right = lane == 63 ? ye[k] : r;
                    const int e = max(abs(right - left), abs(yc[k + 2] - yc[k]));
                    b = __ballot(inner && e >= thresh);
                }
                if (lane == 0) msk[tl][k] = b;
            }
        }
        __syncthreads();
        if ((int)threadIdx.x < cn) {
            const int tl = threadIdx.x;
            int e = 0, a = 0, v = 0;
#pragma unroll
            for (int k = 0; k < FC_ROWS; ++k) {        // words of rows outside the area are zero
                const unsigned long long cur = msk[tl][k], pre = tl ? msk[tl - 1][k] : prv[k];
                e += __popcll(cur);
                a += __popcll(cur & ~pre);
                v += __popcll(pre & ~cur);
            }
            // integer sums: the totals do not depend on the order the blocks arrive in
            int* o = counts + (long)(c0 + tl) * 3;
            if (e) atomicAdd(o, e);
            if (a) atomicAdd(o + 1, a);
            if (v) atomicAdd(o + 2, v);
        }
        __syncthreads();
        if (threadIdx.x < FC_ROWS) prv[threadIdx.x] = msk[cn - 1][threadIdx.x];
        __syncthreads();
    }
    if ((int)threadIdx.x < rows) st[(long)threadIdx.x * wpr] = prv[threadIdx.x];
    if (threadIdx.x == 0) *flag = 1u;
}

}  // namespace

// Called by vse_frame_change (vse_runtime.hip) after it has checked the geometry.
int vse_frame_change_launch(const void* d_bgr, int n, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0, int x1, int edge_thresh,
                            void* d_state, int reset, int32_t* d_counts, void* stream) {
    const int ih = y1 - y0 - 2, iw = x1 - x0 - 2, wpr = (iw + 63) / 64;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(d_counts, 0, (size_t)n * 3 * sizeof(int32_t), st) != hipSuccess) return VSE_E_HIP;
    unsigned* flag = reinterpret_cast<unsigned*>(d_state);
    unsigned long long* words = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(d_state) + 16);
    const uint8_t* src = reinterpret_cast<const uint8_t*>(d_bgr) + (long)y0 * pitch;
    hipLaunchKernelGGL(frame_change_kernel, dim3(wpr, (ih + FC_ROWS - 1) / FC_ROWS), dim3(FC_WAVES * 64), 0, st, src, n, (long)pitch,
                       (long)frame_stride, x0, ih, iw, wpr, edge_thresh, words, flag, reset, reinterpret_cast<int*>(d_counts));
    return hipGetLastError() == hipSuccess ? VSE_OK : VSE_E_HIP;
}
