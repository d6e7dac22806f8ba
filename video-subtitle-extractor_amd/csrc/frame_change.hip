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
//
// The other entry points work on the same tiles and the same mask.  The kernels, in the order of the file:
//   frame_change_kernel               vse_frame_change, above.
//   frame_cells_kernel                vse_frame_cells, the subtitle-area locator: a tile is a CELL that keeps its own counts and runs the
//                                     interval automaton of frame_select.change_intervals on them.
//   frame_cells_multi_kernel          vse_frame_cells_multi, _counts and _masks: the cells for several edge thresholds in one pass over the
//                                     frames (threshold calibration), optionally with the whole region's counts per threshold or with the mask
//                                     words of every frame kept in the caller's buffer.  One template, the extra output a compile-time kind.
//   frame_cells_export_kernel,        one threshold's slice of a cells state as a vse_frame_change state, and the counts of any rectangle
//   frame_masks_replay_kernel         of the region out of the kept mask words, as frame_change_kernel would have counted them on the frames.
//   frame_hold_kernel,                vse_frame_hold: only edge pixels that hold still for `hold` frames are counted, so that the edges of a
//   frame_masks_replay_hold_kernel    moving background drop out; and vse_frame_masks_replay_hold, the same walk (frame_hold_body) on a
//                                     rectangle of the region with the kept mask words in place of the frames.
//   frame_cells_hold_kernel           vse_frame_cells_hold and _hold_masks: the cells and their automaton at several thresholds on the held
//                                     masks, optionally with the EDGE words of every frame kept in the caller's buffer.
//   frame_focus_kernel                vse_frame_focus: per frame, the number of edge pixels that were edge pixels one frame earlier and the
//                                     sum of their gradients.
//   frame_hold_bounded_kernel,        vse_frame_hold_bounded: the held-edge walk, but only runs of hold .. max_hold frames are counted, so that
//   frame_hold_rows_kernel,           the edges of a background that stands still drop out too; and vse_frame_masks_replay_hold_bounded,
//   frame_masks_replay_hold_bounded_kernel  the same walk (frame_hold_bounded_body) on a rectangle of the region with the kept mask words.
//   frame_cells_hold_bounded_kernel   vse_frame_cells_hold_bounded and _bounded_masks: the cells and their automaton at several thresholds
//                                     on the bounded masks, optionally with the EDGE words of every frame kept in the caller's buffer.
// The launchers of the first nine follow frame_focus_kernel; the two bounded sections each end with their own.
//
// What the kernels share is written once where that leaves their code as it was: the tile (tile_lane, tile_masks, tile_masks_multi), the
// automaton (CellRuns, with the load and store of its state), the small pieces of a chunk (zero_steps, edge_bit), and on the host what
// the launchers of the several-threshold kernels build and the choice of the instantiation (CellsLaunch, launch_for_nt).  Two pieces stay
// written out in each kernel that has them, because every shared form that was tried compiled those kernels to other code than the inline
// text does (EXPERIMENTS.md, "One cells kernel template"): the popcount loop over a step's words, and the two ballots with the stepping
// of CellRuns behind them.  A change to either is a change to each of: frame_cells_kernel, frame_cells_multi_kernel, frame_cells_hold_kernel,
// frame_cells_hold_bounded_kernel (the ballots) and frame_hold_kernel (the loop).
#include <type_traits>

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

// ---- the tile, shared by every kernel below ------------------------------------------------------------------------------------------
// The tile and its mask words are frame_change_kernel's above, statement for statement, as two helpers.  frame_change_kernel keeps its
// own inline copy: routed through these helpers it compiled to slightly different code and measured 0.3-0.6 % slower (64 x 1080p,
// alternating with the inline build in one process).
// What a lane reads of its block's tile; fixed for the whole kernel.
struct TileLane {
    int rows;       // interior rows of the tile that lie in the area
    bool inner;     // the lane's column is an interior column
    bool own;       // ... or the right border column (the horizontal neighbour of the last one), which is read too
    bool extra;     // a wave's horizontal neighbours come from the lanes beside it; lanes 0 and 63 read the column outside the word themselves
    int x, xe;      // frame column of the lane, and of that extra read
};

__device__ __forceinline__ TileLane tile_lane(int w, int iy0, int ih, int iw, int x0) {
    const int lane = threadIdx.x & 63;
    const int ix = w * 64 + lane;              // interior column of this lane
    TileLane t;
    t.rows = min(FC_ROWS, ih - iy0);
    t.inner = ix < iw;
    t.own = ix <= iw;
    t.x = x0 + 1 + ix;
    t.extra = t.inner && (lane == 0 || lane == 63);
    t.xe = lane == 0 ? t.x - 1 : t.x + 1;
    return t;
}

// msk[tl][k] = packed mask of the tile's interior row k in frame c0 + tl, for tl < cn: a wave per frame, the waves side by side.
// src points at the tile's first halo row in frame 0 (rows 0 .. rows + 1 and columns x0 .. x0 + iw + 1 of the area are read only).
__device__ __forceinline__ void tile_masks(const uint8_t* __restrict__ src, int c0, int cn, long pitch, long fstride, const TileLane& t,
                                           int thresh, unsigned long long (*msk)[FC_ROWS]) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rows = t.rows;
    for (int tl = wave; tl < cn; tl += FC_WAVES) {
        const uint8_t* f = src + (long)(c0 + tl) * fstride;
        int yc[FC_ROWS + 2], ye[FC_ROWS];
#pragma unroll
        for (int k = 0; k < FC_ROWS + 2; ++k) yc[k] = (k < rows + 2 && t.own) ? luma(f + (long)k * pitch + t.x * 3) : 0;
#pragma unroll
        for (int k = 0; k < FC_ROWS; ++k) ye[k] = (k < rows && t.extra) ? luma(f + (long)(k + 1) * pitch + t.xe * 3) : 0;
#pragma unroll
        for (int k = 0; k < FC_ROWS; ++k) {
            unsigned long long b = 0;
            if (k < rows) {                // block-uniform
                const int l = __shfl_up(yc[k + 1], 1), r = __shfl_down(yc[k + 1], 1);
                const int left = lane == 0 ? ye[k] : l, right = lane == 63 ? ye[k] : r;
                const int e = max(abs(right - left), abs(yc[k + 2] - yc[k]));
                b = __ballot(t.inner && e >= thresh);
            }
            if (lane == 0) msk[tl][k] = b;
        }
    }
}

// Up to FC_WAVES edge thresholds at once: a frame's bytes are read and its lumas and gradients computed once; per threshold only the
// compare / ballot differs.
struct CellThresholds {
    int t[FC_WAVES];        // ascending, each 1..255; those beyond the kernel's NT unused
};

// tile_masks with the ballot repeated per threshold (tile_masks itself stays as it is: split into shared pieces it compiled
// frame_cells_kernel and frame_hold_kernel to different code).
// msk[(q * FC_CHUNK + tl) * FC_ROWS + k] = packed mask at threshold q of the tile's interior row k in frame c0 + tl, for tl < cn.
template <int NT>
__device__ __forceinline__ void tile_masks_multi(const uint8_t* __restrict__ src, int c0, int cn, long pitch, long fstride, const TileLane& t,
                                                 const CellThresholds& th, unsigned long long* msk) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rows = t.rows;
    for (int tl = wave; tl < cn; tl += FC_WAVES) {
        const uint8_t* f = src + (long)(c0 + tl) * fstride;
        int yc[FC_ROWS + 2], ye[FC_ROWS];
#pragma unroll
        for (int k = 0; k < FC_ROWS + 2; ++k) yc[k] = (k < rows + 2 && t.own) ? luma(f + (long)k * pitch + t.x * 3) : 0;
#pragma unroll
        for (int k = 0; k < FC_ROWS; ++k) ye[k] = (k < rows && t.extra) ? luma(f + (long)(k + 1) * pitch + t.xe * 3) : 0;
#pragma unroll
        for (int k = 0; k < FC_ROWS; ++k) {
            int e = -1;                    // below every threshold: the words of rows outside the area are zero
            if (k < rows) {                // block-uniform
                const int l = __shfl_up(yc[k + 1], 1), r = __shfl_down(yc[k + 1], 1);
                const int left = lane == 0 ? ye[k] : l, right = lane == 63 ? ye[k] : r;
                if (t.inner) e = max(abs(right - left), abs(yc[k + 2] - yc[k]));
            }
            unsigned long long b[NT];
#pragma unroll
            for (int q = 0; q < NT; ++q) b[q] = __ballot(e >= th.t[q]);
            if (lane == 0) {
#pragma unroll
                for (int q = 0; q < NT; ++q) msk[(q * FC_CHUNK + tl) * FC_ROWS + k] = b[q];
            }
        }
    }
}

// ---- the pieces of a chunk, shared by the kernels that walk its words ---------------------------------------------------------------------
// The steps real .. cn - 1 of a chunk are the flush, without an edge anywhere: their words are zero at every threshold.  (The kernels of
// one threshold keep msk as [FC_CHUNK][FC_ROWS] and zero it by that index: through this helper their address took one instruction more.)
template <int NT>
__device__ __forceinline__ void zero_steps(unsigned long long* msk, int real, int cn) {
    for (int i = real * FC_ROWS + threadIdx.x; i < cn * FC_ROWS; i += FC_WAVES * 64) {
#pragma unroll
        for (int q = 0; q < NT; ++q) msk[q * FC_CHUNK * FC_ROWS + i] = 0ull;
    }
}

// A wave that walks a row with lane = column holds the row's words with lane = step, as halves lo / hi: the lane's own bit of step tl.
// (`lane` is the kernel's own value: recomputed here from threadIdx.x it changed the compare in all four kernels.)
__device__ __forceinline__ bool edge_bit(int lo, int hi, int tl, int lane) {
    const unsigned half = (unsigned)(lane < 32 ? __builtin_amdgcn_readlane(lo, tl) : __builtin_amdgcn_readlane(hi, tl));
    return (half >> (lane & 31)) & 1u;
}

// ---- the cells' automaton --------------------------------------------------------------------------------------------------------------
// Per-cell state of vse_frame_cells: the FC_ROWS mask words of the cell's last frame, then the length of its open run.
constexpr int CELL_STATE_WORDS = FC_ROWS + 1;

// One cell's interval automaton: frame_select.change_intervals in integers, with the run lengths summed instead of listed.
// Every value here is the same in all lanes of the wave that walks it.
struct CellRuns {
    int run, covered, runs, present, cuts;
    // from the state a call left: the open run (a word of the cells state, or an int of the held states) and the cell's four totals
    template <class R>
    __device__ __forceinline__ void load(const R* open_run, const int* tot) {
        *this = {(int)*open_run, tot[0], tot[1], tot[2], tot[3]};
    }
    // ... and back, by one lane; a flush closes the open run first (frame_cells_hold_bounded_kernel stores its carry between the two and
    // keeps the statements inline: through this function its registers were numbered otherwise)
    template <class R>
    __device__ __forceinline__ void store(R* open_run, int* tot, int flush, const CellRule& r) {
        if (flush) close(r);
        *open_run = (R)run;
        tot[0] = covered;
        tot[1] = runs;
        tot[2] = present;
        tot[3] = cuts;
    }
    __device__ __forceinline__ void close(const CellRule& r) {
        if (run >= r.min_frames && run <= r.max_frames) {
            covered += run;
            ++runs;
        }
        run = 0;
    }
    // is_present: edges >= min_edges; ratio_cut: the ratio test against the frame before (it counts only inside a run)
    __device__ __forceinline__ void step(bool is_present, bool ratio_cut, const CellRule& r) {
        if (!is_present) {
            close(r);
            return;
        }
        ++present;
        if (run && ratio_cut) {
            ++cuts;
            close(r);
        }
        ++run;
    }
};

// ---- vse_frame_cells ------------------------------------------------------------------------------------------------------------
// The grid is gx x gy cells; block (cx, cy) owns cell cy * gx + cx in state, totals and cell_counts alike, for all frames of the call.
// src points at row y0 of frame 0.  Runs with n == 0 too (reset and flush only).
__global__ __launch_bounds__(FC_WAVES * 64) void frame_cells_kernel(const uint8_t* __restrict__ src, int n, long pitch, long fstride,
                                                                    int x0, int ih, int iw, int thresh, CellRule rule,
                                                                    unsigned long long* __restrict__ state, int reset, int flush,
                                                                    int* __restrict__ totals, int* __restrict__ cell_counts) {
    __shared__ unsigned long long msk[FC_CHUNK][FC_ROWS];
    __shared__ unsigned long long prv[FC_ROWS];
    static_assert(FC_CHUNK == 64, "the frames of a chunk are the lanes of wave 0");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int iy0 = blockIdx.y * FC_ROWS;
    const long cell = (long)blockIdx.y * gridDim.x + blockIdx.x, cells = (long)gridDim.y * gridDim.x;
    const TileLane t = tile_lane(blockIdx.x, iy0, ih, iw, x0);
    unsigned long long* st = state + cell * CELL_STATE_WORDS;
    int* tot = totals + cell * 4;
    // words of rows outside the region are zero in every frame, so all FC_ROWS words are kept
    if (threadIdx.x < FC_ROWS) prv[threadIdx.x] = reset ? 0ull : st[threadIdx.x];
    CellRuns cr = {0, 0, 0, 0, 0};
    if (wave == 0 && !reset) cr.load(st + FC_ROWS, tot);

    for (int c0 = 0; c0 < n; c0 += FC_CHUNK) {
        const int cn = min(FC_CHUNK, n - c0);
        tile_masks(src + (long)iy0 * pitch, c0, cn, pitch, fstride, t, thresh, msk);
        __syncthreads();
        if (wave == 0) {                           // lane = frame of the chunk
            const bool live = lane < cn;
            int e = 0, a = 0, v = 0, ep = 0;
            if (live) {
#pragma unroll
                for (int k = 0; k < FC_ROWS; ++k) {
                    const unsigned long long cur = msk[lane][k], pre = lane ? msk[lane - 1][k] : prv[k];
                    e += __popcll(cur);
                    a += __popcll(cur & ~pre);
                    v += __popcll(pre & ~cur);
                    ep += __popcll(pre);           // edges[t-1]
                }
                if (cell_counts) {
                    int* o = cell_counts + ((long)(c0 + lane) * cells + cell) * 3;
                    o[0] = e;
                    o[1] = a;
                    o[2] = v;
                }
            }
            const long long uni = ep + a;          // |E' or E|
            const unsigned long long present = __ballot(live && e >= rule.min_edges);
            const unsigned long long ratio = __ballot(live && uni > 0 && (long long)(a + v) * rule.ratio_den >= (long long)rule.ratio_num * uni);
            for (int f = 0; f < cn; ++f) cr.step((present >> f) & 1, (ratio >> f) & 1, rule);
        }
        __syncthreads();
        if (threadIdx.x < FC_ROWS) prv[threadIdx.x] = msk[cn - 1][threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x < FC_ROWS) st[threadIdx.x] = prv[threadIdx.x];
    if (threadIdx.x == 0) cr.store(st + FC_ROWS, tot, flush, rule);
}

// ---- vse_frame_cells_multi, vse_frame_cells_counts, vse_frame_cells_masks ------------------------------------------------------------------
// frame_cells_kernel for NT = 1 .. FC_WAVES edge thresholds in one pass (a template parameter: the ballots of a row unroll without a branch
// per threshold).  tile_masks_multi leaves the mask words of the NT thresholds side by side in LDS; wave q then walks threshold q's automaton
// exactly as wave 0 does above.  Grid and cell ownership as frame_cells_kernel; threshold q's state is state[(q * cells + cell) *
// CELL_STATE_WORDS ..] and its totals totals[(q * cells + cell) * 4 ..], each slice laid out as vse_frame_cells lays out its own.  Runs with
// n == 0 too (reset and flush only; no extra output is touched).
// OUT names what else a pass writes, with its arguments as the trailing pack x (instantiated with the explicit types of the launcher, so
// that the pointers keep their __restrict__; arguments that a kind lacks are not in its signature, which keeps each kind's code as if it
// were written alone):
//   CELLS_ONLY    nothing.
//   CELLS_COUNTS  int* counts: the cells tile the interior of the region exactly as frame_change_kernel's tiles tile the interior of its
//                 area, and the mask is the same statement for statement, so a frame's (e, a, v) summed over all cells at threshold q is
//                 what frame_change_kernel counts on that area at th.t[q].  Each live lane adds its cell's three integers into
//                 counts[((c0 + lane) * NT + q) * 3 ..] (cleared by the launcher ahead of the kernel); zeros are skipped as
//                 frame_change_kernel skips them, and integer sums do not depend on the order the blocks arrive in.
//   CELLS_MASKS   unsigned long long* masks, long slot0: the mask words a chunk leaves in LDS are also written to the caller's buffer, so
//                 that the counts of ANY rectangle of the region can be made later without the frames (frame_masks_replay_kernel below).
//                 Cell-major: slot f, threshold q, cell c, row k -> word ((f * NT + q) * cells + c) * FC_ROWS + k, which is msk[q][tl][k]
//                 of frame f: wave q copies its own slice, lane l of pass p writing word l % 8 of frame 8 p + l / 8 of the chunk, so one
//                 store instruction writes eight whole 64-byte lines and the LDS reads of a pass are 64 consecutive words.  Words of rows
//                 and columns beyond the interior are zero in LDS (tile_masks_multi) and are written as such.  A block writes only its own
//                 cell's words; the launcher has checked slot0 + n <= cap.  No atomics.  The store loop is kept rolled: unrolled, its
//                 eight addresses cost 127-129 VGPRs and the second block at NT = 5..7.
// LDS is the same for every kind: (FC_CHUNK + 1) * NT * FC_ROWS words, 4160 B at NT = 1 and 33280 B at NT = 8; no scratch.  VGPRs at NT = 1
// and NT = 8 (the compiler's resource usage for gfx950): 92 and 102 alone, 95 and 107 with counts, 99 and 107 with masks.  That is 5 waves
// per SIMD at NT <= 3 and 4 above for the first two, 4 at every NT with masks; a block is two waves per SIMD, so every kind holds two blocks
// on a CU, also at NT = 8 (65 KiB of its 160 KiB LDS).
enum { CELLS_ONLY, CELLS_COUNTS, CELLS_MASKS };

template <class A, class... R>
__device__ __forceinline__ A first_of(A a, R...) { return a; }
template <class A, class B>
__device__ __forceinline__ B second_of(A, B b) { return b; }

template <int NT, int OUT, class... X>
__global__ __launch_bounds__(FC_WAVES * 64) void frame_cells_multi_kernel(const uint8_t* __restrict__ src, int n, long pitch, long fstride,
                                                                          int x0, int ih, int iw, CellThresholds th, CellRule rule,
                                                                          unsigned long long* __restrict__ state, int reset, int flush,
                                                                          int* __restrict__ totals, X... x) {
    __shared__ unsigned long long msk[NT * FC_CHUNK * FC_ROWS];           // [NT][FC_CHUNK][FC_ROWS]
    __shared__ unsigned long long prv[NT * FC_ROWS];
    static_assert(FC_CHUNK == 64, "the frames of a chunk are the lanes of a wave");
    static_assert(NT >= 1 && NT <= FC_WAVES, "wave q owns threshold q");
    static_assert(sizeof...(X) == (OUT == CELLS_ONLY ? 0 : OUT == CELLS_COUNTS ? 1 : 2), "the pack is the kind's arguments");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int iy0 = blockIdx.y * FC_ROWS;
    const long cell = (long)blockIdx.y * gridDim.x + blockIdx.x, cells = (long)gridDim.y * gridDim.x;
    const TileLane t = tile_lane(blockIdx.x, iy0, ih, iw, x0);
    const bool mine = wave < NT;            // wave q owns threshold q
    unsigned long long* st = state + ((long)wave * cells + cell) * CELL_STATE_WORDS;
    int* tot = totals + ((long)wave * cells + cell) * 4;
    unsigned long long* mq = msk + wave * FC_CHUNK * FC_ROWS;
    unsigned long long* pq = prv + wave * FC_ROWS;
    if (mine && lane < FC_ROWS) pq[lane] = reset ? 0ull : st[lane];
    CellRuns cr = {0, 0, 0, 0, 0};
    if (mine && !reset) cr.load(st + FC_ROWS, tot);

    for (int c0 = 0; c0 < n; c0 += FC_CHUNK) {
        const int cn = min(FC_CHUNK, n - c0);
        tile_masks_multi<NT>(src + (long)iy0 * pitch, c0, cn, pitch, fstride, t, th, msk);
        __syncthreads();
        if (mine) {                                // lane = frame of the chunk
            if constexpr (OUT == CELLS_MASKS) {
                static_assert(FC_ROWS == 8, "a lane's word of a store pass is lane % 8 of frame lane / 8");
                // the chunk's words of threshold `wave`: frame c0 + tl < n of the call is slot slot0 + c0 + tl < cap
                const long slot_words = NT * cells * FC_ROWS;
                unsigned long long* out =
                    first_of(x...) + (second_of(x...) + c0 + (lane >> 3)) * slot_words + (wave * cells + cell) * FC_ROWS + (lane & 7);
#pragma unroll 1
                for (int i = lane; i < cn * FC_ROWS; i += 64, out += (FC_CHUNK / FC_ROWS) * slot_words) *out = mq[i];
            }
            const bool live = lane < cn;
            int e = 0, a = 0, v = 0, ep = 0;
            if (live) {
#pragma unroll
                for (int k = 0; k < FC_ROWS; ++k) {
                    const unsigned long long cur = mq[lane * FC_ROWS + k], pre = lane ? mq[(lane - 1) * FC_ROWS + k] : pq[k];
                    e += __popcll(cur);
                    a += __popcll(cur & ~pre);
                    v += __popcll(pre & ~cur);
                    ep += __popcll(pre);           // edges[t-1]
                }
                if constexpr (OUT == CELLS_COUNTS) {
                    // the whole area's counts of frame c0 + lane at threshold `wave`: c0 + lane < n and wave < NT, inside [n][NT][3]
                    int* o = first_of(x...) + ((long)(c0 + lane) * NT + wave) * 3;
                    if (e) atomicAdd(o, e);
                    if (a) atomicAdd(o + 1, a);
                    if (v) atomicAdd(o + 2, v);
                }
            }
            const long long uni = ep + a;          // |E' or E|
            const unsigned long long present = __ballot(live && e >= rule.min_edges);
            const unsigned long long ratio = __ballot(live && uni > 0 && (long long)(a + v) * rule.ratio_den >= (long long)rule.ratio_num * uni);
            for (int f = 0; f < cn; ++f) cr.step((present >> f) & 1, (ratio >> f) & 1, rule);
        }
        __syncthreads();
        if (mine && lane < FC_ROWS) pq[lane] = mq[(cn - 1) * FC_ROWS + lane];
        __syncthreads();
    }
    if (mine && lane < FC_ROWS) st[lane] = pq[lane];
    if (mine && lane == 0) cr.store(st + FC_ROWS, tot, flush, rule);
}

// Slice q of a vse_frame_cells_multi state -> a vse_frame_change state of the same area: a thread per interior row and word copies mask
// word iy % FC_ROWS of cell (iy / FC_ROWS, w).  cell_state points at slice q's first cell; words is the change state behind its header.
// Every word of the change state is written (ih * wpr of them; rows beyond the interior have no word there), then the flag.
__global__ __launch_bounds__(256) void frame_cells_export_kernel(const unsigned long long* __restrict__ cell_state, int ih, int wpr,
                                                                 unsigned long long* __restrict__ words, unsigned* flag) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (long)ih * wpr) {
        const int iy = (int)(i / wpr), w = (int)(i % wpr);
        const long cell = (long)(iy / FC_ROWS) * wpr + w;          // gx == wpr
        words[i] = cell_state[cell * CELL_STATE_WORDS + iy % FC_ROWS];
    }
    if (i == 0) *flag = 1u;
}

// ---- vse_frame_masks_replay -----------------------------------------------------------------------------------------------------
// The counts frame_change_kernel would write on a rectangle of the region, from the words frame_cells_multi_kernel kept (CELLS_MASKS): an edge pixel
// depends on its four neighbours and the threshold only, not on the area it is counted in, so interior pixel (iy, ix) of the rectangle
// [ry0, ry1) x [rx0, rx1) (region coordinates) is interior pixel (ry0 + iy, rx0 + ix) of the region.
struct ReplayRect {
    int ry0, rx0;       // the rectangle's first row and column in the region
    int ih, iw, wpr;    // its interior, and the 64-bit words of an interior row
};

// Word w of the rectangle's interior row iy in one slot's slice of threshold q (`slice` points at its first cell; gx cells per grid row):
// two neighbouring region words funnel-shifted by rx0 % 64, the bits at and beyond the interior width cleared.  The upper word is read
// only where it holds a column of the rectangle's interior, which is inside the region's, so no cell beside the rectangle is touched.
__device__ __forceinline__ unsigned long long replay_word(const unsigned long long* __restrict__ slice, int gx, const ReplayRect& r, int iy,
                                                          int w) {
    const int row = r.ry0 + iy, col = r.rx0 + 64 * w;          // region-interior row, and column of the word's bit 0
    const int cx = col >> 6, s = col & 63, left = r.iw - 64 * w;          // left >= 1: interior columns from bit 0 on
    const unsigned long long* p = slice + ((long)(row >> 3) * gx + cx) * FC_ROWS + (row & 7);
    unsigned long long v = p[0] >> s;
    if (s && 64 - s < left) v |= p[FC_ROWS] << (64 - s);
    return left >= 64 ? v : v & ((1ull << left) - 1);
}

// grid: x over the rectangle's ih * wpr words in blocks of 256, y over the frames f0 .. f1 - 1.  slot_words = nt * cells * FC_ROWS;
// masks points at slot 0's slice of threshold q.  The previous mask of slot f is slot f - 1, or empty for f == f0 with `reset`.  counts
// [f1 - f0, 3] were cleared by the launcher; each wave adds its sums, zeros skipped.  The blocks of the last frame also write its words
// as frame_change_kernel keeps them (words[iy * wpr + w], every one of them) and the flag.
__global__ __launch_bounds__(256) void frame_masks_replay_kernel(const unsigned long long* __restrict__ masks, long slot_words, int gx,
                                                                 ReplayRect r, int f0, int f1, int reset, int* __restrict__ counts,
                                                                 unsigned long long* __restrict__ words, unsigned* flag) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int f = f0 + (int)blockIdx.y;
    int e = 0, a = 0, v = 0;
    if (i < (long)r.ih * r.wpr) {
        const int iy = (int)(i / r.wpr), w = (int)(i % r.wpr);
        const unsigned long long cur = replay_word(masks + (long)f * slot_words, gx, r, iy, w);
        const unsigned long long pre = (reset && f == f0) ? 0ull : replay_word(masks + (long)(f - 1) * slot_words, gx, r, iy, w);
        e = __popcll(cur);
        a = __popcll(cur & ~pre);
        v = __popcll(pre & ~cur);
        if (f == f1 - 1) words[i] = cur;
    }
    if (i == 0 && f == f1 - 1) *flag = 1u;
#pragma unroll
    for (int d = 32; d; d >>= 1) {
        e += __shfl_down(e, d);
        a += __shfl_down(a, d);
        v += __shfl_down(v, d);
    }
    if ((threadIdx.x & 63) == 0) {
        int* o = counts + (long)(f - f0) * 3;
        if (e) atomicAdd(o, e);
        if (a) atomicAdd(o + 1, a);
        if (v) atomicAdd(o + 2, v);
    }
}

// ---- vse_frame_hold -------------------------------------------------------------------------------------------------------------
// H_u = the edge pixels of frame u whose run of consecutive edge frames is at least `hold` frames long.  Per pixel, along the frames t:
//   run[t]   = E[t] ? min(run[t-1] + 1, hold) : 0          S[t] = (run[t] == hold): a run of `hold` frames ends at t
//   cover[t] = S[t] ? hold : max(cover[t-1] - 1, 0)         cover[t] > 0: some S in t-hold+1 .. t
//   H[t-hold+1] = cover[t] > 0
// (u lies in a run of >= hold frames exactly when a run of hold frames ends somewhere in u .. u+hold-1.)  So the mask of a frame comes out
// hold - 1 steps late; a flush feeds hold - 1 frames without an edge, which cuts the runs off at the clip's end.  Steps before frame
// `hold` cannot set S, so the rows of the frames "before frame 1" are empty masks: they are computed like the others and not written.
//
// The tile's mask words meet in LDS exactly as above.  Then wave k walks interior row k of the tile along the frames with lane = column:
// two small counters per pixel in registers, the held pixels of a step gathered by a ballot into the word that replaces the mask word
// in LDS (the words of a chunk enter and leave the walk with lane = frame, one LDS access each way), and the per-frame counting is
// frame_change_kernel's on those words.  A pixel per lane keeps the walk at about ten instructions per frame on all eight waves;
// counters bit-sliced into 64-bit planes would need one lane per word and a dependent chain several times as long on a single wave,
// at the end of the block where nothing hides it.
// State: one uint16 per pixel of the tile words (64 per word, [interior row][word][lane]): run | cover << 6 | held << 12, `held` being
// the pixel's bit in the last mask that was counted.  Zero is the state before frame 1.
constexpr int HOLD_WORD_BYTES = 64 * 2;

// Where the edge words of a chunk's real steps come from is a policy of the body, which is otherwise one text for both kernels:
//   HoldFrames  the frames (tile_masks): frame_hold_kernel;
//   HoldSlots   the words vse_frame_cells_masks / vse_frame_cells_hold_masks kept (replay_word): frame_masks_replay_hold_kernel.
// fill(c0, real, msk) leaves msk[tl][k] = the edge word of the tile's interior row k at step c0 + tl for tl < real, zero for the rows
// beyond the area; `rows` are the tile's interior rows that lie in the area.
struct HoldFrames {
    const uint8_t* __restrict__ src;          // the tile's first halo row in frame 0
    long pitch, fstride;
    int thresh;
    TileLane t;
    __device__ __forceinline__ int rows() const { return t.rows; }
    __device__ __forceinline__ void fill(int c0, int real, unsigned long long (*msk)[FC_ROWS]) const {
        tile_masks(src, c0, real, pitch, fstride, t, thresh, msk);
    }
};

struct HoldSlots {
    const unsigned long long* __restrict__ slice;          // threshold q's first cell in the slot of step 0
    long slot_words;
    int gx;
    ReplayRect r;
    int iy0, w;                               // the tile's first interior row in the rectangle, and its word of a row
    __device__ __forceinline__ int rows() const { return min(FC_ROWS, r.ih - iy0); }
    // thread 8 tl + k fetches the word of step tl and row k: eight lanes read the one or two 64-byte lines of a slot's cell row group
    __device__ __forceinline__ void fill(int c0, int real, unsigned long long (*msk)[FC_ROWS]) const {
        static_assert(FC_WAVES * 64 == FC_CHUNK * FC_ROWS, "a thread per step and row of the chunk");
        const int tl = threadIdx.x / FC_ROWS, k = threadIdx.x % FC_ROWS;
        if (tl < real) msk[tl][k] = iy0 + k < r.ih ? replay_word(slice + (long)(c0 + tl) * slot_words, gx, r, iy0 + k, w) : 0ull;
    }
};

// block (w, iy0 / FC_ROWS) owns the tile's state words state[((iy0 + k) * wpr + w) * 64 ..] for all steps of the call
template <class SRC>
__device__ __forceinline__ void frame_hold_body(const SRC& source, int n, int steps, int iy0, int w, int wpr, int hold, int skip,
                                                unsigned short* __restrict__ state, int fresh, int* __restrict__ counts) {
    __shared__ unsigned long long msk[FC_CHUNK][FC_ROWS];
    __shared__ unsigned long long prv[FC_ROWS];
    static_assert(FC_WAVES == FC_ROWS, "wave k walks interior row k of the tile");
    static_assert(FC_CHUNK == 64, "the frames of a chunk are the lanes of a wave");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool mine = wave < source.rows();    // wave-uniform; the words of the other rows stay zero
    unsigned short* st = state + ((long)(iy0 + wave) * wpr + w) * 64 + lane;
    int run = 0, cover = 0;
    bool held = false;
    if (mine && !fresh) {
        const unsigned s = *st;
        run = s & 63;
        cover = (s >> 6) & 63;
        held = (s >> 12) & 1;
    }
    {
        const unsigned long long b = __ballot(held);
        if (lane == 0) prv[wave] = b;
    }

    for (int c0 = 0; c0 < steps; c0 += FC_CHUNK) {
        const int cn = min(FC_CHUNK, steps - c0);
        const int real = max(0, min(cn, n - c0));          // the steps after frame n are the flush: no edge anywhere
        source.fill(c0, real, msk);
        for (int i = real * FC_ROWS + threadIdx.x; i < cn * FC_ROWS; i += FC_WAVES * 64) msk[i / FC_ROWS][i % FC_ROWS] = 0ull;
        __syncthreads();
        if (mine) {
            // lane = frame of the chunk for the words going in and out, lane = column for the walk: the walk itself stays out of LDS
            const unsigned long long col = lane < cn ? msk[lane][wave] : 0ull;
            const int lo = (int)(unsigned)col, hi = (int)(unsigned)(col >> 32);
            unsigned long long out = 0ull;
            for (int tl = 0; tl < cn; ++tl) {
                const bool edge = edge_bit(lo, hi, tl, lane);
                run = edge ? min(run + 1, hold) : 0;
                cover = run == hold ? hold : max(cover - 1, 0);
                held = cover > 0;
                const unsigned long long b = __ballot(held);
                if (lane == tl) out = b;                   // mask of frame (this step) - hold + 1
            }
            if (lane < cn) msk[lane][wave] = out;
        }
        __syncthreads();
        if ((int)threadIdx.x < cn) {
            const int tl = threadIdx.x, row = c0 + tl - skip;
            if (row >= 0) {
                int e = 0, a = 0, v = 0;
#pragma unroll
                for (int k = 0; k < FC_ROWS; ++k) {
                    const unsigned long long cur = msk[tl][k], pre = tl ? msk[tl - 1][k] : prv[k];
                    e += __popcll(cur);
                    a += __popcll(cur & ~pre);
                    v += __popcll(pre & ~cur);
                }
                // integer sums: the totals do not depend on the order the blocks arrive in
                int* o = counts + (long)row * 3;
                if (e) atomicAdd(o, e);
                if (a) atomicAdd(o + 1, a);
                if (v) atomicAdd(o + 2, v);
            }
        }
        __syncthreads();
        if (threadIdx.x < FC_ROWS) prv[threadIdx.x] = msk[cn - 1][threadIdx.x];
        __syncthreads();
    }
    if (mine) *st = (unsigned short)(run | (cover << 6) | ((int)held << 12));
}

__global__ __launch_bounds__(FC_WAVES * 64) void frame_hold_kernel(const uint8_t* __restrict__ src, int n, int steps, long pitch, long fstride,
                                                                   int x0, int ih, int iw, int wpr, int thresh, int hold, int skip,
                                                                   unsigned short* __restrict__ state, int fresh, int* __restrict__ counts) {
    const int w = blockIdx.x, iy0 = blockIdx.y * FC_ROWS;
    const HoldFrames source = {src + (long)iy0 * pitch, pitch, fstride, thresh, tile_lane(w, iy0, ih, iw, x0)};
    frame_hold_body(source, n, steps, iy0, w, wpr, hold, skip, state, fresh, counts);
}

// ---- vse_frame_masks_replay_hold --------------------------------------------------------------------------------------------------
// frame_hold_kernel on a rectangle of the region, its edge words taken from the kept masks instead of the frames (an edge pixel depends on
// its four neighbours and the threshold only, not on the area it is counted in: frame_masks_replay_kernel above).  Grid and block are
// frame_hold_kernel's on the rectangle: block (w, j) owns word w of the interior rows 8 j .. 8 j + 7 of the rectangle, and the walk, the
// ballots, the counting and the state are frame_hold_body's, so the state this leaves is vse_frame_hold's of that rectangle.  `slice`
// points at threshold q's first cell in the slot of step 0; the n real steps read the slots of steps 0 .. n - 1, the flush steps none.
__global__ __launch_bounds__(FC_WAVES * 64) void frame_masks_replay_hold_kernel(const unsigned long long* __restrict__ slice, long slot_words,
                                                                                int gx, ReplayRect r, int n, int steps, int hold, int skip,
                                                                                unsigned short* __restrict__ state, int fresh,
                                                                                int* __restrict__ counts) {
    const int w = blockIdx.x, iy0 = blockIdx.y * FC_ROWS;
    const HoldSlots source = {slice, slot_words, gx, r, iy0, w};
    frame_hold_body(source, n, steps, iy0, w, r.wpr, hold, skip, state, fresh, counts);
}

// ---- vse_frame_cells_hold --------------------------------------------------------------------------------------------------------
// The locator's cells (frame_cells_multi_kernel) on the held masks of frame_hold_kernel, for moving backgrounds: a block is a cell for all
// frames of the call and for NT thresholds.  Three stages per chunk of steps, all pieces of the kernels above:
//   tile_masks_multi  a frame's bytes, lumas and gradients once, the edge words of the NT thresholds side by side in LDS;
//   the walk          frame_hold_kernel's: wave k walks interior row k with lane = column, here for the NT thresholds in one loop (NT
//                     independent chains per step); the held words replace the edge words in LDS;
//   the tail          frame_cells_multi_kernel's: wave q counts threshold q's words with lane = step and steps its CellRuns.
// The held word of a frame comes out hold - 1 steps late, so the automaton is stepped only for the steps that belong to a frame
// (row >= 0, frame_hold_kernel's `skip`); a flush is hold - 1 steps without an edge and then closes the runs.  Runs with steps == 0 too
// (fresh and flush only).
// Between the stages a lane keeps one register per threshold, run | cover << 6: 8 registers at NT = 8 under tile_masks_multi's 83.
// State: pix[((q * ih + interior row) * wpr + word) * 64 + lane] = frame_hold_kernel's uint16 of threshold q (held: the pixel's bit in the
// last word that was counted), and open_runs[q * cells + cell] = the length of the cell's open run.  Totals as frame_cells_multi_kernel.
// cell_counts (nullable): [NT][count_rows][cells][3] = e, a, v of row `row` of this call, each written by the one block that owns it.
// OUT and the trailing pack x are frame_cells_multi_kernel's: CELLS_ONLY (vse_frame_cells_hold; no argument, and the code this kernel
// compiled to before it had the parameter: the same registers, LDS and scratch at every NT) or CELLS_MASKS (vse_frame_cells_hold_masks;
// unsigned long long* masks, long slot0): the EDGE words a chunk's real steps leave in LDS, before the walk replaces them by held words,
// go to the caller's buffer in that kernel's layout and by its store loop, so a call writes bit for bit what frame_cells_multi_kernel<NT,
// CELLS_MASKS> writes for the same frames.  The loop has wave q reading all eight rows of threshold q while the walk has wave k
// overwriting row k of every threshold, so this kind has one more barrier per chunk, between the stores and the walk.  Only the `real`
// steps are stored (step c0 + tl < n of the call is slot slot0 + c0 + tl < cap, checked by the launcher's caller); a flush's steps have
// no slot.  The other form, each walking wave storing its own row's words from the registers it holds them in (lane = step, 8-byte stores
// a slot apart, no barrier), was built and measured: 1.000-1.002x the kernel without masks at NT = 1 against 1.007x for this form, but
// 1.032-1.034x against 1.018-1.021x at NT = 8 (EXPERIMENTS.md, "Area found in the hold selector's pass").  VGPRs with masks at NT = 1 .. 8: 107 109 109 112 113 113 115 121 against 101 103 103 107 108 109 110 116 without; LDS as
// without; no scratch; four waves per SIMD either way.
template <int NT, int OUT, class... X>
__global__ __launch_bounds__(FC_WAVES * 64) void frame_cells_hold_kernel(const uint8_t* __restrict__ src, int n, int steps, long pitch,
                                                                         long fstride, int x0, int ih, int iw, CellThresholds th, CellRule rule,
                                                                         int hold, int skip, unsigned short* __restrict__ pix,
                                                                         int* __restrict__ open_runs, int fresh, int flush,
                                                                         int* __restrict__ totals, int* __restrict__ cell_counts, int count_rows,
                                                                         X... x) {
    __shared__ unsigned long long msk[NT * FC_CHUNK * FC_ROWS];           // [NT][FC_CHUNK][FC_ROWS]
    __shared__ unsigned long long prv[NT * FC_ROWS];
    static_assert(FC_WAVES == FC_ROWS, "wave k walks interior row k of the tile");
    static_assert(FC_CHUNK == 64, "the steps of a chunk are the lanes of a wave");
    static_assert(NT >= 1 && NT <= FC_WAVES, "wave q owns threshold q");
    static_assert(OUT == CELLS_ONLY || OUT == CELLS_MASKS, "the held cells keep masks or nothing");
    static_assert(sizeof...(X) == (OUT == CELLS_ONLY ? 0 : 2), "the pack is the kind's arguments");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int iy0 = blockIdx.y * FC_ROWS, wpr = gridDim.x;
    const long cell = (long)blockIdx.y * gridDim.x + blockIdx.x, cells = (long)gridDim.y * gridDim.x;
    const TileLane t = tile_lane(blockIdx.x, iy0, ih, iw, x0);
    const bool walks = wave < t.rows;          // wave-uniform; the words of the other rows stay zero
    const bool mine = wave < NT;               // wave q owns threshold q
    unsigned short* ps = pix + ((long)(iy0 + wave) * wpr + blockIdx.x) * 64 + lane;
    const long pslice = (long)ih * wpr * 64;
    int* tot = totals + ((long)wave * cells + cell) * 4;
    unsigned long long* mq = msk + wave * FC_CHUNK * FC_ROWS;
    unsigned long long* pq = prv + wave * FC_ROWS;
    int rc[NT];                                // run | cover << 6
#pragma unroll
    for (int q = 0; q < NT; ++q) {
        const unsigned s = (walks && !fresh) ? ps[q * pslice] : 0u;
        const unsigned long long b = __ballot((s >> 12) & 1u);
        if (lane == 0) prv[q * FC_ROWS + wave] = b;
        rc[q] = (int)(s & 0xfffu);
    }
    CellRuns cr = {0, 0, 0, 0, 0};
    if (mine && !fresh) cr.load(open_runs + ((long)wave * cells + cell), tot);

    for (int c0 = 0; c0 < steps; c0 += FC_CHUNK) {
        const int cn = min(FC_CHUNK, steps - c0);
        const int real = max(0, min(cn, n - c0));          // the steps after frame n are the flush: no edge anywhere
        tile_masks_multi<NT>(src + (long)iy0 * pitch, c0, real, pitch, fstride, t, th, msk);
        zero_steps<NT>(msk, real, cn);
        __syncthreads();
        if constexpr (OUT == CELLS_MASKS) {
            // frame_cells_multi_kernel's store loop on the EDGE words of the chunk's real steps, before the walk replaces them by held words:
            // wave q reads all eight rows of threshold q, which eight walking waves are about to overwrite, hence the barrier behind it
            static_assert(FC_ROWS == 8, "a lane's word of a store pass is lane % 8 of frame lane / 8");
            if (mine) {
                const long slot_words = NT * cells * FC_ROWS;
                unsigned long long* out =
                    first_of(x...) + (second_of(x...) + c0 + (lane >> 3)) * slot_words + (wave * cells + cell) * FC_ROWS + (lane & 7);
#pragma unroll 1
                for (int i = lane; i < real * FC_ROWS; i += 64, out += (FC_CHUNK / FC_ROWS) * slot_words) *out = mq[i];
            }
            __syncthreads();
        }
        if (walks) {
            // lane = step of the chunk for the words going in and out, lane = column for the walk: the walk itself stays out of LDS
            int lo[NT], hi[NT], run[NT], cover[NT];
            unsigned long long out[NT];
#pragma unroll
            for (int q = 0; q < NT; ++q) {
                const unsigned long long col = lane < cn ? msk[(q * FC_CHUNK + lane) * FC_ROWS + wave] : 0ull;
                lo[q] = (int)(unsigned)col;
                hi[q] = (int)(unsigned)(col >> 32);
                out[q] = 0ull;
                run[q] = rc[q] & 63;
                cover[q] = rc[q] >> 6;
            }
            for (int tl = 0; tl < cn; ++tl) {
#pragma unroll
                for (int q = 0; q < NT; ++q) {
                    const bool edge = edge_bit(lo[q], hi[q], tl, lane);
                    run[q] = edge ? min(run[q] + 1, hold) : 0;
                    cover[q] = run[q] == hold ? hold : max(cover[q] - 1, 0);
                    const unsigned long long b = __ballot(cover[q] > 0);
                    if (lane == tl) out[q] = b;            // held word of frame (this step) - hold + 1
                }
            }
#pragma unroll
            for (int q = 0; q < NT; ++q) {
                if (lane < cn) msk[(q * FC_CHUNK + lane) * FC_ROWS + wave] = out[q];
                rc[q] = run[q] | (cover[q] << 6);
            }
        }
        __syncthreads();
        if (mine) {                                // lane = step of the chunk
            const int row = c0 + lane - skip;      // the row of this call that the step completes; < 0: a step before frame 1
            const bool live = lane < cn && row >= 0;
            int e = 0, a = 0, v = 0, ep = 0;
            if (live) {
#pragma unroll
                for (int k = 0; k < FC_ROWS; ++k) {
                    const unsigned long long cur = mq[lane * FC_ROWS + k], pre = lane ? mq[(lane - 1) * FC_ROWS + k] : pq[k];
                    e += __popcll(cur);
                    a += __popcll(cur & ~pre);
                    v += __popcll(pre & ~cur);
                    ep += __popcll(pre);           // held edges of the frame before
                }
                if (cell_counts) {
                    int* o = cell_counts + (((long)wave * count_rows + row) * cells + cell) * 3;
                    o[0] = e;
                    o[1] = a;
                    o[2] = v;
                }
            }
            const long long uni = ep + a;          // |H' or H|
            const unsigned long long present = __ballot(live && e >= rule.min_edges);
            const unsigned long long ratio = __ballot(live && uni > 0 && (long long)(a + v) * rule.ratio_den >= (long long)rule.ratio_num * uni);
            for (int f = max(0, skip - c0); f < cn; ++f) cr.step((present >> f) & 1, (ratio >> f) & 1, rule);
        }
        __syncthreads();
        if (mine && lane < FC_ROWS) pq[lane] = mq[(cn - 1) * FC_ROWS + lane];
        __syncthreads();
    }
    if (walks) {
#pragma unroll
        for (int q = 0; q < NT; ++q) ps[q * pslice] = (unsigned short)(rc[q] | ((rc[q] >> 6) ? 1 << 12 : 0));
    }
    if (mine && lane == 0) cr.store(open_runs + ((long)wave * cells + cell), tot, flush, rule);
}

// ---- vse_frame_focus ------------------------------------------------------------------------------------------------------------
// Per frame, how sharp the edges are that already stood one frame earlier: K = E & E', kept = |K|, focus = the sum over K of the gradient
// g = max(|Y[y][x+1] - Y[y][x-1]|, |Y[y+1][x] - Y[y-1][x]|), the value that E compares with the threshold.  The tile is tile_lane's and
// the loads, lumas and gradients are tile_masks', statement for statement; what differs is who owns which frame.  A lane needs its own
// pixel's bit of the frame before, not the packed word, so a wave takes CONSECUTIVE frames (wave q the frames q * per .. q * per + per - 1,
// per = ceil(n / FC_WAVES)) and carries its eight rows' bits of the last frame in one register: no ballot, no LDS and no barrier between
// the frames of a wave, and g is used where it is computed.  Only the first frame of a wave meets a mask that another wave (or the call
// before) made: its bits and its eight gradients, one byte each in two registers, wait for the one barrier of the kernel, behind which the
// last frame of every wave stands in LDS as packed words, the form the state keeps.  There is no chunk loop: n frames are n / 8 per wave.
// The state is frame_change_kernel's, words and flag, read at the start and written at the end by the block that owns the tile.
// A lane's sums of one frame travel as one integer, focus (<= 8 * 255) | kept (<= 8) << 20; summed over the wave focus < 2^17, kept <= 512.
constexpr int FOCUS_KEPT_SHIFT = 20;

// g[k] = the gradient of the lane's pixel in interior row k of the tile, f pointing at the tile's first halo row in one frame
// -> bit k: that pixel is an edge pixel.
__device__ __forceinline__ unsigned tile_gradients(const uint8_t* __restrict__ f, long pitch, const TileLane& t, int thresh, int (&g)[FC_ROWS]) {
    const int lane = threadIdx.x & 63;
    const int rows = t.rows;
    int yc[FC_ROWS + 2], ye[FC_ROWS];
#pragma unroll
    for (int k = 0; k < FC_ROWS + 2; ++k) yc[k] = (k < rows + 2 && t.own) ? luma(f + (long)k * pitch + t.x * 3) : 0;
#pragma unroll
    for (int k = 0; k < FC_ROWS; ++k) ye[k] = (k < rows && t.extra) ? luma(f + (long)(k + 1) * pitch + t.xe * 3) : 0;
    unsigned bits = 0;
#pragma unroll
    for (int k = 0; k < FC_ROWS; ++k) {
        g[k] = 0;
        if (k < rows) {                // block-uniform
            const int l = __shfl_up(yc[k + 1], 1), r = __shfl_down(yc[k + 1], 1);
            const int left = lane == 0 ? ye[k] : l, right = lane == 63 ? ye[k] : r;
            g[k] = max(abs(right - left), abs(yc[k + 2] - yc[k]));
            if (t.inner && g[k] >= thresh) bits |= 1u << k;
        }
    }
    return bits;
}

// The wave's sums over the pixels in `kept` (bit k: the lane's pixel of row k) -> row `out` of the call's output, one atomic each.
__device__ __forceinline__ void focus_add(unsigned kept, const int (&g)[FC_ROWS], int* out) {
    int acc = __popc(kept) << FOCUS_KEPT_SHIFT;
#pragma unroll
    for (int k = 0; k < FC_ROWS; ++k) acc += (kept >> k) & 1u ? g[k] : 0;
#pragma unroll
    for (int o = 32; o; o >>= 1) acc += __shfl_xor(acc, o);
    // integer sums: the totals do not depend on the order the blocks arrive in
    if ((threadIdx.x & 63) == 0 && acc) {
        atomicAdd(out, acc >> FOCUS_KEPT_SHIFT);
        atomicAdd(out + 1, acc & ((1 << FOCUS_KEPT_SHIFT) - 1));
    }
}

// src, words and flag as frame_change_kernel's; focus [n][2] = kept, focus, cleared before the launch.
__global__ __launch_bounds__(FC_WAVES * 64) void frame_focus_kernel(const uint8_t* __restrict__ src, int n, long pitch, long fstride, int x0,
                                                                    int ih, int iw, int wpr, int thresh, unsigned long long* __restrict__ words,
                                                                    unsigned* flag, int reset, int* __restrict__ focus) {
    __shared__ unsigned long long last[FC_WAVES][FC_ROWS];     // packed mask of the last frame of each wave
    __shared__ unsigned long long prv[FC_ROWS];                // ... and of the last frame of the call before
    static_assert(FC_ROWS == 8, "a frame's gradients are eight bytes in two registers");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int w = blockIdx.x, iy0 = blockIdx.y * FC_ROWS;
    const TileLane t = tile_lane(w, iy0, ih, iw, x0);
    unsigned long long* st = words + (long)iy0 * wpr + w;
    // (the flag: see frame_change_kernel)
    const bool use_prev = !reset && *(volatile unsigned*)flag != 0;
    if (threadIdx.x < FC_ROWS) prv[threadIdx.x] = (use_prev && (int)threadIdx.x < t.rows) ? st[(long)threadIdx.x * wpr] : 0ull;
    const int per = (n + FC_WAVES - 1) / FC_WAVES;
    const int f0 = wave * per, f1 = min(n, f0 + per);          // this wave's frames; a wave that has some follows one that has some
    unsigned first = 0, g_lo = 0, g_hi = 0;                    // the wave's first frame: its bits, and its gradients of rows 0..3 and 4..7
    if (f0 < f1) {
        const uint8_t* f = src + (long)f0 * fstride + (long)iy0 * pitch;
        int g[FC_ROWS];
        first = tile_gradients(f, pitch, t, thresh, g);
        g_lo = (unsigned)g[0] | (unsigned)g[1] << 8 | (unsigned)g[2] << 16 | (unsigned)g[3] << 24;
        g_hi = (unsigned)g[4] | (unsigned)g[5] << 8 | (unsigned)g[6] << 16 | (unsigned)g[7] << 24;
        unsigned pre = first;
        for (int fr = f0 + 1; fr < f1; ++fr) {
            f += fstride;
            const unsigned cur = tile_gradients(f, pitch, t, thresh, g);
            focus_add(cur & pre, g, focus + (long)fr * 2);
            pre = cur;
        }
#pragma unroll
        for (int k = 0; k < FC_ROWS; ++k) {                    // bits of rows outside the area are zero
            const unsigned long long b = __ballot((pre >> k) & 1u);
            if (lane == 0) last[wave][k] = b;
        }
    }
    __syncthreads();
    if (f0 < f1) {
        unsigned pre = 0;
        int g[FC_ROWS];
#pragma unroll
        for (int k = 0; k < FC_ROWS; ++k) {
            const unsigned long long word = wave ? last[wave - 1][k] : prv[k];
            pre |= (unsigned)((word >> lane) & 1ull) << k;
            g[k] = (int)(((k < 4 ? g_lo : g_hi) >> (8 * (k & 3))) & 255u);
        }
        focus_add(first & pre, g, focus + (long)f0 * 2);
    }
    if (wave == (n - 1) / per && lane < t.rows) st[(long)lane * wpr] = last[wave][lane];      // the wave that had the call's last frame
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

// Called by vse_frame_focus (vse_runtime.hip) after it has checked the geometry (n >= 1).
int vse_frame_focus_launch(const void* d_bgr, int n, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0, int x1, int edge_thresh,
                           void* d_state, int reset, int32_t* d_focus, void* stream) {
    const int ih = y1 - y0 - 2, iw = x1 - x0 - 2, wpr = (iw + 63) / 64;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(d_focus, 0, (size_t)n * 2 * sizeof(int32_t), st) != hipSuccess) return VSE_E_HIP;
    unsigned* flag = reinterpret_cast<unsigned*>(d_state);
    unsigned long long* words = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(d_state) + 16);
    const uint8_t* src = reinterpret_cast<const uint8_t*>(d_bgr) + (long)y0 * pitch;
    hipLaunchKernelGGL(frame_focus_kernel, dim3(wpr, (ih + FC_ROWS - 1) / FC_ROWS), dim3(FC_WAVES * 64), 0, st, src, n, (long)pitch,
                       (long)frame_stride, x0, ih, iw, wpr, edge_thresh, words, flag, reset, reinterpret_cast<int*>(d_focus));
    return hipGetLastError() == hipSuccess ? VSE_OK : VSE_E_HIP;
}

int vse_frame_cells_state_words() { return CELL_STATE_WORDS; }

// Called by vse_frame_cells (vse_runtime.hip) after it has checked the arguments.
int vse_frame_cells_launch(const void* d_bgr, int n, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0, int x1, int edge_thresh,
                           const CellRule& rule, void* d_state, int reset, int flush, int32_t* d_totals, int32_t* d_cell_counts,
                           void* stream) {
    const int ih = y1 - y0 - 2, iw = x1 - x0 - 2;
    const uint8_t* src = reinterpret_cast<const uint8_t*>(d_bgr) + (long)y0 * pitch;
    hipLaunchKernelGGL(frame_cells_kernel, dim3((iw + 63) / 64, (ih + FC_ROWS - 1) / FC_ROWS), dim3(FC_WAVES * 64), 0,
                       reinterpret_cast<hipStream_t>(stream), src, n, (long)pitch, (long)frame_stride, x0, ih, iw, edge_thresh, rule,
                       reinterpret_cast<unsigned long long*>(d_state), reset, flush, reinterpret_cast<int*>(d_totals),
                       reinterpret_cast<int*>(d_cell_counts));
    return hipGetLastError() == hipSuccess ? VSE_OK : VSE_E_HIP;
}

int vse_frame_cells_multi_max() { return FC_WAVES; }

namespace {

// What the launchers of the kernels that take several thresholds share: the region's interior, its first row in frame 0, the thresholds
// as the kernels take them, and a block per cell.
struct CellsLaunch {
    int ih, iw;
    const uint8_t* src;
    CellThresholds th;
    dim3 grid, block;
    hipStream_t st;
    CellsLaunch(const void* d_bgr, int64_t pitch, int y0, int y1, int x0, int x1, const int* thresholds, int nt, void* stream)
        : ih(y1 - y0 - 2), iw(x1 - x0 - 2), src(reinterpret_cast<const uint8_t*>(d_bgr) + (long)y0 * pitch), th{},
          grid((iw + 63) / 64, (ih + FC_ROWS - 1) / FC_ROWS), block(FC_WAVES * 64), st(reinterpret_cast<hipStream_t>(stream)) {
        for (int q = 0; q < nt; ++q) th.t[q] = thresholds[q];          // the caller has checked nt <= FC_WAVES
    }
};

// launch(std::integral_constant<int, NT>) for NT == nt, which picks a kernel's instantiation for that many thresholds
template <class F>
int launch_for_nt(int nt, F launch) {
    static_assert(FC_WAVES == 8, "one instantiation per number of thresholds");
    switch (nt) {
        case 1: launch(std::integral_constant<int, 1>()); break;
        case 2: launch(std::integral_constant<int, 2>()); break;
        case 3: launch(std::integral_constant<int, 3>()); break;
        case 4: launch(std::integral_constant<int, 4>()); break;
        case 5: launch(std::integral_constant<int, 5>()); break;
        case 6: launch(std::integral_constant<int, 6>()); break;
        case 7: launch(std::integral_constant<int, 7>()); break;
        case 8: launch(std::integral_constant<int, 8>()); break;
        default: return VSE_E_INVAL;
    }
    return hipGetLastError() == hipSuccess ? VSE_OK : VSE_E_HIP;
}

// frame_cells_multi_kernel<nt, OUT, X...> with the kind's arguments x; X is given explicitly, so that the pointers keep their __restrict__
template <int OUT, class... X>
int cells_multi_launch(const CellsLaunch& l, int n, int64_t pitch, int64_t frame_stride, int x0, int nt, const CellRule& rule, void* d_state,
                       int reset, int flush, int32_t* d_totals, X... x) {
    return launch_for_nt(nt, [&](auto nt_c) {
        hipLaunchKernelGGL((frame_cells_multi_kernel<decltype(nt_c)::value, OUT, X...>), l.grid, l.block, 0, l.st, l.src, n, (long)pitch,
                           (long)frame_stride, x0, l.ih, l.iw, l.th, rule, reinterpret_cast<unsigned long long*>(d_state), reset, flush,
                           reinterpret_cast<int*>(d_totals), x...);
    });
}

}  // namespace

// Called by vse_frame_cells_multi (vse_runtime.hip) after it has checked the arguments (1 <= nt <= vse_frame_cells_multi_max()).
int vse_frame_cells_multi_launch(const void* d_bgr, int n, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0, int x1,
                                 const int* thresholds, int nt, const CellRule& rule, void* d_state, int reset, int flush,
                                 int32_t* d_totals, void* stream) {
    const CellsLaunch l(d_bgr, pitch, y0, y1, x0, x1, thresholds, nt, stream);
    return cells_multi_launch<CELLS_ONLY>(l, n, pitch, frame_stride, x0, nt, rule, d_state, reset, flush, d_totals);
}

// Called by vse_frame_cells_counts (vse_runtime.hip) after it has checked the arguments as vse_frame_cells_multi does.  d_counts is
// cleared on the stream ahead of the kernel, which adds into it.
int vse_frame_cells_counts_launch(const void* d_bgr, int n, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0, int x1,
                                  const int* thresholds, int nt, const CellRule& rule, void* d_state, int reset, int flush,
                                  int32_t* d_totals, int32_t* d_counts, void* stream) {
    const CellsLaunch l(d_bgr, pitch, y0, y1, x0, x1, thresholds, nt, stream);
    if (nt < 1 || nt > FC_WAVES) return VSE_E_INVAL;
    if (n > 0 && hipMemsetAsync(d_counts, 0, (size_t)n * nt * 3 * sizeof(int32_t), l.st) != hipSuccess) return VSE_E_HIP;
    return cells_multi_launch<CELLS_COUNTS, int* __restrict__>(l, n, pitch, frame_stride, x0, nt, rule, d_state, reset, flush, d_totals,
                                                               reinterpret_cast<int*>(d_counts));
}

// Called by vse_frame_cells_masks (vse_runtime.hip) after it has checked the arguments as vse_frame_cells_multi does and 0 <= slot0,
// slot0 + n <= cap of d_masks.
int vse_frame_cells_masks_launch(const void* d_bgr, int n, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0, int x1,
                                 const int* thresholds, int nt, const CellRule& rule, void* d_state, int reset, int flush,
                                 int32_t* d_totals, void* d_masks, int slot0, void* stream) {
    const CellsLaunch l(d_bgr, pitch, y0, y1, x0, x1, thresholds, nt, stream);
    return cells_multi_launch<CELLS_MASKS, unsigned long long* __restrict__, long>(
        l, n, pitch, frame_stride, x0, nt, rule, d_state, reset, flush, d_totals, reinterpret_cast<unsigned long long*>(d_masks), (long)slot0);
}

// Called by vse_frame_cells_export_state (vse_runtime.hip) after it has checked the area and 0 <= q < nt <= vse_frame_cells_multi_max().
int vse_frame_cells_export_launch(const void* d_cells_state, int area_h, int area_w, int q, void* d_change_state, void* stream) {
    const int ih = area_h - 2, iw = area_w - 2, wpr = (iw + 63) / 64;
    const long cells = (long)((ih + FC_ROWS - 1) / FC_ROWS) * wpr, nwords = (long)ih * wpr;
    const unsigned long long* slice = reinterpret_cast<const unsigned long long*>(d_cells_state) + (long)q * cells * CELL_STATE_WORDS;
    unsigned* flag = reinterpret_cast<unsigned*>(d_change_state);
    unsigned long long* words = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(d_change_state) + 16);
    hipLaunchKernelGGL(frame_cells_export_kernel, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                       slice, ih, wpr, words, flag);
    return hipGetLastError() == hipSuccess ? VSE_OK : VSE_E_HIP;
}

// Called by vse_frame_masks_replay (vse_runtime.hip) after it has checked the region, 0 <= q < nt <= vse_frame_cells_multi_max(), the
// slots 0 <= f0 < f1 <= cap (f0 >= 1 without reset) and the rectangle, at least 3 x 3 and inside the region.  d_counts is cleared on
// the stream ahead of the kernel, which adds into it.
int vse_frame_masks_replay_launch(const void* d_masks, int area_h, int area_w, int nt, int q, int f0, int f1, int ry0, int ry1, int rx0,
                                  int rx1, int reset, int32_t* d_counts, void* d_change_state, void* stream) {
    const int gy = (area_h - 2 + FC_ROWS - 1) / FC_ROWS, gx = (area_w - 2 + 63) / 64;
    const long cells = (long)gy * gx;
    ReplayRect r;
    r.ry0 = ry0, r.rx0 = rx0, r.ih = ry1 - ry0 - 2, r.iw = rx1 - rx0 - 2, r.wpr = (r.iw + 63) / 64;
    const long nwords = (long)r.ih * r.wpr;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const unsigned long long* slice = reinterpret_cast<const unsigned long long*>(d_masks) + (long)q * cells * FC_ROWS;
    unsigned* flag = reinterpret_cast<unsigned*>(d_change_state);
    unsigned long long* words = reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(d_change_state) + 16);
    if (hipMemsetAsync(d_counts, 0, (size_t)(f1 - f0) * 3 * sizeof(int32_t), st) != hipSuccess) return VSE_E_HIP;
    // grid.y holds at most 65535 frames: a longer window goes in pieces, each continuing from the slot before it
    for (int g0 = f0; g0 < f1; g0 += 65535) {
        const int g1 = min(f1, g0 + 65535);
        hipLaunchKernelGGL(frame_masks_replay_kernel, dim3((unsigned)((nwords + 255) / 256), (unsigned)(g1 - g0)), dim3(256), 0, st, slice,
                           (long)nt * cells * FC_ROWS, gx, r, g0, g1, reset && g0 == f0, reinterpret_cast<int*>(d_counts) + (long)(g0 - f0) * 3,
                           words, flag);
    }
    return hipGetLastError() == hipSuccess ? VSE_OK : VSE_E_HIP;
}

size_t vse_frame_hold_word_bytes() { return HOLD_WORD_BYTES; }

// Called by vse_frame_hold (vse_runtime.hip) after it has checked the arguments; steps = n (+ hold - 1 with a flush) > 0 and
// skip = the steps whose frame lies before frame 1.
int vse_frame_hold_launch(const void* d_bgr, int n, int steps, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0, int x1,
                          int edge_thresh, int hold, int skip, void* d_state, int fresh, int32_t* d_counts, void* stream) {
    const int ih = y1 - y0 - 2, iw = x1 - x0 - 2, wpr = (iw + 63) / 64;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (steps > skip && hipMemsetAsync(d_counts, 0, (size_t)(steps - skip) * 3 * sizeof(int32_t), st) != hipSuccess) return VSE_E_HIP;
    const uint8_t* src = reinterpret_cast<const uint8_t*>(d_bgr) + (long)y0 * pitch;
    hipLaunchKernelGGL(frame_hold_kernel, dim3(wpr, (ih + FC_ROWS - 1) / FC_ROWS), dim3(FC_WAVES * 64), 0, st, src, n, steps, (long)pitch,
                       (long)frame_stride, x0, ih, iw, wpr, edge_thresh, hold, skip, reinterpret_cast<unsigned short*>(d_state), fresh,
                       reinterpret_cast<int*>(d_counts));
    return hipGetLastError() == hipSuccess ? VSE_OK : VSE_E_HIP;
}

// State of vse_frame_cells_hold for a region with an interior of ih x iw pixels: nt slices of frame_hold_kernel's pixel state, then the
// open runs, int32 [nt][cells], padded to 8 bytes.
static size_t cells_hold_pixel_bytes(int ih, int iw, int nt) { return (size_t)nt * ih * ((iw + 63) / 64) * HOLD_WORD_BYTES; }

size_t vse_frame_cells_hold_bytes(int ih, int iw, int nt) {
    const size_t cells = (size_t)((ih + FC_ROWS - 1) / FC_ROWS) * ((iw + 63) / 64);
    return cells_hold_pixel_bytes(ih, iw, nt) + ((nt * cells * sizeof(int32_t) + 7) & ~(size_t)7);
}

// frame_cells_hold_kernel<nt, OUT, X...> with the kind's arguments x (X given explicitly, as for cells_multi_launch)
template <int OUT, class... X>
static int cells_hold_launch(const CellsLaunch& l, int n, int steps, int64_t pitch, int64_t frame_stride, int x0, int nt, int hold, int skip,
                             const CellRule& rule, void* d_state, int fresh, int flush, int32_t* d_totals, int32_t* d_cell_counts,
                             int count_rows, X... x) {
    unsigned short* pix = reinterpret_cast<unsigned short*>(d_state);
    int* open_runs = reinterpret_cast<int*>(reinterpret_cast<char*>(d_state) + cells_hold_pixel_bytes(l.ih, l.iw, nt));
    return launch_for_nt(nt, [&](auto nt_c) {
        hipLaunchKernelGGL((frame_cells_hold_kernel<decltype(nt_c)::value, OUT, X...>), l.grid, l.block, 0, l.st, l.src, n, steps, (long)pitch,
                           (long)frame_stride, x0, l.ih, l.iw, l.th, rule, hold, skip, pix, open_runs, fresh, flush,
                           reinterpret_cast<int*>(d_totals), reinterpret_cast<int*>(d_cell_counts), count_rows, x...);
    });
}

// Called by vse_frame_cells_hold (vse_runtime.hip) after it has checked the arguments (1 <= nt <= vse_frame_cells_multi_max(), 1 <= hold <=
// 32); steps = n (+ hold - 1 with a flush) >= 0, skip = the steps whose frame lies before frame 1, count_rows = the rows of d_cell_counts
// per threshold.
int vse_frame_cells_hold_launch(const void* d_bgr, int n, int steps, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0, int x1,
                                const int* thresholds, int nt, int hold, int skip, const CellRule& rule, void* d_state, int fresh, int flush,
                                int32_t* d_totals, int32_t* d_cell_counts, int count_rows, void* stream) {
    const CellsLaunch l(d_bgr, pitch, y0, y1, x0, x1, thresholds, nt, stream);
    return cells_hold_launch<CELLS_ONLY>(l, n, steps, pitch, frame_stride, x0, nt, hold, skip, rule, d_state, fresh, flush, d_totals,
                                         d_cell_counts, count_rows);
}

// Called by vse_frame_cells_hold_masks (vse_runtime.hip) after it has checked the arguments as vse_frame_cells_hold does and 0 <= slot0,
// slot0 + n <= cap of d_masks: the n frames are the steps 0 .. n - 1 and take the slots slot0 .. slot0 + n - 1, the flush steps none.
int vse_frame_cells_hold_masks_launch(const void* d_bgr, int n, int steps, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0, int x1,
                                      const int* thresholds, int nt, int hold, int skip, const CellRule& rule, void* d_state, int fresh,
                                      int flush, int32_t* d_totals, int32_t* d_cell_counts, int count_rows, void* d_masks, int slot0,
                                      void* stream) {
    const CellsLaunch l(d_bgr, pitch, y0, y1, x0, x1, thresholds, nt, stream);
    return cells_hold_launch<CELLS_MASKS, unsigned long long* __restrict__, long>(
        l, n, steps, pitch, frame_stride, x0, nt, hold, skip, rule, d_state, fresh, flush, d_totals, d_cell_counts, count_rows,
        reinterpret_cast<unsigned long long*>(d_masks), (long)slot0);
}

// Called by vse_frame_masks_replay_hold (vse_runtime.hip) after it has checked the region, 0 <= q < nt <= vse_frame_cells_multi_max(), the
// slots 0 <= f0 <= f1 <= cap, the rectangle, at least 3 x 3 and inside the region, and 1 <= hold <= 32; n = f1 - f0, steps = n (+ hold - 1
// with a flush) > 0 and skip as for vse_frame_hold_launch.  d_counts is cleared on the stream ahead of the kernel, which adds into it.
int vse_frame_masks_replay_hold_launch(const void* d_masks, int area_h, int area_w, int nt, int q, int f0, int n, int steps, int ry0, int ry1,
                                       int rx0, int rx1, int hold, int skip, void* d_state, int fresh, int32_t* d_counts, void* stream) {
    const int gy = (area_h - 2 + FC_ROWS - 1) / FC_ROWS, gx = (area_w - 2 + 63) / 64;
    const long cells = (long)gy * gx, slot_words = (long)nt * cells * FC_ROWS;
    ReplayRect r;
    r.ry0 = ry0, r.rx0 = rx0, r.ih = ry1 - ry0 - 2, r.iw = rx1 - rx0 - 2, r.wpr = (r.iw + 63) / 64;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (steps > skip && hipMemsetAsync(d_counts, 0, (size_t)(steps - skip) * 3 * sizeof(int32_t), st) != hipSuccess) return VSE_E_HIP;
    const unsigned long long* slice = reinterpret_cast<const unsigned long long*>(d_masks) + (long)f0 * slot_words + (long)q * cells * FC_ROWS;
    hipLaunchKernelGGL(frame_masks_replay_hold_kernel, dim3(r.wpr, (r.ih + FC_ROWS - 1) / FC_ROWS), dim3(FC_WAVES * 64), 0, st, slice, slot_words,
                       gx, r, n, steps, hold, skip, reinterpret_cast<unsigned short*>(d_state), fresh, reinterpret_cast<int*>(d_counts));
    return hipGetLastError() == hipSuccess ? VSE_OK : VSE_E_HIP;
}

// ---- vse_frame_hold_bounded -----------------------------------------------------------------------------------------------------
// B_u = the edge pixels of frame u whose run of consecutive edge frames is L frames long with hold <= L <= max_hold: vse_frame_hold's
// held edges without those that hold for too long (a logo, a static shot).  Membership is per whole run, so nothing is counted until a
// run ends, and then everything about it is known: a run s..t in range is in B_s .. B_t, appears at s and vanishes at t + 1.  Per row
// that is a difference array, a[s] += 1 and v[t + 1] += 1, with |B_u| = |B_{u-1}| + a[u] - v[u].
//
// The tile, its mask words and the walk are frame_hold_kernel's: wave k walks interior row k along the steps with lane = column.  Per
// pixel one run length, saturating at max_hold + 1 (a run that long is out whatever follows).  At a step u where runs end in range the
// wave counts them with one ballot (v[u], gathered with lane = step and summed over the tile's rows in LDS: one atomic per step and
// block) and adds to a[u - L] once per distinct length L among the ending lanes, the lanes of one length found by a ballot each: a
// subtitle's pixels start and end together, so that loop runs once where it matters.
// The pending rows live in a ring in the caller's state, a and v per slot, row r in slot r % ring; integer atomics, so the order the
// blocks arrive in cannot change them.  A launch covers at most FC_CHUNK steps, which with the max_hold rows a run can reach back bounds
// the rows in flight: ring = max_hold + FC_CHUNK slots.  A flush is ONE step without an edge: every open run ends there.
// frame_hold_rows_kernel, one wave behind each such launch on the same stream, turns the rows that can no longer change into counts (a
// running sum of a - v whose carry stays in the state), writes them and clears their slots.
// State: int32 [4] (the carry |B| of the last row written, then padding), the ring int32 [ring][2], then one uint16 run length per
// pixel of the tile words laid out as frame_hold_kernel's.  A clip's first call clears carry and ring and ignores the run lengths.
namespace {

constexpr int HB_HEAD_BYTES = 16;

// n frames, then steps - n steps without an edge (the flush), steps <= FC_CHUNK; slot0 = the ring slot of the first step's frame.
// The edge words come from frame_hold_body's policies, HoldFrames (frame_hold_bounded_kernel) or HoldSlots
// (frame_masks_replay_hold_bounded_kernel): one text for both kernels, block (w, iy0 / FC_ROWS) owning the tile's run lengths.
template <class SRC>
__device__ __forceinline__ void frame_hold_bounded_body(const SRC& source, int n, int steps, int iy0, int w, int wpr, int hold, int max_hold,
                                                        int slot0, int ring_slots, unsigned short* __restrict__ state, int fresh,
                                                        int* __restrict__ ring) {
    __shared__ unsigned long long msk[FC_CHUNK][FC_ROWS];
    static_assert(FC_WAVES == FC_ROWS, "wave k walks interior row k of the tile");
    static_assert(FC_CHUNK == 64, "the steps of a launch are the lanes of a wave");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool mine = wave < source.rows();    // wave-uniform; the words of the other rows stay zero
    unsigned short* st = state + ((long)(iy0 + wave) * wpr + w) * 64 + lane;
    int run = (mine && !fresh) ? (int)*st : 0;

    source.fill(0, n, msk);
    for (int i = n * FC_ROWS + threadIdx.x; i < steps * FC_ROWS; i += FC_WAVES * 64) msk[i / FC_ROWS][i % FC_ROWS] = 0ull;
    __syncthreads();
    if (mine) {
        // lane = step for the words going in and the counts going out, lane = column for the walk
        const unsigned long long col = lane < steps ? msk[lane][wave] : 0ull;
        const int lo = (int)(unsigned)col, hi = (int)(unsigned)(col >> 32);
        int ended = 0;                         // runs of this row that ended in range at step `lane`
        int slot = slot0;                      // ring slot of this step's frame
        for (int tl = 0; tl < steps; ++tl) {
            const bool edge = edge_bit(lo, hi, tl, lane);
            const int len = run;
            run = edge ? min(run + 1, max_hold + 1) : 0;
            const bool ends = !edge && len >= hold && len <= max_hold;
            unsigned long long m = __ballot(ends);
            if (m) {                           // wave-uniform
                if (lane == tl) ended = __popcll(m);
                do {
                    const int l = __builtin_amdgcn_readlane(len, __ffsll((long long)m) - 1);
                    const unsigned long long same = __ballot(ends && len == l);
                    int s = slot - l;          // the run's first frame: 1 <= l <= max_hold < ring_slots
                    if (s < 0) s += ring_slots;
                    if (lane == 0) atomicAdd(ring + 2 * s, __popcll(same));
                    m &= ~same;
                } while (m);
            }
            slot = slot + 1 == ring_slots ? 0 : slot + 1;
        }
        if (lane < steps) msk[lane][wave] = (unsigned long long)ended;
        *st = (unsigned short)run;
    }
    __syncthreads();
    if ((int)threadIdx.x < steps) {
        int v = 0;
#pragma unroll
        for (int k = 0; k < FC_ROWS; ++k) v += (int)msk[threadIdx.x][k];       // words of rows outside the area are zero
        int s = slot0 + (int)threadIdx.x;      // < 2 * ring_slots: steps <= FC_CHUNK < ring_slots
        if (s >= ring_slots) s -= ring_slots;
        if (v) atomicAdd(ring + 2 * s + 1, v);
    }
}

// A gfx950 compile before the body became a template: 68 VGPRs, 96 SGPRs, 4096 bytes of LDS, no scratch, 7 waves per SIMD; after it the
// same five figures.  (frame_masks_replay_hold_bounded_kernel below, which has no gradients to compute: 18 VGPRs, 40 SGPRs, 4096 bytes.)
__global__ __launch_bounds__(FC_WAVES * 64) void frame_hold_bounded_kernel(const uint8_t* __restrict__ src, int n, int steps, long pitch,
                                                                           long fstride, int x0, int ih, int iw, int wpr, int thresh, int hold,
                                                                           int max_hold, int slot0, int ring_slots,
                                                                           unsigned short* __restrict__ state, int fresh, int* __restrict__ ring) {
    const int w = blockIdx.x, iy0 = blockIdx.y * FC_ROWS;
    const HoldFrames source = {src + (long)iy0 * pitch, pitch, fstride, thresh, tile_lane(w, iy0, ih, iw, x0)};
    frame_hold_bounded_body(source, n, steps, iy0, w, wpr, hold, max_hold, slot0, ring_slots, state, fresh, ring);
}

// vse_frame_masks_replay_hold_bounded: frame_hold_bounded_kernel on a rectangle of the region, its edge words taken from the kept masks
// (frame_masks_replay_hold_kernel's argument: an edge bit does not depend on the area it is counted in).  Grid and block are
// frame_hold_bounded_kernel's on the rectangle, the walk, the ring and the run lengths are frame_hold_bounded_body's, so the state this
// leaves is vse_frame_hold_bounded's of that rectangle.  `slice` points at threshold q's first cell in the slot of step 0; the n real
// steps read the slots of steps 0 .. n - 1, the flush step none.
__global__ __launch_bounds__(FC_WAVES * 64) void frame_masks_replay_hold_bounded_kernel(const unsigned long long* __restrict__ slice,
                                                                                        long slot_words, int gx, ReplayRect r, int n, int steps,
                                                                                        int hold, int max_hold, int slot0, int ring_slots,
                                                                                        unsigned short* __restrict__ state, int fresh,
                                                                                        int* __restrict__ ring) {
    const int w = blockIdx.x, iy0 = blockIdx.y * FC_ROWS;
    const HoldSlots source = {slice, slot_words, gx, r, iy0, w};
    frame_hold_bounded_body(source, n, steps, iy0, w, r.wpr, hold, max_hold, slot0, ring_slots, state, fresh, ring);
}

// One wave: the `rows` rows from ring slot `slot` on (rows <= ring_slots) -> out [rows][3] = |B|, appeared, vanished; their slots cleared.
__global__ __launch_bounds__(64) void frame_hold_rows_kernel(int* __restrict__ ring, int* __restrict__ carry, int ring_slots, int slot, int rows,
                                                             int* __restrict__ out) {
    const int lane = threadIdx.x;
    int e = *carry;
    for (int base = 0; base < rows; base += 64) {
        const int i = base + lane;
        const bool live = i < rows;
        int s = slot + i;
        if (s >= ring_slots) s -= ring_slots;
        const int a = live ? ring[2 * s] : 0, v = live ? ring[2 * s + 1] : 0;
        int d = a - v;                         // inclusive scan over the lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(d, o);
            if (lane >= o) d += up;
        }
        if (live) {
            out[(long)i * 3] = e + d;
            out[(long)i * 3 + 1] = a;
            out[(long)i * 3 + 2] = v;
            ring[2 * s] = 0;
            ring[2 * s + 1] = 0;
        }
        e += __shfl(d, 63);
    }
    if (lane == 0) *carry = e;
}

}  // namespace

size_t vse_frame_hold_bounded_bytes(int ih, int iw, int max_hold) {
    return HB_HEAD_BYTES + (size_t)(max_hold + FC_CHUNK) * 2 * sizeof(int32_t) + (size_t)ih * ((iw + 63) / 64) * HOLD_WORD_BYTES;
}

// The loop of both bounded launchers: the call is worked through in pieces of FC_CHUNK steps, each a launch of the walk, walk(at, frames,
// steps, slot0, ring_slots, pix, fresh, ring) over the frames at .. at + frames - 1 of the call, and, where it completes rows, one of the
// finishing kernel.
template <class WALK>
static int hold_bounded_pieces(int n, int max_hold, void* d_state, int64_t fed, int flush, int32_t* d_counts, hipStream_t st, WALK walk) {
    const int ring_slots = max_hold + FC_CHUNK;
    int* carry = reinterpret_cast<int*>(d_state);
    int* ring = reinterpret_cast<int*>(reinterpret_cast<char*>(d_state) + HB_HEAD_BYTES);
    unsigned short* pix = reinterpret_cast<unsigned short*>(ring + 2 * (size_t)ring_slots);
    if (fed == 0 && hipMemsetAsync(d_state, 0, HB_HEAD_BYTES + (size_t)ring_slots * 2 * sizeof(int32_t), st) != hipSuccess) return VSE_E_HIP;
    const int64_t first = fed > max_hold ? fed - max_hold : 0;         // rows up to this frame went out with earlier calls
    int64_t written = first;
    const int64_t total = (int64_t)n + (flush ? 1 : 0);
    for (int64_t at = 0; at < total; at += FC_CHUNK) {
        const int steps = (int)(total - at < FC_CHUNK ? total - at : FC_CHUNK);
        const int frames = (int)(n - at < steps ? n - at : steps);
        const int64_t done = fed + at + frames;                        // frames of the clip seen after this piece
        walk(at, frames, steps, (int)((fed + at + 1) % ring_slots), ring_slots, pix, (int)(fed == 0 && at == 0), ring);
        // a row is final once max_hold further frames have been seen: a run that still covers it is then too long
        const int64_t upto = (flush && at + steps == total) ? done : (done > max_hold ? done - max_hold : 0);
        if (upto > written) {                                          // at most max_hold + FC_CHUNK - 1 rows, the flush's
            hipLaunchKernelGGL(frame_hold_rows_kernel, dim3(1), dim3(64), 0, st, ring, carry, ring_slots, (int)((written + 1) % ring_slots),
                               (int)(upto - written), reinterpret_cast<int*>(d_counts) + (written - first) * 3);
            written = upto;
        }
    }
    return hipGetLastError() == hipSuccess ? VSE_OK : VSE_E_HIP;
}

// Called by vse_frame_hold_bounded (vse_runtime.hip) after it has checked the arguments (1 <= hold <= max_hold, n + flush >= 1).
int vse_frame_hold_bounded_launch(const void* d_bgr, int n, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0, int x1, int edge_thresh,
                                  int hold, int max_hold, void* d_state, int64_t fed, int flush, int32_t* d_counts, void* stream) {
    const int ih = y1 - y0 - 2, iw = x1 - x0 - 2, wpr = (iw + 63) / 64;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const uint8_t* src = reinterpret_cast<const uint8_t*>(d_bgr) + (long)y0 * pitch;
    return hold_bounded_pieces(n, max_hold, d_state, fed, flush, d_counts, st,
                               [&](int64_t at, int frames, int steps, int slot0, int ring_slots, unsigned short* pix, int fresh, int* ring) {
        hipLaunchKernelGGL(frame_hold_bounded_kernel, dim3(wpr, (ih + FC_ROWS - 1) / FC_ROWS), dim3(FC_WAVES * 64), 0, st,
                           src + at * frame_stride, frames, steps, (long)pitch, (long)frame_stride, x0, ih, iw, wpr, edge_thresh, hold, max_hold,
                           slot0, ring_slots, pix, fresh, ring);
    });
}

// Called by vse_frame_masks_replay_hold_bounded (vse_runtime.hip) after it has checked what vse_frame_masks_replay_hold_launch's caller
// checks and 1 <= hold <= max_hold <= 4000; n = f1 - f0, n + flush >= 1.  The slice pointer of a piece advances by slots.
int vse_frame_masks_replay_hold_bounded_launch(const void* d_masks, int area_h, int area_w, int nt, int q, int f0, int n, int ry0, int ry1,
                                               int rx0, int rx1, int hold, int max_hold, void* d_state, int64_t fed, int flush,
                                               int32_t* d_counts, void* stream) {
    const int gy = (area_h - 2 + FC_ROWS - 1) / FC_ROWS, gx = (area_w - 2 + 63) / 64;
    const long cells = (long)gy * gx, slot_words = (long)nt * cells * FC_ROWS;
    ReplayRect r;
    r.ry0 = ry0, r.rx0 = rx0, r.ih = ry1 - ry0 - 2, r.iw = rx1 - rx0 - 2, r.wpr = (r.iw + 63) / 64;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const unsigned long long* slice = reinterpret_cast<const unsigned long long*>(d_masks) + (long)f0 * slot_words + (long)q * cells * FC_ROWS;
    return hold_bounded_pieces(n, max_hold, d_state, fed, flush, d_counts, st,
                               [&](int64_t at, int frames, int steps, int slot0, int ring_slots, unsigned short* pix, int fresh, int* ring) {
        hipLaunchKernelGGL(frame_masks_replay_hold_bounded_kernel, dim3(r.wpr, (r.ih + FC_ROWS - 1) / FC_ROWS), dim3(FC_WAVES * 64), 0, st,
                           slice + at * slot_words, slot_words, gx, r, frames, steps, hold, max_hold, slot0, ring_slots, pix, fresh, ring);
    });
}

// ---- vse_frame_cells_hold_bounded -------------------------------------------------------------------------------------------------
// The locator's cells (frame_cells_hold_kernel) on the bounded masks of frame_hold_bounded_kernel, for busy backgrounds that stand still: a
// block is a cell for all frames of the call and for NT thresholds.  Three stages per chunk of steps, all pieces of the kernels above:
//   tile_masks_multi  a frame's bytes, lumas and gradients once, the edge words of the NT thresholds side by side in LDS;
//   the walk          frame_hold_bounded_kernel's: wave k walks interior row k with lane = column and one saturating run length per pixel
//                     and threshold; a run that ends in range at step u with length L is a[u - L] += 1 and v[u] += 1, one add per
//                     distinct length among the ending lanes for a, one per step with an ending run for v (gathered with lane = step);
//   the tail          for the rows that can no longer change (max_hold further frames seen, or the flush), wave q takes threshold q
//                     with lane = row: e by frame_hold_rows_kernel's running sum of a - v with the carry in the state, the slot cleared,
//                     cell_counts written, and CellRuns stepped with frame_cells_hold_kernel's two ballots.
// The pending rows live in a ring PER CELL AND THRESHOLD in the caller's state, row r in slot r % ring, ring = max_hold + FC_CHUNK slots as
// in frame_hold_bounded_kernel.  A slot is one uint32, a | v << 16: a cell has 512 pixels and each starts at most one run and ends at most one
// in a frame, so neither half passes 512.  Only the block that owns the cell touches its ring.  Its eight row-waves add to a slot with
// integer atomics and the tail takes a slot and clears it with one atomic exchange, so every access to the ring is served by the same
// cache level; __syncthreads() orders the walk before the tail and the tail before the next chunk's walk.  No two blocks share a word.
// A flush is ONE step without an edge, which ends every open run, then the tail over all rows that are left, then the runs are closed.
// Rows are numbered within the call as vse_frame_hold_bounded numbers them: row i of the call is frame first + 1 + i of the clip, first =
// max(0, fed - max_hold) being the last frame whose row went out with an earlier call; step j of the call (frame fed + 1 + j) is row
// lagged + j, lagged = fed - first.  slot_w = the ring slot of row 0.
// State: pix as frame_cells_hold_kernel's, the uint16 being the run length (saturating at max_hold + 1); ring uint32 [NT][cells][ring];
// carry int32 [NT][cells] = |B| of the cell's last finished row; open_runs as frame_cells_hold_kernel's.  A clip's first call finds ring,
// carry and open runs cleared by the launcher and ignores pix.
namespace {

// OUT and the trailing pack x are frame_cells_multi_kernel's: CELLS_ONLY (vse_frame_cells_hold_bounded; no argument, and the code this
// kernel compiled to before it had the parameter) or CELLS_MASKS (vse_frame_cells_hold_bounded_masks; unsigned long long* masks, long
// slot0): the edge words a chunk's real steps leave in LDS go to the caller's buffer in that kernel's layout and by its store loop, wave q
// storing threshold q's rows in 64-byte lines, so a call writes bit for bit what frame_cells_multi_kernel<NT, CELLS_MASKS> writes for the
// same frames.  Only the `real` steps are stored (step c0 + tl < n of the call is slot slot0 + c0 + tl < cap, checked by the launcher's
// caller); the flush step has no slot.  This kind adds NO barrier: unlike the held walk, the bounded walk only reads msk (its words go to
// registers once, its counts leave through the ring), so the words stay what tile_masks_multi left until the next chunk refills them.
// The stores stand between the barrier behind the fill and the walk, and every wave, those with wave >= NT that skip the tail included,
// passes the barrier behind the walk before it refills msk; a storing wave reaches that barrier only with its LDS reads done.  Issued
// ahead of the walk, the stores drain under it.
// VGPRs at NT = 1 .. 8 of a gfx950 compile:
//   CELLS_ONLY before the parameter   85  98  96 100 103 102 114 112
//   CELLS_ONLY with it                85  98  96 100 103 102 114 112
//   CELLS_MASKS                       91 102 102 104 107 106 118 116
// 106 SGPRs, 4096 NT bytes of LDS and no scratch in all three rows.  Waves per SIMD 5 4 5 4 4 4 4 4 without masks; with them NT = 3
// drops from 5 to 4 (102 VGPRs), the other counts stay.
template <int NT, int OUT, class... X>
__global__ __launch_bounds__(FC_WAVES * 64) void frame_cells_hold_bounded_kernel(const uint8_t* __restrict__ src, int n, int steps, long pitch,
                                                                                 long fstride, int x0, int ih, int iw, CellThresholds th,
                                                                                 CellRule rule, int hold, int max_hold, int ring_slots, int slot_w,
                                                                                 int lagged, unsigned short* __restrict__ pix, unsigned* ring,
                                                                                 int* __restrict__ carry, int* __restrict__ open_runs, int fresh,
                                                                                 int flush, int* __restrict__ totals, int* __restrict__ cell_counts,
                                                                                 int count_rows, X... x) {
    __shared__ unsigned long long msk[NT * FC_CHUNK * FC_ROWS];           // [NT][FC_CHUNK][FC_ROWS]
    static_assert(FC_WAVES == FC_ROWS, "wave k walks interior row k of the tile");
    static_assert(FC_CHUNK == 64, "the steps of a chunk are the lanes of a wave");
    static_assert(NT >= 1 && NT <= FC_WAVES, "wave q owns threshold q");
    static_assert(OUT == CELLS_ONLY || OUT == CELLS_MASKS, "the bounded cells keep masks or nothing");
    static_assert(sizeof...(X) == (OUT == CELLS_ONLY ? 0 : 2), "the pack is the kind's arguments");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int iy0 = blockIdx.y * FC_ROWS, wpr = gridDim.x;
    const long cell = (long)blockIdx.y * gridDim.x + blockIdx.x, cells = (long)gridDim.y * gridDim.x;
    const TileLane t = tile_lane(blockIdx.x, iy0, ih, iw, x0);
    const bool walks = wave < t.rows;          // wave-uniform; the words of the other rows stay zero
    const bool mine = wave < NT;               // wave q owns threshold q
    unsigned short* ps = pix + ((long)(iy0 + wave) * wpr + blockIdx.x) * 64 + lane;
    const long pslice = (long)ih * wpr * 64;
    const long mycell = (long)(mine ? wave : 0) * cells + cell;
    int* tot = totals + mycell * 4;
    int run[NT];
#pragma unroll
    for (int q = 0; q < NT; ++q) run[q] = (walks && !fresh) ? (int)ps[q * pslice] : 0;
    CellRuns cr = {0, 0, 0, 0, 0};
    int ecar = 0;                              // |B| of the last finished row
    if (mine && !fresh) {
        cr.load(open_runs + mycell, tot);
        ecar = carry[mycell];
    }
    long done_rows = 0;                        // rows of this call that are finished

    for (int c0 = 0; c0 < steps; c0 += FC_CHUNK) {
        const int cn = min(FC_CHUNK, steps - c0);
        const int real = max(0, min(cn, n - c0));          // the step after frame n is the flush: no edge anywhere
        const int cslot = (int)(((long)slot_w + lagged + c0) % ring_slots);     // ring slot of the chunk's first step
        tile_masks_multi<NT>(src + (long)iy0 * pitch, c0, real, pitch, fstride, t, th, msk);
        zero_steps<NT>(msk, real, cn);
        __syncthreads();
        if constexpr (OUT == CELLS_MASKS) {
            // frame_cells_multi_kernel's store loop on the edge words of the chunk's real steps; nothing writes msk before the barrier
            // behind the walk, which every wave passes before the next fill
            static_assert(FC_ROWS == 8, "a lane's word of a store pass is lane % 8 of frame lane / 8");
            if (mine) {
                const unsigned long long* mq = msk + wave * FC_CHUNK * FC_ROWS;
                const long slot_words = NT * cells * FC_ROWS;
                unsigned long long* out =
                    first_of(x...) + (second_of(x...) + c0 + (lane >> 3)) * slot_words + (wave * cells + cell) * FC_ROWS + (lane & 7);
#pragma unroll 1
                for (int i = lane; i < real * FC_ROWS; i += 64, out += (FC_CHUNK / FC_ROWS) * slot_words) *out = mq[i];
            }
        }
        if (walks) {
            // lane = step of the chunk for the words going in and the counts going out, lane = column for the walk
            int lo[NT], hi[NT], ended[NT];
#pragma unroll
            for (int q = 0; q < NT; ++q) {
                const unsigned long long col = lane < cn ? msk[(q * FC_CHUNK + lane) * FC_ROWS + wave] : 0ull;
                lo[q] = (int)(unsigned)col;
                hi[q] = (int)(unsigned)(col >> 32);
                ended[q] = 0;                  // runs of this row that ended in range at step `lane`
            }
            int slot = cslot;                  // ring slot of this step's frame
            for (int tl = 0; tl < cn; ++tl) {
#pragma unroll
                for (int q = 0; q < NT; ++q) {
                    const bool edge = edge_bit(lo[q], hi[q], tl, lane);
                    const int len = run[q];
                    run[q] = edge ? min(len + 1, max_hold + 1) : 0;
                    const bool ends = !edge && len >= hold && len <= max_hold;
                    unsigned long long m = __ballot(ends);
                    if (m) {                   // wave-uniform
                        unsigned* rq = ring + ((long)q * cells + cell) * ring_slots;
                        if (lane == tl) ended[q] = __popcll(m);
                        do {
                            const int l = __builtin_amdgcn_readlane(len, __ffsll((long long)m) - 1);
                            const unsigned long long same = __ballot(ends && len == l);
                            int s = slot - l;  // the run's first frame: 1 <= l <= max_hold < ring_slots
                            if (s < 0) s += ring_slots;
                            if (lane == 0) atomicAdd(rq + s, (unsigned)__popcll(same));
                            m &= ~same;
                        } while (m);
                    }
                }
                slot = slot + 1 == ring_slots ? 0 : slot + 1;
            }
            int s = cslot + lane;              // < 2 * ring_slots: FC_CHUNK < ring_slots
            if (s >= ring_slots) s -= ring_slots;
#pragma unroll
            for (int q = 0; q < NT; ++q) {
                if (ended[q]) atomicAdd(ring + ((long)q * cells + cell) * ring_slots + s, (unsigned)ended[q] << 16);      // lane < cn
            }
        }
        __syncthreads();
        // a row is final once max_hold further frames have been seen: a run that still covers it is then too long
        const bool last = c0 + cn == steps;
        const long seen = min(c0 + cn, n);
        const long upto = (flush && last) ? (long)lagged + n : max(0l, lagged + seen - max_hold);
        if (mine) {                                // lane = row
            unsigned* rq = ring + mycell * ring_slots;
            for (long base = done_rows; base < upto; base += FC_CHUNK) {
                const long i = base + lane;
                const bool live = i < upto;
                int s = (int)((slot_w + base) % ring_slots) + lane;
                if (s >= ring_slots) s -= ring_slots;
                const unsigned word = live ? atomicExch(rq + s, 0u) : 0u;
                const int a = (int)(word & 0xffffu), v = (int)(word >> 16);
                int d = a - v;                     // inclusive scan over the lanes
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int up = __shfl_up(d, o);
                    if (lane >= o) d += up;
                }
                const int e = ecar + d, ep = e - a + v;        // |B_u|, |B_{u-1}|
                if (live && cell_counts) {
                    int* o = cell_counts + (((long)wave * count_rows + i) * cells + cell) * 3;
                    o[0] = e;
                    o[1] = a;
                    o[2] = v;
                }
                const long long uni = ep + a;      // |B' or B|
                const unsigned long long present = __ballot(live && e >= rule.min_edges);
                const unsigned long long ratio = __ballot(live && uni > 0 && (long long)(a + v) * rule.ratio_den >= (long long)rule.ratio_num * uni);
                const int cnt = (int)min((long)FC_CHUNK, upto - base);
                for (int f = 0; f < cnt; ++f) cr.step((present >> f) & 1, (ratio >> f) & 1, rule);
                ecar += __shfl(d, 63);
            }
        }
        done_rows = max(done_rows, upto);
    }
    if (walks) {
#pragma unroll
        for (int q = 0; q < NT; ++q) ps[q * pslice] = (unsigned short)run[q];
    }
    if (mine && lane == 0) {
        if (flush) cr.close(rule);
        open_runs[mycell] = cr.run;
        carry[mycell] = ecar;
        tot[0] = cr.covered;
        tot[1] = cr.runs;
        tot[2] = cr.present;
        tot[3] = cr.cuts;
    }
}

// The parts of vse_frame_cells_hold_bounded's state for an interior of ih x iw pixels, in this order: pix, ring, carry, open runs.
struct CellsHoldBoundedLayout {
    size_t cells, pix_bytes, ring_bytes, per_cell_bytes, total;
};

CellsHoldBoundedLayout cells_hold_bounded_layout(int ih, int iw, int nt, int max_hold) {
    CellsHoldBoundedLayout l;
    l.cells = (size_t)((ih + FC_ROWS - 1) / FC_ROWS) * ((iw + 63) / 64);
    l.pix_bytes = (size_t)nt * ih * ((iw + 63) / 64) * HOLD_WORD_BYTES;
    l.ring_bytes = (size_t)nt * l.cells * (max_hold + FC_CHUNK) * sizeof(uint32_t);
    l.per_cell_bytes = (size_t)nt * l.cells * sizeof(int32_t);
    l.total = (l.pix_bytes + l.ring_bytes + 2 * l.per_cell_bytes + 7) & ~(size_t)7;
    return l;
}

}  // namespace

size_t vse_frame_cells_hold_bounded_bytes(int ih, int iw, int nt, int max_hold) { return cells_hold_bounded_layout(ih, iw, nt, max_hold).total; }

// frame_cells_hold_bounded_kernel<nt, OUT, X...> with the kind's arguments x (X given explicitly, as for cells_multi_launch).  One launch,
// and before a clip's first one a clear of everything in the state but the run lengths.
template <int OUT, class... X>
static int cells_hold_bounded_launch(const CellsLaunch& l, int n, int64_t pitch, int64_t frame_stride, int x0, int nt, int hold, int max_hold,
                                     const CellRule& rule, void* d_state, int64_t fed, int flush, int32_t* d_totals, int32_t* d_cell_counts,
                                     int count_rows, X... x) {
    const CellsHoldBoundedLayout lay = cells_hold_bounded_layout(l.ih, l.iw, nt, max_hold);
    char* base = reinterpret_cast<char*>(d_state);
    unsigned short* pix = reinterpret_cast<unsigned short*>(base);
    unsigned* ring = reinterpret_cast<unsigned*>(base + lay.pix_bytes);
    int* carry = reinterpret_cast<int*>(base + lay.pix_bytes + lay.ring_bytes);
    int* open_runs = reinterpret_cast<int*>(base + lay.pix_bytes + lay.ring_bytes + lay.per_cell_bytes);
    if (fed == 0 && hipMemsetAsync(ring, 0, lay.ring_bytes + 2 * lay.per_cell_bytes, l.st) != hipSuccess) return VSE_E_HIP;
    const int ring_slots = max_hold + FC_CHUNK;
    const int64_t first = fed > max_hold ? fed - max_hold : 0;         // rows up to this frame went out with earlier calls
    const int steps = n + (flush ? 1 : 0);
    return launch_for_nt(nt, [&](auto nt_c) {
        hipLaunchKernelGGL((frame_cells_hold_bounded_kernel<decltype(nt_c)::value, OUT, X...>), l.grid, l.block, 0, l.st, l.src, n, steps,
                           (long)pitch, (long)frame_stride, x0, l.ih, l.iw, l.th, rule, hold, max_hold, ring_slots,
                           (int)((first + 1) % ring_slots), (int)(fed - first), pix, ring, carry, open_runs, fed == 0, flush,
                           reinterpret_cast<int*>(d_totals), reinterpret_cast<int*>(d_cell_counts), count_rows, x...);
    });
}

// Called by vse_frame_cells_hold_bounded (vse_runtime.hip) after it has checked the arguments (1 <= nt <= vse_frame_cells_multi_max(), 1 <=
// hold <= max_hold <= 4000, n + flush >= 1, n + max_hold fits an int); count_rows = the rows of d_cell_counts per threshold.
int vse_frame_cells_hold_bounded_launch(const void* d_bgr, int n, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0, int x1,
                                        const int* thresholds, int nt, int hold, int max_hold, const CellRule& rule, void* d_state,
                                        int64_t fed, int flush, int32_t* d_totals, int32_t* d_cell_counts, int count_rows, void* stream) {
    const CellsLaunch l(d_bgr, pitch, y0, y1, x0, x1, thresholds, nt, stream);
    return cells_hold_bounded_launch<CELLS_ONLY>(l, n, pitch, frame_stride, x0, nt, hold, max_hold, rule, d_state, fed, flush, d_totals,
                                                 d_cell_counts, count_rows);
}

// Called by vse_frame_cells_hold_bounded_masks (vse_runtime.hip) after it has checked the arguments as vse_frame_cells_hold_bounded does and
// 0 <= slot0, slot0 + n <= cap of d_masks: the n frames are the steps 0 .. n - 1 and take the slots slot0 .. slot0 + n - 1, the flush none.
int vse_frame_cells_hold_bounded_masks_launch(const void* d_bgr, int n, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0, int x1,
                                              const int* thresholds, int nt, int hold, int max_hold, const CellRule& rule, void* d_state,
                                              int64_t fed, int flush, int32_t* d_totals, int32_t* d_cell_counts, int count_rows, void* d_masks,
                                              int slot0, void* stream) {
    const CellsLaunch l(d_bgr, pitch, y0, y1, x0, x1, thresholds, nt, stream);
    return cells_hold_bounded_launch<CELLS_MASKS, unsigned long long* __restrict__, long>(
        l, n, pitch, frame_stride, x0, nt, hold, max_hold, rule, d_state, fed, flush, d_totals, d_cell_counts, count_rows,
        reinterpret_cast<unsigned long long*>(d_masks), (long)slot0);
}
