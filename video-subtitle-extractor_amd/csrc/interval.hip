// Interval composite (vse_interval_accumulate / vse_interval_composite, include/vse_hip.h): a subtitle stands still while the picture
// behind it moves, so a per-byte reduction over the frames of one subtitle interval keeps the text and flattens the background.  The
// integers are the specification (tests/interval_ref.py restates them in numpy, bit for bit), for every byte b of the area
// [y0, y1) x [x0, x1) x 3 over the frames accumulated since the last reset:
//   mn[b] = min, mx[b] = max, sm[b] = sum (uint32)
//   composite: mode 0 = mn, 1 = mx, 2 = (2 sm + frames) / (2 frames)      (the mean, halves rounded up)
// HBM-bound byte work: one pass over the area's bytes of every frame, six state bytes per area byte read and written once per call.
//
// Layout: a lane owns a 16-byte run of one area row (run c = bytes 16 c .. 16 c + 15 of the row's 3 area_w bytes), consecutive lanes
// consecutive runs, for ALL frames of the call: mn / mx / sm of its 16 bytes stay in registers while IV_DEPTH frames' loads are in
// flight, and the state is read and written once.  Frames are not split across lanes: a byte min / max has no atomic.
// State: three planes over rows padded to whole runs (rb16 = 16 ceil(3 area_w / 16) bytes): mn, then mx (uint8 [area_h][rb16] each),
// then sm (uint32 [area_h][rb16]); every state access is an aligned 16-byte one.  The padding bytes hold nothing of meaning.
// Two loads of a run:
//   wide     one 16-byte load; needs the run whole (16 area bytes) and 16-byte aligned in every frame: base + 3 x0, pitch and frame
//            stride multiples of 16.
//   general  any byte alignment, pitch and stride, and the short run that ends a row: the aligned dwords that hold the run's bytes
//            (at most five), shifted into place.  No dword without a byte of the area's row is touched, so at most 3 bytes beside a
//            row's ends are fetched with it and dropped; they share an aligned dword with a byte of the area.
// The bytes are unpacked into ints before min / max / add and packed again by shifts: no packed-byte arithmetic in the source (see
// clip8 in yuv.hip for what hipcc made of one on this target).
//
// Interval rank (vse_interval_rank): the per-byte ORDER STATISTIC over the n <= 63 frames of one call: out[b] = element `rank` of the
// ascending sort of frame[f][b].  Stateless, one launch, no atomics.
// Layout: a lane owns ONE dword of an area row (dword c = bytes 4 c .. 4 c + 3 of the row's 3 area_w bytes) for all n frames, so the
// n samples of its four bytes are n registers; a 16-byte run per lane, as above, would need 4 n.  The sample loops are unrolled over
// a compile-time bucket KB of 8, 16, 32 or 64 slots (a runtime-indexed array would go to scratch); the slots from n on are filled
// with 0xFF bytes without a load, which leaves the rank-th smallest as it is for every rank < n.
// Two loads of a dword:
//   wide     one aligned dword load; needs base + 3 x0, pitch and frame stride multiples of 4 (the short run that ends a row is
//            then the aligned dword that holds its bytes).
//   general  any byte alignment, pitch and stride: the one or two aligned dwords that hold the run's bytes, shifted into place.
//            No dword without a byte of the area's row is touched.
// Selection: per byte lane a bitwise binary search of the answer, most significant bit first: the answer is the largest t with
// |{f : v[f] < t}| <= rank, that count never falls as t grows, so each of 8 rounds tries t | bit and keeps it when the count of
// samples below it is at most rank.  No per-sample state beside the value.  Cost per OUTPUT byte: 8 rounds of KB compares (hipcc
// selects the byte inside the compare, so nothing is extracted beforehand), KB / 2 selects and KB / 2 adds with carry (two compares
// feed one add), about 16 KB + 40 vector instructions with everything around them; counted in the gfx950 ISA, wide loads: 171, 306,
// 576 and 1116 per output byte at KB = 8, 16, 32, 64, and one s_nop per pair of compares.  The accumulate kernel spends 3 per byte
// and frame (48 for 16 frames): this kernel is bound by the vector ALU, not by HBM (EXPERIMENTS.md, section V).
#include <cstdio>

#include "common.h"

void vse_set_error(const char* msg);      // vse_runtime.hip

namespace {

constexpr int IV_THREADS = 64;       // one wave per block: a 1080p band is ~1100 waves, and whole waves spread evenly over the CUs
constexpr int IV_DEPTH = 8;          // frames whose loads are in flight per lane
constexpr int MAX_FRAMES = 4194304;  // composite: 2 sm + frames <= 2 * 255 * 2^22 + 2^22 < 2^32

struct Acc {
    unsigned mn[16], mx[16], sm[16];
};

__device__ __forceinline__ void fold(Acc& a, const unsigned (&w)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned b = (w[q] >> (8 * k)) & 255u;
            a.mn[4 * q + k] = min(a.mn[4 * q + k], b);
            a.mx[4 * q + k] = max(a.mx[4 * q + k], b);
            a.sm[4 * q + k] += b;
        }
    }
}

__device__ __forceinline__ unsigned pack4(const unsigned* b) { return b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24); }

// The raw dwords of one run in one frame: WIDE = the 16 bytes themselves; general = the aligned dwords around them.
template <bool WIDE>
struct Raw {
    unsigned d[WIDE ? 4 : 5];
    unsigned sh;      // general: bytes the run starts behind d[0]
};

template <bool WIDE>
__device__ __forceinline__ Raw<WIDE> load_run(const uint8_t* p, int nb) {
    Raw<WIDE> r;
    if (WIDE) {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        r.d[0] = v.x, r.d[1] = v.y, r.d[2] = v.z, r.d[3] = v.w;
        r.sh = 0;
    } else {
        r.sh = (unsigned)(reinterpret_cast<uintptr_t>(p) & 3);
        const unsigned* q = reinterpret_cast<const unsigned*>(p - r.sh);
        const int last = (int)((r.sh + (unsigned)nb + 3) >> 2) - 1;       // index of the last dword that holds a byte of the run (0..4)
#pragma unroll
        for (int k = 0; k < 5; ++k) r.d[k] = q[min(k, last)];             // unconditional loads: all in flight at once
    }
    return r;
}

template <bool WIDE>
__device__ __forceinline__ void unpack(const Raw<WIDE>& r, unsigned (&w)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (WIDE) {
            w[k] = r.d[k];
        } else {
            const unsigned long long pair = ((unsigned long long)r.d[k + 1] << 32) | r.d[k];
            w[k] = (unsigned)(pair >> (8 * r.sh));
        }
    }
}

// p = the run in frame 0.  Bytes of a short run beyond nb come out as whatever the clamped loads held: they land in state padding.
template <bool WIDE>
__device__ __forceinline__ void accumulate_run(Acc& a, const uint8_t* p, int n, long fstride, int nb) {
    for (int f0 = 0; f0 < n; f0 += IV_DEPTH) {
        Raw<WIDE> raw[IV_DEPTH];
#pragma unroll
        for (int u = 0; u < IV_DEPTH; ++u) raw[u] = load_run<WIDE>(p + (long)min(f0 + u, n - 1) * fstride, nb);
#pragma unroll
        for (int u = 0; u < IV_DEPTH; ++u) {
            if (f0 + u < n) {          // uniform
                unsigned w[4];
                unpack<WIDE>(raw[u], w);
                fold(a, w);
            }
        }
    }
}

// src points at byte 3 x0 of row y0 of frame 0; rb = 3 area_w bytes per row in cpr = ceil(rb / 16) runs; items = area_h * cpr.
template <bool WIDE>
__global__ __launch_bounds__(IV_THREADS) void interval_accumulate_kernel(const uint8_t* __restrict__ src, int n, long pitch, long fstride,
                                                                         int rb, unsigned cpr, unsigned items, uint8_t* __restrict__ state,
                                                                         long plane, int reset) {
    const unsigned i = blockIdx.x * IV_THREADS + threadIdx.x;
    if (i >= items) return;
    const unsigned r = i / cpr, c = i - r * cpr;
    const int nb = min(16, rb - 16 * (int)c);
    uint4* smn = reinterpret_cast<uint4*>(state + (long)i * 16);
    uint4* smx = reinterpret_cast<uint4*>(state + plane + (long)i * 16);
    uint4* ssm = reinterpret_cast<uint4*>(state + 2 * plane + (long)i * 64);
    Acc a;
    if (reset) {
#pragma unroll
        for (int k = 0; k < 16; ++k) a.mn[k] = 255u, a.mx[k] = 0u, a.sm[k] = 0u;
    } else {
        const uint4 vn = *smn, vx = *smx;
        const unsigned wn[4] = {vn.x, vn.y, vn.z, vn.w}, wx[4] = {vx.x, vx.y, vx.z, vx.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 vs = ssm[q];
            a.sm[4 * q] = vs.x, a.sm[4 * q + 1] = vs.y, a.sm[4 * q + 2] = vs.z, a.sm[4 * q + 3] = vs.w;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                a.mn[4 * q + k] = (wn[q] >> (8 * k)) & 255u;
                a.mx[4 * q + k] = (wx[q] >> (8 * k)) & 255u;
            }
        }
    }
    const uint8_t* p = src + (long)r * pitch + 16 * (long)c;
    if (WIDE && nb == 16)
        accumulate_run<true>(a, p, n, fstride, nb);
    else
        accumulate_run<false>(a, p, n, fstride, nb);
    *smn = make_uint4(pack4(a.mn), pack4(a.mn + 4), pack4(a.mn + 8), pack4(a.mn + 12));
    *smx = make_uint4(pack4(a.mx), pack4(a.mx + 4), pack4(a.mx + 8), pack4(a.mx + 12));
#pragma unroll
    for (int q = 0; q < 4; ++q) ssm[q] = make_uint4(a.sm[4 * q], a.sm[4 * q + 1], a.sm[4 * q + 2], a.sm[4 * q + 3]);
}

// One run of the output per lane: exactly the nb bytes of the run are written, as one 16-byte store where the run is whole and
// 16-byte aligned in the output, byte by byte otherwise.
__global__ __launch_bounds__(IV_THREADS) void interval_composite_kernel(const uint8_t* __restrict__ state, long plane, int rb, unsigned cpr,
                                                                        unsigned items, unsigned frames, int mode, uint8_t* __restrict__ out,
                                                                        long out_pitch) {
    const unsigned i = blockIdx.x * IV_THREADS + threadIdx.x;
    if (i >= items) return;
    const unsigned r = i / cpr, c = i - r * cpr;
    const int nb = min(16, rb - 16 * (int)c);
    unsigned w[4];
    if (mode == 2) {
        const uint4* ssm = reinterpret_cast<const uint4*>(state + 2 * plane + (long)i * 64);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 vs = ssm[q];
            const unsigned s[4] = {vs.x, vs.y, vs.z, vs.w};
            unsigned b[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) b[k] = ((2u * s[k] + frames) / (2u * frames)) & 255u;       // (a byte for every true count; padding may hold more)
            w[q] = pack4(b);
        }
    } else {
        const uint4 v = *reinterpret_cast<const uint4*>(state + (mode == 1 ? plane : 0) + (long)i * 16);
        w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    }
    uint8_t* o = out + (long)r * out_pitch + 16 * (long)c;
    if (nb == 16 && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
        *reinterpret_cast<uint4*>(o) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (int k = 0; k < nb; ++k) o[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    }
}

// ---- interval stream ----------------------------------------------------------------------------------------------------------
// vse_interval_stream: the accumulate and composite kernels above in ONE launch over any number of segments, plus a ring of parked
// frames behind the accumulators (state = mn | mx | sm | cap slots of one padded band each, frame f in slot f % cap).  The lane layout
// is the accumulate kernel's: a lane owns run i of the padded band for the whole call, in the batch, in every ring slot, in the
// accumulators and in every patch, so its segment reads and its ring stores touch no byte another lane touches and their order is
// program order within the lane: all segments first, then the stores.  Frames are numbered relative to the call, rel = f - fed:
// rel >= 1 is batch frame rel - 1, rel <= 0 the ring frame in slot (fed % cap + rel) mod cap.  A segment is folded as up to three
// runs of evenly strided frames (ring up to the wrap, ring behind it, batch), each through accumulate_run with IV_DEPTH loads in
// flight; ring runs are whole and aligned whatever the area, so they always take the 16-byte load.  The segments travel as kernel
// arguments (uniform, read through scalar loads): no device copy of host memory.
struct StreamSegs {
    int lo[VSE_INTERVAL_STREAM_MAX_SEGS], hi[VSE_INTERVAL_STREAM_MAX_SEGS];        // rel of first and last
    int flags[VSE_INTERVAL_STREAM_MAX_SEGS], frames[VSE_INTERVAL_STREAM_MAX_SEGS], out[VSE_INTERVAL_STREAM_MAX_SEGS];
};

__device__ __forceinline__ void acc_reset(Acc& a) {
#pragma unroll
    for (int k = 0; k < 16; ++k) a.mn[k] = 255u, a.mx[k] = 0u, a.sm[k] = 0u;
}

// p = this lane's run in batch frame 0 (unused where n == 0), ring = its run in slot 0, slot = bytes from one slot to the next.
template <bool WIDE>
__device__ __forceinline__ void stream_lane(const uint8_t* p, int n, long fstride, int nb, uint8_t* ring, long slot, int cap, int base,
                                            const StreamSegs& sg, int nseg, int store_rel, int mode, uint4* smn, uint4* smx, uint4* ssm,
                                            uint8_t* o, long out_stride) {
    Acc a;
    for (int s = 0; s < nseg; ++s) {
        const int lo = sg.lo[s], hi = sg.hi[s], flags = sg.flags[s];
        if (flags & VSE_INTERVAL_SEG_CONTINUE) {          // (the first segment only)
            const uint4 vn = *smn, vx = *smx;
            const unsigned wn[4] = {vn.x, vn.y, vn.z, vn.w}, wx[4] = {vx.x, vx.y, vx.z, vx.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint4 vs = ssm[q];
                a.sm[4 * q] = vs.x, a.sm[4 * q + 1] = vs.y, a.sm[4 * q + 2] = vs.z, a.sm[4 * q + 3] = vs.w;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    a.mn[4 * q + k] = (wn[q] >> (8 * k)) & 255u;
                    a.mx[4 * q + k] = (wx[q] >> (8 * k)) & 255u;
                }
            }
        } else {
            acc_reset(a);
        }
        if (lo <= 0) {
            const int count = min(hi, 0) - lo + 1;
            int s0 = base + lo;
            s0 += s0 < 0 ? cap : 0;
            const int c1 = min(count, cap - s0);
            accumulate_run<true>(a, ring + (long)s0 * slot, c1, slot, 16);
            accumulate_run<true>(a, ring, count - c1, slot, 16);
        }
        if (hi >= 1) {
            const int blo = max(lo, 1);
            accumulate_run<WIDE>(a, p + (long)(blo - 1) * fstride, hi - blo + 1, fstride, nb);
        }
        if (flags & VSE_INTERVAL_SEG_EMIT) {
            unsigned w[4];
            if (mode == 2) {
                const unsigned frames = (unsigned)sg.frames[s];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    unsigned b[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) b[k] = ((2u * a.sm[4 * q + k] + frames) / (2u * frames)) & 255u;
                    w[q] = pack4(b);
                }
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    unsigned b[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) b[k] = mode == 1 ? a.mx[4 * q + k] : a.mn[4 * q + k];      // (selects: no pointer into registers)
                    w[q] = pack4(b);
                }
            }
            uint8_t* op = o + (long)sg.out[s] * out_stride;
            if (nb == 16 && (reinterpret_cast<uintptr_t>(op) & 15) == 0) {
                *reinterpret_cast<uint4*>(op) = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
                for (int k = 0; k < nb; ++k) op[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
            }
        } else {                                           // (the last segment only)
            *smn = make_uint4(pack4(a.mn), pack4(a.mn + 4), pack4(a.mn + 8), pack4(a.mn + 12));
            *smx = make_uint4(pack4(a.mx), pack4(a.mx + 4), pack4(a.mx + 8), pack4(a.mx + 12));
#pragma unroll
            for (int q = 0; q < 4; ++q) ssm[q] = make_uint4(a.sm[4 * q], a.sm[4 * q + 1], a.sm[4 * q + 2], a.sm[4 * q + 3]);
        }
    }
    // the stores: batch frames rel = store_rel .. n into their slots, IV_DEPTH loads in flight
    if (store_rel > n) return;
    int sidx = (int)(((unsigned)base + (unsigned)store_rel) % (unsigned)cap);
    for (int r0 = store_rel; r0 <= n; r0 += IV_DEPTH) {
        Raw<WIDE> raw[IV_DEPTH];
#pragma unroll
        for (int u = 0; u < IV_DEPTH; ++u) raw[u] = load_run<WIDE>(p + (long)(min(r0 + u, n) - 1) * fstride, nb);
#pragma unroll
        for (int u = 0; u < IV_DEPTH; ++u) {
            if (r0 + u <= n) {         // uniform
                unsigned w[4];
                unpack<WIDE>(raw[u], w);
                *reinterpret_cast<uint4*>(ring + (long)sidx * slot) = make_uint4(w[0], w[1], w[2], w[3]);
                sidx = sidx + 1 == cap ? 0 : sidx + 1;
            }
        }
    }
}

// src, rb, cpr, items, plane as for interval_accumulate_kernel; the ring starts 6 planes into the state and a slot is one plane.
template <bool WIDE>
__global__ __launch_bounds__(IV_THREADS) void interval_stream_kernel(const uint8_t* __restrict__ src, int n, long pitch, long fstride, int rb,
                                                                     unsigned cpr, unsigned items, uint8_t* state, long plane, int cap,
                                                                     int base, const StreamSegs sg, int nseg, int store_rel, int mode,
                                                                     uint8_t* __restrict__ out, long out_pitch, long out_stride) {
    const unsigned i = blockIdx.x * IV_THREADS + threadIdx.x;
    if (i >= items) return;
    const unsigned r = i / cpr, c = i - r * cpr;
    const int nb = min(16, rb - 16 * (int)c);
    uint4* smn = reinterpret_cast<uint4*>(state + (long)i * 16);
    uint4* smx = reinterpret_cast<uint4*>(state + plane + (long)i * 16);
    uint4* ssm = reinterpret_cast<uint4*>(state + 2 * plane + (long)i * 64);
    uint8_t* ring = state + 6 * plane + (long)i * 16;
    const uint8_t* p = src + (long)r * pitch + 16 * (long)c;
    uint8_t* o = out + (long)r * out_pitch + 16 * (long)c;
    if (WIDE && nb == 16)
        stream_lane<true>(p, n, fstride, nb, ring, plane, cap, base, sg, nseg, store_rel, mode, smn, smx, ssm, o, out_stride);
    else
        stream_lane<false>(p, n, fstride, nb, ring, plane, cap, base, sg, nseg, store_rel, mode, smn, smx, ssm, o, out_stride);
}

// ---- interval rank ----------------------------------------------------------------------------------------------------------
// The samples of the run of nb bytes at p in frames 0 .. n - 1, slots from n on 0xFF bytes.  WIDE: p and fstride are 4-byte aligned and
// a slot is one aligned dword.  General: the aligned dwords around the run (the second one only where it holds a byte of the run,
// else the first again), the loads of up to 32 frames issued before the first is shifted into place.  Bytes of a slot beyond nb come
// out as whatever those dwords held: they are never stored.
// n sits in a vector register: the compiler then masks the lanes of each load (all or none) instead of branching around it; with a
// chain of uniform branches it waited for each load before it issued the next.  No load is issued beyond the n frames.
template <int KB, bool WIDE>
__device__ __forceinline__ void load_samples(unsigned (&s)[KB], const uint8_t* p, int n, long fstride, int nb) {
    int nv = n;
    asm volatile("" : "+v"(nv));
    if (WIDE) {
#pragma unroll
        for (int f = 0; f < KB; ++f) {
            s[f] = 0xFFFFFFFFu;
            if (f < nv) s[f] = *reinterpret_cast<const unsigned*>(p);
            p += fstride;
        }
    } else {
        // 32 frames at a time: their 64 raw dwords beside the slots already shifted into place stay near 100 registers at KB = 64
        constexpr int CH = KB < 32 ? KB : 32;
        const unsigned p0 = (unsigned)reinterpret_cast<uintptr_t>(p), fs = (unsigned)fstride;       // the low bits are all sh needs
#pragma unroll
        for (int c0 = 0; c0 < KB; c0 += CH) {
            unsigned hi[CH];
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int f = c0 + u;
                const unsigned sh = (p0 + (unsigned)f * fs) & 3u;
                s[f] = hi[u] = 0xFFFFFFFFu;
                if (f < nv) {
                    const unsigned* q = reinterpret_cast<const unsigned*>(p - sh);
                    s[f] = q[0];
                    hi[u] = q[sh + (unsigned)nb > 4u ? 1 : 0];
                }
                p += fstride;
            }
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int f = c0 + u;
                const unsigned sh = (p0 + (unsigned)f * fs) & 3u;
                s[f] = (unsigned)((((unsigned long long)hi[u] << 32) | s[f]) >> (8 * sh));
            }
        }
    }
}

// Element `rank` of the ascending sort of byte SHIFT / 8 of the KB samples.
template <int KB, int SHIFT>
__device__ __forceinline__ unsigned select_byte(const unsigned (&s)[KB], unsigned rank) {
    unsigned v[KB];
#pragma unroll
    for (int f = 0; f < KB; ++f) v[f] = (s[f] >> SHIFT) & 255u;
    unsigned t = 0;
#pragma unroll
    for (unsigned bit = 128; bit; bit >>= 1) {
        const unsigned cand = t | bit;
        unsigned below = 0;
#pragma unroll
        for (int f = 0; f < KB; ++f) below += v[f] < cand ? 1u : 0u;
        t = below <= rank ? cand : t;
    }
    return t;
}

// src points at byte 3 x0 of row y0 of frame 0; rb = 3 area_w bytes per row in dpr = ceil(rb / 4) dwords; items = area_h * dpr;
// 1 <= n <= KB, n <= 63, rank < n.
template <int KB, bool WIDE>
__global__ __launch_bounds__(IV_THREADS) void interval_rank_kernel(const uint8_t* __restrict__ src, int n, long pitch, long fstride, int rb,
                                                                   unsigned dpr, unsigned items, unsigned rank, uint8_t* __restrict__ out,
                                                                   long out_pitch) {
    const unsigned i = blockIdx.x * IV_THREADS + threadIdx.x;
    if (i >= items) return;
    const unsigned r = i / dpr, c = i - r * dpr;
    const int nb = min(4, rb - 4 * (int)c);
    const uint8_t* p = src + (long)r * pitch + 4 * (long)c;
    unsigned s[KB];
    load_samples<KB, WIDE>(s, p, n, fstride, nb);
    const unsigned b0 = select_byte<KB, 0>(s, rank), b1 = select_byte<KB, 8>(s, rank), b2 = select_byte<KB, 16>(s, rank),
                   b3 = select_byte<KB, 24>(s, rank);
    const unsigned w = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
    uint8_t* o = out + (long)r * out_pitch + 4 * (long)c;
    if (nb == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        *reinterpret_cast<unsigned*>(o) = w;
    } else {
        for (int k = 0; k < nb; ++k) o[k] = (uint8_t)(w >> (8 * k));
    }
}

template <int KB>
void launch_rank(bool wide, dim3 grid, hipStream_t st, const uint8_t* src, int n, long pitch, long fstride, int rb, unsigned dpr, unsigned items,
                 unsigned rank, uint8_t* out, long out_pitch) {
    if (wide)
        hipLaunchKernelGGL((interval_rank_kernel<KB, true>), grid, dim3(IV_THREADS), 0, st, src, n, pitch, fstride, rb, dpr, items, rank, out,
                           out_pitch);
    else
        hipLaunchKernelGGL((interval_rank_kernel<KB, false>), grid, dim3(IV_THREADS), 0, st, src, n, pitch, fstride, rb, dpr, items, rank, out,
                           out_pitch);
}

// ---- interval ring rank -------------------------------------------------------------------------------------------------------
// vse_interval_ring_rank: the rank kernel above on samples that are not evenly strided: the frames a group names sit in the ring
// of a vse_interval_stream state (frame f in slot f % cap), so consecutive samples are slots apart by whatever the sampling and the
// wrap make of them.  The host turns frame numbers into slots; the table of all groups travels as a kernel argument (uniform, read
// through scalar loads, as StreamSegs), indexed by blockIdx.y.  A lane owns one aligned dword of a slot row for all samples of its
// group: slot rows are padded to 16 bytes, so there is the wide load only.  One launch serves groups of any n: the kernel is
// instantiated for the bucket KB of the LARGEST n of the call and holds the bodies of the buckets up to it behind uniform branches, so
// a group of 5 samples beside one of 63 does the compares of 8 slots, in the registers of 64.  Only the ring is read; nothing but the
// patches is written.
// Resource report (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): interval_ring_rank_kernel<8> 19 VGPRs, <16> 29,
// <32> 45, <64> 77; 0 bytes of scratch and of LDS each, no dynamic stack: the dynamic group index stays a scalar offset into
// the kernel arguments.
struct RingGroups {
    int n[VSE_INTERVAL_RING_MAX_GROUPS], rank[VSE_INTERVAL_RING_MAX_GROUPS], out[VSE_INTERVAL_RING_MAX_GROUPS];
    int slot[VSE_INTERVAL_RING_MAX_GROUPS][64];       // slot of sample k; from n on unused (63 samples at most: the last is never read)
};

// p = this lane's dword in slot 0, plane = bytes from one slot to the next.  The loads as load_samples<KB, true> issues them: n in a
// vector register, so none beyond the n samples.
template <int KB>
__device__ __forceinline__ unsigned ring_rank_dword(const uint8_t* p, long plane, const int (&slot)[64], int n, unsigned rank) {
    unsigned s[KB];
    int nv = n;
    asm volatile("" : "+v"(nv));
    // 16 slots at a time are fetched into scalar registers before the first masked load that needs one: left inside the masked
    // blocks, every scalar load was waited for on its own, sample after sample.
    constexpr int CH = KB < 16 ? KB : 16;
#pragma unroll
    for (int c0 = 0; c0 < KB; c0 += CH) {
        int sl[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            sl[u] = slot[c0 + u];
            asm volatile("" : "+s"(sl[u]));
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            s[c0 + u] = 0xFFFFFFFFu;
            if (c0 + u < nv) s[c0 + u] = *reinterpret_cast<const unsigned*>(p + (long)sl[u] * plane);
        }
    }
    const unsigned b0 = select_byte<KB, 0>(s, rank), b1 = select_byte<KB, 8>(s, rank), b2 = select_byte<KB, 16>(s, rank),
                   b3 = select_byte<KB, 24>(s, rank);
    return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
}

// The smallest bucket of 8 .. KB that holds n (uniform branches).
template <int KB>
__device__ __forceinline__ unsigned ring_rank_bucket(const uint8_t* p, long plane, const int (&slot)[64], int n, unsigned rank) {
    if constexpr (KB > 8) {
        if (n <= KB / 2) return ring_rank_bucket<KB / 2>(p, plane, slot, n, rank);
    }
    return ring_rank_dword<KB>(p, plane, slot, n, rank);
}

// ring = slot 0 of the state's ring; rb = 3 area_w bytes per row of rb16 = 16 ceil(rb / 16) in the ring, in dpr = ceil(rb / 4) dwords;
// items = area_h * dpr; plane = area_h * rb16.  grid.y = groups; every group's n <= KBMAX.
template <int KBMAX>
__global__ __launch_bounds__(IV_THREADS) void interval_ring_rank_kernel(const uint8_t* __restrict__ ring, long plane, int rb, unsigned rb16,
                                                                        unsigned dpr, unsigned items, const RingGroups rg,
                                                                        uint8_t* __restrict__ out, long out_pitch, long out_stride) {
    const unsigned i = blockIdx.x * IV_THREADS + threadIdx.x;
    if (i >= items) return;
    const unsigned g = blockIdx.y;
    const int n = rg.n[g];
    const unsigned rank = (unsigned)rg.rank[g];
    const unsigned r = i / dpr, c = i - r * dpr;
    const int nb = min(4, rb - 4 * (int)c);
    const uint8_t* p = ring + (long)r * rb16 + 4 * (long)c;
    const unsigned w = ring_rank_bucket<KBMAX>(p, plane, rg.slot[g], n, rank);
    uint8_t* o = out + (long)rg.out[g] * out_stride + (long)r * out_pitch + 4 * (long)c;
    if (nb == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        *reinterpret_cast<unsigned*>(o) = w;
    } else {
        for (int k = 0; k < nb; ++k) o[k] = (uint8_t)(w >> (8 * k));
    }
}

// rows padded to whole runs; 0 where the area is empty or its runs do not fit the 32-bit work-item index
size_t row_bytes16(int area_w) { return (((size_t)area_w * 3 + 15) / 16) * 16; }
bool area_fits(int area_h, int area_w) {
    return area_h >= 1 && area_w >= 1 && (size_t)area_h * (row_bytes16(area_w) / 16) <= 0x7fffffffu;
}
bool multiple16(int64_t v) { return (v & 15) == 0; }
bool multiple4(int64_t v) { return (v & 3) == 0; }

}  // namespace

extern "C" {

size_t vse_interval_state_bytes(int area_h, int area_w) {
    if (!area_fits(area_h, area_w)) return 0;
    return (size_t)area_h * row_bytes16(area_w) * 6;
}

int vse_interval_accumulate(vse_ctx* c, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride, int y0, int y1,
                            int x0, int x1, void* d_state, int reset, void* stream) {
    char msg[320];
    if (!c || !d_bgr || !d_state || n < 1 || n > 65535 || src_h < 1 || src_w < 1 || pitch < (int64_t)src_w * 3 ||
        (n > 1 && frame_stride < (int64_t)(src_h - 1) * pitch + (int64_t)src_w * 3) || (reinterpret_cast<uintptr_t>(d_state) & 15)) {
        snprintf(msg, sizeof msg, "vse_interval_accumulate: bad arguments (n %d of 1..65535, frame %d x %d, pitch %lld of at least 3 w, frame "
                 "stride %lld, state 16-byte aligned)", n, src_h, src_w, (long long)pitch, (long long)frame_stride);
        vse_set_error(msg);
        return VSE_E_INVAL;
    }
    if (y0 < 0 || x0 < 0 || y1 > src_h || x1 > src_w || y1 <= y0 || x1 <= x0 || !area_fits(y1 - y0, x1 - x0)) {
        snprintf(msg, sizeof msg, "vse_interval_accumulate: area [%d, %d) x [%d, %d) is empty or outside the %d x %d frame", y0, y1, x0, x1,
                 src_h, src_w);
        vse_set_error(msg);
        return VSE_E_INVAL;
    }
    const int ah = y1 - y0, rb = (x1 - x0) * 3;
    const unsigned cpr = (unsigned)(row_bytes16(x1 - x0) / 16), items = (unsigned)ah * cpr;
    const long plane = (long)ah * (long)cpr * 16;
    const uint8_t* src = reinterpret_cast<const uint8_t*>(d_bgr) + (int64_t)y0 * pitch + (int64_t)x0 * 3;
    uint8_t* state = reinterpret_cast<uint8_t*>(d_state);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((items + IV_THREADS - 1) / IV_THREADS), block(IV_THREADS);
    const bool wide = (reinterpret_cast<uintptr_t>(src) & 15) == 0 && multiple16(pitch) && (n == 1 || multiple16(frame_stride));
    if (wide)
        hipLaunchKernelGGL(interval_accumulate_kernel<true>, grid, block, 0, st, src, n, (long)pitch, (long)frame_stride, rb, cpr, items, state,
                           plane, reset);
    else
        hipLaunchKernelGGL(interval_accumulate_kernel<false>, grid, block, 0, st, src, n, (long)pitch, (long)frame_stride, rb, cpr, items, state,
                           plane, reset);
    if (hipGetLastError() != hipSuccess) {
        vse_set_error("vse_interval_accumulate: launch failed");
        return VSE_E_HIP;
    }
    return VSE_OK;
}

int vse_interval_composite(vse_ctx* c, const void* d_state, int area_h, int area_w, int frames, int mode, void* d_out, int64_t out_pitch,
                           void* stream) {
    if (!c || !d_state || !d_out || !area_fits(area_h, area_w) || frames < 1 || frames > MAX_FRAMES || mode < 0 || mode > 2 ||
        out_pitch < (int64_t)area_w * 3 || (reinterpret_cast<uintptr_t>(d_state) & 15)) {
        char msg[320];
        snprintf(msg, sizeof msg, "vse_interval_composite: bad arguments (area %d x %d, frames %d of 1..%d, mode %d of 0 | 1 | 2, output pitch "
                 "%lld of at least 3 w, state 16-byte aligned)", area_h, area_w, frames, MAX_FRAMES, mode, (long long)out_pitch);
        vse_set_error(msg);
        return VSE_E_INVAL;
    }
    const unsigned cpr = (unsigned)(row_bytes16(area_w) / 16), items = (unsigned)area_h * cpr;
    hipLaunchKernelGGL(interval_composite_kernel, dim3((items + IV_THREADS - 1) / IV_THREADS), dim3(IV_THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const uint8_t*>(d_state), (long)area_h * (long)cpr * 16, area_w * 3,
                       cpr, items, (unsigned)frames, mode, reinterpret_cast<uint8_t*>(d_out), (long)out_pitch);
    if (hipGetLastError() != hipSuccess) {
        vse_set_error("vse_interval_composite: launch failed");
        return VSE_E_HIP;
    }
    return VSE_OK;
}

size_t vse_interval_stream_state_bytes(int area_h, int area_w, int cap) {
    if (!area_fits(area_h, area_w) || cap < 1) return 0;
    return (size_t)area_h * row_bytes16(area_w) * (6 + (size_t)cap);
}

int vse_interval_stream(vse_ctx* c, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0,
                        int x1, void* d_state, int cap, int64_t fed, const vse_interval_seg* segs, int nseg, int64_t store_from, int mode,
                        void* d_out, int64_t out_pitch, int64_t out_stride, void* stream) {
    char msg[400];
    if (!c || !d_state || n < 0 || n > 65535 || (n > 0 && !d_bgr) || src_h < 1 || src_w < 1 || pitch < (int64_t)src_w * 3 ||
        (n > 1 && frame_stride < (int64_t)(src_h - 1) * pitch + (int64_t)src_w * 3) || (reinterpret_cast<uintptr_t>(d_state) & 15)) {
        snprintf(msg, sizeof msg, "vse_interval_stream: bad arguments (n %d of 0..65535, frame %d x %d, pitch %lld of at least 3 w, frame "
                 "stride %lld, state 16-byte aligned)", n, src_h, src_w, (long long)pitch, (long long)frame_stride);
        vse_set_error(msg);
        return VSE_E_INVAL;
    }
    if (y0 < 0 || x0 < 0 || y1 > src_h || x1 > src_w || y1 <= y0 || x1 <= x0 || !area_fits(y1 - y0, x1 - x0)) {
        snprintf(msg, sizeof msg, "vse_interval_stream: area [%d, %d) x [%d, %d) is empty or outside the %d x %d frame", y0, y1, x0, x1, src_h,
                 src_w);
        vse_set_error(msg);
        return VSE_E_INVAL;
    }
    if (cap < 1 || fed < 0 || fed > ((int64_t)1 << 62) || nseg < 0 || nseg > VSE_INTERVAL_STREAM_MAX_SEGS || (nseg > 0 && !segs) || mode < 0 ||
        mode > 2) {
        snprintf(msg, sizeof msg, "vse_interval_stream: cap %d of at least 1, fed %lld of 0..2^62, %d segments of 0..%d, mode %d of 0 | 1 | 2",
                 cap, (long long)fed, nseg, VSE_INTERVAL_STREAM_MAX_SEGS, mode);
        vse_set_error(msg);
        return VSE_E_INVAL;
    }
    StreamSegs sg = {};
    int64_t prev = fed - cap;                 // every frame read is behind this one
    for (int s = 0; s < nseg; ++s) {
        const vse_interval_seg& g = segs[s];
        const bool emit = g.flags & VSE_INTERVAL_SEG_EMIT;
        const char* bad = nullptr;
        if (g.first > g.last || g.first < 1 || g.first <= prev || g.last > fed + n)
            bad = "its frames (1-based) must ascend behind the segment before it inside (fed - cap, fed + n]";
        else if (g.flags & ~(VSE_INTERVAL_SEG_CONTINUE | VSE_INTERVAL_SEG_EMIT))
            bad = "unknown flags";
        else if ((g.flags & VSE_INTERVAL_SEG_CONTINUE) && s != 0)
            bad = "only the first segment may CONTINUE";
        else if (!emit && s != nseg - 1)
            bad = "only the last segment may lack EMIT";
        else if (emit && (!d_out || g.out < 0 || out_pitch < (int64_t)(x1 - x0) * 3))
            bad = "an EMIT needs d_out, out >= 0 and out_pitch of at least 3 area_w";
        else if (emit && mode == 2 && (g.frames < 1 || g.frames > MAX_FRAMES))
            bad = "frames of a mean must be 1..4194304";
        if (bad) {
            snprintf(msg, sizeof msg, "vse_interval_stream: segment %d (frames %lld..%lld, flags %d, frames %d, out %d; fed %lld, n %d, cap %d): %s",
                     s, (long long)g.first, (long long)g.last, g.flags, g.frames, g.out, (long long)fed, n, cap, bad);
            vse_set_error(msg);
            return VSE_E_INVAL;
        }
        prev = g.last;
        sg.lo[s] = (int)(g.first - fed), sg.hi[s] = (int)(g.last - fed);         // in (-cap, n]
        sg.flags[s] = g.flags, sg.frames[s] = emit && mode == 2 ? g.frames : 1, sg.out[s] = emit ? g.out : 0;
    }
    const int64_t from = store_from > fed + 1 ? store_from : fed + 1;
    const int store_rel = from > fed + n ? n + 1 : (int)(from - fed);            // 1 .. n + 1
    if (nseg == 0 && store_rel > n) return VSE_OK;                               // nothing to read, nothing to store
    const int ah = y1 - y0, rb = (x1 - x0) * 3;
    const unsigned cpr = (unsigned)(row_bytes16(x1 - x0) / 16), items = (unsigned)ah * cpr;
    const long plane = (long)ah * (long)cpr * 16;
    const uint8_t* src = n ? reinterpret_cast<const uint8_t*>(d_bgr) + (int64_t)y0 * pitch + (int64_t)x0 * 3 : nullptr;
    const long kp = n ? (long)pitch : 0, ks = n > 1 ? (long)frame_stride : 0;    // (no stride to speak of without frames)
    const dim3 grid((items + IV_THREADS - 1) / IV_THREADS), block(IV_THREADS);
    const bool wide = n > 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0 && multiple16(pitch) && (n == 1 || multiple16(frame_stride));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    uint8_t* state = reinterpret_cast<uint8_t*>(d_state);
    uint8_t* out = reinterpret_cast<uint8_t*>(d_out);
    const int base = (int)(fed % cap);
    if (wide)
        hipLaunchKernelGGL(interval_stream_kernel<true>, grid, block, 0, st, src, n, kp, ks, rb, cpr, items, state, plane, cap, base, sg, nseg,
                           store_rel, mode, out, (long)out_pitch, (long)out_stride);
    else
        hipLaunchKernelGGL(interval_stream_kernel<false>, grid, block, 0, st, src, n, kp, ks, rb, cpr, items, state, plane, cap, base, sg, nseg,
                           store_rel, mode, out, (long)out_pitch, (long)out_stride);
    if (hipGetLastError() != hipSuccess) {
        vse_set_error("vse_interval_stream: launch failed");
        return VSE_E_HIP;
    }
    return VSE_OK;
}

int vse_interval_rank(vse_ctx* c, const void* d_bgr, int n, int src_h, int src_w, int64_t pitch, int64_t frame_stride, int y0, int y1, int x0,
                      int x1, int rank, void* d_out, int64_t out_pitch, void* stream) {
    char msg[320];
    if (!c || !d_bgr || !d_out || n < 1 || n > VSE_INTERVAL_RANK_MAX || src_h < 1 || src_w < 1 || pitch < (int64_t)src_w * 3 ||
        (n > 1 && frame_stride < (int64_t)(src_h - 1) * pitch + (int64_t)src_w * 3)) {
        snprintf(msg, sizeof msg, "vse_interval_rank: bad arguments (n %d of 1..%d, frame %d x %d, pitch %lld of at least 3 w, frame stride %lld, "
                 "an output)", n, VSE_INTERVAL_RANK_MAX, src_h, src_w, (long long)pitch, (long long)frame_stride);
        vse_set_error(msg);
        return VSE_E_INVAL;
    }
    if (y0 < 0 || x0 < 0 || y1 > src_h || x1 > src_w || y1 <= y0 || x1 <= x0 || !area_fits(y1 - y0, x1 - x0) ||
        (size_t)(y1 - y0) * (((size_t)(x1 - x0) * 3 + 3) / 4) > 0x7fffffffu) {
        snprintf(msg, sizeof msg, "vse_interval_rank: area [%d, %d) x [%d, %d) is empty or outside the %d x %d frame", y0, y1, x0, x1, src_h,
                 src_w);
        vse_set_error(msg);
        return VSE_E_INVAL;
    }
    if (rank < 0 || rank >= n || out_pitch < (int64_t)(x1 - x0) * 3) {
        snprintf(msg, sizeof msg, "vse_interval_rank: rank %d of 0..%d, output pitch %lld of at least 3 area_w = %d", rank, n - 1,
                 (long long)out_pitch, (x1 - x0) * 3);
        vse_set_error(msg);
        return VSE_E_INVAL;
    }
    const int ah = y1 - y0, rb = (x1 - x0) * 3;
    const unsigned dpr = (unsigned)((rb + 3) / 4), items = (unsigned)ah * dpr;
    const uint8_t* src = reinterpret_cast<const uint8_t*>(d_bgr) + (int64_t)y0 * pitch + (int64_t)x0 * 3;
    uint8_t* out = reinterpret_cast<uint8_t*>(d_out);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((items + IV_THREADS - 1) / IV_THREADS);
    const bool wide = (reinterpret_cast<uintptr_t>(src) & 3) == 0 && multiple4(pitch) && (n == 1 || multiple4(frame_stride));
    if (n <= 8)
        launch_rank<8>(wide, grid, st, src, n, (long)pitch, (long)frame_stride, rb, dpr, items, (unsigned)rank, out, (long)out_pitch);
    else if (n <= 16)
        launch_rank<16>(wide, grid, st, src, n, (long)pitch, (long)frame_stride, rb, dpr, items, (unsigned)rank, out, (long)out_pitch);
    else if (n <= 32)
        launch_rank<32>(wide, grid, st, src, n, (long)pitch, (long)frame_stride, rb, dpr, items, (unsigned)rank, out, (long)out_pitch);
    else
        launch_rank<64>(wide, grid, st, src, n, (long)pitch, (long)frame_stride, rb, dpr, items, (unsigned)rank, out, (long)out_pitch);
    if (hipGetLastError() != hipSuccess) {
        vse_set_error("vse_interval_rank: launch failed");
        return VSE_E_HIP;
    }
    return VSE_OK;
}

int vse_interval_ring_rank(vse_ctx* c, const void* d_state, int area_h, int area_w, int cap, int64_t fed, const vse_interval_ring_group* groups,
                           int ngroups, void* d_out, int64_t out_pitch, int64_t out_stride, void* stream) {
    char msg[400];
    if (!c || !d_state || (reinterpret_cast<uintptr_t>(d_state) & 15) || !d_out || !area_fits(area_h, area_w) ||
        (size_t)area_h * (((size_t)area_w * 3 + 3) / 4) > 0x7fffffffu || cap < 1 || fed < 0 || fed > ((int64_t)1 << 62) || ngroups < 0 ||
        ngroups > VSE_INTERVAL_RING_MAX_GROUPS || (ngroups > 0 && !groups) || out_pitch < (int64_t)area_w * 3) {
        snprintf(msg, sizeof msg, "vse_interval_ring_rank: bad arguments (a state, 16-byte aligned, and an output; area %d x %d, cap %d of at "
                 "least 1, fed %lld of 0..2^62, %d groups of 0..%d, output pitch %lld of at least 3 area_w)", area_h, area_w, cap,
                 (long long)fed, ngroups, VSE_INTERVAL_RING_MAX_GROUPS, (long long)out_pitch);
        vse_set_error(msg);
        return VSE_E_INVAL;
    }
    RingGroups rg = {};
    int nmax = 0;
    for (int g = 0; g < ngroups; ++g) {
        const vse_interval_ring_group& q = groups[g];
        const char* bad = nullptr;
        if (q.n < 1 || q.n > VSE_INTERVAL_RANK_MAX)
            bad = "n must be 1..VSE_INTERVAL_RANK_MAX";
        else if (q.rank < 0 || q.rank >= q.n)
            bad = "rank must be 0..n - 1";
        else if (q.out < 0)
            bad = "out must not be negative";
        int64_t prev = fed - cap > 0 ? fed - cap : 0;         // every frame named is behind this one (and 1-based)
        for (int k = 0; !bad && k < q.n; ++k) {
            if (q.frames[k] <= prev || q.frames[k] > fed) bad = "its frames (1-based) must ascend strictly inside (fed - cap, fed]";
            prev = q.frames[k];
        }
        if (bad) {
            snprintf(msg, sizeof msg, "vse_interval_ring_rank: group %d (n %d, rank %d, out %d; fed %lld, cap %d): %s", g, q.n, q.rank, q.out,
                     (long long)fed, cap, bad);
            vse_set_error(msg);
            return VSE_E_INVAL;
        }
        rg.n[g] = q.n, rg.rank[g] = q.rank, rg.out[g] = q.out;
        for (int k = 0; k < q.n; ++k) rg.slot[g][k] = (int)(q.frames[k] % cap);
        nmax = q.n > nmax ? q.n : nmax;
    }
    if (ngroups == 0) return VSE_OK;
    const int rb = area_w * 3;
    const unsigned rb16 = (unsigned)row_bytes16(area_w), dpr = (unsigned)((rb + 3) / 4), items = (unsigned)area_h * dpr;
    const long plane = (long)area_h * (long)rb16;
    const uint8_t* ring = reinterpret_cast<const uint8_t*>(d_state) + 6 * plane;
    uint8_t* out = reinterpret_cast<uint8_t*>(d_out);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((items + IV_THREADS - 1) / IV_THREADS, (unsigned)ngroups), block(IV_THREADS);
    if (nmax <= 8)
        hipLaunchKernelGGL(interval_ring_rank_kernel<8>, grid, block, 0, st, ring, plane, rb, rb16, dpr, items, rg, out, (long)out_pitch,
                           (long)out_stride);
    else if (nmax <= 16)
        hipLaunchKernelGGL(interval_ring_rank_kernel<16>, grid, block, 0, st, ring, plane, rb, rb16, dpr, items, rg, out, (long)out_pitch,
                           (long)out_stride);
    else if (nmax <= 32)
        hipLaunchKernelGGL(interval_ring_rank_kernel<32>, grid, block, 0, st, ring, plane, rb, rb16, dpr, items, rg, out, (long)out_pitch,
                           (long)out_stride);
    else
        hipLaunchKernelGGL(interval_ring_rank_kernel<64>, grid, block, 0, st, ring, plane, rb, rb16, dpr, items, rg, out, (long)out_pitch,
                           (long)out_stride);
    if (hipGetLastError() != hipSuccess) {
        vse_set_error("vse_interval_ring_rank: launch failed");
        return VSE_E_HIP;
    }
    return VSE_OK;
}

}  // extern "C"
