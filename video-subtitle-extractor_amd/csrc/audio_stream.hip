// Timeline sync: a WAV's int16 PCM -> Sushi's uint8 search stream on the device (vse_audio_stream_*, include/vse_hip.h), the
// bytes vse_amd.timeline_sync.AudioStream builds on the host.  The integer form is the specification (tests/audio_stream_ref.py
// restates it in numpy, byte for byte); F frames of C interleaved int16 channels at rate R, search rate S <= R:
//   sample_count = ceil(F / (double)R * S), P = 10 R, L = 20 R + sample_count, K = ceil(F / R) chunks of one second;
//   chunk k: n_k = min(R, F - k R) frames -> new_k = rint(n_k * (S / (double)R)) samples at P + k S (a full chunk gives S);
//   sample j of chunk k = the int32 sum over the channels of frame j (S == R) or of frame
//     min((int64)floor((double)j * scale_k), n_k - 1), scale_k = 1.0 / ((double)new_k / (double)n_k);
//   an element no chunk writes (the lengths can sum to one short of sample_count) is 0;
//   data[0:P] = data[P], data[L-P:L] = data[L-P-1];
//   f(s) = (float)s for C == 1, else (float)s / (float)C;  hi / lo = 3 x the median of {f(s) : s >= 0} / {f(s) : s <= 0};
//   out = (uint8)(((min(max(f(s), lo), hi) - lo) / (hi - lo)) * 255.0f + 0.5f), every float32 operation rounded on its own.
// f is monotone, so both medians are order statistics of the integers: a histogram of s + 32768 C over all L elements (uint32
// bins, integer atomics: exact and independent of arrival order) and one scan over the bins.
//
// feed    audio_stream_gather: a lane owns four consecutive stream elements at an absolute index that is a multiple of 4, so whole
//         groups leave as one 16-byte store; the groups at a chunk's ends store their elements one by one.  A frame is read with
//         4-byte loads where C is even and the piece 4-byte aligned, else with 2-byte loads; on the copy path (S == R) of mono and
//         stereo a lane's four frames are one 8- / 16-byte load where every group's address allows it.  The index arithmetic is
//         double (v_mul_f64, v_floor_f64); scale_k comes from the host.  The last chunk also writes the zeros up to sample_count.
// finish  clear the bins; audio_stream_count; audio_stream_select; audio_stream_map.
//   count   only the sample_count elements between the paddings are read (16-byte loads); each padding adds P to one bin.  Audio
//           piles up around zero, so a block keeps the 2 AS_WIN bins around zero in LDS and adds them to memory once at its end;
//           the tails go to memory directly.  A wave whose lanes all hold one value (digital silence) adds it once.
//   select  one block: per-lane sums of bin segments, a block scan, then the lanes that hold one of the four ranks walk their
//           segment; lane 0 does the float steps and writes the result record.
//   map     16 elements per lane, 16-byte loads and one 16-byte store where the output address allows it.  The paddings are the
//           index clamped to [P, L - P - 1].  Returns at once when the record's status is not 0.
// The float steps are single operations under -ffp-contract=off (the build's flag) and the bytes are packed by shifts from ints
// (see clip8 in yuv.hip for what hipcc made of packed-byte arithmetic on this target).
#include <cmath>
#include <cstdio>

#include "common.h"

void vse_set_error(const char* msg);      // vse_runtime.hip

namespace {

constexpr int AS_THREADS = 256;
constexpr int AS_WIN = 4096;              // bins each side of zero a count block keeps in LDS (32 KiB)
constexpr int AS_SCAN = 1024;             // lanes of the select block
constexpr long AS_MAX_L = 0x7fffffffL;

struct AsGeom {
    long frames, L, P, sample_count, K;
    int C, R, S;
    int n_last, new_last;                 // frames / samples of the last chunk
    double scale_full, scale_last;        // _resize_nearest's scale of a full / of the last chunk
    int zbin, seg;                        // bin of s = 0; bins per select lane (a multiple of 4)
    unsigned nbins;
    size_t samp_bytes, hist_bytes;
};

size_t as_align(size_t x) { return (x + 255) & ~(size_t)255; }

// false for what the entry points refuse: channels outside 1..8, rate < sample_rate, frames < 1, L > 2^31 - 1.
bool as_geometry(int64_t frames, int C, int R, int S, AsGeom& g) {
    if (C < 1 || C > 8 || S < 1 || R < S || frames < 1) return false;
    const double count = ceil((double)frames / (double)R * (double)S);
    if (!(count <= (double)AS_MAX_L)) return false;
    g.frames = frames;
    g.C = C, g.R = R, g.S = S;
    g.sample_count = (long)count;
    g.P = 10L * R;
    g.L = 20L * R + g.sample_count;
    if (g.L > AS_MAX_L) return false;
    g.K = (frames + R - 1) / R;
    const double ratio = (double)S / (double)R;
    g.n_last = (int)(frames - (g.K - 1) * R);
    g.new_last = (int)nearbyint((double)g.n_last * ratio);      // ties to even (the default rounding mode), as Python's round
    g.scale_full = 1.0 / ((double)S / (double)R);
    g.scale_last = g.new_last > 0 ? 1.0 / ((double)g.new_last / (double)g.n_last) : 0.0;
    g.zbin = 32768 * C;
    g.nbins = 65535u * (unsigned)C + 1u;
    g.seg = (int)(((g.nbins + AS_SCAN - 1) / AS_SCAN + 3) & ~3u);
    g.samp_bytes = as_align((size_t)g.L * 4);
    g.hist_bytes = (size_t)g.seg * AS_SCAN * 4;                // whole segments: the bins beyond nbins stay 0
    return true;
}

struct AsFeed {
    const int16_t* pcm;                   // the piece: chunk `first` starts at its first frame
    int* samp;
    long first, K, P, sample_count;
    int C, R, S, n_last, new_last, copy;
    double scale_full, scale_last;
    unsigned bpc;                         // blocks per chunk
};

// the int32 sum of one frame's channels; W = bytes per load
template <int W>
__device__ __forceinline__ int frame_sum(const int16_t* p, int C) {
    int s = 0;
    if (W == 4) {
        const int* q = reinterpret_cast<const int*>(p);
        for (int c = 0; c < (C >> 1); ++c) {
            const int v = q[c];
            s += ((v << 16) >> 16) + (v >> 16);
        }
    } else {
        for (int c = 0; c < C; ++c) s += p[c];
    }
    return s;
}

// MODE 0: 2-byte loads; 1: 4-byte loads (C even, piece 4-byte aligned); 2 / 3: as 0 / 1, and a whole group of the copy path of
// C = 1 / C = 2 is one 8- / 16-byte load (the host has checked every group's address)
template <int MODE>
__global__ __launch_bounds__(AS_THREADS) void audio_stream_gather(const AsFeed a) {
    constexpr int W = (MODE & 1) ? 4 : 2;
    const unsigned c = blockIdx.x / a.bpc, w = blockIdx.x - c * a.bpc;
    const long k = a.first + c;
    const bool last = k == a.K - 1;
    const int n_k = last ? a.n_last : a.R, new_k = last ? a.new_last : a.S;
    const double scale = last ? a.scale_last : a.scale_full;
    const long at = a.P + k * a.S, stop = a.P + a.sample_count;
    long end = last ? stop : at + new_k;                        // the last chunk zero-fills up to sample_count
    end = end < stop ? end : stop;
    const long g = (at & ~3L) + 4L * ((long)w * AS_THREADS + threadIdx.x);
    if (g >= end) return;
    const int16_t* src = a.pcm + (long)c * a.R * a.C;
    const bool whole = g >= at && g + 4 <= end;
    int v[4];
    if (MODE >= 2 && whole && g + 4 <= at + new_k) {
        const long j = g - at;
        if (MODE == 2) {
            const uint2 q = *reinterpret_cast<const uint2*>(src + j);
            v[0] = ((int)q.x << 16) >> 16, v[1] = (int)q.x >> 16;
            v[2] = ((int)q.y << 16) >> 16, v[3] = (int)q.y >> 16;
        } else {
            const uint4 q = *reinterpret_cast<const uint4*>(src + 2 * j);
            v[0] = (((int)q.x << 16) >> 16) + ((int)q.x >> 16);
            v[1] = (((int)q.y << 16) >> 16) + ((int)q.y >> 16);
            v[2] = (((int)q.z << 16) >> 16) + ((int)q.z >> 16);
            v[3] = (((int)q.w << 16) >> 16) + ((int)q.w >> 16);
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long j = g + e - at;
            v[e] = 0;
            if (j >= 0 && j < new_k) {
                long idx = j;
                if (!a.copy) {
                    idx = (long)floor((double)j * scale);
                    idx = idx < n_k - 1 ? idx : n_k - 1;
                }
                v[e] = frame_sum<W>(src + idx * a.C, a.C);
            }
        }
    }
    if (whole) {
        *reinterpret_cast<int4*>(a.samp + g) = make_int4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (g + e >= at && g + e < end) a.samp[g + e] = v[e];
    }
}

// one element into the histogram; every lane of the wave calls it (valid = this lane holds an element)
__device__ __forceinline__ void count_one(int s, bool valid, unsigned* win, unsigned* hist, int zbin, unsigned nbins) {
    valid = valid && (unsigned)(s + zbin) < nbins;              // (a value no feed wrote is not counted)
    const unsigned long long act = __ballot(valid);
    if (!act) return;
    const int lead = __ffsll((long long)act) - 1;
    const int s0 = __shfl(s, lead);
    unsigned n = 1;
    if (__ballot(valid && s == s0) == act) {                    // the whole wave holds one value: one add
        valid = (int)(threadIdx.x & 63) == lead;
        n = (unsigned)__popcll(act);
    }
    if (valid) {
        if (s > -AS_WIN && s < AS_WIN) atomicAdd(win + (s + AS_WIN), n);
        else atomicAdd(hist + (s + zbin), n);
    }
}

__global__ __launch_bounds__(AS_THREADS) void audio_stream_count(const int* samp, long P, long count, unsigned* hist, int zbin,
                                                                  unsigned nbins) {
    __shared__ unsigned win[2 * AS_WIN];
    for (int i = threadIdx.x; i < 2 * AS_WIN; i += AS_THREADS) win[i] = 0;
    __syncthreads();
    const long lo = P, hi = P + count, g0 = lo & ~3L, groups = (hi - g0 + 3) >> 2;
    for (long b = (long)blockIdx.x * AS_THREADS; b < groups; b += (long)gridDim.x * AS_THREADS) {
        const long t = b + threadIdx.x;
        const bool in = t < groups;
        const long i = g0 + 4 * t;
        int4 v = make_int4(0, 0, 0, 0);
        if (in) v = *reinterpret_cast<const int4*>(samp + i);
        count_one(v.x, in && i >= lo && i < hi, win, hist, zbin, nbins);
        count_one(v.y, in && i + 1 >= lo && i + 1 < hi, win, hist, zbin, nbins);
        count_one(v.z, in && i + 2 >= lo && i + 2 < hi, win, hist, zbin, nbins);
        count_one(v.w, in && i + 3 >= lo && i + 3 < hi, win, hist, zbin, nbins);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {                  // the paddings: P copies of the first and of the last element
        const int a = samp[lo], z = samp[hi - 1];
        if ((unsigned)(a + zbin) < nbins) atomicAdd(hist + (a + zbin), (unsigned)P);
        if ((unsigned)(z + zbin) < nbins) atomicAdd(hist + (z + zbin), (unsigned)P);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * AS_WIN; i += AS_THREADS) {
        const unsigned n = win[i];
        if (n) atomicAdd(hist + (i - AS_WIN + zbin), n);
    }
}

__device__ __forceinline__ float level(int s, int C) { return C == 1 ? (float)s : __fdiv_rn((float)s, (float)C); }

// 3 x the median of a set of n values whose elements of ranks n/2 - 1 (even n only) and n/2 are a and b
__device__ __forceinline__ float median3(unsigned n, int a, int b, int C) {
    const float m = (n & 1) ? level(b, C) : __fdiv_rn(__fadd_rn(level(a, C), level(b, C)), 2.0f);
    return __fmul_rn(m, 3.0f);
}

__global__ __launch_bounds__(AS_SCAN) void audio_stream_select(const unsigned* hist, int seg, int zbin, int C,
                                                               vse_audio_stream_result* res) {
    __shared__ unsigned wave_sum[AS_SCAN / 64];
    __shared__ unsigned sh[8];                                  // 0: count below zero, 1: count of zero, 2: total, 4..7: rank bins
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned* mine = hist + (long)tid * seg;
    unsigned sum = 0;
    for (int q = 0; q < seg; q += 4) {
        const uint4 v = *reinterpret_cast<const uint4*>(mine + q);
        sum += v.x + v.y + v.z + v.w;
    }
    unsigned inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned t = __shfl_up(inc, o);
        if (lane >= o) inc += t;
    }
    if (lane == 63) wave_sum[wv] = inc;
    __syncthreads();
    unsigned excl = inc - sum;
    for (int i = 0; i < wv; ++i) excl += wave_sum[i];
    if (tid == AS_SCAN - 1) sh[2] = excl + sum;
    if (zbin / seg == tid) {
        unsigned below = excl;
        for (int b = tid * seg; b < zbin; ++b) below += hist[b];
        sh[0] = below;
        sh[1] = hist[zbin];
    }
    __syncthreads();
    const unsigned below = sh[0], n_le0 = below + sh[1], n_ge0 = sh[2] - below;
    // the element of rank r of the <= 0 set is the first bin whose inclusive running count exceeds r; of the >= 0 set, r + below
    unsigned want[4];
    want[0] = (n_le0 & 1) ? n_le0 / 2 : n_le0 / 2 - 1;
    want[1] = n_le0 / 2;
    want[2] = below + ((n_ge0 & 1) ? n_ge0 / 2 : n_ge0 / 2 - 1);
    want[3] = below + n_ge0 / 2;
    bool holds = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool set = i < 2 ? n_le0 > 0 : n_ge0 > 0;
        holds = holds || (set && want[i] >= excl && want[i] - excl < sum);
    }
    if (holds) {
        unsigned run = excl;
        for (int q = 0; q < seg; ++q) {
            const unsigned next = run + mine[q];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if ((i < 2 ? n_le0 > 0 : n_ge0 > 0) && want[i] >= run && want[i] < next) sh[4 + i] = (unsigned)(tid * seg + q);
            run = next;
        }
    }
    __syncthreads();
    if (tid == 0) {
        float lo = __uint_as_float(0x7fc00000u), hi = lo;
        if (n_le0) lo = median3(n_le0, (int)sh[4] - zbin, (int)sh[5] - zbin, C);
        if (n_ge0) hi = median3(n_ge0, (int)sh[6] - zbin, (int)sh[7] - zbin, C);
        const bool ok = n_le0 && n_ge0 && __fsub_rn(hi, lo) != 0.0f;
        res->lo_bits = __float_as_uint(lo);
        res->hi_bits = __float_as_uint(hi);
        res->count_ge0 = n_ge0;
        res->count_le0 = n_le0;
        res->status = ok ? 0 : 1;
        res->reserved[0] = res->reserved[1] = res->reserved[2] = 0;
    }
}

__device__ __forceinline__ unsigned map_one(int s, int C, float lo, float hi, float range) {
    float x = level(s, C);
    x = fminf(fmaxf(x, lo), hi);
    const float y = __fadd_rn(__fmul_rn(__fdiv_rn(__fsub_rn(x, lo), range), 255.0f), 0.5f);
    return (unsigned)(int)y;
}

// lane t owns the 16 elements from 16 t - mis, mis = the output address & 15: whole groups are one aligned 16-byte store.
// VEC: mis is a multiple of 4, so a group between the paddings is four aligned 16-byte loads.
template <bool VEC>
__global__ __launch_bounds__(AS_THREADS) void audio_stream_map(const int* samp, long P, long L, int C, const vse_audio_stream_result* res,
                                                                uint8_t* out, int mis) {
    if (res->status != 0) return;
    const float lo = __uint_as_float(res->lo_bits), hi = __uint_as_float(res->hi_bits), range = __fsub_rn(hi, lo);
    const long e0 = 16L * ((long)blockIdx.x * AS_THREADS + threadIdx.x) - mis;
    if (e0 >= L) return;
    const long ilo = P, ihi = L - P - 1;
    int s[16];
    if (VEC && e0 >= ilo && e0 + 15 <= ihi) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int4 v = *reinterpret_cast<const int4*>(samp + e0 + 4 * q);
            s[4 * q] = v.x, s[4 * q + 1] = v.y, s[4 * q + 2] = v.z, s[4 * q + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            long i = e0 + e;
            i = i < ilo ? ilo : i;
            i = i > ihi ? ihi : i;
            s[e] = samp[i];
        }
    }
    unsigned w[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        w[q] = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[q] |= (map_one(s[4 * q + e], C, lo, hi, range) & 255u) << (8 * e);
    }
    if (e0 >= 0 && e0 + 16 <= L) {
        *reinterpret_cast<uint4*>(out + e0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int e = 0; e < 16; ++e)
            if (e0 + e >= 0 && e0 + e < L) out[e0 + e] = (uint8_t)(w[e >> 2] >> (8 * (e & 3)));
    }
}

int refuse(const char* msg) {
    vse_set_error(msg);
    return VSE_E_INVAL;
}

// the checks feed and finish share -> VSE_OK with g filled
int as_check(const char* who, vse_ctx* c, int64_t frames, int channels, int rate, int sample_rate, const void* d_ws, size_t ws_bytes,
             AsGeom& g) {
    char msg[320];
    if (!c || !as_geometry(frames, channels, rate, sample_rate, g)) {
        snprintf(msg, sizeof msg, "%s: bad arguments (%lld frames of at least 1, %d channels of 1..8, rate %d of at least the search rate "
                 "%d, stream length of at most 2^31 - 1)", who, (long long)frames, channels, rate, sample_rate);
        return refuse(msg);
    }
    if (!d_ws || (reinterpret_cast<uintptr_t>(d_ws) & 255) || ws_bytes < g.samp_bytes + g.hist_bytes) {
        snprintf(msg, sizeof msg, "%s: the workspace must be 256-byte aligned and hold %zu bytes (%zu given)", who,
                 g.samp_bytes + g.hist_bytes, ws_bytes);
        return refuse(msg);
    }
    if (g.new_last == 0 && sample_rate != rate) {
        snprintf(msg, sizeof msg, "%s: the last %d frames are too few to resample", who, g.n_last);
        return refuse(msg);
    }
    return VSE_OK;
}

int low_bit(uintptr_t v) { return (int)(v & (~v + 1)); }

}  // namespace

extern "C" {

int64_t vse_audio_stream_length(int64_t frames, int channels, int rate, int sample_rate) {
    AsGeom g;
    return as_geometry(frames, channels, rate, sample_rate, g) ? g.L : 0;
}

size_t vse_audio_stream_workspace_bytes(int64_t frames, int channels, int rate, int sample_rate) {
    AsGeom g;
    return as_geometry(frames, channels, rate, sample_rate, g) ? g.samp_bytes + g.hist_bytes : 0;
}

int vse_audio_stream_feed(vse_ctx* c, const int16_t* d_pcm, int64_t piece_frames, int64_t first_second, int64_t frames, int channels,
                          int rate, int sample_rate, void* d_ws, size_t ws_bytes, void* stream) {
    AsGeom g;
    const int rc = as_check("vse_audio_stream_feed", c, frames, channels, rate, sample_rate, d_ws, ws_bytes, g);
    if (rc != VSE_OK) return rc;
    char msg[320];
    if (!d_pcm || (reinterpret_cast<uintptr_t>(d_pcm) & 1) || piece_frames < 1 || first_second < 0 || first_second >= g.K ||
        piece_frames > frames - first_second * rate || (piece_frames % rate != 0 && first_second * rate + piece_frames != frames)) {
        snprintf(msg, sizeof msg, "vse_audio_stream_feed: a piece is whole seconds of 2-byte aligned PCM inside the file, only the last may "
                 "end in the partial second (%lld frames from second %lld of %lld frames at %d Hz)", (long long)piece_frames,
                 (long long)first_second, (long long)frames, rate);
        return refuse(msg);
    }
    AsFeed a;
    a.pcm = d_pcm;
    a.samp = static_cast<int*>(d_ws);
    a.first = first_second, a.K = g.K, a.P = g.P, a.sample_count = g.sample_count;
    a.C = channels, a.R = rate, a.S = sample_rate, a.n_last = g.n_last, a.new_last = g.new_last, a.copy = rate == sample_rate;
    a.scale_full = g.scale_full, a.scale_last = g.scale_last;
    a.bpc = (unsigned)(((sample_rate + 6) / 4 + AS_THREADS - 1) / AS_THREADS);
    const long chunks = (piece_frames + rate - 1) / rate;
    const long blocks = chunks * a.bpc;                         // chunks <= K <= L / S and bpc ~ S / 1024: below 2^31
    const uintptr_t base = reinterpret_cast<uintptr_t>(d_pcm);
    int mode = (channels % 2 == 0 && base % 4 == 0) ? 1 : 0;
    if (a.copy && channels <= 2) {
        // group g of chunk k starts at frame g - (P + k R) of the file's second k: address base + 2 C (g - (10 + first) R) with
        // 4 | g, so every whole group is 8 C-byte aligned iff base - 2 C (10 + first) R is
        const uintptr_t shift = (uintptr_t)2 * channels * (uintptr_t)(10 + first_second) * (uintptr_t)rate;
        if (low_bit((base - shift) | 16) >= 8 * channels) mode += 2;
    }
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks), block(AS_THREADS);
    switch (mode) {
        case 0: hipLaunchKernelGGL(audio_stream_gather<0>, grid, block, 0, st, a); break;
        case 1: hipLaunchKernelGGL(audio_stream_gather<1>, grid, block, 0, st, a); break;
        case 2: hipLaunchKernelGGL(audio_stream_gather<2>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(audio_stream_gather<3>, grid, block, 0, st, a); break;
    }
    if (hipGetLastError() != hipSuccess) {
        vse_set_error("vse_audio_stream_feed: launch failed");
        return VSE_E_HIP;
    }
    return VSE_OK;
}

int vse_audio_stream_finish(vse_ctx* c, int64_t frames, int channels, int rate, int sample_rate, void* d_ws, size_t ws_bytes,
                            uint8_t* d_out, vse_audio_stream_result* d_result, void* stream) {
    AsGeom g;
    const int rc = as_check("vse_audio_stream_finish", c, frames, channels, rate, sample_rate, d_ws, ws_bytes, g);
    if (rc != VSE_OK) return rc;
    if (!d_out || !d_result || (reinterpret_cast<uintptr_t>(d_result) & 3))
        return refuse("vse_audio_stream_finish: the output stream or the 4-byte aligned result record is missing");
    int* samp = static_cast<int*>(d_ws);
    unsigned* hist = reinterpret_cast<unsigned*>(static_cast<char*>(d_ws) + g.samp_bytes);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(hist, 0, g.hist_bytes, st) != hipSuccess) {
        vse_set_error("vse_audio_stream_finish: clearing the bins failed");
        return VSE_E_HIP;
    }
    const long groups = (g.sample_count + 6) / 4;
    const int cus = vse_cu_count();
    long blocks = (groups + AS_THREADS - 1) / AS_THREADS;
    const long cap = 2L * (cus > 0 ? cus : 256);               // two blocks (2 x 32 KiB of LDS bins) per CU, each flushed once
    blocks = blocks < cap ? blocks : cap;
    hipLaunchKernelGGL(audio_stream_count, dim3((unsigned)blocks), dim3(AS_THREADS), 0, st, samp, g.P, g.sample_count, hist, g.zbin, g.nbins);
    hipLaunchKernelGGL(audio_stream_select, dim3(1), dim3(AS_SCAN), 0, st, hist, g.seg, g.zbin, channels, d_result);
    const int mis = (int)(reinterpret_cast<uintptr_t>(d_out) & 15);
    const dim3 grid((unsigned)(((g.L + mis + 15) / 16 + AS_THREADS - 1) / AS_THREADS)), block(AS_THREADS);
    if (mis % 4 == 0)
        hipLaunchKernelGGL(audio_stream_map<true>, grid, block, 0, st, samp, g.P, g.L, channels, d_result, d_out, mis);
    else
        hipLaunchKernelGGL(audio_stream_map<false>, grid, block, 0, st, samp, g.P, g.L, channels, d_result, d_out, mis);
    if (hipGetLastError() != hipSuccess) {
        vse_set_error("vse_audio_stream_finish: launch failed");
        return VSE_E_HIP;
    }
    return VSE_OK;
}

}  // extern "C"
