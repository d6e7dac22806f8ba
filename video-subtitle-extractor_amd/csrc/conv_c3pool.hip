// 3x3 stride-1 pad-1 convolution with the 3x3 / stride-2 / pad-1 MAX-POOL that follows it taken inside the kernel (gfx950 / CDNA4).
//
// The detector's full-resolution stem writes its largest tensor (64 x 272 x 480 x 128 fp16 = 2.1 GB) only so that pool_kernel can read
// it back and keep a quarter of it.  Here the conv values of a tile go to LDS as the fp16 values the unfused conv stores, the window
// maxima are taken there, and only the pooled NHWC tile leaves the CU.  vse_runtime.hip decides at plan creation whether a conv + pool
// pair may run this way (conv_pool_select, conv_select.hip); the compiler's records and weight packing are those of the unfused pair.
//
//   K loop   = conv_patch_kernel's LIGHT form (conv_patch.hip) as it runs this layer: 8 x 32 conv pixels x BN couts per tile, 8 waves =
//              4 (rows 2w, 2w+1) x 2 (cout halves), 352-pixel patch double-buffered over 32-channel chunks, two taps per step through a
//              2-stage weight ring, F_PATCH's weight stream [chunk][tap][Np][32], taps column-major.  The same MFMAs in the same order:
//              every conv value has the bits the unfused kernel gives it.  Two blocks per CU.
//   overlap  = a pooled row 2r needs conv rows 2r-1 .. 2r+1.  With tiles of their own, an 8-row tile would yield 3 pooled rows (8 / 6 of
//              the MFMAs).  Instead a block WALKS DOWN a column strip of tiles and carries the last conv row of a tile — already reduced
//              to its column maxima, one half8 register per thread — into the next: rows are never recomputed inside a strip.  A strip
//              that does not start at the top of the map runs the tile above it first for the carry alone (1 / strip length extra).
//              Columns: a tile starts at conv column 30 tx - 1 and yields 15 pooled columns from 31 conv columns (32 / 30).
//   epilogue = after the K loop the patch and ring are free: bias / activation -> fp16 -> LDS [8][32][BN] (16-byte slots XOR-swizzled
//              by the column, conflict-free for the writers and the readers), barrier, then thread (8-channel group, pooled column, row
//              half) takes the column maxima of 5 conv rows and from them its two pooled rows, and stores 16 bytes per pooled pixel.
//              Padding positions do not take part, as in pool_kernel; the running maximum starts at -65504 as it does there.
#include "conv_common.h"

template <int BN>
__global__ __launch_bounds__(512, 4) void conv_c3pool_kernel(const ConvParams p) {
    constexpr int PTH = 8, WCO = 2;
    constexpr int TN = BN / (32 * WCO);                 // 32-cout MFMA tiles per wave
    constexpr int PPIX = 352, PNPL = 3, TPS = 2, RING = 2;
    constexpr int PW = PTW + 2, P = PW * (PTH + 2);     // 34 x 10 halo patch
    constexpr int PATCH_HALFS = PPIX * 32, WSTAGE_HALFS = TPS * BN * 32, DUMMY_HALFS = 2 * 512;
    constexpr int NCG = BN / 8;                         // 8-channel groups (16-byte slots) per pixel
    static_assert(BN == 64 || BN == 128, "cout tile");
    static_assert(PTH * PTW * BN <= 2 * PATCH_HALFS + RING * WSTAGE_HALFS + DUMMY_HALFS, "the fp16 conv tile must fit the patch + ring");
    __shared__ __attribute__((aligned(16))) half_t lds[2 * PATCH_HALFS + RING * WSTAGE_HALFS + DUMMY_HALFS + 2 * BN];   // the ONLY LDS object
    float* const sbias = reinterpret_cast<float*>(lds + 2 * PATCH_HALFS + RING * WSTAGE_HALFS + DUMMY_HALFS);
    half_t* const patch0 = lds;
    half_t* const ring0 = lds + 2 * PATCH_HALFS;
    half_t* const dummy0 = ring0 + RING * WSTAGE_HALFS;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wpx = wave / WCO, wco = wave % WCO;

    // XCD-aware bijective block order (see conv_mfma.hip): contiguous logical range per XCD, cout tiles innermost
    unsigned t = xcd_block(blockIdx.x, gridDim.x);
    const int nt = t % p.ntn;  t /= p.ntn;
    const int tx = t % p.tiles_w;  t /= p.tiles_w;
    const int seg = t % p.pool_nseg;
    const long img = t / p.pool_nseg;
    const int ox0 = tx * (PTW - 2) - 1, n0 = nt * BN;
    const int ty_first = seg * p.pool_seg, ty_end = min(ty_first + p.pool_seg, p.tiles_h);
    const int PHp = (p.OH - 1) / 2 + 1, PWp = (p.OW - 1) / 2 + 1;      // pooled map

    const int nchunks = (p.cinp + 31) >> 5;
    // (run-time tap counts, as in conv_patch_kernel: with literals hipcc unrolls the five steps of a chunk and keeps every step's
    // fragment addresses in registers the K loop does not have)
    const int taps = p.kh * p.kw, pairs = (taps + TPS - 1) / TPS;

    const int kv = (lane & 3) ^ ((lane >> 4) & 3);        // logical k-vector this lane fetches (source-side swizzle)
    const int wr = BN == 128 ? (tid >> 2) : ((tid >> 2) & 63);
    const bool wok = n0 + wr < p.Np;
    const long winc = wok ? (long)p.Np * 32 * TPS : 0;

    // fragment addressing (conv_patch.hip)
    const int fx = lane & 31, fj = lane >> 5;
    unsigned woffb[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int r = wco * (BN / WCO) + j * 32 + conv_wrow(fx);
        woffb[j] = (unsigned)(r * 64 + ((fj ^ ((r >> 2) & 3)) << 4));
    }
    const int qb0 = (2 * wpx) * PW + fx, qb1 = qb0 + PW;
    const char* const ring_b = reinterpret_cast<const char*>(ring0);

    const half_t lowest = (half_t)-65504.f;
    const half8 lowest8 = {lowest, lowest, lowest, lowest, lowest, lowest, lowest, lowest};
    half8 carry = lowest8;                              // rp == 0: column maxima of conv row 8 ty - 1 (nothing above row 0)

    conv_stage_consts<true>(sbias, p.bias, p.zero, n0, BN, p.Np, wave, lane);                      // waves 0 .. BN/64-1, once per block

    for (int ty = ty_first > 0 ? ty_first - 1 : 0; ty < ty_end; ++ty) {
        const int oy0 = ty * PTH;
        // ---- DMA source state of this tile ------------------------------------------------------------------------
        // (what only the prologue or the pool phase needs is derived from a laundered thread id inside the tile loop: hoisted out of it,
        // those values would live across the K loop, which has no register to spare)
        int ptid = tid, twave = wave;
        asm volatile("" : "+v"(ptid), "+s"(twave));
        long poff[PNPL];
        bool pok[PNPL];
#pragma unroll
        for (int j = 0; j < PNPL; ++j) {
            const int q = 16 * (twave + 8 * j) + ((ptid & 63) >> 2);    // patch pixel index; wave instruction covers 16 pixels
            const int py = q / PW, px = q - py * PW;
            const int iy = oy0 - 1 + py, ix = ox0 - 1 + px;
            pok[j] = (q < P) && (iy >= 0) && (iy < p.H) && (ix >= 0) && (ix < p.W);
            poff[j] = ((img * p.Hs + iy) * p.Ws + ix) * (long)p.in_ld + ((ptid & 3) ^ ((ptid >> 4) & 3)) * 8;
        }
        const int pwr = BN == 128 ? (ptid >> 2) : ((ptid >> 2) & 63);
        const half_t* wptr = n0 + pwr < p.Np ? p.w + (long)(n0 + pwr) * 32 + ((ptid & 3) ^ ((ptid >> 4) & 3)) * 8
                                                   + (BN == 128 ? 0 : (long)(twave >> 2) * p.Np * 32)
                                             : p.zero;
        auto issue_patch = [&](int cc, int buf) {
            half_t* base = patch0 + buf * PATCH_HALFS;
            const bool live = (cc < nchunks) && (cc * 32 + kv * 8 < p.cinp);   // channel tail of the last chunk -> zeros
#pragma unroll
            for (int j = 0; j < PNPL; ++j) {
                const half_t* src = p.zero;
                if (live && pok[j]) src = p.in + poff[j] + cc * 32;
                half_t* dst = base + (twave + 8 * j) * 16 * 32;
                if (j == PNPL - 1 && twave >= 6) { src = p.zero; dst = dummy0 + (twave - 6) * 512; }  // pixels >= 352
                glds16_asm(src, dst);
            }
        };
        auto issue_w = [&](int s) {                            // ring stage = taps 2s, 2s+1 of the packed stream
            half_t* st = ring0 + (s & (RING - 1)) * WSTAGE_HALFS;
            if constexpr (BN == 128) {                   // two taps x 128 rows: both taps from every thread
                glds16_asm(wptr, st + twave * 16 * 32);
                glds16_asm(wptr + (wok ? (long)p.Np * 32 : 0), st + BN * 32 + twave * 16 * 32);
            } else {                                     // two taps x 64 rows: waves 0-3 tap 0, waves 4-7 tap 1
                glds16_asm(wptr, st + (twave >> 2) * BN * 32 + (twave & 3) * 16 * 32);
            }
            wptr += winc;
        };
        // both rows below the map: DMA issue and barriers only; so too, in the tile a strip runs for its carry alone, every wave but
        // the two that own the tile's last row
        const bool wave_live = (oy0 + 2 * wpx) < p.OH && (ty >= ty_first || wpx == PTH / 2 - 1);

        float16v acc[2][TN];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

        issue_patch(0, 0);
        issue_w(0);

        int s = 0;
        for (int cc = 0; cc < nchunks; ++cc) {
            const char* const pb = reinterpret_cast<const char*>(patch0 + (cc & 1) * PATCH_HALFS);
            const bool klim1 = (p.cinp - cc * 32) <= 16;
            int tapoff = 0, dx = 0, dy = 0, tap = 0;           // tapoff = dy*PW + dx of tap
            half8 xc[2];                                       // row-1 fragments of the previous tap (k halves)
            xc[0] = xc[1] = half8{0, 0, 0, 0, 0, 0, 0, 0};
            for (int pr = 0; pr < pairs; ++pr, ++s) {
                // the stage consumed now is the youngest weight DMA; only the next chunk's patch DMAs, issued after it in the
                // previous step, may still fly (the pooled stores of the previous tile are older than both)
                if (pr == 1) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
                asm volatile("" ::: "memory");
                issue_w(s + 1);
                if (pr == 0) issue_patch(cc + 1, (cc + 1) & 1);
                const unsigned wsb = (unsigned)(s & (RING - 1)) * (WSTAGE_HALFS * 2);
#pragma unroll
                for (int h = 0; h < TPS; ++h) {
                    if (h >= 1 && tap >= taps) break;          // the appended zero-weight tap does no work
                    const unsigned q0 = (unsigned)(qb0 + tapoff), q1 = (unsigned)(qb1 + tapoff);
                    const unsigned a0 = (q0 << 6) + ((fj ^ ((q0 >> 2) & 3)) << 4), a1 = (q1 << 6) + ((fj ^ ((q1 >> 2) & 3)) << 4);
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        if (!wave_live) break;
                        if (ks == 1 && klim1) break;           // channel tail <= 16: upper half of the chunk is all zeros
                        half8 wf[TN], xf[2];
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            wf[j] = *reinterpret_cast<const half8*>(ring_b + wsb + h * (BN * 64) + (woffb[j] ^ (ks << 5)));
                        if (dy == 0) xf[0] = *reinterpret_cast<const half8*>(pb + (a0 ^ (ks << 5)));
                        else xf[0] = xc[ks];
                        xf[1] = *reinterpret_cast<const half8*>(pb + (a1 ^ (ks << 5)));
                        xc[ks] = xf[1];
#pragma unroll
                        for (int i = 0; i < 2; ++i)
#pragma unroll
                            for (int j = 0; j < TN; ++j)
                                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[j], xf[i], acc[i][j], 0, 0, 0);
                    }
                    if (++tap < taps) {
                        if (++dy == p.kh) { dy = 0; tapoff = ++dx; } else { tapoff += PW; }
                    }
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // drain the look-ahead and the zero-page dummies: LDS changes hands
        __syncthreads();                                        // every wave is done with the patch and the ring

        // ---- conv values -> fp16 -> LDS [row][column][BN], 16-byte slot (c / 8) ^ (column & (NCG - 1)) -------------------
        int elane = lane;
        asm volatile("" : "+v"(elane));
        const int ex = elane & 31, ej = elane >> 5;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            half_t* const px = lds + ((2 * wpx + i) * PTW + ex) * BN;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                float bias[16], v[16];
                conv_epilogue_consts(sbias, wco * (BN / WCO) + j * 32, elane, bias);
                // conv_epilogue_tile's value (no residual, no gate): + bias -> activation -> scalar affine -> activation2 -> fp16
#pragma unroll
                for (int e = 0; e < 16; ++e) v[e] = acc[i][j][e] + bias[e];
                vse_act_n(v, p.act, p.act_a, p.act_b);
                if (p.post_a != 1.f || p.post_b != 0.f) {
#pragma unroll
                    for (int e = 0; e < 16; ++e) v[e] = v[e] * p.post_a + p.post_b;
                }
                vse_act_n(v, p.act2, 0.f, 0.f);
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    const int c8 = (wco * (BN / WCO) + j * 32 + g * 16 + ej * 8) >> 3;
                    const float* w = v + g * 8;
                    *reinterpret_cast<half8*>(px + ((c8 ^ (ex & (NCG - 1))) << 3)) =
                        half8{(half_t)w[0], (half_t)w[1], (half_t)w[2], (half_t)w[3], (half_t)w[4], (half_t)w[5], (half_t)w[6], (half_t)w[7]};
                }
            }
        }
        __syncthreads();

        // ---- window maxima: thread -> (8-channel group, pooled column of the tile, row half) ---------------------------------
        int qtid = tid;
        asm volatile("" : "+v"(qtid));
        const int cg = qtid & (NCG - 1), pc = (qtid / NCG) & 15, rp = (qtid / (NCG * 16)) & 1;
        if (qtid < NCG * 32 && pc < 15) {
            // column maxima of conv row r of the tile over the pooled column's three conv columns; rows / columns off the map stay out
            auto colmax = [&](int r) {
                half8 m = lowest8;
                if (oy0 + r >= p.OH) return m;
#pragma unroll
                for (int dc = 0; dc < 3; ++dc) {
                    const int lc = 2 * pc + dc, gx = ox0 + lc;
                    if (gx < 0 || gx >= p.OW) continue;
                    m = __builtin_elementwise_max(m, *reinterpret_cast<const half8*>(lds + (r * PTW + lc) * BN + ((cg ^ (lc & (NCG - 1))) << 3)));
                }
                return m;
            };
            // rp 0: pooled rows 0, 1 of the tile = conv rows {-1 (carry), 0, 1}, {1, 2, 3}, and row 7 for the next tile's carry;
            // rp 1: pooled rows 2, 3 = conv rows {3, 4, 5}, {5, 6, 7}
            const int rb = 4 * rp;
            const half8 e = colmax(rp ? 3 : 7);
            const half8 first = rp ? e : carry;
            const half8 a = colmax(rb), b = colmax(rb + 1), c = colmax(rb + 2), d = colmax(rb + 3);
            carry = rp ? carry : e;
            const int pcol = tx * 15 + pc, prow = 4 * ty + 2 * rp;
            if (ty >= ty_first && pcol < PWp && n0 + cg * 8 < p.Np) {
                half_t* const op = reinterpret_cast<half_t*>(p.out) + ((img * PHp + prow) * PWp + pcol) * (long)p.out_ld + n0 + cg * 8;
                if (prow < PHp) *reinterpret_cast<half8*>(op) = __builtin_elementwise_max(__builtin_elementwise_max(first, a), b);
                if (prow + 1 < PHp)
                    *reinterpret_cast<half8*>(op + (long)PWp * p.out_ld) = __builtin_elementwise_max(__builtin_elementwise_max(b, c), d);
            }
        }
        __syncthreads();                                        // the next tile's DMAs overwrite the conv tile
    }
}

// Rows of tiles a block walks (conv_c3pool_kernel): whole column strips when the batch alone gives every block slot of the chip (2 x 256
// CUs) two blocks, else the fewest, longest strips that do; every strip but the topmost pays a carry-only tile, so none is shorter than 4.
// (The stem at batch 64, timed alone: 1024 blocks of 34 tiles 1.58-1.60 ms, 2048 of 17 + 1: 1.62-1.63, 4096 of 9 + 1: 1.64-1.65.)
static void conv_c3pool_strips(long images, int tiles_h, int tiles_w, int ntn, int* seg, int* nseg) {
    int n = 1;
    while (images * tiles_w * ntn * n < 1024 && (tiles_h + n) / (n + 1) >= 4) ++n;
    *seg = (tiles_h + n - 1) / n;
    *nseg = (tiles_h + *seg - 1) / *seg;
}

// arg = BN (conv_select.hip: conv_pool_select); p = the conv's parameters with p.out / p.out_ld = the POOL's output view
static const ConvInst kC3poolInst[] = {CONV_INST(128, 0, 0, conv_c3pool_kernel<128>), CONV_INST(64, 0, 0, conv_c3pool_kernel<64>)};

static int launch_conv_c3pool(const ConvParams& pin, const ConvKernel& k, hipStream_t st) {
    const ConvInst* inst = conv_inst(conv_c3pool_family(), k);
    if (!inst) return VSE_E_UNSUPPORTED;
    ConvParams p = pin;
    if (p.kh != 3 || p.kw != 3 || p.sh != 1 || p.sw != 1 || p.ph != 1 || p.pw != 1 || (p.cinp & 7) || p.inshift || p.OH != p.H || p.OW != p.W)
        return VSE_E_INVAL;
    if ((p.flags & ~F_PATCH) || p.out_f32 || p.lo_off || p.wl_out || (p.out_ld & 7) || (reinterpret_cast<uintptr_t>(p.out) & 15) || (p.Np & 7))
        return VSE_E_INVAL;
    const int bn = k.arg[0];
    p.ntn = (unsigned)((p.Np + bn - 1) / bn);
    p.tiles_h = (p.OH + 7) / 8;                                   // 4 pooled rows each
    p.tiles_w = ((p.OW - 1) / 2 + 1 + 14) / 15;                   // 15 pooled columns each
    conv_c3pool_strips(conv_images(p), p.tiles_h, p.tiles_w, (int)p.ntn, &p.pool_seg, &p.pool_nseg);
    const unsigned long long blocks = (unsigned long long)conv_images(p) * p.pool_nseg * p.tiles_w * p.ntn;
    if (blocks == 0 || blocks > 0x7fffffffull) return VSE_E_INVAL;
    hipLaunchKernelGGL(inst->fn, dim3((unsigned)blocks), dim3(512), 0, st, p);
    return hipGetLastError() == hipSuccess ? VSE_OK : VSE_E_HIP;
}
ConvFamily conv_c3pool_family() { return conv_family(launch_conv_c3pool, kC3poolInst); }
