// The argument checks of every entry point of csrc/yuv.hip under the host sanitizers, as a program of its own: no GPU is needed, every
// call here is refused before anything touches the device.  Build and run on any machine with hipcc:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I include tools/yuv_refusals.cpp video-subtitle-extractor_amd/csrc/yuv.hip -o yuv_refusals && ./yuv_refusals
// It prints every refusal's message (pointers as PTR, so that two revisions of yuv.hip compare line for line) and exits 0 when every call
// returned VSE_E_INVAL with a message that begins with the entry point's name and no buffer was written.  Where csrc/yuv_planes.h exists
// it then sweeps the plane geometry against the frame sizes the library reports.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <regex>
#include <string>

#include "vse_hip.h"
#if __has_include("../video-subtitle-extractor_amd/csrc/yuv_planes.h")
#include "../video-subtitle-extractor_amd/csrc/yuv_planes.h"
#define HAVE_PLANES 1
#endif

static std::string last_error;
void vse_set_error(const char* msg) { last_error = msg; }          // vse_runtime.hip's, which this program does not link

// host memory stands in for the device's: a refused call reads none of it
constexpr unsigned char FILL = 0xA5;
alignas(16) static unsigned char src[4096], out[4096], table[1024];
alignas(16) static uint32_t stats[16];
enum Where { OUT, SRC, TABLE, STATS };
static unsigned char* base(Where w) { return w == OUT ? out : w == SRC ? src : w == TABLE ? table : reinterpret_cast<unsigned char*>(stats); }

// The arguments of all entry points; each reads the ones it has.  The defaults are accepted calls: 2 pictures of 8 x 16, 10-bit planar
// 4:2:0 (384 bytes), the tests' (tests/test_gpu_*.py test_refusals_launch_nothing).  w2 / h2: the output columns of resample, rows of vscale.
struct Args {
    int n = 2, h = 8, w = 16, w2 = 24, h2 = 12, layout = 0, parity = 0, sub_x = 1, sub_y = 1, chroma = 1, depth = 10, msb = 0, matrix = 1, full = 0;
    int keep = 0, mode = 0, thresh = 10, comb_thresh = 10, comb_limit = 20, s0 = 0, s1 = 8, y0 = 0, y1 = 12, ky = 2, kc = 2;
    int64_t sstride = 384, pstride = 384, ostride = 384, pitch = 48, dstride = 8 * 16 * 3;
    long soff = 0, poff = 0, ooff = 0, stats_off = 0, ty = 0, tc = 512, tone = 0;          // ty, tc, tone: offsets into `table`, -1: no table
    Where out_in = OUT, stats_in = STATS;
    bool prev = true, null_ctx = false, null_src = false, null_out = false, null_stats = false, null_gamut = false;
    int32_t gamut[9] = {16384, 0, 0, 0, 16384, 0, 0, 0, 16384};
};
typedef void (*Change)(Args&);
struct Case {
    const char* what;
    Change change;
};
#define CASE(what, ...) {what, [](Args& a) { __VA_ARGS__; }}

static long ctx_word;
static vse_ctx* ctx_of(const Args& a) { return a.null_ctx ? nullptr : reinterpret_cast<vse_ctx*>(&ctx_word); }
static void* src_of(const Args& a) { return a.null_src ? nullptr : src + a.soff; }
static void* out_of(const Args& a) { return a.null_out ? nullptr : base(a.out_in) + a.ooff; }
static const void* tab(long off) { return off < 0 ? nullptr : table + off; }

// ---- the format's checks, which all but vse_yuv420_to_bgr share, and the lists of the tests
#define FORMAT_CASES                                                                                                                          \
    CASE("h 0", a.h = 0), CASE("w 0", a.w = 0), CASE("n 0", a.n = 0), CASE("h -1", a.h = -1), CASE("w -1", a.w = -1), CASE("n -1", a.n = -1),    \
    CASE("subsampling 0, 1", a.sub_x = 0; a.sub_y = 1), CASE("subsampling 2", a.sub_x = 2), CASE("sub_y -1", a.sub_y = -1),                    \
    CASE("chroma 3", a.chroma = 3), CASE("chroma -1", a.chroma = -1), CASE("chroma 0 with subsampling", a.chroma = 0),                          \
    CASE("semi-planar 4:2:2", a.chroma = 2; a.sub_y = 0), CASE("depth 7", a.depth = 7), CASE("depth 17", a.depth = 17),                         \
    CASE("msb at depth 8", a.depth = 8; a.msb = 1), CASE("msb 2", a.msb = 2), CASE("msb -1", a.msb = -1),                                       \
    CASE("h * w above 2^31 - 1", a.h = 1 << 16; a.w = 1 << 15), CASE("no context", a.null_ctx = true), CASE("no pictures", a.null_src = true),  \
    CASE("no output", a.null_out = true)
#define CONVERSION_CASES                                                                                                                      \
    FORMAT_CASES, CASE("matrix 3", a.matrix = 3), CASE("matrix -1", a.matrix = -1), CASE("full range 2", a.full = 2),                           \
    CASE("full range -1", a.full = -1), CASE("parity 2", a.parity = 2), CASE("parity -1", a.parity = -1),                                       \
    CASE("parity 1 without vertical subsampling", a.sub_y = 0; a.parity = 1), CASE("pitch below the row", a.pitch = 47),                        \
    CASE("stride below the frame", a.sstride = 382), CASE("odd stride", a.sstride = 385), CASE("odd base", a.soff = 1),                         \
    CASE("output stride below the frame", a.dstride = 383), CASE("output stride below the pitched frame", a.pitch = 52; a.dstride = 7 * 52 + 47)
#define FIELDS_CASES                                                                                                                          \
    FORMAT_CASES, CASE("keep 2", a.keep = 2), CASE("keep -1", a.keep = -1), CASE("thresh -1", a.thresh = -1), CASE("thresh 256", a.thresh = 256), \
    CASE("picture stride below the frame", a.sstride = 382), CASE("previous stride below the frame", a.pstride = 382),                          \
    CASE("output stride below the frame", a.ostride = 382), CASE("odd picture stride of 2-byte samples", a.sstride = 385),                      \
    CASE("odd previous stride", a.pstride = 385), CASE("odd output stride", a.ostride = 385), CASE("odd picture base", a.soff = 385),           \
    CASE("odd previous base of 2-byte samples", a.poff = 1), CASE("odd output base of 2-byte samples", a.ooff = 1),                             \
    CASE("the output is the pictures", a.out_in = SRC; a.ooff = 384), CASE("the output is the previous pictures", a.out_in = SRC; a.ooff = 0),   \
    CASE("INT64_MIN stride", a.sstride = INT64_MIN)
#define SCALER_CASES(out_end_y, out_end_c)                                                                                                    \
    FORMAT_CASES, CASE("luma taps 3", a.ky = 3), CASE("luma taps 0", a.ky = 0), CASE("luma taps 18", a.ky = 18), CASE("luma taps -2", a.ky = -2), \
    CASE("chroma taps 5", a.kc = 5), CASE("chroma taps 0", a.kc = 0), CASE("chroma taps 18", a.kc = 18), CASE("no luma table", a.ty = -1),      \
    CASE("luma table at 4", a.ty = 4), CASE("luma table at 8", a.ty = 8), CASE("no chroma table", a.tc = -1),                                   \
    CASE("chroma table at 4", a.tc = 516), CASE("chroma table at 8", a.tc = 520), CASE("stride below the frame", a.sstride -= 2),               \
    CASE("output stride below the frame", a.ostride -= 2), CASE("odd stride", a.sstride += 1), CASE("odd output stride", a.ostride += 1),        \
    CASE("odd base", a.soff = 1), CASE("odd output base", a.ooff = 1), CASE("the output is the pictures", a.out_in = SRC),                      \
    CASE("the output is the second picture", a.out_in = SRC; a.ooff = 384), CASE("the output on the pictures' last bytes", a.out_in = SRC; a.ooff = 766), \
    CASE("the output is the luma table", a.out_in = TABLE), CASE("the output on the luma table's last bytes", a.out_in = TABLE; a.ooff = out_end_y), \
    CASE("the output on the chroma table's last bytes", a.out_in = TABLE; a.ooff = out_end_c)

static const Case yuv420_cases[] = {
    CASE("h 0", a.h = 0), CASE("w 0", a.w = 0), CASE("n 0", a.n = 0), CASE("h -1", a.h = -1), CASE("layout 2", a.layout = 2),
    CASE("layout -1", a.layout = -1), CASE("parity 2", a.parity = 2), CASE("parity -1", a.parity = -1), CASE("pitch below the row", a.pitch = 47),
    CASE("stride below the frame", a.sstride = 191), CASE("output stride below the frame", a.dstride = 383),
    CASE("output stride below the pitched frame", a.pitch = 52; a.dstride = 7 * 52 + 47), CASE("matrix 2", a.matrix = 2),
    CASE("no context", a.null_ctx = true), CASE("no pictures", a.null_src = true), CASE("no output", a.null_out = true)};
static const Case format_cases[] = {CONVERSION_CASES};
static const Case tonemap_cases[] = {
    CONVERSION_CASES, CASE("no table", a.tone = -1), CASE("table at 1", a.tone = 1), CASE("table at 8", a.tone = 8), CASE("no gamut", a.null_gamut = true),
    CASE("gamut row above 32767", a.gamut[1] = 1; a.gamut[0] = 32767), CASE("gamut row below -32768", a.gamut[3] = -32768; a.gamut[4] = 32767; a.gamut[5] = -1),
    CASE("gamut row 20000 + 12768", a.gamut[6] = 20000; a.gamut[7] = 12768; a.gamut[8] = 0), CASE("gamut INT_MAX twice", a.gamut[0] = a.gamut[1] = 0x7fffffff)};
static const Case deinterlace_cases[] = {FIELDS_CASES, CASE("mode 2", a.mode = 2), CASE("mode -1", a.mode = -1)};
static const Case field_match_cases[] = {
    FIELDS_CASES,
    CASE("no stats", a.null_stats = true),
    CASE("stats at an odd byte", a.stats_off = 1),
    CASE("stats at a 2-byte boundary", a.stats_off = 2),
    CASE("stats inside the pictures", a.stats_in = SRC; a.stats_off = 384),
    CASE("stats inside the previous pictures", a.stats_in = SRC; a.stats_off = 8),
    CASE("stats on the last bytes of the pictures", a.stats_in = SRC; a.stats_off = 3 * 384 - 4),
    CASE("stats inside the output", a.stats_in = OUT; a.stats_off = 2 * 384 - 16),
    CASE("stats at the output", a.stats_in = OUT),
    CASE("comb_thresh -1", a.comb_thresh = -1),
    CASE("comb_thresh 256", a.comb_thresh = 256),
    CASE("comb_limit 1001", a.comb_limit = 1001),
    CASE("comb_limit INT_MAX", a.comb_limit = 0x7fffffff),
    CASE("INT64_MAX strides with the stats behind them", a.sstride = a.pstride = a.ostride = INT64_MAX - 1; a.stats_in = SRC; a.stats_off = 0)};
static const Case resample_cases[] = {
    SCALER_CASES(190, 512 + 94), CASE("w_out 0", a.w2 = 0), CASE("w_out -4", a.w2 = -4), CASE("h * w_out above 2^31 - 1", a.h = 1 << 16; a.w2 = 1 << 15),
    CASE("parity 2", a.parity = 2), CASE("parity -1", a.parity = -1), CASE("parity 1 without vertical subsampling", a.sub_y = 0; a.parity = 1)};
static const Case vscale_cases[] = {
    SCALER_CASES(94, 512 + 46), CASE("h_out 0", a.h2 = 0), CASE("h_out -3", a.h2 = -3), CASE("h_out * w above 2^31 - 1", a.h2 = 1 << 16; a.w = 1 << 15),
    CASE("s0 -1", a.s0 = -1), CASE("s1 past the picture", a.s1 = 9), CASE("empty band at the end", a.s0 = 8), CASE("empty band", a.s0 = 4; a.s1 = 4),
    CASE("band backwards", a.s0 = 5; a.s1 = 3), CASE("s1 0", a.s1 = 0), CASE("y0 -1", a.y0 = -1), CASE("y1 past the picture", a.y1 = 13),
    CASE("no output rows at the end", a.y0 = 12), CASE("no output rows", a.y0 = 6; a.y1 = 6), CASE("output rows backwards", a.y0 = 7; a.y1 = 2),
    CASE("y1 0", a.y1 = 0)};

// ---- the entry points
struct Entry {
    const char* name;          // what its messages begin with
    const Case* cases;
    size_t count;
    Change defaults;
    int (*call)(const Args&);
};
#define ENTRY(name, cases, defaults, ...) {name, cases, sizeof cases / sizeof cases[0], [](Args& a) { defaults; }, [](const Args& a) -> int { return __VA_ARGS__; }}

static const Entry entries[] = {
    ENTRY("vse_yuv420_to_bgr", yuv420_cases, a.sstride = 192; a.matrix = 0,
          a.matrix == 0 ? vse_yuv420_to_bgr(ctx_of(a), src_of(a), a.n, a.h, a.w, a.layout, a.parity, a.sstride, out_of(a), a.pitch, a.dstride, nullptr)
                        : vse_yuv_to_bgr_matrix(ctx_of(a), src_of(a), a.n, a.h, a.w, a.layout, a.parity, a.sstride, out_of(a), a.pitch, a.dstride, a.matrix,
                                                nullptr)),
    ENTRY("vse_yuv_to_bgr_format", format_cases, (void)a,
          vse_yuv_to_bgr_format(ctx_of(a), src_of(a), a.n, a.h, a.w, a.sub_x, a.sub_y, a.chroma, a.depth, a.msb, a.matrix, a.full, a.parity, a.sstride,
                                out_of(a), a.pitch, a.dstride, nullptr)),
    ENTRY("vse_yuv_to_bgr_tonemap", tonemap_cases, (void)a,
          vse_yuv_to_bgr_tonemap(ctx_of(a), src_of(a), a.n, a.h, a.w, a.sub_x, a.sub_y, a.chroma, a.depth, a.msb, a.matrix, a.full, a.parity, a.sstride,
                                 out_of(a), a.pitch, a.dstride, tab(a.tone), a.null_gamut ? nullptr : a.gamut, nullptr)),
    ENTRY("vse_yuv_deinterlace", deinterlace_cases, a.soff = 384,
          vse_yuv_deinterlace(ctx_of(a), src_of(a), a.prev ? src + a.poff : nullptr, a.n, a.h, a.w, a.sub_x, a.sub_y, a.chroma, a.depth, a.msb, a.keep,
                              a.mode, a.thresh, a.sstride, a.pstride, out_of(a), a.ostride, nullptr)),
    ENTRY("vse_yuv_field_match", field_match_cases, a.soff = 384,
          vse_yuv_field_match(ctx_of(a), src_of(a), a.prev ? src + a.poff : nullptr, a.n, a.h, a.w, a.sub_x, a.sub_y, a.chroma, a.depth, a.msb, a.keep,
                              a.comb_thresh, a.comb_limit, a.thresh, a.sstride, a.pstride, out_of(a), a.ostride,
                              a.null_stats ? nullptr : base(a.stats_in) + a.stats_off, nullptr)),
    ENTRY("vse_yuv_resample", resample_cases, a.ostride = 576,
          vse_yuv_resample(ctx_of(a), src_of(a), a.n, a.h, a.w, a.w2, a.sub_x, a.sub_y, a.chroma, a.depth, a.msb, a.parity, tab(a.ty), a.ky, tab(a.tc),
                           a.kc, a.sstride, out_of(a), a.ostride, nullptr)),
    ENTRY("vse_yuv_vscale", vscale_cases, a.ostride = 576,
          vse_yuv_vscale(ctx_of(a), src_of(a), a.n, a.w, a.h, a.h2, a.s0, a.s1, a.y0, a.y1, a.sub_x, a.sub_y, a.chroma, a.depth, a.msb, tab(a.ty), a.ky,
                         tab(a.tc), a.kc, a.sstride, out_of(a), a.ostride, nullptr)),
};

static int refusals() {
    memset(out, FILL, sizeof out);
    memset(stats, FILL, sizeof stats);
    for (size_t i = 0; i < sizeof table; ++i) table[i] = (unsigned char)(i * 7);
    const std::regex pointer("0x[0-9a-f]+|\\(nil\\)");
    int failures = 0, calls = 0;
    for (const Entry& e : entries) {
        for (size_t k = 0; k < e.count; ++k, ++calls) {
            Args a;
            e.defaults(a);
            e.cases[k].change(a);
            last_error.clear();
            const int rc = e.call(a);
            const bool ok = rc == VSE_E_INVAL && last_error.find(std::string(e.name) + ": bad arguments (") == 0;
            printf("%s, %s: %s (%d)\n    %s\n", e.name, e.cases[k].what, ok ? "refused" : "NOT REFUSED", rc,
                   std::regex_replace(last_error, pointer, "PTR").c_str());
            failures += ok ? 0 : 1;
        }
    }
    // nothing was written
    for (unsigned char v : src) failures += v ? 1 : 0;
    for (unsigned char v : out) failures += v != FILL ? 1 : 0;
    for (uint32_t v : stats) failures += v != 0x01010101u * FILL ? 1 : 0;
    for (size_t i = 0; i < sizeof table; ++i) failures += table[i] != (unsigned char)(i * 7) ? 1 : 0;
    printf("%d of %d calls not refused as they must be, or bytes written\n", failures, calls);
    return failures;
}

// The geometry behind vse_yuv420_frame_bytes and vse_yuv_frame_bytes: h, w in 1..9, every format, depth 8 and 10, every legal row parity.
static int geometry() {
    int failures = 0, cases = 0;
#ifdef HAVE_PLANES
    for (int sub_x = 0; sub_x <= 1; ++sub_x) for (int sub_y = 0; sub_y <= 1; ++sub_y) for (int chroma = 0; chroma <= 2; ++chroma)
    for (int depth = 8; depth <= 10; depth += 2) for (int parity = 0; parity <= sub_y && yuv_format_ok(sub_x, sub_y, chroma, depth); ++parity)
    for (int h = 1; h <= 9; ++h) for (int w = 1; w <= 9; ++w, ++cases) {
        const YuvPlanes pl = yuv_planes(h, w, sub_x, sub_y, chroma, depth, parity);
        // the planes lie back to back and end where the frame does
        bool ok = pl.count == (chroma == 0 ? 1 : chroma == 1 ? 3 : 2) && pl.rows[0] == h && pl.row[0] == w;
        long end = 0;
        for (int p = 0; p < pl.count; ++p) {
            ok = ok && pl.off[p] == end && pl.rows[p] >= 1 && pl.row[p] >= 1;
            end += pl.rows[p] * pl.row[p];
        }
        ok = ok && end == pl.total && (size_t)end * (depth > 8 ? 2 : 1) == vse_yuv_frame_bytes(h, w, sub_x, sub_y, chroma, depth, parity);
        if (sub_x == 1 && sub_y == 1 && chroma == 1 && depth == 8) ok = ok && (size_t)end == vse_yuv420_frame_bytes(h, w, parity);
        // as rows [parity, parity + h) of a picture of parity + h rows it is vse_yuv_vscale's band: the chroma rows that those luma rows
        // touch, as wide as the whole picture's
        const YuvPlanes whole = yuv_planes(parity + h, w, sub_x, sub_y, chroma, depth, 0);
        for (int p = 1; p < pl.count; ++p)
            ok = ok && pl.rows[p] == ((parity + h - 1) >> sub_y) + 1 - (parity >> sub_y) && pl.rows[p] == whole.rows[p] - (parity >> sub_y) &&
                 pl.row[p] == whole.row[p];
        if (!ok) printf("geometry: %d x %d, subsampling %d, %d, chroma %d, depth %d, parity %d\n", h, w, sub_x, sub_y, chroma, depth, parity);
        failures += ok ? 0 : 1;
    }
    printf("%d of %d plane geometries wrong\n", failures, cases);
#endif
    return failures;
}

int main() {
    const int bad = refusals();
    return bad + geometry() ? 1 : 0;
}
