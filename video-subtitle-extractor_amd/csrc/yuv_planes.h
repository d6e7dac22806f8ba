// The geometry of one packed picture (include/vse_hip.h vse_yuv_frame_bytes): host code, written once.  yuv.hip derives the frame sizes
// and every kernel's plane arguments from it, and tools/yuv_refusals.cpp sweeps it against the sizes the library reports.
#pragma once
#include <stdint.h>

constexpr int CHROMA_NONE = 0, CHROMA_PLANAR = 1, CHROMA_SEMI = 2;
constexpr long YUV_MAX_PIXELS = 0x7fffffffL;           // per frame: the per-frame work-item index stays an int

inline bool yuv_format_ok(int sub_x, int sub_y, int chroma, int depth) {
    const bool sub = (sub_x == 0 && sub_y == 0) || (sub_x == 1 && sub_y == 0) || (sub_x == 1 && sub_y == 1);
    return sub && chroma >= CHROMA_NONE && chroma <= CHROMA_SEMI && depth >= 8 && depth <= 16 && (chroma != CHROMA_NONE || sub_x + sub_y == 0) &&
           (chroma != CHROMA_SEMI || sub_x + sub_y == 2);
}

// Planes Y, then U and V (planar) or the interleaved UV plane (semi-planar), back to back.  All in samples: rows[p] rows of row[p]
// samples (an interleaved UV row counts 2 cw) from sample off[p]; total = the picture.  count 0: not a picture the library takes.
struct YuvPlanes {
    int count;
    int rows[3];
    long row[3], off[3], total;
};

// h x w pixels whose first row has parity row_parity in its whole picture: chroma column x >> sub_x, chroma row (r + row_parity) >> sub_y.
// A band of rows [a, b) of a picture is the picture of b - a rows and parity a & sub_y.
inline YuvPlanes yuv_planes(int h, int w, int sub_x, int sub_y, int chroma, int depth, int row_parity) {
    YuvPlanes pl = {};
    if (h < 1 || w < 1 || !yuv_format_ok(sub_x, sub_y, chroma, depth) || row_parity < 0 || row_parity > sub_y || (long)h * w > YUV_MAX_PIXELS) return pl;
    const long cw = ((long)w + sub_x) >> sub_x, ch = (((long)h - 1 + row_parity) >> sub_y) + 1;
    pl.count = chroma == CHROMA_NONE ? 1 : chroma == CHROMA_PLANAR ? 3 : 2;
    for (int p = 0; p < pl.count; ++p) {
        pl.rows[p] = p ? (int)ch : h;
        pl.row[p] = !p ? w : chroma == CHROMA_SEMI ? 2 * cw : cw;
        pl.off[p] = pl.total;
        pl.total += pl.rows[p] * pl.row[p];
    }
    return pl;
}
