// so_scale.h — argument blocks and tile sizing of the polyphase resampler
// (so_scale.hip; the arithmetic is stated in include/streamoptima.h, "Scaling").
#pragma once
#include "so_common.h"

namespace so {

constexpr int kScaleBatch = 32;       // frames per launch (device pointers by value)
constexpr int kScaleThreads = 256;
constexpr int kScaleMaxTaps = 32;
constexpr int kScaleTileW = 64;       // a tile's output columns: one wave stores one output row
constexpr size_t kScaleLdsBudget = 64 * 1024;   // per workgroup: at least two resident per CU (160 KiB)
// a tile's tap rows in LDS: 64 horizontal and up to 64 vertical rows of 32 int16, and their `first`
constexpr size_t kScaleTableBytes = 2 * kScaleTileW * kScaleMaxTaps * sizeof(int16_t) + 2 * kScaleTileW * sizeof(int32_t);

struct ScaleTable {
    const int16_t* coef;   // [n_dst][taps]
    const int32_t* first;  // [n_dst]
    int32_t taps;
};

// one kind of plane: luma, or the two half-size chroma planes
struct ScalePlane {
    int32_t hs, ws;        // source picture
    int32_t hd, wd;        // destination picture
    int32_t Hp, Wp;        // destination plane (pitch Wp)
    size_t spitch;         // source row pitch in bytes
    ScaleTable h, v;
    int32_t capw, caph;    // source columns / rows a tile may need (scale_span)
    int32_t ntx, nty;      // tiles across and down the destination plane
};

struct ScalePtrs {
    const uint8_t* s[3][kScaleBatch];   // Y, U, V
    uint8_t* d[3][kScaleBatch];
};

struct ScaleGeom {
    ScalePlane p[2];       // luma, chroma
    int32_t nplanes;       // 1 (luma only) or 3
    int32_t th;            // a tile's output rows
    int32_t srows;         // source rows staged at a time (<= 64: a lane each in the horizontal pass)
    int32_t lpitch;        // bytes per staged source row (4 x an odd number)
    int32_t mpitch;        // int16 per column of the intermediate (2 x an odd number)
};

// The source samples that n consecutive outputs of an n_src -> n_dst table with `taps` taps can
// touch.  Every row holds its largest tap, which sits within half a sample of the row's centre, so
// row j lies inside [c_j - taps + 1/2, c_j + taps - 1/2]; the centres of n rows span (n - 1) n_src /
// n_dst.  Never more than the source has.
inline int scale_span(int n, int n_src, int n_dst, int taps) {
    const int live = n < n_dst ? n : n_dst;
    const long long s = (long long)(live - 1) * n_src / n_dst + 2 * taps + 1;
    return (int)(s < n_src ? s : n_src);
}

// fills th, srows, lpitch, mpitch and the planes' capw / caph / ntx / nty; false: no tile fits the LDS
bool scale_tiles(ScaleGeom* g);
size_t scale_lds_bytes(const ScaleGeom& g);
int scale_launch(const ScalePtrs& ptrs, int nframes, const ScaleGeom& g, hipStream_t st);

}  // namespace so
