// so_deblock.h — argument blocks and tile geometry of the deblocking post-filter
// (so_deblock.hip; the arithmetic is stated in include/streamoptima.h, "Deblocking").
#pragma once
#include "so_common.h"

namespace so {

constexpr int kDeblockBatch = 32;      // frames per launch (device pointers by value)
constexpr int kDeblockThreads = 256;
constexpr int kDeblockTileW = 128;     // a tile's samples across: 256 lanes x 16 bytes cover 32 rows of it
constexpr int kDeblockTileH = 32;
constexpr int kDeblockHalo = 3;        // samples a line reads on either side of its edge
// LDS row: 16 bytes whose last three are the left halo, the tile's 128 samples (16-byte aligned),
// 16 bytes whose first three are the right halo
constexpr int kDeblockPitch = 16 + kDeblockTileW + 16;
constexpr int kDeblockRows = kDeblockTileH + 2 * kDeblockHalo;
constexpr int kDeblockCellsX = kDeblockTileW / 8 + 2;   // the tile's 8 x 8 cells and one ring around them
constexpr int kDeblockCellsY = kDeblockTileH / 8 + 2;

struct DeblockPtrs {
    const uint8_t* s[3][kDeblockBatch];   // Y, U, V
    uint8_t* d[3][kDeblockBatch];
    const uint8_t* split[kDeblockBatch];  // [nb] or NULL: no block is split
    const int32_t* qp_row[kDeblockBatch]; // [H / bs] or NULL
    const int32_t* qp_map[kDeblockBatch]; // [nb] or NULL: rows, then the scalar
};

struct DeblockGeom {
    int32_t H, W;          // luma plane; the chroma planes are H/2 x W/2
    int32_t bs;            // 16 or 8
    int32_t nplanes;       // 1 (luma only) or 3
    int32_t qp;
    int32_t chroma_qp_offset;
    int32_t strength;
    int32_t ntx[2], nty[2];   // tiles across and down a luma / a chroma plane
};

inline void deblock_tiles(DeblockGeom* g) {
    for (int k = 0; k < 2; ++k) {
        const int h = k ? g->H / 2 : g->H, w = k ? g->W / 2 : g->W;
        g->ntx[k] = (w + kDeblockTileW - 1) / kDeblockTileW;
        g->nty[k] = (h + kDeblockTileH - 1) / kDeblockTileH;
    }
}

int deblock_launch(const DeblockPtrs& ptrs, int nframes, const DeblockGeom& g, hipStream_t st);

}  // namespace so
