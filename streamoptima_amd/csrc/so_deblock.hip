// so_deblock.hip — the display-side deblocking post-filter of 8-bit 4:2:0 planes (so_deblock_yuv420;
// include/streamoptima.h "Deblocking" states the arithmetic, tests/deblockref.py restates it).
//
// One launch covers Y, U and V of a batch.  A workgroup of four waves owns a tile of 32 x 128 samples
// of one plane (tiles start at multiples of 32 and 128, so always on a cell border):
//   cells    the 8 x 8 cells of the tile and one ring of cells around it get their QP and their split
//            flag in LDS, one lane per cell: blockqp from the map, the row list or the scalar, clamped
//            to 0..20, then the split / chroma rule.  The block index comes from the coordinates alone,
//            so whatever the map holds is clamped and used, never followed;
//   stage    the tile and a halo of three samples go to LDS.  The tile's own columns are 16-byte
//            aligned in LDS; where the plane's address and width are too they are copied as 16-byte
//            (or 8-byte) words, otherwise byte by byte.  The halo columns are gathered as bytes.
//            Nothing outside the plane is read;
//   pass 1   vertical edges: a lane takes one line (one row, one edge) of the 38 staged rows, reads the
//            two dwords around the edge, filters and writes them back in place.  The halo rows take
//            the cells of the neighbouring blocks.  Lines of one pass are 8 apart and write two
//            samples on each side, so no two touch the same dword;
//   pass 2   horizontal edges, from pass 1's result: a lane takes four adjacent columns of one edge
//            (one dword of each of six rows), lanes along the row: the 32 lanes of a half-wave read
//            consecutive LDS banks.  In a full tile lanes 32..63 work on the next edge, 8 LDS rows
//            (320 dwords) further on: the same 32 banks as lanes 0..31, which costs nothing for
//            ds_read_b32 / ds_write_b32 (banking is per 32-lane half);
//   store    the tile's own samples leave LDS as 16-byte reads and go out as 16-byte (8-byte, byte)
//            stores.  Untouched samples are copied, the intermediate never leaves LDS.
// The tile filters both sides of its border edges in LDS and stores its own side only, so every
// sample of the plane is written by exactly one workgroup.
#include "so_deblock.h"

namespace so {

SO_DEV int deblock_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

struct DeblockThr {
    int alpha, beta, tc, tc1;
};

SO_DEV DeblockThr deblock_thr(int cq_p, int cq_q, int strength) {
    const int q = deblock_clamp(max(cq_p, cq_q) + strength, 0, 20);
    const int s = 1 << q;
    DeblockThr t;
    t.alpha = min(s, 255);
    t.beta = min((3 * s) >> 3, 255);
    t.tc = min(s >> 2, 255);
    t.tc1 = t.tc >> 1;
    return t;
}

// one line p2 p1 p0 | q0 q1 q2: p1, p0, q0, q1 are replaced
SO_DEV void deblock_line(const DeblockThr& t, int p2, int& p1, int& p0, int& q0, int& q1, int q2) {
    const int d = q0 - p0;
    if (!(abs(d) < t.alpha && abs(p1 - p0) < t.beta && abs(q1 - q0) < t.beta)) return;
    const bool ap = abs(p2 - p0) < t.beta, aq = abs(q2 - q0) < t.beta;
    const int dl = deblock_clamp((4 * d + (p1 - q1) + 4) >> 3, -t.tc, t.tc);
    const int avg = (p0 + q0 + 1) >> 1;
    const int np1 = p1 + deblock_clamp((p2 + avg - 2 * p1) >> 1, -t.tc1, t.tc1);
    const int nq1 = q1 + deblock_clamp((q2 + avg - 2 * q1) >> 1, -t.tc1, t.tc1);
    p0 = deblock_clamp(p0 + dl, 0, 255);
    q0 = deblock_clamp(q0 - dl, 0, 255);
    if (ap) p1 = np1;
    if (aq) q1 = nq1;
}

SO_DEV int deblock_byte(uint32_t w, int k) { return (int)((w >> (8 * k)) & 255u); }

template <typename V>
SO_DEV void deblock_stage(uint8_t* lds, const uint8_t* src, int W, int x0, int tw, int gy_lo, int r_lo, int nrows) {
    constexpr int n = (int)sizeof(V);
    const int per = tw / n;
    for (int i = threadIdx.x; i < nrows * per; i += kDeblockThreads) {
        const int r = i / per, c = i - r * per;
        *reinterpret_cast<V*>(lds + (r_lo + r) * kDeblockPitch + 16 + c * n) =
            *reinterpret_cast<const V*>(src + (size_t)(gy_lo + r) * W + x0 + c * n);
    }
}

template <typename V>
SO_DEV void deblock_store(const uint8_t* lds, uint8_t* dst, int W, int x0, int y0, int tw, int th) {
    constexpr int n = (int)sizeof(V);
    const int per = tw / n;
    for (int i = threadIdx.x; i < th * per; i += kDeblockThreads) {
        const int r = i / per, c = i - r * per;
        *reinterpret_cast<V*>(dst + (size_t)(y0 + r) * W + x0 + c * n) =
            *reinterpret_cast<const V*>(lds + (kDeblockHalo + r) * kDeblockPitch + 16 + c * n);
    }
}

__global__ void __launch_bounds__(kDeblockThreads)
deblock_yuv420_kernel(const DeblockPtrs ptrs, const DeblockGeom g) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kDeblockRows * kDeblockPitch];
    __shared__ int8_t cell_qp[kDeblockCellsY * kDeblockCellsX];
    __shared__ uint8_t cell_split[kDeblockCellsY * kDeblockCellsX];

    int b = blockIdx.x, pl = 0;
    const int nluma = g.ntx[0] * g.nty[0];
    if (b >= nluma) {
        b -= nluma;
        const int nchroma = g.ntx[1] * g.nty[1];
        pl = b >= nchroma ? 2 : 1;
        if (b >= nchroma) b -= nchroma;
    }
    const int k = pl != 0;
    const int H = k ? g.H >> 1 : g.H, W = k ? g.W >> 1 : g.W;
    const int ty = b / g.ntx[k], tx = b - ty * g.ntx[k];
    const int y0 = ty * kDeblockTileH, x0 = tx * kDeblockTileW;
    const int th = min(kDeblockTileH, H - y0), tw = min(kDeblockTileW, W - x0);
    const int f = blockIdx.y;
    const uint8_t* src = ptrs.s[pl][f];
    uint8_t* dst = ptrs.d[pl][f];
    // cells of a block along one axis: 2 for luma at block size 16, 1 for luma at 8 and for chroma
    const int cpb = (pl == 0 && g.bs == 16) ? 2 : 1;

    // ---- cells ----
    if (threadIdx.x < kDeblockCellsY * kDeblockCellsX) {
        const int cyi = threadIdx.x / kDeblockCellsX, cxi = threadIdx.x - cyi * kDeblockCellsX;
        const int cy = (y0 >> 3) - 1 + cyi, cx = (x0 >> 3) - 1 + cxi;
        int cq = 0, sp = 0;
        if (cy >= 0 && cx >= 0 && cy < (H >> 3) && cx < (W >> 3)) {
            const int by = cy / cpb, bx = cx / cpb, nbx = (W >> 3) / cpb;
            const int blk = by * nbx + bx;
            const int32_t* map = ptrs.qp_map[f];
            const int32_t* row = ptrs.qp_row[f];
            const int bq = deblock_clamp(map ? map[blk] : row ? row[by] : g.qp, 0, 20);
            if (pl == 0) {
                const uint8_t* split = ptrs.split[f];
                sp = split != nullptr && split[blk] != 0;
                cq = sp ? max(bq - 1, 0) : bq;
            } else {
                cq = deblock_clamp(bq + g.chroma_qp_offset, 0, 20);
            }
        }
        cell_qp[threadIdx.x] = (int8_t)cq;
        cell_split[threadIdx.x] = (uint8_t)sp;
    }

    // ---- stage ----
    const int gy_lo = max(0, y0 - kDeblockHalo), gy_hi = min(H, y0 + th + kDeblockHalo);
    const int r_lo = gy_lo - (y0 - kDeblockHalo), nrows = gy_hi - gy_lo;
    {
        const unsigned al = (unsigned)(reinterpret_cast<uintptr_t>(src) | (uintptr_t)W) & 15u;
        if (al == 0) deblock_stage<uint4>(lds, src, W, x0, tw, gy_lo, r_lo, nrows);
        else if ((al & 7u) == 0) deblock_stage<uint2>(lds, src, W, x0, tw, gy_lo, r_lo, nrows);
        else deblock_stage<uint8_t>(lds, src, W, x0, tw, gy_lo, r_lo, nrows);
        const bool left = x0 > 0, right = x0 + tw < W;   // a tile that ends inside the plane is a full one
        for (int i = threadIdx.x; i < nrows * 2 * kDeblockHalo; i += kDeblockThreads) {
            const int r = i / (2 * kDeblockHalo), c = i - r * (2 * kDeblockHalo);
            const int dx = c < kDeblockHalo ? c - kDeblockHalo : tw + c - kDeblockHalo;
            if (c < kDeblockHalo ? left : right)
                lds[(r_lo + r) * kDeblockPitch + 16 + dx] = src[(size_t)(gy_lo + r) * W + x0 + dx];
        }
    }
    __syncthreads();

    uint32_t* words = reinterpret_cast<uint32_t*>(lds);
    constexpr int kPitchW = kDeblockPitch / 4;

    // ---- pass 1: vertical edges, lines along rows ----
    {
        const int nedge = tw / 8 + 1;
        for (int i = threadIdx.x; i < nrows * nedge; i += kDeblockThreads) {
            const int rr = i / nedge, e = i - rr * nedge;
            const int r = r_lo + rr, gx = x0 + 8 * e;
            if (gx <= 0 || gx >= W) continue;
            const int cyi = ((gy_lo + rr) >> 3) - (y0 >> 3) + 1, cxi = e + 1;   // the cell on the q side
            const int cq = cyi * kDeblockCellsX + cxi;
            if (cpb == 2 && ((gx >> 3) & 1) && !cell_split[cq]) continue;       // inside an unsplit block
            const DeblockThr t = deblock_thr(cell_qp[cq - 1], cell_qp[cq], g.strength);
            if (t.tc == 0) continue;
            uint32_t* w = words + r * kPitchW + 3 + 2 * e;
            const uint32_t a = w[0], c = w[1];
            int p1 = deblock_byte(a, 2), p0 = deblock_byte(a, 3), q0 = deblock_byte(c, 0), q1 = deblock_byte(c, 1);
            deblock_line(t, deblock_byte(a, 1), p1, p0, q0, q1, deblock_byte(c, 2));
            w[0] = (a & 0x0000ffffu) | ((uint32_t)p1 << 16) | ((uint32_t)p0 << 24);
            w[1] = (c & 0xffff0000u) | (uint32_t)q0 | ((uint32_t)q1 << 8);
        }
    }
    __syncthreads();

    // ---- pass 2: horizontal edges, lines along columns, four columns a lane ----
    {
        const int ncol = tw / 4, nedge = th / 8 + 1;
        for (int i = threadIdx.x; i < nedge * ncol; i += kDeblockThreads) {
            const int e = i / ncol, c = i - e * ncol;
            const int gy = y0 + 8 * e;
            if (gy <= 0 || gy >= H) continue;
            const int cyi = e + 1, cxi = (c >> 1) + 1;                          // the cell on the q side
            const int cq = cyi * kDeblockCellsX + cxi;
            if (cpb == 2 && ((gy >> 3) & 1) && !cell_split[cq]) continue;
            const DeblockThr t = deblock_thr(cell_qp[cq - kDeblockCellsX], cell_qp[cq], g.strength);
            if (t.tc == 0) continue;
            uint32_t* w = words + (8 * e) * kPitchW + 4 + c;   // LDS row 8e is the edge's p2
            uint32_t v[6];
#pragma unroll
            for (int j = 0; j < 6; ++j) v[j] = w[j * kPitchW];
            uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                int p1 = deblock_byte(v[1], s), p0 = deblock_byte(v[2], s), q0 = deblock_byte(v[3], s),
                    q1 = deblock_byte(v[4], s);
                deblock_line(t, deblock_byte(v[0], s), p1, p0, q0, q1, deblock_byte(v[5], s));
                o[0] |= (uint32_t)p1 << (8 * s);
                o[1] |= (uint32_t)p0 << (8 * s);
                o[2] |= (uint32_t)q0 << (8 * s);
                o[3] |= (uint32_t)q1 << (8 * s);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) w[(j + 1) * kPitchW] = o[j];
        }
    }
    __syncthreads();

    // ---- store ----
    {
        const unsigned al = (unsigned)(reinterpret_cast<uintptr_t>(dst) | (uintptr_t)W) & 15u;
        if (al == 0) deblock_store<uint4>(lds, dst, W, x0, y0, tw, th);
        else if ((al & 7u) == 0) deblock_store<uint2>(lds, dst, W, x0, y0, tw, th);
        else deblock_store<uint8_t>(lds, dst, W, x0, y0, tw, th);
    }
}

int deblock_launch(const DeblockPtrs& ptrs, int nframes, const DeblockGeom& g, hipStream_t st) {
    unsigned tiles = (unsigned)(g.ntx[0] * g.nty[0]);
    if (g.nplanes > 1) tiles += 2u * (unsigned)(g.ntx[1] * g.nty[1]);
    hipLaunchKernelGGL(deblock_yuv420_kernel, dim3(tiles, nframes), dim3(kDeblockThreads), 0, st, ptrs, g);
    return check_launch("deblock_yuv420_kernel");
}

}  // namespace so
