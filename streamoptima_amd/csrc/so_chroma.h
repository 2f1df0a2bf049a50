// so_chroma.h — the argument block of the chroma kernels (so_chroma.hip), filled by the C-ABI
// entry points so_chroma_encode_frame / so_chroma_recon_frame (so_capi.hip).
#pragma once
#include "so_common.h"

namespace so {

struct ChromaPlanes {
    const uint8_t* cur;    // ENC only
    RefSet refs;           // P-frames only
    int16_t* qtc;          // ENC: written; !ENC: read
    uint8_t* recon;
};

struct ChromaArgs {
    ChromaPlanes pl[2];    // U, V
    int nref, Hc, Wc, nbx, nb, frame_type;
    const uint8_t* split;  // luma symbols (P-frames)
    const int16_t* mv;     // int16 [nb][4][3]
    int qp;
    const int32_t* qp_row;
    const int32_t* qp_map;
    int qp_offset;
    int32_t* tokens;       // int32 [2][nb]   (ENC)
    int32_t* sse;          // int32 [2][nb]   (ENC)
};

// ---- the prediction, shared by chroma_kernel (so_chroma.hip) and the fused decoder (so_decode.hip) ----
SO_DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Four prediction samples of plane row Y starting at column X for the chroma MV (dx, dy) in
// half-sample units.  Inside the plane (the lane's 5 x 2 footprint; every lane of a block whose
// 9 x 9 footprint lies inside takes it) the two rows come as aligned dwords funnel-shifted to
// the sample, as fetch_row does -- only dwords that hold a needed byte are read, so nothing
// outside the plane is touched; otherwise every coordinate is clamped.
SO_DEV void chroma_pred4(const uint8_t* __restrict__ R, int Wc, int Hc, int X, int Y, int dx, int dy, int* out) {
    const int ix = dx >> 1, fx = dx & 1, iy = dy >> 1, fy = dy & 1;
    const int xs = X + ix, ys = Y + iy;
    if (xs >= 0 && xs + 3 + fx < Wc && ys >= 0 && ys + fy < Hc) {
        uint32_t lo[2], hi[2];   // row y: samples 0..3, sample 4
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint8_t* p = R + (size_t)(ys + (r ? fy : 0)) * Wc + xs;
            const uintptr_t a = reinterpret_cast<uintptr_t>(p);
            const uint32_t* q = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
            const uint32_t sh = (uint32_t)(a & 3);
            const uint32_t w0 = q[0];
            const uint32_t w1 = (sh + (uint32_t)fx) ? q[1] : 0u;   // holds a needed byte only then
            lo[r] = __builtin_amdgcn_alignbyte(w1, w0, sh);
            hi[r] = (w1 >> (8 * sh)) & 255u;   // byte sh + 4 of the pair
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t a0 = (lo[0] >> (8 * k)) & 255u, b0 = (lo[1] >> (8 * k)) & 255u;
            const uint32_t a1n = k < 3 ? (lo[0] >> (8 * k + 8)) & 255u : hi[0];
            const uint32_t b1n = k < 3 ? (lo[1] >> (8 * k + 8)) & 255u : hi[1];
            const uint32_t a1 = fx ? a1n : a0, b1 = fx ? b1n : b0;
            out[k] = (int)((a0 + a1 + b0 + b1 + 2u) >> 2);
        }
    } else {
        const int y0 = clampi(ys, 0, Hc - 1), y1 = clampi(ys + fy, 0, Hc - 1);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x0 = clampi(xs + k, 0, Wc - 1), x1 = clampi(xs + k + fx, 0, Wc - 1);
            out[k] = ((int)R[(size_t)y0 * Wc + x0] + (int)R[(size_t)y0 * Wc + x1] + (int)R[(size_t)y1 * Wc + x0] +
                      (int)R[(size_t)y1 * Wc + x1] + 2) >> 2;
        }
    }
}

SO_DEV const uint8_t* pick_ref(const RefSet& rs, int r) {
    const uint8_t* p = rs.p[0];
    p = r == 1 ? rs.p[1] : p;
    p = r == 2 ? rs.p[2] : p;
    p = r == 3 ? rs.p[3] : p;
    return p;
}

int chroma_launch(const ChromaArgs& a, bool encode, hipStream_t st);

}  // namespace so
