// so_chroma.h — the argument block of the chroma kernels (so_chroma.hip), filled by the C-ABI
// entry points so_chroma_encode_frame(_ex) / so_chroma_recon_frame(_ex) (so_capi.hip).
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
    int mv_frac_bits;      // 1: full-sample luma vectors; 2: half-sample (FME)
};

// ---- the prediction, shared by chroma_kernel (so_chroma.hip) and the fused decoder (so_decode.hip) ----
SO_DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Four prediction samples of plane row Y starting at column X for the chroma MV (dx, dy) with S
// fractional bits (S = 1: the luma vectors are full-sample, half a chroma sample; S = 2: they are
// half-sample under FME, a quarter of a chroma sample).  With D = 1 << S, fx = dx & (D - 1):
//   P = ((D-fx)(D-fy) R[y0][x0] + fx(D-fy) R[y0][x1] + (D-fx)fy R[y1][x0] + fx fy R[y1][x1]
//        + (1 << (2S-1))) >> 2S,   x1 = clamp(X + (dx >> S) + (fx != 0)),  y alike,
// which at S = 1 is the rounded mean of the four taps.  Inside the plane (the lane's 5 x 2
// footprint; every lane of a block whose 9 x 9 footprint lies inside takes it) the two rows come
// as aligned dwords funnel-shifted to the sample, as fetch_row does -- only dwords that hold a
// needed byte are read, so nothing outside the plane is touched; otherwise every coordinate is
// clamped.  At S = 2 the four weights (each <= 16) are one packed dword per run and a sample is
// one v_dot4_u32_u8 of it against (a0, a1, b0, b1) gathered by v_perm_b32; a tap whose weight is
// zero may hold any byte, so no select on fx is needed.
template <int S>
SO_DEV void chroma_pred4(const uint8_t* __restrict__ R, int Wc, int Hc, int X, int Y, int dx, int dy, int* out) {
    static_assert(S == 1 || S == 2, "half- or quarter-sample chroma vectors");
    constexpr int D = 1 << S;
    const int ix = dx >> S, fx = dx & (D - 1), iy = dy >> S, fy = dy & (D - 1);
    const int nx = fx != 0, ny = fy != 0;   // the second tap's step (at S = 1: fx, fy)
    const int xs = X + ix, ys = Y + iy;
    if (xs >= 0 && xs + 3 + nx < Wc && ys >= 0 && ys + ny < Hc) {
        uint32_t lo[2], hi[2];   // row y: samples 0..3, sample 4
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint8_t* p = R + (size_t)(ys + (r ? ny : 0)) * Wc + xs;
            const uintptr_t a = reinterpret_cast<uintptr_t>(p);
            const uint32_t* q = reinterpret_cast<const uint32_t*>(a & ~(uintptr_t)3);
            const uint32_t sh = (uint32_t)(a & 3);
            const uint32_t w0 = q[0];
            const uint32_t w1 = (sh + (uint32_t)nx) ? q[1] : 0u;   // holds a needed byte only then
            lo[r] = __builtin_amdgcn_alignbyte(w1, w0, sh);
            hi[r] = (w1 >> (8 * sh)) & 255u;   // byte sh + 4 of the pair
        }
        if constexpr (S == 1) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t a0 = (lo[0] >> (8 * k)) & 255u, b0 = (lo[1] >> (8 * k)) & 255u;
                const uint32_t a1n = k < 3 ? (lo[0] >> (8 * k + 8)) & 255u : hi[0];
                const uint32_t b1n = k < 3 ? (lo[1] >> (8 * k + 8)) & 255u : hi[1];
                const uint32_t a1 = fx ? a1n : a0, b1 = fx ? b1n : b0;
                out[k] = (int)((a0 + a1 + b0 + b1 + 2u) >> 2);
            }
        } else {
            const uint32_t gx = (uint32_t)(D - fx), gy = (uint32_t)(D - fy);
            const uint32_t wt = gx * gy | ((uint32_t)fx * gy) << 8 | (gx * (uint32_t)fy) << 16 |
                                (uint32_t)(fx * fy) << 24;   // weights of (a0, a1, b0, b1), sum D * D
            constexpr uint32_t rnd = 1u << (2 * S - 1);
#pragma unroll
            for (int k = 0; k < 3; ++k) {   // bytes (k, k + 1) of row a, then of row b
                const uint32_t t = __builtin_amdgcn_perm(lo[1], lo[0], 0x05040100u + 0x01010101u * (uint32_t)k);
                out[k] = (int)(__builtin_amdgcn_udot4(t, wt, rnd, false) >> (2 * S));
            }
            const uint32_t pa = __builtin_amdgcn_alignbyte(hi[0], lo[0], 3);   // a3 | a4 << 8
            const uint32_t pb = __builtin_amdgcn_alignbyte(hi[1], lo[1], 3);
            out[3] = (int)(__builtin_amdgcn_udot4(pa | pb << 16, wt, rnd, false) >> (2 * S));
        }
    } else {
        const int y0 = clampi(ys, 0, Hc - 1), y1 = clampi(ys + ny, 0, Hc - 1);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int x0 = clampi(xs + k, 0, Wc - 1), x1 = clampi(xs + k + nx, 0, Wc - 1);
            const int a0 = R[(size_t)y0 * Wc + x0], a1 = R[(size_t)y0 * Wc + x1];
            const int b0 = R[(size_t)y1 * Wc + x0], b1 = R[(size_t)y1 * Wc + x1];
            if constexpr (S == 1)
                out[k] = (a0 + a1 + b0 + b1 + 2) >> 2;
            else
                out[k] = ((D - fx) * (D - fy) * a0 + fx * (D - fy) * a1 + (D - fx) * fy * b0 + fx * fy * b1 +
                          (1 << (2 * S - 1))) >> (2 * S);
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

// mv_frac_bits of the _ex entry points (so_capi.hip, so_decode.hip): the instantiations that exist
inline int check_mv_frac_bits(const char* fn, int mv_frac_bits) {
    if (mv_frac_bits != 1 && mv_frac_bits != 2) {
        set_error("%s: mv_frac_bits %d (1 = full-sample luma vectors, 2 = half-sample)", fn, mv_frac_bits);
        return SO_E_INVALID;
    }
    return SO_OK;
}

}  // namespace so
