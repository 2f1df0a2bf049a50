// so_chroma.hip — 4:2:0 chroma (U and V) encode and reconstruction from the luma frame's motion,
// for gfx950.  The reference codes luma only; the chroma arithmetic is this project's own
// (DESIGN.md "Chroma 4:2:0") built from the reference's per-block functions at N = 8.
//
// Luma block b = (bx, by) of a 16x16 grid owns the 8x8 block at (8 bx, 8 by) of each chroma
// plane (Hc x Wc = H/2 x W/2, pitch Wc).  Per block:
//   prediction  I-frame: 128.  P-frame: the luma MV (dx, dy, r) of the block -- of its 4x4
//               quadrant when the luma block is split -- halved: ix = dx >> 1, fx = dx & 1,
//               P = (R[y0][x0] + R[y0][x1] + R[y1][x0] + R[y1][x1] + 2) >> 2 with
//               x0 = clamp(X + ix), x1 = clamp(X + ix + fx) (y alike) on the chroma
//               reconstruction R of reference clamp(r, 0, nref - 1).  That is the case S = 1
//               of chroma_pred4<S> (so_chroma.h); with half-sample luma vectors (FME,
//               mv_frac_bits = 2) the S = 2 instantiation weights the four taps by the
//               quarter-sample phase;
//   transform   residual -> apply_2d_dct (Encoder.py:779) -> quantize_TC (:787) with
//               generate_Q_matrix(8, qpc) (:938) -> len(entropy_encoder_block) (:1086) ->
//               rescale_QTC (:820) -> apply_2d_idct (:810) -> (P + idct).astype(uint8) (:824);
//   qpc         clamp(base + qp_offset, 0, 20), base = the block's QP-map entry, else its
//               row's qp_row entry, else the frame QP.
// One kernel template (x S): ENC = true is the encoder (residual .. reconstruction, tokens, SSE),
// ENC = false the decoder (qtc -> reconstruction).  One launch covers both planes: task
// t < nb is block t of U, t >= nb block t - nb of V.  8 lanes of a wavefront own a block
// (lane l = block row l, so_block.h), 32 blocks per 256-thread workgroup, an 8 x 9 FP64 LDS
// transpose tile per block, wave-scope synchronisation only.
#include "so_block.h"
#include "so_chroma.h"

namespace so {

template <bool ENC, int S>
__global__ void __launch_bounds__(256) chroma_kernel(const ChromaArgs a) {
    constexpr int N = 8, P = N + 1, G = 256 / N;
    __shared__ double lds[G * N * P];
    const int g = threadIdx.x / N, l = threadIdx.x % N;
    const int t = blockIdx.x * G + g;
    if (t >= 2 * a.nb) return;   // the whole lane group leaves; only wave-scope exchange below
    const int pi = t >= a.nb ? 1 : 0, b = t - pi * a.nb;
    const ChromaPlanes& pl = a.pl[pi];
    const int bx = b % a.nbx, by = b / a.nbx, X = bx * N, Y = by * N + l;
    double* s = lds + g * N * P;

    const int base = a.qp_map ? a.qp_map[b] : (a.qp_row ? a.qp_row[by] : a.qp);
    const int qpc = clampi(base + a.qp_offset, 0, 20);

    int pred[N];
    if (a.frame_type == 0) {
#pragma unroll
        for (int c = 0; c < N; ++c) pred[c] = 128;
    } else {
        const int16_t* m = a.mv + (size_t)b * 12;
        const int q0 = a.split[b] ? 2 * (l >> 2) : 0, q1 = a.split[b] ? q0 + 1 : 0;   // Z order
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int16_t* mq = m + 3 * (h ? q1 : q0);
            const int dx = mq[0], dy = mq[1], r = clampi(mq[2], 0, a.nref - 1);
            chroma_pred4<S>(pick_ref(pl.refs, r), a.Wc, a.Hc, X + 4 * h, Y, dx, dy, pred + 4 * h);
        }
    }

    int q[N], crow[N];
    if constexpr (ENC) {
        load_cur_row<N>(pl.cur, a.Wc, X, Y, crow);
        int res[N];
#pragma unroll
        for (int c = 0; c < N; ++c) res[c] = crow[c] - pred[c];
        double tcr[N];
        xform2d_rows<N, false>(s, l, res, tcr);
        int tc[N];
#pragma unroll
        for (int c = 0; c < N; ++c) tc[c] = (int)__builtin_rint(tcr[c]);   // np.round(...).astype(int)
        quant_row_i<N>(tc, l, qpc, q);
        store_row_i16<N>(pl.qtc + (size_t)b * N * N + l * N, q);
        const int tok = block_tokens<N>(nullptr, l, q);
        if (l == 0) a.tokens[(size_t)pi * a.nb + b] = tok;
    } else {
        load_row_i16<N>(pl.qtc + (size_t)b * N * N + l * N, q);
    }

    double dq[N], rd[N];
    dequant_row_i<N>(q, l, qpc, dq);
    xform2d_rows<N, true>(s, l, dq, rd);
    int rec[N];
#pragma unroll
    for (int c = 0; c < N; ++c) rec[c] = pred[c] + (int)__builtin_rint(rd[c]);
    store_row_u8<N>(pl.recon, a.Wc, X, Y, rec);   // astype(uint8): mod 256
    if constexpr (ENC) {
        int sse = 0;
#pragma unroll
        for (int c = 0; c < N; ++c) {
            const int d = crow[c] - (rec[c] & 255);
            sse += d * d;
        }
        sse = group_sum<N>(sse);
        if (l == 0) a.sse[(size_t)pi * a.nb + b] = sse;
    }
}

int chroma_launch(const ChromaArgs& a, bool encode, hipStream_t st) {
    const dim3 grid((2 * a.nb + 31) / 32), blk(256);
    if (a.mv_frac_bits == 2) {
        if (encode)
            hipLaunchKernelGGL((chroma_kernel<true, 2>), grid, blk, 0, st, a);
        else
            hipLaunchKernelGGL((chroma_kernel<false, 2>), grid, blk, 0, st, a);
    } else if (encode) {
        hipLaunchKernelGGL((chroma_kernel<true, 1>), grid, blk, 0, st, a);
    } else {
        hipLaunchKernelGGL((chroma_kernel<false, 1>), grid, blk, 0, st, a);
    }
    return check_launch("chroma_kernel");
}

}  // namespace so
