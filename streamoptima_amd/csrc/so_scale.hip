// so_scale.hip — separable polyphase resampling of 8-bit 4:2:0 planes (so_scale_yuv420;
// include/streamoptima.h "Scaling" states the arithmetic, tests/scaleref.py restates it).
//
// One launch covers Y, U and V of a batch.  A workgroup of four waves owns a tile of th x 64 samples
// of one destination plane (th = 64 .. 8, chosen on the host from the ratio and the tap count so that
// the LDS below stays within 64 KiB: two or more workgroups per CU at the 32-tap worst case):
//   tables      the tile's tap rows (64 horizontal, th vertical) are copied to LDS once: the passes
//               below read a tap as one broadcast LDS word instead of waiting on global memory
//               for every column and row;
//   window      wave 0 finds the source columns the tile's 64 tap rows touch, wave 1 the source rows
//               (min and max over the clamped table entries, a shuffle reduction);
//   stage       up to `srows` (64) source rows of the window go to LDS as dwords: a dword that lies
//               wholly inside the row segment is one aligned global load (each row is staged at its
//               own address modulo 4, so any base and any pitch keep the loads aligned), the ragged
//               ends are gathered byte by byte.  Nothing outside the source's picture area is read;
//   horizontal  a wave takes four columns j at a time, its lanes the staged rows: the tap row is wave-uniform, the
//               samples come from LDS a byte per lane (row pitch 4 x odd: no bank conflicts), and the
//               6-fractional-bit result goes to the int16 intermediate, stored column-major so that
//               the lanes' stores are contiguous.  Staging and this pass repeat until the window's
//               rows are done; the intermediate never leaves LDS;
//   vertical    a wave takes four output rows i at a time, its lanes the 64 columns: again a wave-uniform tap row,
//               int16 reads at a pitch of 2 x odd, and one contiguous 64-byte store per row.
// The grid covers the PADDED destination planes: samples outside the picture are stored as 128.
// Tables are device memory nobody validated: every index derived from them is clamped twice (to the
// source, then to the staged window) and the sums wrap in uint32, so a bad table gives a wrong
// picture and nothing worse.
#include "so_scale.h"

namespace so {

constexpr int kScaleUnroll = 4;   // columns (rows) a wave works on at once: independent chains hide the LDS latency

SO_DEV int scale_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }
// clamp(first + t, 0, n - 1) for 0 <= t < 32 is unchanged by this, and first + t cannot overflow
SO_DEV int scale_first(int first, int n) { return scale_clamp(first, -kScaleMaxTaps, n); }

SO_DEV void scale_minmax(int& lo, int& hi) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off));
        hi = max(hi, __shfl_xor(hi, off));
    }
}

__global__ void __launch_bounds__(kScaleThreads)
scale_yuv420_kernel(const ScalePtrs ptrs, const ScaleGeom g) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    __shared__ int win[4];   // first and last source column, first and last source row
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);

    int b = blockIdx.x, pl = 0;
    const int nluma = g.p[0].ntx * g.p[0].nty;
    if (b >= nluma) {
        b -= nluma;
        const int nchroma = g.p[1].ntx * g.p[1].nty;
        pl = b >= nchroma ? 2 : 1;
        if (b >= nchroma) b -= nchroma;
    }
    const ScalePlane& P = pl ? g.p[1] : g.p[0];
    const int ty = b / P.ntx, tx = b - ty * P.ntx;
    const int i0 = ty * g.th, j0 = tx * kScaleTileW;
    const uint8_t* src = ptrs.s[pl][blockIdx.y];
    uint8_t* dst = ptrs.d[pl][blockIdx.y];
    const int prow = min(g.th, P.Hp - i0), pcol = min(kScaleTileW, P.Wp - j0);          // of the plane
    const int nr = max(0, min(g.th, P.hd - i0)), nc = max(0, min(kScaleTileW, P.wd - j0));   // of the picture
    const int th_taps = P.h.taps, tv_taps = P.v.taps;

    // LDS: horizontal taps | vertical taps | both `first` lists | staged source rows | intermediate
    int16_t* tab_h = reinterpret_cast<int16_t*>(lds);
    int16_t* tab_v = tab_h + kScaleTileW * kScaleMaxTaps;
    int32_t* tab_first = reinterpret_cast<int32_t*>(tab_v + kScaleTileW * kScaleMaxTaps);
    uint8_t* rows_lds = lds + kScaleTableBytes;
    int16_t* mid = reinterpret_cast<int16_t*>(rows_lds + (size_t)g.srows * g.lpitch);
    int y_lo = 0, nrows = 1;
    if (nr > 0 && nc > 0) {
        {
            const int16_t* ch = P.h.coef + (size_t)j0 * th_taps;
            const int16_t* cv = P.v.coef + (size_t)i0 * tv_taps;
            for (int i = threadIdx.x; i < nc * th_taps; i += kScaleThreads) tab_h[i] = ch[i];
            for (int i = threadIdx.x; i < nr * tv_taps; i += kScaleThreads) tab_v[i] = cv[i];
        }
        if (wave < 2) {
            const int n = wave ? nr : nc, len = wave ? P.hs : P.ws, t = wave ? tv_taps : th_taps;
            const int32_t* first = wave ? P.v.first + i0 : P.h.first + j0;
            int lo = INT32_MAX, hi = INT32_MIN;
            if (lane < n) {
                const int f0 = scale_first(first[lane], len);
                tab_first[kScaleTileW * wave + lane] = f0;
                lo = scale_clamp(f0, 0, len - 1);
                hi = scale_clamp(f0 + t - 1, 0, len - 1);
            }
            scale_minmax(lo, hi);
            if (lane == 0) { win[2 * wave] = lo; win[2 * wave + 1] = hi; }
        }
        __syncthreads();
        const int x_lo = win[0], ncw = min(win[1] - x_lo + 1, P.capw);
        y_lo = win[2];
        nrows = min(win[3] - y_lo + 1, P.caph);
        const int ndw = (ncw + 6) >> 2, lwords = g.lpitch >> 2;
        uint32_t* stage = reinterpret_cast<uint32_t*>(rows_lds);

        for (int s0 = 0; s0 < nrows; s0 += g.srows) {
            const int ns = min(g.srows, nrows - s0);
            if (s0) __syncthreads();   // the horizontal pass has finished with the previous rows
            for (int idx = threadIdx.x; idx < ns * ndw; idx += kScaleThreads) {
                const int r = idx / ndw, d = idx - r * ndw;
                const uint8_t* p = src + (size_t)(y_lo + s0 + r) * P.spitch + x_lo;
                const int k0 = 4 * d - (int)(reinterpret_cast<uintptr_t>(p) & 3);   // dword d starts k0 bytes from p
                uint32_t w = 0;
                if (k0 >= 0 && k0 + 4 <= ncw) {
                    w = *reinterpret_cast<const uint32_t*>(p + k0);
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k0 + k >= 0 && k0 + k < ncw) w |= (uint32_t)p[k0 + k] << (8 * k);
                }
                stage[r * lwords + d] = w;
            }
            __syncthreads();
            const uint8_t* rowp = src + (size_t)(y_lo + s0 + lane) * P.spitch + x_lo;
            const uint8_t* row = rows_lds + lane * g.lpitch + (reinterpret_cast<uintptr_t>(rowp) & 3);
            // four columns at a time: four independent chains of LDS reads and multiply-adds per lane
            for (int jb = wave * kScaleUnroll; jb < nc; jb += (kScaleThreads / 64) * kScaleUnroll) {
                const int16_t* c[kScaleUnroll];
                int f0[kScaleUnroll];
#pragma unroll
                for (int u = 0; u < kScaleUnroll; ++u) {
                    const int j = min(jb + u, nc - 1);   // past the tile's last column: that column again, not stored
                    c[u] = tab_h + j * th_taps;
                    f0[u] = __builtin_amdgcn_readfirstlane(tab_first[j]);   // one value per wave: the index math is scalar
                }
                if (lane < ns) {
                    uint32_t acc[kScaleUnroll] = {};
                    for (int t = 0; t < th_taps; ++t) {
#pragma unroll
                        for (int u = 0; u < kScaleUnroll; ++u) {
                            const int xi = scale_clamp(scale_clamp(f0[u] + t, 0, P.ws - 1) - x_lo, 0, ncw - 1);
                            acc[u] += (uint32_t)__mul24((int)c[u][t], (int)row[xi]);
                        }
                    }
#pragma unroll
                    for (int u = 0; u < kScaleUnroll; ++u) {
                        const int m = (int)(acc[u] + 128u) >> 8;
                        if (jb + u < nc) mid[(jb + u) * g.mpitch + s0 + lane] = (int16_t)scale_clamp(m, -32768, 32767);
                    }
                }
            }
        }
        __syncthreads();
    }

    for (int ib = wave * kScaleUnroll; ib < prow; ib += (kScaleThreads / 64) * kScaleUnroll) {
        int o[kScaleUnroll];
#pragma unroll
        for (int u = 0; u < kScaleUnroll; ++u) o[u] = 128;
        if (ib < nr && lane < nc) {
            const int16_t* c[kScaleUnroll];
            int f0[kScaleUnroll];
#pragma unroll
            for (int u = 0; u < kScaleUnroll; ++u) {
                const int i = min(ib + u, nr - 1);
                c[u] = tab_v + i * tv_taps;
                f0[u] = __builtin_amdgcn_readfirstlane(tab_first[kScaleTileW + i]);
            }
            const int16_t* col = mid + lane * g.mpitch;
            uint32_t acc[kScaleUnroll] = {};
            for (int t = 0; t < tv_taps; ++t) {
#pragma unroll
                for (int u = 0; u < kScaleUnroll; ++u) {
                    const int yi = scale_clamp(scale_clamp(f0[u] + t, 0, P.hs - 1) - y_lo, 0, nrows - 1);
                    acc[u] += (uint32_t)__mul24((int)c[u][t], (int)col[yi]);
                }
            }
#pragma unroll
            for (int u = 0; u < kScaleUnroll; ++u)
                if (ib + u < nr) o[u] = scale_clamp((int)(acc[u] + (1u << 19)) >> 20, 0, 255);
        }
#pragma unroll
        for (int u = 0; u < kScaleUnroll; ++u)
            if (ib + u < prow && lane < pcol) dst[(size_t)(i0 + ib + u) * P.Wp + j0 + lane] = (uint8_t)o[u];
    }
}

size_t scale_lds_bytes(const ScaleGeom& g) {
    return kScaleTableBytes + (size_t)g.srows * g.lpitch + (size_t)kScaleTileW * g.mpitch * sizeof(int16_t);
}

bool scale_tiles(ScaleGeom* g) {
    static const int kRows[] = {64, 32, 16}, kTh[] = {64, 32, 16, 8};
    for (int srows : kRows)
        for (int th : kTh) {
            int capw = 1, caph = 1;
            for (int k = 0; k < (g->nplanes > 1 ? 2 : 1); ++k) {
                ScalePlane& p = g->p[k];
                p.capw = scale_span(kScaleTileW, p.ws, p.wd, p.h.taps);
                p.caph = scale_span(th, p.hs, p.hd, p.v.taps);
                p.ntx = (p.Wp + kScaleTileW - 1) / kScaleTileW;
                p.nty = (p.Hp + th - 1) / th;
                capw = capw > p.capw ? capw : p.capw;
                caph = caph > p.caph ? caph : p.caph;
            }
            g->th = th;
            g->srows = srows;
            g->lpitch = 4 * (((capw + 6) >> 2) | 1);   // the row, up to 3 bytes of alignment, a ragged dword
            g->mpitch = 2 * (((caph + 1) >> 1) | 1);
            if (capw <= (1 << 20) && caph <= (1 << 20) && scale_lds_bytes(*g) <= kScaleLdsBudget) return true;
        }
    return false;
}

int scale_launch(const ScalePtrs& ptrs, int nframes, const ScaleGeom& g, hipStream_t st) {
    unsigned tiles = (unsigned)(g.p[0].ntx * g.p[0].nty);
    if (g.nplanes > 1) tiles += 2u * (unsigned)(g.p[1].ntx * g.p[1].nty);
    hipLaunchKernelGGL(scale_yuv420_kernel, dim3(tiles, nframes), dim3(kScaleThreads), scale_lds_bytes(g), st, ptrs, g);
    return check_launch("scale_yuv420_kernel");
}

}  // namespace so
