// so_colour.hip — 8-bit RGB <-> the codec's padded 4:2:0 planes (so_rgb_to_yuv420, so_yuv420_to_rgb;
// include/streamoptima.h "Colour conversion" states the arithmetic, tests/colourref.py restates it).
//
// Pure streaming kernels: every source byte is read once, every destination byte written once, no
// LDS, no atomics.  A lane owns a cell of 2 rows x 8 pixels, so the four 2 x 2 chroma sums of the
// cell never leave its registers:
//   forward  reads 2 x 24 B (hwc) or 3 x 2 x 8 B (chw), writes 2 x 8 B of Y and 4 B each of U, V;
//   inverse  the other way round.
// The 64 lanes of a wave sit side by side on one pair of rows, so a wave's loads and stores of a row
// are one contiguous run (1536 B of hwc, 512 B of Y, 256 B of U).
// A row segment goes as dwords when the lane's whole 8-pixel cell lies inside the row AND the
// segment's address is dword-aligned; otherwise that segment alone goes byte by byte (a cell cut by
// the picture's or the plane's right edge, a pitch or a base that is not a multiple of 4, such as
// hwc rows of 50 pixels).  Nothing outside the source's picture area is read; nothing outside the
// destination planes (forward) or the destination's picture area (inverse) is written.
// The forward grid covers the PADDED planes: a lane whose pixels lie outside the picture stores 128.
#include "so_colour.h"

namespace so {

constexpr int kHwc = SO_LAYOUT_HWC, kChw = SO_LAYOUT_CHW;

template <int NW>
struct __attribute__((packed, aligned(4))) ColourWords {
    uint32_t v[NW];
};

// out[0 .. NW) = n bytes at p (the rest 0), n <= 4 NW
template <int NW>
SO_DEV void colour_load(const uint8_t* p, int n, uint32_t* out) {
    if (n == 4 * NW && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        const ColourWords<NW> w = *reinterpret_cast<const ColourWords<NW>*>(p);
#pragma unroll
        for (int i = 0; i < NW; ++i) out[i] = w.v[i];
        return;
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) out[i] = 0;
#pragma unroll
    for (int i = 0; i < 4 * NW; ++i)
        if (i < n) out[i >> 2] |= (uint32_t)p[i] << (8 * (i & 3));
}

// the first n bytes of w[0 .. NW) to p, n <= 4 NW
template <int NW>
SO_DEV void colour_store(uint8_t* p, int n, const uint32_t* w) {
    if (n == 4 * NW && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        ColourWords<NW> o;
#pragma unroll
        for (int i = 0; i < NW; ++i) o.v[i] = w[i];
        *reinterpret_cast<ColourWords<NW>*>(p) = o;
        return;
    }
#pragma unroll
    for (int i = 0; i < 4 * NW; ++i)
        if (i < n) p[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}

SO_DEV int colour_byte(const uint32_t* w, int i) { return (int)((w[i >> 2] >> (8 * (i & 3))) & 255u); }
// clip(v >> S, 0, 255), the clamp taken before the shift: 0 <= v < 2^(8 + S) is exactly the range
// whose shifted value lies in 0..255
template <int S>
SO_DEV int colour_clip_shr(int v) { return min(max(v, 0), (256 << S) - 1) >> S; }
// c * x for a table entry (|c| < 2^18) and a sample, a cell sum or a centred sample (|x| <= 1020):
// both fit 24 signed bits and the product fits int32, so the full-rate 24-bit multiply is exact
// (v_mad_i32_i24 with the addition that follows; a 32-bit v_mul_lo is quarter rate)
SO_DEV int colour_mul(int c, int x) { return __mul24(c, x); }

// channel c of pixel p of a row held as 6 words (hwc: byte 3 p + c) or as 3 x 2 words (chw)
template <int LAYOUT>
SO_DEV int colour_px(const uint32_t* row, int p, int c) {
    return LAYOUT == kHwc ? colour_byte(row, 3 * p + c) : colour_byte(row + 2 * c, p);
}

template <int LAYOUT>
__global__ void __launch_bounds__(kColourThreads)
rgb_to_yuv420_kernel(const ColourPtrs ptrs, const ColourGeom g) {
    const int ncx = (g.Wp + kColourCellW - 1) / kColourCellW;
    const int idx = blockIdx.x * kColourThreads + threadIdx.x;
    const int cy = idx / ncx, cx = idx - cy * ncx;
    if (cy >= (g.Hp >> 1)) return;
    const int x0 = cx * kColourCellW, y0 = 2 * cy;
    const int nd = min(kColourCellW, g.Wp - x0);                              // pixels of the plane (even)
    const int nv = y0 < g.h ? max(0, min(kColourCellW, g.w - x0)) : 0;        // ... of the picture (even)
    const int f = blockIdx.y;

    uint32_t src[2][6];
    if (nv > 0) {
        const uint8_t* base = ptrs.rgb[f];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint8_t* row = base + (size_t)(y0 + r) * g.pitch;
            if (LAYOUT == kHwc) {
                colour_load<6>(row + 3 * x0, 3 * nv, src[r]);
            } else {
#pragma unroll
                for (int c = 0; c < 3; ++c) colour_load<2>(row + (size_t)c * g.plane + x0, nv, src[r] + 2 * c);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) (&src[0][0])[i] = 0;
    }

    const int yadd = (g.yoff << 16) + 32768, cadd = (128 << 18) + (1 << 17);
    uint32_t yw[2][2] = {{0, 0}, {0, 0}}, uw = 0, vw = 0;
#pragma unroll
    for (int j = 0; j < kColourCellW / 2; ++j) {
        int sr = 0, sg = 0, sb = 0;
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int p = 2 * j; p < 2 * j + 2; ++p) {
                const int R = colour_px<LAYOUT>(src[r], p, 0), G = colour_px<LAYOUT>(src[r], p, 1),
                          B = colour_px<LAYOUT>(src[r], p, 2);
                sr += R; sg += G; sb += B;
                const int Y = colour_clip_shr<16>(colour_mul(g.c[0], R) + colour_mul(g.c[1], G) + colour_mul(g.c[2], B) + yadd);
                yw[r][p >> 2] |= (uint32_t)(p < nv ? Y : 128) << (8 * (p & 3));
            }
        const int U = colour_clip_shr<18>(colour_mul(g.c[3], sr) + colour_mul(g.c[4], sg) + colour_mul(g.c[5], sb) + cadd);
        const int V = colour_clip_shr<18>(colour_mul(g.c[6], sr) + colour_mul(g.c[7], sg) + colour_mul(g.c[8], sb) + cadd);
        uw |= (uint32_t)(2 * j < nv ? U : 128) << (8 * j);
        vw |= (uint32_t)(2 * j < nv ? V : 128) << (8 * j);
    }

    uint8_t* yp = ptrs.y[f] + (size_t)y0 * g.Wp + x0;
    colour_store<2>(yp, nd, yw[0]);
    colour_store<2>(yp + g.Wp, nd, yw[1]);
    const size_t co = (size_t)cy * (g.Wp >> 1) + (x0 >> 1);
    colour_store<1>(ptrs.u[f] + co, nd >> 1, &uw);
    colour_store<1>(ptrs.v[f] + co, nd >> 1, &vw);
}

template <int LAYOUT>
__global__ void __launch_bounds__(kColourThreads)
yuv420_to_rgb_kernel(const ColourPtrs ptrs, const ColourGeom g) {
    const int ncx = (g.w + kColourCellW - 1) / kColourCellW;
    const int idx = blockIdx.x * kColourThreads + threadIdx.x;
    const int cy = idx / ncx, cx = idx - cy * ncx;
    if (cy >= (g.h >> 1)) return;
    const int x0 = cx * kColourCellW, y0 = 2 * cy;
    const int nv = min(kColourCellW, g.w - x0);                               // pixels of the picture (even)
    const int f = blockIdx.y;

    uint32_t yw[2][2], uw, vw;
    const uint8_t* yp = ptrs.y[f] + (size_t)y0 * g.Wp + x0;
    colour_load<2>(yp, nv, yw[0]);
    colour_load<2>(yp + g.Wp, nv, yw[1]);
    const size_t co = (size_t)cy * (g.Wp >> 1) + (x0 >> 1);
    colour_load<1>(ptrs.u[f] + co, nv >> 1, &uw);
    colour_load<1>(ptrs.v[f] + co, nv >> 1, &vw);

    uint32_t dst[2][6] = {{0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0}};
#pragma unroll
    for (int j = 0; j < kColourCellW / 2; ++j) {
        const int U = colour_byte(&uw, j) - 128, V = colour_byte(&vw, j) - 128;
        int cc[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) cc[c] = colour_mul(g.c[3 * c + 1], U) + colour_mul(g.c[3 * c + 2], V) + 32768;
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int p = 2 * j; p < 2 * j + 2; ++p) {
                const int Y = colour_byte(yw[r], p) - g.yoff;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint32_t o = (uint32_t)colour_clip_shr<16>(colour_mul(g.c[3 * c], Y) + cc[c]);
                    const int i = LAYOUT == kHwc ? 3 * p + c : 8 * c + p;     // byte of the row's words
                    dst[r][i >> 2] |= o << (8 * (i & 3));
                }
            }
    }

    uint8_t* base = ptrs.rgb[f];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        uint8_t* row = base + (size_t)(y0 + r) * g.pitch;
        if (LAYOUT == kHwc) {
            colour_store<6>(row + 3 * x0, 3 * nv, dst[r]);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) colour_store<2>(row + (size_t)c * g.plane + x0, nv, dst[r] + 2 * c);
        }
    }
}

template <typename K>
static int colour_launch(K kernel, const char* name, ColourPtrs& p, int m, int cells, const ColourGeom& g,
                         hipStream_t st) {
    const unsigned blocks = (unsigned)((cells + kColourThreads - 1) / kColourThreads);
    hipLaunchKernelGGL(kernel, dim3(blocks, m), dim3(kColourThreads), 0, st, p, g);
    return check_launch(name);
}

int colour_forward_launch(int layout, const uint8_t* const* rgb, uint8_t* const* y, uint8_t* const* u,
                          uint8_t* const* v, int nframes, const ColourGeom& g, hipStream_t st) {
    const int cells = ((g.Wp + kColourCellW - 1) / kColourCellW) * (g.Hp / 2);
    for (int f0 = 0; f0 < nframes; f0 += kColourBatch) {
        const int m = nframes - f0 < kColourBatch ? nframes - f0 : kColourBatch;
        ColourPtrs p{};
        for (int i = 0; i < m; ++i) {
            p.rgb[i] = const_cast<uint8_t*>(rgb[f0 + i]);
            p.y[i] = y[f0 + i]; p.u[i] = u[f0 + i]; p.v[i] = v[f0 + i];
        }
        const int rc = layout == kHwc ? colour_launch(rgb_to_yuv420_kernel<kHwc>, "rgb_to_yuv420_kernel<hwc>", p, m, cells, g, st)
                                      : colour_launch(rgb_to_yuv420_kernel<kChw>, "rgb_to_yuv420_kernel<chw>", p, m, cells, g, st);
        if (rc != SO_OK) return rc;
    }
    return SO_OK;
}

int colour_inverse_launch(int layout, const uint8_t* const* y, const uint8_t* const* u, const uint8_t* const* v,
                          uint8_t* const* rgb, int nframes, const ColourGeom& g, hipStream_t st) {
    const int cells = ((g.w + kColourCellW - 1) / kColourCellW) * (g.h / 2);
    for (int f0 = 0; f0 < nframes; f0 += kColourBatch) {
        const int m = nframes - f0 < kColourBatch ? nframes - f0 : kColourBatch;
        ColourPtrs p{};
        for (int i = 0; i < m; ++i) {
            p.rgb[i] = rgb[f0 + i];
            p.y[i] = const_cast<uint8_t*>(y[f0 + i]);
            p.u[i] = const_cast<uint8_t*>(u[f0 + i]);
            p.v[i] = const_cast<uint8_t*>(v[f0 + i]);
        }
        const int rc = layout == kHwc ? colour_launch(yuv420_to_rgb_kernel<kHwc>, "yuv420_to_rgb_kernel<hwc>", p, m, cells, g, st)
                                      : colour_launch(yuv420_to_rgb_kernel<kChw>, "yuv420_to_rgb_kernel<chw>", p, m, cells, g, st);
        if (rc != SO_OK) return rc;
    }
    return SO_OK;
}

}  // namespace so
