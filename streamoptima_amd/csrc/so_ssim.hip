// so_ssim.hip — per-frame SSIM of uint8 plane pairs (so_ssim_u8, include/streamoptima.h):
// skimage.metrics.structural_similarity(a, b, win_size=win) as the reference calls it
// (Encoder.py:935): uniform win x win window, sample covariance, K1 0.01, K2 0.03, data range
// 255, the mean over the windows that lie fully inside the picture.  DESIGN.md "Device SSIM".
//
// One workgroup (256 threads) per tile of 16 x 64 window positions of one frame:
//   1. the tile's (16 + win - 1) x (64 + win - 1) pixels of both planes go into LDS as the
//      aligned 32-bit words that hold them (a row's first pixel sits `address & 3` bytes into
//      its LDS row, so planes of any base alignment and pitch load as whole words);
//   2. horizontal box sums of x, y, x^2, y^2, xy per LDS row, sliding over 8 columns, in integers
//      (sum x | sum y << 16 in one word: 15 * 15 * 255 < 2^16 holds for the 2-D sums too);
//   3. each thread slides the vertical sums down 4 positions of one column and evaluates S in
//      FP64 from the exact integer sums (every intermediate integer is below 2^53);
//   4. the tile's sum of S, reduced in a fixed order, is stored to the caller's workspace.
// A second kernel adds a frame's partials in a fixed order and divides by the window count:
// no floating-point atomics, the same bits from run to run and for any batching.
#include "so_common.h"
#include "so_launch.h"

#pragma clang fp contract(off)   // an identical pair must give exactly 1.0 (no FMA on one side only)

namespace so {

constexpr int kSsimTH = 16, kSsimTW = 64;   // window positions per tile
constexpr int kSsimThreads = 256;
constexpr int kSsimPos = kSsimTH * kSsimTW / kSsimThreads;   // positions per thread, down one column
constexpr int kSsimMaxWin = 15;
constexpr int kSsimRows = kSsimTH + kSsimMaxWin - 1;                    // 30 pixel rows at most
constexpr int kSsimRowWords = (3 + kSsimTW + kSsimMaxWin - 1 + 3) / 4;  // 21: odd, rows spread over the banks
// the last horizontal run (columns 56..63) reads words up to 14 + (3 + win - 1) / 4 + 2 of its row
static_assert((kSsimTW / 8 - 1) * 2 + (3 + kSsimMaxWin - 1) / 4 + 2 < kSsimRowWords, "row words");
static_assert((kSsimTW / 8 - 1) * 2 + 4 < kSsimRowWords, "row words (leaving bytes)");
constexpr int kSsimLoads = (2 * kSsimRows * kSsimRowWords + kSsimThreads - 1) / kSsimThreads;   // words per thread
constexpr int kSsimHStride = kSsimTW + 1;                               // uint4 per row of sums (+1: bank spread)
constexpr int kSsimBatch = 32;                                          // frames per launch (pointers by value)
constexpr int kSsimSeg = 8;                                             // columns per horizontal sliding run
static_assert(kSsimRowWords % 2 == 1, "odd word stride");
static_assert(kSsimTH * kSsimTW == kSsimPos * kSsimThreads && kSsimTW == 64, "a lane per column, a wave per kSsimPos rows");
static_assert(kSsimTH - 1 + kSsimMaxWin - 1 < kSsimRows, "the unrolled vertical pass stays inside hs");

struct SsimArgs {
    const uint8_t* a[kSsimBatch];
    const uint8_t* b[kSsimBatch];
};

SO_DEV double ssim_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// out[0..4) = the 16 bytes starting t bytes into the aligned words w[0..]; reads w[t / 4 .. t / 4 + 4]
SO_DEV void ssim_bytes16(const uint32_t* w, int t, uint32_t out[4]) {
    const uint32_t* q = w + (t >> 2);
    uint32_t v[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) v[i] = q[i];
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = __builtin_amdgcn_alignbyte(v[i + 1], v[i], (uint32_t)(t & 3));
}

// the same for 8 bytes; reads w[t / 4 .. t / 4 + 2]
SO_DEV void ssim_bytes8(const uint32_t* w, int t, uint32_t out[2]) {
    const uint32_t* q = w + (t >> 2);
    uint32_t v[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) v[i] = q[i];
#pragma unroll
    for (int i = 0; i < 2; ++i) out[i] = __builtin_amdgcn_alignbyte(v[i + 1], v[i], (uint32_t)(t & 3));
}

SO_DEV uint32_t ssim_byte(const uint32_t* v, int k) { return (v[k >> 2] >> (8 * (k & 3))) & 255u; }

__global__ void __launch_bounds__(kSsimThreads)
ssim_tile_kernel(const SsimArgs args, int H, int W, size_t pitch_a, size_t pitch_b, int win, int tiles_x,
                 double* __restrict__ ws) {
    __shared__ uint32_t raw[2][kSsimRows * kSsimRowWords];
    __shared__ uint4 hs[kSsimRows * kSsimHStride];
    __shared__ double part[kSsimThreads / 64];
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * kSsimTH, x0 = tx * kSsimTW;
    // pixel rows / columns of the tile that exist (the last tiles are cut by the picture)
    const int R = min(kSsimTH + win - 1, H - y0);
    const int C = min(kSsimTW + win - 1, W - x0);
    const uint8_t* ga = args.a[blockIdx.y] + (size_t)y0 * pitch_a + x0;   // the tile's first pixels
    const uint8_t* gb = args.b[blockIdx.y] + (size_t)y0 * pitch_b + x0;
    const uintptr_t pa = reinterpret_cast<uintptr_t>(ga), pb = reinterpret_cast<uintptr_t>(gb);

    // 1. the aligned words holding pixels [x0, x0 + C) of rows [y0, y0 + R): every load of a
    // thread is issued before the first LDS store waits for one
    uint32_t word[kSsimLoads];
    int slot[kSsimLoads];   // LDS word of raw[0..1], -1: nothing to load
#pragma unroll
    for (int u = 0; u < kSsimLoads; ++u) {
        const int it = tid + u * kSsimThreads;
        const int pl = it >= R * kSsimRowWords;
        const int k = it - pl * R * kSsimRowWords;
        const int r = k / kSsimRowWords, j = k - r * kSsimRowWords;
        const uint8_t* p = (pl ? gb : ga) + (size_t)r * (pl ? pitch_b : pitch_a);
        const int sh = (int)(reinterpret_cast<uintptr_t>(p) & 3);
        const bool ok = it < 2 * R * kSsimRowWords && 4 * j < sh + C;
        slot[u] = ok ? pl * (kSsimRows * kSsimRowWords) + r * kSsimRowWords + j : -1;
        // unconditional and branch-free (a lane with nothing to load re-reads the tile's first
        // word): after a branch every load would wait for the one before it
        const ptrdiff_t off = ok ? (ptrdiff_t)r * (ptrdiff_t)(pl ? pitch_b : pitch_a) + 4 * j - sh : -(ptrdiff_t)(pl ? pb & 3 : pa & 3);
        word[u] = *reinterpret_cast<const uint32_t*>((pl ? gb : ga) + off);
    }
#pragma unroll
    for (int u = 0; u < kSsimLoads; ++u)
        if (slot[u] >= 0) (&raw[0][0])[slot[u]] = word[u];
    __syncthreads();

    // 2. horizontal sums: a thread slides along 8 columns of one row (lanes on different rows).
    // The row's bytes are taken as aligned words and shifted into place (v_alignbyte): 16 bytes
    // from the run's first pixel (the first win - 1 start the sums, the first 8 leave the window)
    // and the 8 that enter it (win - 1 further on).
    for (int it = tid; it < R * (kSsimTW / kSsimSeg); it += kSsimThreads) {
        const int s = it / R, r = it - s * R;
        const uint32_t* wa = raw[0] + r * kSsimRowWords + (kSsimSeg / 4) * s;
        const uint32_t* wb = raw[1] + r * kSsimRowWords + (kSsimSeg / 4) * s;
        const int sha = (int)((pa + (size_t)r * pitch_a) & 3), shb = (int)((pb + (size_t)r * pitch_b) & 3);
        uint32_t oa[4], ob[4], na[2], nb[2];   // old (leaving) and new (entering) bytes of a and b
        ssim_bytes16(wa, sha, oa);
        ssim_bytes16(wb, shb, ob);
        ssim_bytes8(wa, sha + win - 1, na);
        ssim_bytes8(wb, shb + win - 1, nb);
        uint32_t s1 = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
        for (int k = 0; k < kSsimMaxWin - 1; ++k)
            if (k < win - 1) {
                const uint32_t x = ssim_byte(oa, k), y = ssim_byte(ob, k);
                s1 += x | (y << 16); sxx += x * x; syy += y * y; sxy += x * y;
            }
        uint4* dst = hs + r * kSsimHStride + kSsimSeg * s;
#pragma unroll
        for (int j = 0; j < kSsimSeg; ++j) {
            uint32_t x = ssim_byte(na, j), y = ssim_byte(nb, j);
            s1 += x | (y << 16); sxx += x * x; syy += y * y; sxy += x * y;
            dst[j] = make_uint4(s1, sxx, syy, sxy);
            x = ssim_byte(oa, j); y = ssim_byte(ob, j);
            s1 -= x | (y << 16); sxx -= x * x; syy -= y * y; sxy -= x * y;
        }
    }
    __syncthreads();

    // 3. vertical sums and S: lane = column, wave = kSsimPos rows of positions
    const int c = tid & 63, g = tid >> 6;
    const int nv = x0 + c <= W - win ? min(kSsimPos, H - win + 1 - (y0 + kSsimPos * g)) : 0;   // positions of this thread
    double acc = 0.0;
    if (nv > 0) {
        const double np = (double)(win * win);
        const double inv_np = 1.0 / np, cov = 1.0 / (np * (np - 1.0));
        const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
        const uint4* col = hs + (kSsimPos * g) * kSsimHStride + c;
        uint32_t s1 = 0, sxx = 0, syy = 0, sxy = 0;
        for (int k = 0; k < win - 1; ++k) {
            const uint4 v = col[k * kSsimHStride];
            s1 += v.x; sxx += v.y; syy += v.z; sxy += v.w;
        }
        // all the positions, unrolled so that their FP64 chains overlap; positions past nv read
        // rows of hs that exist but may hold anything, and their S is dropped by the select
#pragma unroll
        for (int i = 0; i < kSsimPos; ++i) {
            uint4 v = col[(i + win - 1) * kSsimHStride];
            s1 += v.x; sxx += v.y; syy += v.z; sxy += v.w;
            const double sx = (double)(s1 & 0xffffu), sy = (double)(s1 >> 16);
            const double ux = sx * inv_np, uy = sy * inv_np;
            const double vx = (np * (double)sxx - sx * sx) * cov;
            const double vy = (np * (double)syy - sy * sy) * cov;
            const double vxy = (np * (double)sxy - sx * sy) * cov;
            const double S = ((2.0 * ux * uy + C1) * (2.0 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
            acc += i < nv ? S : 0.0;
            v = col[i * kSsimHStride];
            s1 -= v.x; sxx -= v.y; syy -= v.z; sxy -= v.w;
        }
    }

    // 4. the tile's partial
    acc = ssim_wave_sum(acc);
    if (c == 0) part[g] = acc;
    __syncthreads();
    if (tid == 0) ws[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

// out[f] = (sum of frame f's tile partials, in a fixed order) / window positions
__global__ void __launch_bounds__(kSsimThreads)
ssim_mean_kernel(const double* __restrict__ ws, int ntiles, double count, double* __restrict__ out) {
    __shared__ double part[kSsimThreads / 64];
    const double* p = ws + (size_t)blockIdx.x * ntiles;
    double t = 0.0;
    for (int i = threadIdx.x; i < ntiles; i += kSsimThreads) t += p[i];
    t = ssim_wave_sum(t);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = (((part[0] + part[1]) + part[2]) + part[3]) / count;
}

// tiles of one frame (0 for a geometry so_ssim_u8 rejects)
size_t ssim_tiles(int H, int W, int win) {
    if (win < 3 || win > kSsimMaxWin || win % 2 == 0 || H < win || W < win) return 0;
    const size_t ty = ((size_t)(H - win + 1) + kSsimTH - 1) / kSsimTH;
    const size_t tx = ((size_t)(W - win + 1) + kSsimTW - 1) / kSsimTW;
    return tx * ty;
}

int ssim_launch(const uint8_t* const* a, const uint8_t* const* b, int nframes, int H, int W, size_t pitch_a,
                size_t pitch_b, int win, double* out, double* ws, hipStream_t st) {
    const int tiles_x = (W - win + 1 + kSsimTW - 1) / kSsimTW;
    const int ntiles = (int)ssim_tiles(H, W, win);
    for (int f0 = 0; f0 < nframes; f0 += kSsimBatch) {
        const int m = nframes - f0 < kSsimBatch ? nframes - f0 : kSsimBatch;
        SsimArgs args{};
        for (int i = 0; i < m; ++i) {
            args.a[i] = a[f0 + i];
            args.b[i] = b[f0 + i];
        }
        hipLaunchKernelGGL(ssim_tile_kernel, dim3(ntiles, m), dim3(kSsimThreads), 0, st, args, H, W, pitch_a, pitch_b,
                           win, tiles_x, ws + (size_t)f0 * ntiles);
        const int rc = check_launch("ssim_tile_kernel");
        if (rc != SO_OK) return rc;
    }
    const double count = (double)(H - win + 1) * (double)(W - win + 1);
    hipLaunchKernelGGL(ssim_mean_kernel, dim3(nframes), dim3(kSsimThreads), 0, st, ws, ntiles, count, out);
    return check_launch("ssim_mean_kernel");
}

}  // namespace so
