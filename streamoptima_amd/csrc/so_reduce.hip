// so_reduce.hip — the small reductions behind so_sum_i32_rows, so_sse_u8 and so_qp_map: kernels
// and launchers (argument validation stays in so_capi.hip).
#include "so_launch.h"

namespace so {

// ---- per-frame sums of the encode kernels' per-block / per-row SSE ---------------------------
struct SumArgs {
    const int32_t* p[kSumMax];
};

// one workgroup of 1024 threads per array: int64 sum of len int32 values into out[blockIdx.x];
// 16-byte loads, eight in flight per thread (a 4K frame's 32,400 per-block values are ~130 KB:
// 256 threads left it latency-bound at 10 us for 30 frames)
constexpr int kSumThreads = 1024;
__global__ void __launch_bounds__(kSumThreads) sum_rows_kernel(const SumArgs a, int len, long long* __restrict__ out) {
    __shared__ long long part[kSumThreads / 64];
    const int32_t* p = a.p[blockIdx.x];
    long long acc = 0;
    const int n4 = (reinterpret_cast<uintptr_t>(p) & 15) ? 0 : len / 4;
    const int4* p4 = reinterpret_cast<const int4*>(p);
    int i = threadIdx.x;
    // guarded loads, all eight issued before the adds (a separate remainder loop ran its loads
    // one round trip at a time: 8 us for a 4K GOP's 30 frames)
    for (; i < n4; i += 8 * kSumThreads) {
        int4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = i + k * kSumThreads < n4 ? p4[i + k * kSumThreads] : make_int4(0, 0, 0, 0);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += (long long)v[k].x + v[k].y + v[k].z + v[k].w;
    }
    for (int j = 4 * n4 + threadIdx.x; j < len; j += kSumThreads) acc += p[j];
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long t = 0;
#pragma unroll
        for (int w = 0; w < kSumThreads / 64; ++w) t += part[w];
        out[blockIdx.x] = t;
    }
}

int sum_rows_launch(const int32_t* const* rows, int n, int len, int64_t* out, hipStream_t st) {
    SumArgs a{};
    for (int i = 0; i < n; ++i) a.p[i] = rows[i];
    hipLaunchKernelGGL(sum_rows_kernel, dim3(n), dim3(kSumThreads), 0, st, a, len, reinterpret_cast<long long*>(out));
    return check_launch("sum_rows_kernel");
}

// ---- SSE (PSNR) -------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) sse_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                  int64_t n, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long part[4];
    unsigned long long acc = 0;
    const int64_t n16 = n / 16;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) {
        const uint4 va = reinterpret_cast<const uint4*>(a)[i];
        const uint4 vb = reinterpret_cast<const uint4*>(b)[i];
        const uint32_t wa[4] = {va.x, va.y, va.z, va.w}, wb[4] = {vb.x, vb.y, vb.z, vb.w};
        uint32_t s = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int d = (int)((wa[k] >> (8 * e)) & 255) - (int)((wb[k] >> (8 * e)) & 255);
                s += (uint32_t)(d * d);
            }
        acc += s;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = n16 * 16; i < n; ++i) {
            const int d = (int)a[i] - (int)b[i];
            acc += (unsigned long long)(d * d);
        }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, part[0] + part[1] + part[2] + part[3]);
}

int sse_launch(const uint8_t* a, const uint8_t* b, int64_t n, uint64_t* out, hipStream_t st) {
    int64_t blocks = (n / 16 + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(sse_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, b, n,
                       reinterpret_cast<unsigned long long*>(out));
    return check_launch("sse_kernel");
}

// Per-block QP map (build extension, DESIGN.md "ROI and two-pass rate control"): one
// workgroup per block row.  Two-pass: with pass-1 token counts t (stripe-local records) the
// row mean is m / n (m = sum, n = blocks per row) and
//   delta = [t n >= 2m] + [t n >= 4m] - [2 t n < m] - [4 t n < m]      (in [-2, 2], exact)
// i.e. blocks at >= 2x / 4x the row's mean bits are quantised 1 / 2 QP coarser and blocks at
// < 1/2 / < 1/4 of it 1 / 2 QP finer.  qp = clamp(base + delta + roi, qp_lo, qp_hi) with
// base = qp_row[by] (rate-control schedule) or qp_rd.  tokens == NULL: ROI only (delta 0).
__global__ void __launch_bounds__(256)
qp_map_kernel(const int32_t* __restrict__ tokens, int nbx, int by0, int qp_rd, const int32_t* __restrict__ qp_row,
              const int32_t* __restrict__ roi, int qp_lo, int qp_hi, int32_t* __restrict__ out) {
    __shared__ long long part[4];
    const int by = by0 + blockIdx.x;
    const int32_t* t = tokens ? tokens + (size_t)blockIdx.x * nbx : nullptr;
    long long m = 0;
    if (t) {
        for (int bx = threadIdx.x; bx < nbx; bx += blockDim.x) m += t[bx];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) m += __shfl_xor(m, s, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
        __syncthreads();
        m = part[0] + part[1] + part[2] + part[3];
    }
    const int base = qp_row ? qp_row[by] : qp_rd;
    for (int bx = threadIdx.x; bx < nbx; bx += blockDim.x) {
        int d = 0;
        if (t) {
            const long long tn = (long long)t[bx] * nbx;
            d = (tn >= 2 * m) + (tn >= 4 * m) - (2 * tn < m) - (4 * tn < m);
        }
        int q = base + d + (roi ? roi[(size_t)by * nbx + bx] : 0);
        q = q < qp_lo ? qp_lo : (q > qp_hi ? qp_hi : q);
        out[(size_t)by * nbx + bx] = q;
    }
}

int qp_map_launch(const int32_t* tokens, int nbx, int by0, int by1, int qp_rd, const int32_t* qp_row,
                  const int32_t* roi, int qp_lo, int qp_hi, int32_t* out, hipStream_t st) {
    hipLaunchKernelGGL(qp_map_kernel, dim3(by1 - by0), dim3(256), 0, st, tokens, nbx, by0, qp_rd, qp_row, roi, qp_lo,
                       qp_hi, out);
    return check_launch("qp_map_kernel");
}

}  // namespace so
