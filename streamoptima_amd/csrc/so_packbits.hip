// so_packbits.hip — the packed symbol stream in the "bits" coding: the symbols of so_pack.hip
// (split, mv values, the RLE token list of every (sub-)block, per block in raster order) as
// bit-granular Exp-Golomb codes instead of byte-granular varints.  The format is normative in
// include/streamoptima.h (so_pack_frames_bits); in short, MSB-first within each byte:
//     split (1 bit) | k (2 bits) | mv values se | tokens se, coefficient values se_k | zero pad
// with ue(z) = bit_length(z + 1) - 1 zeros then z + 1, ue_k(z) = ue(z >> k) then the low k bits
// of z, se / se_k on zz(v), and k the order in 0..3 that minimises the block's coefficient bits
// (ties to the smallest).  Every block starts on a byte, so blocks decode in parallel from the
// same per-block byte offsets as the varint stream.
//
// Two facts the kernels lean on:
//   * ue_k(z) is the integer z + 2^k written in 2 * bit_length((z >> k) + 1) - 1 + k =
//     63 - k - 2 * clz(z + 2^k) bits: the prefix zeros are that integer's own leading zeros, so a
//     code is one (value, length) pair and its length one clz;
//   * a code is at most 33 bits, so at any bit offset s < 32 inside a 32-bit word it spans at
//     most two words: (uint64)code << (64 - s - len) is exact, its shift always in [0, 63].
//
// Passes as so_pack.hip: per-block byte counts (one wave per block), pack_scan_kernel (reused
// unchanged, so_pack.hip) for the offsets and per-frame totals, then the bytes.  Same capacity
// guard: a block whose end offset passes `cap` is not written.
#include "so_common.h"

namespace so {

// as so_pack.hip / so_capi.hip declare them
struct PackFrame {
    const uint8_t* split;
    const int16_t* mv;
    const int16_t* qtc;
    uint32_t* offs;
    uint8_t* out;
    int frame_type;
};
constexpr int kPackMax = 32;
struct PackArgs {
    PackFrame f[kPackMax];
};
struct UnpackFrame {
    const uint8_t* in;
    const uint32_t* offs;
    uint8_t* split;
    int16_t* mv;
    int16_t* qtc;
    int frame_type;
};
struct UnpackArgs {
    UnpackFrame f[kPackMax];
};
void pack_scan_launch(const PackArgs& a, int nframes, int nb, uint32_t* totals, hipStream_t st);   // so_pack.hip

// Worst case of one block: split + k, 12 mv values of 33 bits, nn coefficients of 33 bits, and
// nn / 2 + 4 tokens of 19 bits (|token| <= 256).  Loose on purpose, like pack_block_bound: no
// block has nn coefficients and that many tokens at once.
constexpr int pack_bits_block_bits(int bs) { return 3 + 12 * 33 + 33 * bs * bs + 19 * (bs * bs / 2 + 4); }
size_t pack_bits_block_bound(int bs) { return (size_t)(pack_bits_block_bits(bs) + 7) / 8; }
constexpr int kBitsStageWords = (pack_bits_block_bits(16) + 31) / 32;

// scan position -> row-major index in an n x n block (anti-diagonal order), as so_pack.hip's
__constant__ uint8_t c_bscan16[256];
__constant__ uint8_t c_bscan8[64];

static bool g_bscan_ready = false;

static int init_bits_scan_tables() {
    if (g_bscan_ready) return SO_OK;
    uint8_t t16[256], t8[64];
    for (int n : {16, 8}) {
        uint8_t* t = n == 16 ? t16 : t8;
        int p = 0;
        for (int k = 0; k < 2 * n - 1; ++k) {
            int i = k < n ? 0 : k - n + 1, j = k < n ? k : n - 1;
            while (i < n && j >= 0) t[p++] = (uint8_t)(i * n + j), ++i, --j;
        }
    }
    if (hipMemcpyToSymbol(HIP_SYMBOL(c_bscan16), t16, sizeof(t16)) != hipSuccess ||
        hipMemcpyToSymbol(HIP_SYMBOL(c_bscan8), t8, sizeof(t8)) != hipSuccess) {
        set_error("so_pack_frames_bits: scan tables: %s", hipGetErrorString(hipGetLastError()));
        return SO_E_INVALID;
    }
    g_bscan_ready = true;
    return SO_OK;
}

SO_DEV uint32_t bzz(int v) { return ((uint32_t)v << 1) ^ (uint32_t)(v >> 31); }
// bits of ue(z), z <= 65535: 2 * bit_length(z + 1) - 1
SO_DEV int ue_len(uint32_t z) { return 63 - 2 * __builtin_clz(z + 1u); }

// exclusive prefix sums over the wave; *total = the wave's sums (x: independent 16-bit fields
// whose wave sums stay below 2^16, so nothing carries from one into the next)
SO_DEV unsigned long long wave_excl_scan64(unsigned long long x, int lane, unsigned long long* total) {
    unsigned long long s = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long y = __shfl_up(s, d);
        if (lane >= d) s += y;
    }
    *total = __shfl(s, 63);
    return s - x;
}

SO_DEV int wave_excl_scan32(int x, int lane, int* total) {
    int s = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(s, d);
        if (lane >= d) s += y;
    }
    *total = __shfl(s, 63);
    return s - x;
}

// The wave's LDS stage: 32-bit words, the stream's first bit the top bit of word 0.  Touched
// only through aligned 32-bit accesses.  Lanes merge their bits with an atomic OR per touched
// word into the zeroed stage: OR commutes, so the bytes do not depend on lane timing.
SO_DEV void stage_or(uint32_t* stage, int w, uint32_t x) {
    if (x != 0 && w < kBitsStageWords)   // x != 0 only where the block has bits, i.e. inside its bound
        __hip_atomic_fetch_or(stage + w, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// One code of 1..33 bits at bit position pos.
SO_DEV void stage_put(uint32_t* stage, int pos, uint32_t code, int len) {
    const unsigned long long W = (unsigned long long)code << (64 - (pos & 31) - len);
    stage_or(stage, pos >> 5, (uint32_t)(W >> 32));
    stage_or(stage, (pos >> 5) + 1, (uint32_t)W);
}

// A lane's consecutive codes, assembled into words before they are merged: `cur` holds the
// `fill` (< 32) bits of word w written so far, at its top.  A lane can own ~300 bits.
struct BitAcc {
    uint32_t* stage;
    int w, fill;
    uint32_t cur;
    SO_DEV void put(uint32_t code, int len) {   // 1 <= len <= 33, code < 2^len
        const unsigned long long W = (unsigned long long)code << (64 - fill - len);   // shift in [0, 63]
        cur |= (uint32_t)(W >> 32);
        fill += len;                            // <= 64
        if (fill >= 32) {
            stage_or(stage, w++, cur);
            cur = (uint32_t)W;
            fill -= 32;
            if (fill == 32) {                   // 31 bits before a 33-bit code: two words complete
                stage_or(stage, w++, cur);
                cur = 0;
                fill = 0;
            }
        }
    }
    SO_DEV void finish() { stage_or(stage, w, cur); }
};

// A block's inputs, loaded one block ahead (as so_pack.hip's pack_load).
struct PackBitsIn {
    uint2 q;          // this lane's 4 coefficients (row-major)
    int sp;           // split flag
    int hv;           // mv value lane - 1 (lanes 1..nmv)
    uint32_t o0, o1;  // offs[b], offs[b + 1] (write pass)
};

template <bool WRITE, int bs>
SO_DEV PackBitsIn pack_bits_load(const PackFrame& f, int b, int nb, int lane) {
    b = b < nb ? b : nb - 1;   // branch-free: every lane loads, the index clamped
    constexpr int nn = bs * bs;
    const int nmv = f.frame_type == 1 ? 12 : 4;
    const int qi = lane * 4 < nn ? lane * 4 : 0;
    const int mi = lane >= 1 && lane <= nmv ? lane - 1 : 0;
    // the split byte through an opaque zero, so that its load stays a vector load
    int z;
    asm volatile("v_mov_b32 %0, 0" : "=v"(z));
    PackBitsIn in;
    in.q = *reinterpret_cast<const uint2*>(f.qtc + (size_t)b * nn + qi);
    in.sp = f.split[b + z];
    in.hv = f.mv[(size_t)b * nmv + mi];
    in.o0 = WRITE ? f.offs[b] : 0;
    in.o1 = WRITE ? f.offs[b + 1] : 0;
    return in;
}

// One block by one wave; lane l owns the R = nn / 64 consecutive scan positions R*l + j.  Runs
// and tokens as so_pack.hip's pack_one_block (run starts by XOR with the previous position,
// run lengths by ballot).  A position's bits are its run token (se) if it starts a run, then
// its value (se_k) if non-zero; two wave scans of the lanes' sums give the block's totals at
// the four orders -- which pick k -- and every lane's bit offset at the chosen order.  The
// header sits on lanes 0..H-1: split and k (3 bits) on lane 0, the mv values after it.
template <bool WRITE, int bs>
SO_DEV void pack_bits_one_block(const PackFrame& f, int b, unsigned long long cap, int lane, const PackBitsIn& in,
                                int16_t* __restrict__ sq, uint32_t* __restrict__ stage, const int* idx_whole,
                                const int* idx_split) {
    constexpr int nn = bs * bs, R = nn >> 6;
    if (lane * 4 < nn) *reinterpret_cast<uint2*>(&sq[lane * 4]) = in.q;
    const int sp = in.sp != 0;
    const int inter = f.frame_type == 1, H = 1 + (sp ? 4 : 1) * (inter ? 3 : 1);
    const int S = (sp && bs == 16) ? 64 : nn;   // segment length in scan positions
    __builtin_amdgcn_wave_barrier();            // LDS ops of one wave run in order

    int v[4];
    unsigned nzb = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        v[j] = 0;
        if (j < R) {
            v[j] = sq[S == 64 && bs == 16 ? idx_split[j] : idx_whole[j]];
            nzb |= (v[j] != 0) << j;
        }
    }
    const unsigned prev_last = __shfl_up((nzb >> (R - 1)) & 1, 1);
    const unsigned prevb = ((nzb << 1) | (lane > 0 ? prev_last : 0u)) & ((1u << R) - 1);
    unsigned stb = nzb ^ prevb;
    if ((R * lane) % S == 0) stb |= 1u;
    const unsigned long long lanes_with_start = __ballot(stb != 0);
    const unsigned long long above = lane == 63 ? 0ull : lanes_with_start & (~0ull << (lane + 1));
    const int nl = above ? __builtin_ctzll(above) : lane;
    const int nfs = __shfl((int)__builtin_ctz(stb | 0x10u), nl);
    const int next_lane_start = above ? R * nl + nfs : nn;

    // ue_k(z) is z + 2^k in 63 - k - 2 * clz(z + 2^k) bits, so a block's coefficient bits at order k
    // are CNT * (63 - k) - 2 * C_k with CNT its non-zero values and C_k the sum of their clz(z + 2^k):
    // a lane sums the four clz (16-bit fields of two words: <= 31 each, <= 7,936 per block), its
    // token bits tb (<= 3 per position) and its count, and the orders are compared on the sums
    uint32_t zt[4], zv[4];
    uint32_t c01 = 0, c23 = 0, tb = 0;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const unsigned later = stb & ~((2u << j) - 1);
        const int nxt = later ? R * lane + __builtin_ctz(later | 0x10u) : next_lane_start;
        const int run = nxt - (R * lane + j);
        const int nzj = (nzb >> j) & 1, stj = (stb >> j) & 1;
        const int tok = nzj ? -run : ((nxt & (S - 1)) == 0 ? 0 : run);   // a trailing zero run is one 0
        zt[j] = bzz(tok);
        zv[j] = bzz(v[j]);
        tb += (uint32_t)(ue_len(zt[j]) & -stj);
        const uint32_t m = (uint32_t)-nzj;
        c01 += (__builtin_clz(zv[j] + 1u) & m) + ((__builtin_clz(zv[j] + 2u) & m) << 16);
        c23 += (__builtin_clz(zv[j] + 4u) & m) + ((__builtin_clz(zv[j] + 8u) & m) << 16);
    }
    // one scan of the clz sums, one of header bits (10 bits: <= 399) | count (10: <= 256) | token bits
    // (12: <= 768); no field's wave sum reaches its width
    const int hb = lane == 0 ? 3 : (lane < H ? ue_len(bzz(in.hv)) : 0);
    unsigned long long ctot;
    const unsigned long long cex = wave_excl_scan64((unsigned long long)c23 << 32 | c01, lane, &ctot);
    int mtot;
    const int mex = wave_excl_scan32(hb | __builtin_popcount(nzb) << 10 | (int)(tb << 20), lane, &mtot);
    const int cnt = (mtot >> 10) & 0x3FF, hsum = mtot & 0x3FF;
    int k = 0, best = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {               // strictly smaller only: ties go to the smallest k
        const int t = cnt * (63 - c) - 2 * (int)((ctot >> (16 * c)) & 0xFFFF);
        if (c == 0 || t < best) best = t, k = c;
    }
    const int total_bits = hsum + (int)((unsigned)mtot >> 20) + best;
    const int nbytes = (total_bits + 7) >> 3;
    if (!WRITE) {
        if (lane == 0) f.offs[b] = (uint32_t)nbytes;
        return;
    }
    if (in.o1 > cap) return;
    for (int i = lane; i < (nbytes + 3) >> 2; i += 64) stage[i] = 0;
    __builtin_amdgcn_wave_barrier();
    if (lane < H) stage_put(stage, mex & 0x3FF, lane == 0 ? (uint32_t)(sp << 2 | k) : bzz(in.hv) + 1u, hb);
    const int pos = hsum + (int)((unsigned)mex >> 20) + ((mex >> 10) & 0x3FF) * (63 - k) -
                    2 * (int)((cex >> (16 * k)) & 0xFFFF);
    BitAcc acc{stage, pos >> 5, pos & 31, 0u};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j >= R) break;
        if ((stb >> j) & 1) acc.put(zt[j] + 1u, ue_len(zt[j]));
        const uint32_t code = zv[j] + (1u << k);
        if ((nzb >> j) & 1) acc.put(code, 63 - k - 2 * __builtin_clz(code));
    }
    acc.finish();
    __builtin_amdgcn_wave_barrier();
    // consecutive lanes store consecutive bytes
    uint8_t* out = f.out + in.o0;
    for (int i = lane; i < nbytes; i += 64) out[i] = (uint8_t)(stage[i >> 2] >> (24 - 8 * (i & 3)));
}

// Each wave packs blocks b = wave, wave + nwaves, ... of its frame (blockIdx.y), the next
// block's inputs loaded before the current one is packed (as pack_block_kernel).
template <bool WRITE, int bs>
__global__ void __launch_bounds__(256) pack_bits_block_kernel(const PackArgs a, int nb, unsigned long long cap) {
    __shared__ alignas(16) int16_t sq[4][256];
    __shared__ uint32_t stage[WRITE ? 4 : 1][WRITE ? kBitsStageWords : 1];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int w0 = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wv), nw = gridDim.x * 4;
    const PackFrame f = a.f[blockIdx.y];
    constexpr int R = (bs * bs) >> 6;
    int idx_whole[4], idx_split[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int P = R * lane + j;
        idx_whole[j] = j < R ? (bs == 16 ? c_bscan16[P] : c_bscan8[P]) : 0;
        idx_split[j] = j < R ? (P & ~63) + c_bscan8[P & 63] : 0;
    }
    PackBitsIn x = pack_bits_load<WRITE, bs>(f, w0, nb, lane);
    for (int b = w0; b < nb; b += 2 * nw) {
        const PackBitsIn y = pack_bits_load<WRITE, bs>(f, b + nw, nb, lane);
        pack_bits_one_block<WRITE, bs>(f, b, cap, lane, x, sq[wv], stage[WRITE ? wv : 0], idx_whole, idx_split);
        if (b + nw >= nb) break;
        x = pack_bits_load<WRITE, bs>(f, b + 2 * nw, nb, lane);
        pack_bits_one_block<WRITE, bs>(f, b + nw, cap, lane, y, sq[wv], stage[WRITE ? wv : 0], idx_whole, idx_split);
    }
}

// ---- unpack (so_unpack_frames_bits) ---------------------------------------------------------
// One thread per block parses its bytes [offs[b], offs[b+1]) sequentially into the zeroed
// block.  The bit reader never reads outside those bytes (past the end it sees zeros, and a
// code that needs them is malformed).  Malformed input (the rules in include/streamoptima.h)
// sets *err = 1 + that block's index.
template <int BS>
__global__ void __launch_bounds__(256) unpack_bits_block_kernel(const UnpackArgs a, int nb, int32_t* __restrict__ err) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    const UnpackFrame& f = a.f[blockIdx.y];
    const uint32_t o0 = f.offs[b], o1 = f.offs[b + 1];
    bool bad = o1 < o0;
    const uint8_t* const p = f.in + o0;
    const unsigned long long nbytes = bad ? 0ull : (unsigned long long)(o1 - o0), nbits = nbytes * 8;
    unsigned long long pos = 0;
    // the next 41+ bits at the top of a 64-bit word, zeros past the block's last byte
    auto peek = [&]() -> unsigned long long {
        const unsigned long long by = pos >> 3;
        unsigned long long w = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) w = (w << 8) | (by + i < nbytes ? p[by + i] : 0u);
        return w << (16 + (int)(pos & 7));
    };
    auto take = [&](int n) -> uint32_t {   // n plain bits, 1 <= n <= 8
        if (pos + n > nbits) {
            bad = true;
            return 0;
        }
        const uint32_t x = (uint32_t)(peek() >> (64 - n));
        pos += n;
        return x;
    };
    // se_k: at most 16 prefix zeros, then 17 + k bits at most -> 36 of the 41 peeked
    auto next = [&](int k) -> int {
        const unsigned long long W = peek();
        const int lz = __builtin_clzll(W | (1ull << 46));   // 17 when the first 17 bits are zero
        const int len = 2 * lz + 1 + k;
        if (lz > 16 || pos + len > nbits) {
            bad = true;
            return 0;
        }
        const uint32_t z = (uint32_t)(W >> (64 - len)) - (1u << k);
        if (z > 65535u) {
            bad = true;
            return 0;
        }
        pos += len;
        return (int)(z >> 1) ^ -(int)(z & 1u);
    };
    constexpr int NN = BS * BS;
    int16_t* q = f.qtc + (size_t)b * NN;
#pragma unroll
    for (int i = 0; i < NN / 8; ++i) reinterpret_cast<uint4*>(q)[i] = make_uint4(0, 0, 0, 0);
    const int sp = (int)take(1);
    const int kk = (int)take(2);
    if (sp == 1 && BS != 16) bad = true;
    f.split[b] = (uint8_t)(sp == 1 && !bad);
    const int inter = f.frame_type == 1, nmv = (sp == 1) ? 4 : 1;
    if (inter) {
        int16_t* m = f.mv + (size_t)b * 12;
        for (int j = 0; j < 12; ++j) m[j] = (int16_t)(j < 3 * nmv && !bad ? next(0) : 0);
    } else {
        int16_t* m = f.mv + (size_t)b * 4;
        for (int j = 0; j < 4; ++j) m[j] = (int16_t)(j < nmv && !bad ? next(0) : 0);
    }
    const int nsub = sp == 1 ? 4 : 1, n = sp == 1 ? 8 : BS, nn = n * n;
    const uint8_t* scan = n == 16 ? c_bscan16 : c_bscan8;
    for (int j = 0; j < nsub && !bad; ++j) {
        int16_t* qs = q + j * nn;
        int k = 0;
        while (k < nn && !bad) {
            const int t = next(0);
            if (bad) break;
            if (t < 0) {
                if (-t > nn - k) { bad = true; break; }
                for (int i = 0; i < -t && !bad; ++i) qs[scan[k + i]] = (int16_t)next(kk);
                k -= t;
            } else if (t == 0) {
                break;
            } else {
                if (t > nn - k) { bad = true; break; }
                k += t;
            }
        }
    }
    if (!bad) {   // fewer than 8 bits left, all of them zero
        const unsigned long long left = nbits - pos;
        if (left >= 8 || (left > 0 && (p[nbytes - 1] & ((1u << left) - 1u)) != 0)) bad = true;
    }
    if (bad) __hip_atomic_store(err, b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

int unpack_bits_frames_launch(const UnpackFrame* frames, int nframes, int nb, int bs, int32_t* err, hipStream_t st) {
    const int trc = init_bits_scan_tables();
    if (trc != SO_OK) return trc;
    for (int f0 = 0; f0 < nframes; f0 += kPackMax) {
        const int n = nframes - f0 < kPackMax ? nframes - f0 : kPackMax;
        UnpackArgs a{};
        for (int i = 0; i < n; ++i) a.f[i] = frames[f0 + i];
        const dim3 grid((nb + 255) / 256, n);
        if (bs == 16) hipLaunchKernelGGL(unpack_bits_block_kernel<16>, grid, dim3(256), 0, st, a, nb, err);
        else hipLaunchKernelGGL(unpack_bits_block_kernel<8>, grid, dim3(256), 0, st, a, nb, err);
        const int rc = check_launch("unpack_bits_block_kernel");
        if (rc != SO_OK) return rc;
    }
    return SO_OK;
}

int pack_bits_frames_launch(const PackFrame* frames, int nframes, int nb, int bs, unsigned long long cap,
                            uint32_t* totals, hipStream_t st) {
    const int trc = init_bits_scan_tables();
    if (trc != SO_OK) return trc;
    for (int f0 = 0; f0 < nframes; f0 += kPackMax) {
        const int n = nframes - f0 < kPackMax ? nframes - f0 : kPackMax;
        PackArgs a{};
        for (int i = 0; i < n; ++i) a.f[i] = frames[f0 + i];
        const int per_wave = 8;
        const dim3 grid((nb + 4 * per_wave - 1) / (4 * per_wave), n);
        if (bs == 16) hipLaunchKernelGGL((pack_bits_block_kernel<false, 16>), grid, dim3(256), 0, st, a, nb, cap);
        else hipLaunchKernelGGL((pack_bits_block_kernel<false, 8>), grid, dim3(256), 0, st, a, nb, cap);
        pack_scan_launch(a, n, nb, totals ? totals + f0 : nullptr, st);
        if (bs == 16) hipLaunchKernelGGL((pack_bits_block_kernel<true, 16>), grid, dim3(256), 0, st, a, nb, cap);
        else hipLaunchKernelGGL((pack_bits_block_kernel<true, 8>), grid, dim3(256), 0, st, a, nb, cap);
        const int rc = check_launch("pack bits kernels");
        if (rc != SO_OK) return rc;
    }
    return SO_OK;
}

}  // namespace so
