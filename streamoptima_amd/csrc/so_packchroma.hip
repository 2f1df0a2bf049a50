// so_packchroma.hip — the chroma coefficients of a frame (so_chroma_encode_frame's qtc_u / qtc_v,
// int16 [nb][64] each) as a packed stream, in both codings of the luma stream (so_pack.hip:
// varints; so_packbits.hip: Exp-Golomb bits).  The format is normative in include/streamoptima.h
// (so_pack_chroma_frames); in short, one record per luma block b in raster order:
//     varint:  U's token list | V's token list                       (every number a varint)
//     bits:    k (2 bits) | U's list | V's list | zero pad           (tokens se, values se_k)
// a list being exactly an 8x8 (sub-)block list of the luma format: scan_order(8), "-L" and L
// values, "Z" zeros, "0" the trailing zero run, the end also after 64 coefficients.  No split
// flag, no motion vectors: a record is two segments of 64 scan positions, which is the split
// luma block's run machinery (segment length 64) on 128 positions instead of 256.
//
// Passes as so_pack.hip: per-record byte counts (one wave per record), pack_scan_kernel (reused
// unchanged) for the offsets and the per-frame totals, then the bytes.  Same capacity guard: a
// record whose end offset passes `cap` is not written.
#include "so_common.h"

namespace so {

// as so_pack.hip declares them: the scan reads only `offs`
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
void pack_scan_launch(const PackArgs& a, int nframes, int nb, uint32_t* totals, hipStream_t st);   // so_pack.hip

struct ChromaPackFrame {
    const int16_t* qu;
    const int16_t* qv;
    uint32_t* offs;        // [nb + 1] exclusive offsets (pass 1 writes counts)
    uint8_t* out;
};
struct ChromaPackArgs {
    ChromaPackFrame f[kPackMax];
};
struct ChromaUnpackFrame {
    const uint8_t* in;
    const uint32_t* offs;
    int16_t* qu;
    int16_t* qv;
};
struct ChromaUnpackArgs {
    ChromaUnpackFrame f[kPackMax];
};

// Worst cases of one record, loose on purpose like pack_block_bound: two lists of 64 values,
// 32 run tokens and 4 more, 3 bytes each; 2 bits of k and two lists of 64 values of 33 bits and
// 36 tokens of 19 bits.
constexpr int kChromaBound = 2 * 3 * (64 + 32 + 4);                           // 600
constexpr int kChromaBitsBound = (2 + 2 * (33 * 64 + 19 * 36) + 7) / 8;       // 700
size_t pack_chroma_record_bound(bool bits) { return bits ? kChromaBitsBound : kChromaBound; }
constexpr int kChromaStageWords = (kChromaBitsBound + 3) / 4 + 1;

// scan position -> row-major index in an 8 x 8 block (anti-diagonal order, as so_pack.hip's)
struct Scan8 {
    uint8_t t[64];
};
constexpr Scan8 make_scan8() {
    Scan8 s{};
    int p = 0;
    for (int k = 0; k < 15; ++k) {
        int i = k < 8 ? 0 : k - 7, j = k < 8 ? k : 7;
        while (i < 8 && j >= 0) s.t[p++] = (uint8_t)(i * 8 + j), ++i, --j;
    }
    return s;
}
__constant__ Scan8 c_cscan8 = make_scan8();

// accesses that reinterpret int16 storage: may_alias, so that type-based alias analysis keeps them
// in order with the int16 accesses to the same bytes
typedef uint32_t __attribute__((may_alias)) u32_alias;
typedef uint4 __attribute__((may_alias)) uint4_alias;

SO_DEV uint32_t czz(int v) { return ((uint32_t)v << 1) ^ (uint32_t)(v >> 31); }
// LEB128 length of z (so_pack.hip vlen)
SO_DEV int cvlen(uint32_t z) { return (((31 - __builtin_clz(z | 1u)) * 37) >> 8) + 1; }
// bits of ue(z), z <= 65535 (so_packbits.hip ue_len)
SO_DEV int cue_len(uint32_t z) { return 63 - 2 * __builtin_clz(z + 1u); }

SO_DEV void cput_varint(uint8_t* p, int v) {
    uint32_t z = czz(v);
    do {
        *p++ = (uint8_t)(z & 0x7F) | (z > 0x7F ? 0x80 : 0);
        z >>= 7;
    } while (z);
}

// exclusive prefix sums over the wave; *total = the wave's sum
template <typename T>
SO_DEV T cwave_excl_scan(T x, int lane, T* total) {
    T s = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(s, d);
        if (lane >= d) s += y;
    }
    *total = __shfl(s, 63);
    return s - x;
}

// A record's inputs, loaded one record ahead (as so_pack.hip's pack_load): lanes 0..31 hold
// U's 64 coefficients (two each, row-major), lanes 32..63 V's.
struct ChromaIn {
    uint32_t q;
    uint32_t o0, o1;  // offs[b], offs[b + 1] (write pass)
};

template <bool WRITE>
SO_DEV ChromaIn chroma_load(const ChromaPackFrame& f, int b, int nb, int lane) {
    b = b < nb ? b : nb - 1;   // branch-free: every lane loads, the index clamped
    const int16_t* src = lane < 32 ? f.qu : f.qv;
    ChromaIn in;
    in.q = *reinterpret_cast<const u32_alias*>(src + (size_t)b * 64 + (lane & 31) * 2);
    in.o0 = WRITE ? f.offs[b] : 0;
    in.o1 = WRITE ? f.offs[b + 1] : 0;
    return in;
}

// What both codings share: the record through LDS into scan order, lane l owning positions 2l
// and 2l + 1 of the U|V sequence, and the runs (so_pack.hip pack_one_block at R = 2, S = 64:
// a position starts a run when it opens a list -- positions 0 and 64 -- or its non-zero flag
// differs from the previous position's; a run's length is the distance to the next start).
struct ChromaRuns {
    int v[2], tok[2];
    unsigned nzb, stb;
};

SO_DEV ChromaRuns chroma_runs(const ChromaIn& in, int lane, int16_t* __restrict__ sq, const int* idx) {
    reinterpret_cast<u32_alias*>(sq)[lane] = in.q;
    __builtin_amdgcn_wave_barrier();   // LDS ops of one wave run in order
    ChromaRuns r;
    r.v[0] = sq[idx[0]];
    r.v[1] = sq[idx[1]];
    r.nzb = (unsigned)(r.v[0] != 0) | ((unsigned)(r.v[1] != 0) << 1);
    const unsigned prev_last = __shfl_up((r.nzb >> 1) & 1, 1);
    const unsigned prevb = ((r.nzb << 1) | (lane > 0 ? prev_last : 0u)) & 3u;
    r.stb = r.nzb ^ prevb;
    if ((lane & 31) == 0) r.stb |= 1u;            // a list opens at this lane's first position
    const unsigned long long lanes_with_start = __ballot(r.stb != 0);
    const unsigned long long above = lane == 63 ? 0ull : lanes_with_start & (~0ull << (lane + 1));
    const int nl = above ? __builtin_ctzll(above) : lane;
    const int nfs = __shfl((int)__builtin_ctz(r.stb | 4u), nl);
    const int next_lane_start = above ? 2 * nl + nfs : 128;
#pragma unroll
    for (int j = 0; j < 2; ++j) {   // branch-free: every position computes its would-be token
        const unsigned later = r.stb & ~((2u << j) - 1);
        const int nxt = later ? 2 * lane + 1 : next_lane_start;   // later: only bit 1 after j = 0
        const int run = nxt - (2 * lane + j);
        r.tok[j] = (r.nzb >> j) & 1 ? -run : ((nxt & 63) == 0 ? 0 : run);   // a trailing zero run is one 0
    }
    return r;
}

// ---- varint coding -------------------------------------------------------------------------------
template <bool WRITE>
SO_DEV void pack_chroma_one(const ChromaPackFrame& f, int b, unsigned long long cap, int lane, const ChromaIn& in,
                            int16_t* __restrict__ sq, uint8_t* __restrict__ stage, const int* idx) {
    const ChromaRuns r = chroma_runs(in, lane, sq, idx);
    int nbytes = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int nzj = (r.nzb >> j) & 1, stj = (r.stb >> j) & 1;
        nbytes += (cvlen(czz(r.tok[j])) & -stj) + (cvlen(czz(r.v[j])) & -nzj);
    }
    int total;
    const int ex = cwave_excl_scan(nbytes, lane, &total);
    if (!WRITE) {
        if (lane == 0) f.offs[b] = (uint32_t)total;
        return;
    }
    if (in.o1 > cap) return;
    // bytes into the wave's LDS stage, then out with consecutive lanes on consecutive bytes
    uint8_t* p = stage + ex;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if ((r.stb >> j) & 1) {
            cput_varint(p, r.tok[j]);
            p += cvlen(czz(r.tok[j]));
        }
        if (r.v[j] != 0) {
            cput_varint(p, r.v[j]);
            p += cvlen(czz(r.v[j]));
        }
    }
    __builtin_amdgcn_wave_barrier();
    uint8_t* out = f.out + in.o0;
    for (int i = lane; i < total; i += 64) out[i] = stage[i];
}

// ---- bits coding ---------------------------------------------------------------------------------
// The wave's LDS stage as so_packbits.hip's: 32-bit words, the stream's first bit the top bit of
// word 0, lanes merging their bits with an atomic OR per touched word into the zeroed stage.
SO_DEV void cstage_or(uint32_t* stage, int w, uint32_t x) {
    if (x != 0 && w < kChromaStageWords)   // x != 0 only where the record has bits, i.e. inside its bound
        __hip_atomic_fetch_or(stage + w, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// A lane's consecutive codes (so_packbits.hip BitAcc): `cur` holds the `fill` (< 32) bits of word
// w written so far, at its top.
struct ChromaBitAcc {
    uint32_t* stage;
    int w, fill;
    uint32_t cur;
    SO_DEV void put(uint32_t code, int len) {   // 1 <= len <= 33, code < 2^len
        const unsigned long long W = (unsigned long long)code << (64 - fill - len);   // shift in [0, 63]
        cur |= (uint32_t)(W >> 32);
        fill += len;                            // <= 64
        if (fill >= 32) {
            cstage_or(stage, w++, cur);
            cur = (uint32_t)W;
            fill -= 32;
            if (fill == 32) {                   // 31 bits before a 33-bit code: two words complete
                cstage_or(stage, w++, cur);
                cur = 0;
                fill = 0;
            }
        }
    }
    SO_DEV void finish() { cstage_or(stage, w, cur); }
};

// The order k as so_packbits.hip's pack_bits_one_block picks it, over both lists: ue_k(z) is
// z + 2^k in 63 - k - 2 * clz(z + 2^k) bits, so the record's coefficient bits at order k are
// CNT * (63 - k) - 2 * C_k with CNT its non-zero values and C_k the sum of their clz(z + 2^k).
template <bool WRITE>
SO_DEV void pack_chroma_bits_one(const ChromaPackFrame& f, int b, unsigned long long cap, int lane,
                                 const ChromaIn& in, int16_t* __restrict__ sq, uint32_t* __restrict__ stage,
                                 const int* idx) {
    const ChromaRuns r = chroma_runs(in, lane, sq, idx);
    uint32_t zt[2], zv[2];
    uint32_t c01 = 0, c23 = 0, tb = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int nzj = (r.nzb >> j) & 1, stj = (r.stb >> j) & 1;
        zt[j] = czz(r.tok[j]);
        zv[j] = czz(r.v[j]);
        tb += (uint32_t)(cue_len(zt[j]) & -stj);
        const uint32_t m = (uint32_t)-nzj;
        c01 += (__builtin_clz(zv[j] + 1u) & m) + ((__builtin_clz(zv[j] + 2u) & m) << 16);
        c23 += (__builtin_clz(zv[j] + 4u) & m) + ((__builtin_clz(zv[j] + 8u) & m) << 16);
    }
    // one scan of the clz sums (16-bit fields: <= 31 * 128), one of count (10 bits: <= 128) | token bits
    // (a token is at most 15 bits, |token| <= 64; their sum stays below 3 * 128 + 4 < 2^12)
    unsigned long long ctot;
    const unsigned long long cex = cwave_excl_scan((unsigned long long)c23 << 32 | c01, lane, &ctot);
    int mtot;
    const int mex = cwave_excl_scan(__builtin_popcount(r.nzb) | (int)(tb << 10), lane, &mtot);
    const int cnt = mtot & 0x3FF;
    int k = 0, best = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {               // strictly smaller only: ties go to the smallest k
        const int t = cnt * (63 - c) - 2 * (int)((ctot >> (16 * c)) & 0xFFFF);
        if (c == 0 || t < best) best = t, k = c;
    }
    const int total_bits = 2 + (mtot >> 10) + best;
    const int nbytes = (total_bits + 7) >> 3;
    if (!WRITE) {
        if (lane == 0) f.offs[b] = (uint32_t)nbytes;
        return;
    }
    if (in.o1 > cap) return;
    for (int i = lane; i < (nbytes + 3) >> 2; i += 64) stage[i] = 0;
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) cstage_or(stage, 0, (uint32_t)k << 30);
    const int pos = 2 + (mex >> 10) + (mex & 0x3FF) * (63 - k) - 2 * (int)((cex >> (16 * k)) & 0xFFFF);
    ChromaBitAcc acc{stage, pos >> 5, pos & 31, 0u};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        if ((r.stb >> j) & 1) acc.put(zt[j] + 1u, cue_len(zt[j]));
        const uint32_t code = zv[j] + (1u << k);
        if ((r.nzb >> j) & 1) acc.put(code, 63 - k - 2 * __builtin_clz(code));
    }
    acc.finish();
    __builtin_amdgcn_wave_barrier();
    // consecutive lanes store consecutive bytes
    uint8_t* out = f.out + in.o0;
    for (int i = lane; i < nbytes; i += 64) out[i] = (uint8_t)(stage[i >> 2] >> (24 - 8 * (i & 3)));
}

// Each wave packs records b = wave, wave + nwaves, ... of its frame (blockIdx.y), the next
// record's inputs loaded before the current one is packed, in two register sets (as
// pack_block_kernel).
template <bool WRITE, bool BITS>
__global__ void __launch_bounds__(256) pack_chroma_kernel(const ChromaPackArgs a, int nb, unsigned long long cap) {
    __shared__ alignas(4) int16_t sq[4][128];
    __shared__ uint32_t stage[WRITE ? 4 : 1][WRITE ? (BITS ? kChromaStageWords : kChromaBound / 4 + 2) : 1];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int w0 = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wv), nw = gridDim.x * 4;
    const ChromaPackFrame f = a.f[blockIdx.y];   // a copy: its pointers stay in SGPRs
    // this lane's two scan positions as int16 indices into the staged record (U at 0, V at 64)
    int idx[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int P = 2 * lane + j;
        idx[j] = (P & 64) + c_cscan8.t[P & 63];
    }
    auto one = [&](int b, const ChromaIn& in) {
        if constexpr (BITS)
            pack_chroma_bits_one<WRITE>(f, b, cap, lane, in, sq[wv], stage[WRITE ? wv : 0], idx);
        else   // the varint stage is bytes: character accesses alias anything
            pack_chroma_one<WRITE>(f, b, cap, lane, in, sq[wv], reinterpret_cast<uint8_t*>(stage[WRITE ? wv : 0]), idx);
    };
    ChromaIn x = chroma_load<WRITE>(f, w0, nb, lane);
    for (int b = w0; b < nb; b += 2 * nw) {
        const ChromaIn y = chroma_load<WRITE>(f, b + nw, nb, lane);
        one(b, x);
        if (b + nw >= nb) break;
        x = chroma_load<WRITE>(f, b + 2 * nw, nb, lane);
        one(b + nw, y);
    }
}

// ---- unpack: one thread per record ---------------------------------------------------------------
// Each thread zeroes both 8x8 blocks and parses U's list then V's from its bytes
// [offs[b], offs[b+1]).  Malformed input (the rules in include/streamoptima.h; also
// offs[b + 1] < offs[b]) sets *err = 1 + the record's index.
SO_DEV void chroma_zero(int16_t* q) {
#pragma unroll
    for (int i = 0; i < 8; ++i) reinterpret_cast<uint4_alias*>(q)[i] = make_uint4(0, 0, 0, 0);
}

// the two token lists, `next(is_coef)` the next number of the record
template <typename Next>
SO_DEV void chroma_lists(int16_t* qu, int16_t* qv, bool& bad, Next next) {
    for (int j = 0; j < 2 && !bad; ++j) {
        int16_t* qs = j ? qv : qu;
        int k = 0;
        while (k < 64 && !bad) {
            const int t = next(false);
            if (bad) break;
            if (t < 0) {
                if (-t > 64 - k) { bad = true; break; }
                for (int i = 0; i < -t && !bad; ++i) qs[c_cscan8.t[k + i]] = (int16_t)next(true);
                k -= t;
            } else if (t == 0) {
                break;
            } else {
                if (t > 64 - k) { bad = true; break; }
                k += t;
            }
        }
    }
}

__global__ void __launch_bounds__(256) unpack_chroma_kernel(const ChromaUnpackArgs a, int nb, int32_t* __restrict__ err) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    const ChromaUnpackFrame& f = a.f[blockIdx.y];
    const uint32_t o0 = f.offs[b], o1 = f.offs[b + 1];
    bool bad = o1 < o0;
    const uint8_t* p = f.in + o0;
    const uint8_t* const end = bad ? p : f.in + o1;
    // a varint of 1-5 bytes whose zigzag value stays below 2^16 (so_pack.hip unpack_block_kernel)
    auto next = [&](bool) -> int {
        uint32_t z = 0, hi = 0;
        for (int sh = 0; sh < 35; sh += 7) {
            if (p >= end) break;
            const uint32_t c = *p++;
            if (sh < 21) z |= (c & 0x7Fu) << sh;
            else hi |= c & 0x7Fu;
            if (!(c & 0x80u)) {
                if (hi | (z >> 16)) break;
                return (int)(z >> 1) ^ -(int)(z & 1u);
            }
        }
        bad = true;
        return 0;
    };
    int16_t* qu = f.qu + (size_t)b * 64;
    int16_t* qv = f.qv + (size_t)b * 64;
    chroma_zero(qu);
    chroma_zero(qv);
    chroma_lists(qu, qv, bad, next);
    if (p != end) bad = true;
    if (bad) __hip_atomic_store(err, b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The bit reader never reads outside the record's bytes (past the end it sees zeros, and a code
// that needs them is malformed), as so_packbits.hip's unpack_bits_block_kernel.
__global__ void __launch_bounds__(256) unpack_chroma_bits_kernel(const ChromaUnpackArgs a, int nb,
                                                                 int32_t* __restrict__ err) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    const ChromaUnpackFrame& f = a.f[blockIdx.y];
    const uint32_t o0 = f.offs[b], o1 = f.offs[b + 1];
    bool bad = o1 < o0;
    const uint8_t* const p = f.in + o0;
    const unsigned long long nbytes = bad ? 0ull : (unsigned long long)(o1 - o0), nbits = nbytes * 8;
    unsigned long long pos = 0;
    // the next 41+ bits at the top of a 64-bit word, zeros past the record's last byte
    auto peek = [&]() -> unsigned long long {
        const unsigned long long by = pos >> 3;
        unsigned long long w = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) w = (w << 8) | (by + i < nbytes ? p[by + i] : 0u);
        return w << (16 + (int)(pos & 7));
    };
    int kk = 0;
    if (nbits < 2) bad = true;
    else kk = (int)(peek() >> 62), pos = 2;
    // se / se_k: at most 16 prefix zeros, then 17 + k bits at most -> 36 of the 41 peeked
    auto next = [&](bool coef) -> int {
        const int k = coef ? kk : 0;
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
    int16_t* qu = f.qu + (size_t)b * 64;
    int16_t* qv = f.qv + (size_t)b * 64;
    chroma_zero(qu);
    chroma_zero(qv);
    chroma_lists(qu, qv, bad, next);
    if (!bad) {   // fewer than 8 bits left, all of them zero
        const unsigned long long left = nbits - pos;
        if (left >= 8 || (left > 0 && (p[nbytes - 1] & ((1u << left) - 1u)) != 0)) bad = true;
    }
    if (bad) __hip_atomic_store(err, b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

int pack_chroma_frames_launch(const ChromaPackFrame* frames, int nframes, int nb, bool bits, unsigned long long cap,
                              uint32_t* totals, hipStream_t st) {
    for (int f0 = 0; f0 < nframes; f0 += kPackMax) {
        const int n = nframes - f0 < kPackMax ? nframes - f0 : kPackMax;
        ChromaPackArgs a{};
        PackArgs sa{};
        for (int i = 0; i < n; ++i) {
            a.f[i] = frames[f0 + i];
            sa.f[i].offs = frames[f0 + i].offs;
        }
        const int per_wave = 8;
        const dim3 grid((nb + 4 * per_wave - 1) / (4 * per_wave), n);
        if (bits) hipLaunchKernelGGL((pack_chroma_kernel<false, true>), grid, dim3(256), 0, st, a, nb, cap);
        else hipLaunchKernelGGL((pack_chroma_kernel<false, false>), grid, dim3(256), 0, st, a, nb, cap);
        pack_scan_launch(sa, n, nb, totals ? totals + f0 : nullptr, st);
        if (bits) hipLaunchKernelGGL((pack_chroma_kernel<true, true>), grid, dim3(256), 0, st, a, nb, cap);
        else hipLaunchKernelGGL((pack_chroma_kernel<true, false>), grid, dim3(256), 0, st, a, nb, cap);
        const int rc = check_launch("pack chroma kernels");
        if (rc != SO_OK) return rc;
    }
    return SO_OK;
}

int unpack_chroma_frames_launch(const ChromaUnpackFrame* frames, int nframes, int nb, bool bits, int32_t* err,
                                hipStream_t st) {
    for (int f0 = 0; f0 < nframes; f0 += kPackMax) {
        const int n = nframes - f0 < kPackMax ? nframes - f0 : kPackMax;
        ChromaUnpackArgs a{};
        for (int i = 0; i < n; ++i) a.f[i] = frames[f0 + i];
        const dim3 grid((nb + 255) / 256, n);
        if (bits) hipLaunchKernelGGL(unpack_chroma_bits_kernel, grid, dim3(256), 0, st, a, nb, err);
        else hipLaunchKernelGGL(unpack_chroma_kernel, grid, dim3(256), 0, st, a, nb, err);
        const int rc = check_launch("unpack chroma kernels");
        if (rc != SO_OK) return rc;
    }
    return SO_OK;
}

}  // namespace so
