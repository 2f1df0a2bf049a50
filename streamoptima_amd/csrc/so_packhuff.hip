// so_packhuff.hip — the packed symbol stream in the "huff" coding: the symbols of so_packbits.hip
// (split, mv values, the RLE token list of every (sub-)block, per block in raster order; chroma:
// U's list then V's) as canonical Huffman codes from tables built per frame.  The format is
// normative in include/streamoptima.h (so_pack_frames_huff); in short, MSB-first within each byte:
//     luma block:     split (1 raw bit) | mv values | tokens and coefficient values | zero pad
//     chroma record:  U's tokens and values | V's tokens and values | zero pad
//     a value v:      z = zz(v); z < 32: symbol z; else n = bit_length(z) in 6..16: symbol 26 + n,
//                     then the low n - 1 bits of z raw.  43 symbols, code lengths 1..15.
//     its table:      mv values: table 0; a token before which p coefficients of its (sub-)block are
//                     covered: tok[cls(p)]; a coefficient at scan position p: coef[cls(p)], with
//                     cls(p) = min(bit_length(p), 6).  Luma: mv, tok0..6, coef0..6; chroma: tok0..6,
//                     coef0..6.
//     the tables:     43 four-bit code lengths each, in that order, at the head of record 0.
// A code and its raw bits are at most 30 bits, so so_packfmt.h's two-word writer carries over, and
// code lengths add like Exp-Golomb lengths do: one wave per record, a wave scan of the lanes' bits,
// byte-aligned records, pack_scan_kernel for the offsets, the same capacity guard.
//
// Passes, all stream-ordered: the histogram (one wave per record, counts in LDS per workgroup, then
// vector atomics on the frame's counters), the table build (one workgroup per frame, one lane per
// table), per-record byte counts, pack_scan_kernel, the bytes.  The frame's counters, code entries
// and table bytes live in scratch taken from and returned to the device's stream-ordered pool, so
// the host never waits.
#include "so_packfmt.h"

namespace so {

// ---- the value mapping (the contexts: so_packfmt.h huff_cls) -----------------------------------
// symbol of z <= 65535; *nx = the raw bits that follow its code
SO_DEV int huff_sym(uint32_t z, int* nx) {
    if (z < 32u) {
        *nx = 0;
        return (int)z;
    }
    const int n = 32 - __builtin_clz(z);
    *nx = n - 1;
    return 26 + n;
}

// One value through table t of the frame's entries (length << 16 | code): code and raw bits as one
// number of *len <= 30 bits.
SO_DEV uint32_t huff_code(const uint32_t* entries, int t, uint32_t z, int* len) {
    int nx;
    const uint32_t e = entries[t * kHuffSyms + huff_sym(z, &nx)];
    *len = (int)(e >> 16) + nx;
    return ((e & 0xFFFFu) << nx) | (z & ((1u << nx) - 1u));
}

// ---- histogram -----------------------------------------------------------------------------------
// a lane's tokens and values into the workgroup's counts; TOK0: the first token table
template <int TOK0, int R>
SO_DEV void huff_count(uint32_t* hist, const PackRuns<R>& r, int S, int lane) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int c = huff_cls((R * lane + j) & (S - 1));
        int nx;
        if ((r.stb >> j) & 1)
            __hip_atomic_fetch_add(hist + (TOK0 + c) * kHuffSyms + huff_sym(zz(r.tok[j]), &nx), 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);
        if ((r.nzb >> j) & 1)
            __hip_atomic_fetch_add(hist + (TOK0 + kHuffCtx + c) * kHuffSyms + huff_sym(zz(r.v[j]), &nx), 1u,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}

// the workgroup's counts to the frame's counters (zeroed before the launch)
SO_DEV void huff_hist_flush(const uint32_t* hist, uint32_t* counts, int n) {
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256)
        if (hist[i]) __hip_atomic_fetch_add(counts + i, hist[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int bs>
__global__ void __launch_bounds__(256) huff_hist_kernel(const PackArgs a, int nb, uint32_t* __restrict__ scr) {
    __shared__ alignas(16) int16_t sq[4][256];
    __shared__ uint32_t hist[kHuffTableWords];
    for (int i = threadIdx.x; i < kHuffTableWords; i += 256) hist[i] = 0;
    __syncthreads();
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int w0 = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wv), nw = gridDim.x * 4;
    const PackFrame f = a.f[blockIdx.y];
    const LumaIdx<bs> idx(lane);
    pack_loop(
        w0, nw, nb, [&](int b) { return pack_load<false, bs>(f, b, nb, lane); },
        [&](int, const PackIn& in) {
            const int sp = in.sp != 0;
            const int H = 1 + (sp ? 4 : 1) * (f.frame_type == 1 ? 3 : 1);
            const auto r = luma_runs<bs>(in, sp, lane, sq[wv], idx);
            int nx;
            if (lane >= 1 && lane < H)
                __hip_atomic_fetch_add(hist + huff_sym(zz(in.hv), &nx), 1u, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
            huff_count<1>(hist, r, (sp && bs == 16) ? 64 : bs * bs, lane);
        });
    huff_hist_flush(hist, scr + (size_t)blockIdx.y * kHuffScratchWords, kHuffTableWords);
}

__global__ void __launch_bounds__(256) huff_chroma_hist_kernel(const ChromaPackArgs a, int nb, uint32_t* __restrict__ scr) {
    __shared__ alignas(4) int16_t sq[4][128];
    __shared__ uint32_t hist[kHuffTableWords];
    for (int i = threadIdx.x; i < kHuffTableWords; i += 256) hist[i] = 0;
    __syncthreads();
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int w0 = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wv), nw = gridDim.x * 4;
    const ChromaPackFrame f = a.f[blockIdx.y];
    const int idx[2] = {((2 * lane) & 64) + c_scan8.t[(2 * lane) & 63], ((2 * lane + 1) & 64) + c_scan8.t[(2 * lane + 1) & 63]};
    pack_loop(
        w0, nw, nb, [&](int b) { return chroma_load<false>(f, b, nb, lane); },
        [&](int, const ChromaIn& in) { huff_count<0>(hist, chroma_runs(in, lane, sq[wv], idx), 64, lane); });
    huff_hist_flush(hist, scr + (size_t)blockIdx.y * kHuffScratchWords, kHuffChromaTables * kHuffSyms);
}

// ---- table build ---------------------------------------------------------------------------------
// One workgroup per frame, lane t builds table t from the frame's counts -- the canonical-length
// rule of include/streamoptima.h, exactly:
//   * nodes 0..42 are the symbols' leaves (those with a non-zero count), merged nodes are numbered
//     43, 44, ... as they are made; each step merges the two live nodes smallest by (weight, index),
//     the new weight their sum; a symbol's length is its leaf's depth;
//   * one used symbol: length 1; none: all lengths 0;
//   * a length above 15: every non-zero count c becomes (c + 1) >> 1, and the build is repeated.
// Codes are canonical: by (length, symbol), the first code of a length the previous length's next
// code shifted left.  Output: the frame's entries (length << 16 | code) and its table bytes (the
// lengths as nibbles, high nibble first, all tables back to back, the last nibble 0).
constexpr int kHuffNodes = 2 * kHuffSyms;
__global__ void __launch_bounds__(64) huff_tables_kernel(uint32_t* __restrict__ scr, int ntab) {
    __shared__ uint32_t cw[kHuffLumaTables][kHuffSyms];
    __shared__ uint32_t w[kHuffLumaTables][kHuffNodes];
    __shared__ uint8_t par[kHuffLumaTables][kHuffNodes];   // 255: live, 254: not a node, else the parent
    __shared__ uint8_t dep[kHuffLumaTables][kHuffNodes];
    __shared__ uint8_t lens[kHuffTableWords + 1];
    uint32_t* const counts = scr + (size_t)blockIdx.x * kHuffScratchWords;
    uint32_t* const entries = counts + kHuffTableWords;
    uint8_t* const bytes = reinterpret_cast<uint8_t*>(entries + kHuffTableWords);
    const int t = threadIdx.x;
    if (t == 0) lens[ntab * kHuffSyms] = 0;
    if (t < ntab) {
        int used = 0, only = 0;
        for (int s = 0; s < kHuffSyms; ++s) {
            cw[t][s] = counts[t * kHuffSyms + s];
            if (cw[t][s]) ++used, only = s;
            dep[t][s] = 0;
        }
        if (used == 1) dep[t][only] = 1;
        while (used > 1) {
            for (int s = 0; s < kHuffSyms; ++s) w[t][s] = cw[t][s], par[t][s] = cw[t][s] ? 255 : 254;
            int next = kHuffSyms;
            for (int m = 0; m + 1 < used; ++m) {
                unsigned long long k1 = ~0ull, k2 = ~0ull;
                for (int i = 0; i < next; ++i) {
                    if (par[t][i] != 255) continue;
                    const unsigned long long k = (unsigned long long)w[t][i] << 8 | (unsigned)i;
                    if (k < k1) k2 = k1, k1 = k;
                    else if (k < k2) k2 = k;
                }
                const int i1 = (int)(k1 & 0xFF), i2 = (int)(k2 & 0xFF);
                w[t][next] = w[t][i1] + w[t][i2];
                par[t][i1] = par[t][i2] = (uint8_t)next;
                par[t][next] = 255;
                ++next;
            }
            int longest = 0;
            dep[t][next - 1] = 0;
            for (int i = next - 2; i >= 0; --i) {
                if (par[t][i] == 254) {
                    dep[t][i] = 0;
                    continue;
                }
                dep[t][i] = (uint8_t)(dep[t][par[t][i]] + 1);
                if (i < kHuffSyms && dep[t][i] > longest) longest = dep[t][i];
            }
            if (longest <= kHuffMaxLen) break;
            for (int s = 0; s < kHuffSyms; ++s)
                if (cw[t][s]) cw[t][s] = (cw[t][s] + 1) >> 1;
        }
        // canonical codes; w[t][1..15] serves as the next code of each length
        for (int l = 0; l <= kHuffMaxLen + 1; ++l) w[t][l] = 0;
        for (int s = 0; s < kHuffSyms; ++s) w[t][dep[t][s] + 1] += dep[t][s] ? 1u : 0u;   // counts, one up
        uint32_t code = 0, cnt_prev = 0;
        for (int l = 1; l <= kHuffMaxLen; ++l) {
            const uint32_t cnt = w[t][l + 1];
            code = (code + cnt_prev) << 1;
            w[t][l] = code;
            cnt_prev = cnt;
        }
        for (int s = 0; s < kHuffSyms; ++s) {
            const int l = dep[t][s];
            lens[t * kHuffSyms + s] = (uint8_t)l;
            entries[t * kHuffSyms + s] = l ? (uint32_t)l << 16 | w[t][l]++ : 0u;
        }
    }
    __syncthreads();
    const int nbytes = huff_table_bytes(ntab);
    for (int i = t; i < nbytes; i += 64) bytes[i] = (uint8_t)(lens[2 * i] << 4 | lens[2 * i + 1]);
}

// ---- pack ----------------------------------------------------------------------------------------
// a lane's codes: its run tokens where it starts runs, its non-zero values; `bits` their sum
template <int R>
struct HuffLane {
    uint32_t tc[R], vc[R];
    int tl[R], vl[R], bits;
};

template <int TOK0, int R>
SO_DEV HuffLane<R> huff_lane(const uint32_t* entries, const PackRuns<R>& r, int S, int lane) {
    HuffLane<R> l;
    l.bits = 0;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int c = huff_cls((R * lane + j) & (S - 1));
        l.tc[j] = huff_code(entries, TOK0 + c, zz(r.tok[j]), &l.tl[j]);
        l.vc[j] = huff_code(entries, TOK0 + kHuffCtx + c, zz(r.v[j]), &l.vl[j]);
        l.bits += (l.tl[j] & -(int)((r.stb >> j) & 1)) + (l.vl[j] & -(int)((r.nzb >> j) & 1));
    }
    return l;
}

template <int WORDS, int R>
SO_DEV void huff_put(uint32_t* stage, int pos, const PackRuns<R>& r, const HuffLane<R>& l) {
    BitAcc<WORDS> acc{stage, pos >> 5, pos & 31, 0u};
#pragma unroll
    for (int j = 0; j < R; ++j) {
        if ((r.stb >> j) & 1) acc.put(l.tc[j], l.tl[j]);
        if ((r.nzb >> j) & 1) acc.put(l.vc[j], l.vl[j]);
    }
    acc.finish();
}

// the frame's entries into the workgroup's LDS
SO_DEV void huff_load_entries(uint32_t* entries, const uint32_t* __restrict__ fscr, int n) {
    for (int i = threadIdx.x; i < n; i += 256) entries[i] = fscr[kHuffTableWords + i];
    __syncthreads();
}

// the table bytes in front of record 0, by its wave
SO_DEV void huff_store_tables(uint8_t* out, const uint32_t* __restrict__ fscr, int nbytes, int lane) {
    const uint8_t* src = reinterpret_cast<const uint8_t*>(fscr + 2 * kHuffTableWords);
    for (int i = lane; i < nbytes; i += 64) out[i] = src[i];
}

// One luma block by one wave, as so_packbits.hip pack_bits_one_block: the header on lanes 0..H-1
// (the split bit on lane 0, the mv values after it), one wave scan of header bits (10 bits: <= 361)
// | body bits (<= 10,848).  Block 0 carries the frame's table bytes in front of its codes.
template <bool WRITE, int bs>
SO_DEV void pack_huff_one_block(const PackFrame& f, int b, unsigned long long cap, int lane, const PackIn& in,
                                int16_t* __restrict__ sq, uint32_t* __restrict__ stage, const LumaIdx<bs>& idx,
                                const uint32_t* entries, const uint32_t* __restrict__ fscr) {
    const int sp = in.sp != 0;
    const int inter = f.frame_type == 1, H = 1 + (sp ? 4 : 1) * (inter ? 3 : 1);
    const auto r = luma_runs<bs>(in, sp, lane, sq, idx);
    const auto l = huff_lane<1>(entries, r, (sp && bs == 16) ? 64 : bs * bs, lane);
    int hl;
    uint32_t hc = huff_code(entries, 0, zz(in.hv), &hl);
    if (lane == 0) hc = (uint32_t)sp, hl = 1;
    const int hb = lane < H ? hl : 0;
    int mtot;
    const int mex = wave_excl_scan(hb | l.bits << 10, lane, &mtot);
    const int hsum = mtot & 0x3FF;
    const int nbytes = (hsum + (mtot >> 10) + 7) >> 3;
    const int head = b == 0 ? kHuffLumaTableBytes : 0;
    if (!WRITE) {
        if (lane == 0) f.offs[b] = (uint32_t)(head + nbytes);
        return;
    }
    if (in.o1 > cap) return;
    stage_zero(stage, nbytes, lane);
    __builtin_amdgcn_wave_barrier();
    if (lane < H) {
        const int pos = mex & 0x3FF;
        const unsigned long long W = (unsigned long long)hc << (64 - (pos & 31) - hb);
        stage_or<kHuffStageWords>(stage, pos >> 5, (uint32_t)(W >> 32));
        stage_or<kHuffStageWords>(stage, (pos >> 5) + 1, (uint32_t)W);
    }
    huff_put<kHuffStageWords>(stage, hsum + (mex >> 10), r, l);
    __builtin_amdgcn_wave_barrier();
    if (head) huff_store_tables(f.out + in.o0, fscr, head, lane);
    stage_store(f.out + in.o0 + head, stage, nbytes, lane);
}

template <bool WRITE, int bs>
__global__ void __launch_bounds__(256) pack_huff_block_kernel(const PackArgs a, int nb, unsigned long long cap,
                                                              const uint32_t* __restrict__ scr) {
    __shared__ alignas(16) int16_t sq[4][256];
    __shared__ uint32_t stage[WRITE ? 4 : 1][WRITE ? kHuffStageWords : 1];
    __shared__ uint32_t entries[kHuffTableWords];
    const uint32_t* fscr = scr + (size_t)blockIdx.y * kHuffScratchWords;
    huff_load_entries(entries, fscr, kHuffTableWords);
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int w0 = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wv), nw = gridDim.x * 4;
    const PackFrame f = a.f[blockIdx.y];
    const LumaIdx<bs> idx(lane);
    pack_loop(
        w0, nw, nb, [&](int b) { return pack_load<WRITE, bs>(f, b, nb, lane); },
        [&](int b, const PackIn& in) {
            pack_huff_one_block<WRITE, bs>(f, b, cap, lane, in, sq[wv], stage[WRITE ? wv : 0], idx, entries, fscr);
        });
}

// One chroma record by one wave, as so_packchroma.hip pack_chroma_bits_one without the order.
template <bool WRITE>
SO_DEV void pack_chroma_huff_one(const ChromaPackFrame& f, int b, const ChromaDst& d, int lane, const ChromaIn& in,
                                 int16_t* __restrict__ sq, uint32_t* __restrict__ stage, const int* idx,
                                 const uint32_t* entries, const uint32_t* __restrict__ fscr) {
    const PackRuns<2> r = chroma_runs(in, lane, sq, idx);
    const HuffLane<2> l = huff_lane<0>(entries, r, 64, lane);
    int tot;
    const int ex = wave_excl_scan(l.bits, lane, &tot);
    const int nbytes = (tot + 7) >> 3;
    const int head = b == 0 ? kHuffChromaTableBytes : 0;
    if (!WRITE) {
        if (lane == 0) f.offs[b] = (uint32_t)(head + nbytes);
        return;
    }
    if (in.o1 > d.cap) return;
    stage_zero(stage, nbytes, lane);
    __builtin_amdgcn_wave_barrier();
    huff_put<kChromaHuffStageWords>(stage, ex, r, l);
    __builtin_amdgcn_wave_barrier();
    if (head) huff_store_tables(d.out + in.o0, fscr, head, lane);
    stage_store(d.out + in.o0 + head, stage, nbytes, lane);
}

// AFTER: the frame's base as so_packchroma.hip pack_chroma_kernel reads it, the totals from here.
template <bool WRITE, bool AFTER = false>
__global__ void __launch_bounds__(256) pack_chroma_huff_kernel(const ChromaPackArgs a, int nb, unsigned long long cap,
                                                               uint32_t* totals, const uint32_t* __restrict__ scr) {
    __shared__ alignas(4) int16_t sq[4][128];
    __shared__ uint32_t stage[WRITE ? 4 : 1][WRITE ? kChromaHuffStageWords : 1];
    __shared__ uint32_t entries[kHuffChromaTables * kHuffSyms];
    const uint32_t* fscr = scr + (size_t)blockIdx.y * kHuffScratchWords;
    huff_load_entries(entries, fscr, kHuffChromaTables * kHuffSyms);
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int w0 = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wv), nw = gridDim.x * 4;
    const ChromaPackFrame f = a.f[blockIdx.y];
    ChromaDst d{f.out, cap};
    if constexpr (WRITE && AFTER) {
        const uint32_t base = f.base ? *f.base : 0u;
        d.out += base;
        d.cap = cap > base ? cap - base : 0ull;
        if (totals && blockIdx.x == 0 && threadIdx.x == 0)
            __hip_atomic_store(totals + blockIdx.y, base + f.offs[nb], __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    int idx[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int P = 2 * lane + j;
        idx[j] = (P & 64) + c_scan8.t[P & 63];
    }
    pack_loop(
        w0, nw, nb, [&](int b) { return chroma_load<WRITE>(f, b, nb, lane); },
        [&](int b, const ChromaIn& in) {
            pack_chroma_huff_one<WRITE>(f, b, d, lane, in, sq[wv], stage[WRITE ? wv : 0], idx, entries, fscr);
        });
}

// ---- unpack --------------------------------------------------------------------------------------
// The decoder itself -- the tables' rule, HuffDec, HuffReader, the list parser and the two record
// bodies -- is the plain layer of so_packfmt.h; here only the workgroup's cooperation around it.

// The frame's tables, by the whole workgroup: false (the frame is malformed at record 0) when
// record 0 is shorter than the table bytes, the last nibble is set (huff_tables_head_ok) or a
// table's Kraft sum exceeds 1 (huff_dec_build, lane t for table t).  Reads nothing but the table
// bytes, and those only when record 0 holds them.
SO_DEV bool huff_dec_tables(HuffDec* tabs, int* bad, const uint8_t* in, const uint32_t* offs, int ntab) {
    const uint32_t o0 = offs[0], o1 = offs[1];
    const bool fits = o1 >= o0 && o1 - o0 >= (uint32_t)huff_table_bytes(ntab);
    if (threadIdx.x == 0) *bad = !fits || !huff_tables_head_ok(in + o0, o1 - o0, ntab);
    __syncthreads();
    if (fits && (int)threadIdx.x < ntab && !huff_dec_build(tabs[threadIdx.x], in + o0, threadIdx.x))
        __hip_atomic_store(bad, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    return *bad == 0;
}

// One thread per block, the frame's tables validated and expanded once per workgroup.
template <int BS>
__global__ void __launch_bounds__(256) unpack_huff_block_kernel(const UnpackArgs a, int nb, int32_t* __restrict__ err) {
    __shared__ HuffDec tabs[kHuffLumaTables];
    __shared__ int tbad;
    const UnpackFrame& f = a.f[blockIdx.y];
    if (!huff_dec_tables(tabs, &tbad, f.in, f.offs, kHuffLumaTables)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    const uint32_t o0 = f.offs[b] + (b == 0 ? kHuffLumaTableBytes : 0), o1 = f.offs[b + 1];
    int16_t* q = f.qtc + (size_t)b * (BS * BS);
    zero_i16<BS * BS>(q);
    const int inter = f.frame_type == 1;
    HuffReader r(f.in + o0, o1 - o0, o1 < o0, tabs);
    unpack_huff_luma_record<BS>(r, inter, f.split + b, f.mv + (size_t)b * (inter ? 12 : 4), q);
    if (r.bad) __hip_atomic_store(err, b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(256) unpack_chroma_huff_kernel(const ChromaUnpackArgs a, int nb, int32_t* __restrict__ err) {
    __shared__ HuffDec tabs[kHuffChromaTables];
    __shared__ int tbad;
    const ChromaUnpackFrame& f = a.f[blockIdx.y];
    if (!huff_dec_tables(tabs, &tbad, f.in, f.offs, kHuffChromaTables)) {
        if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    const uint32_t o0 = f.offs[b] + (b == 0 ? kHuffChromaTableBytes : 0), o1 = f.offs[b + 1];
    int16_t* qu = f.qu + (size_t)b * 64;
    int16_t* qv = f.qv + (size_t)b * 64;
    zero_i16<64>(qu);
    zero_i16<64>(qv);
    HuffReader r(f.in + o0, o1 - o0, o1 < o0, tabs);
    unpack_huff_chroma_record(r, qu, qv);
    if (r.bad) __hip_atomic_store(err, b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- host ----------------------------------------------------------------------------------------
// a chunk's scratch, zeroed, from the device's stream-ordered pool (no host synchronisation)
static int huff_scratch(uint32_t** scr, int n, hipStream_t st) {
    const size_t bytes = (size_t)n * kHuffScratchWords * sizeof(uint32_t);
    hipError_t e = hipMallocAsync(reinterpret_cast<void**>(scr), bytes, st);
    if (e == hipSuccess) e = hipMemsetAsync(*scr, 0, bytes, st);
    if (e != hipSuccess) {
        set_error("huff pack scratch: %s", hipGetErrorString(e));
        return (int)e;
    }
    return SO_OK;
}

int pack_huff_frames_launch(const PackFrame* frames, int nframes, int nb, int bs, unsigned long long cap,
                            uint32_t* totals, hipStream_t st) {
    int rc = SO_OK;
    const int all = for_frame_chunks<PackArgs>(frames, nframes, "pack huff kernels", [&](const PackArgs& a, int n, int f0) {
        uint32_t* scr = nullptr;
        if (rc != SO_OK || (rc = huff_scratch(&scr, n, st)) != SO_OK) return;
        const dim3 grid = pack_grid(nb, n);
        if (bs == 16) hipLaunchKernelGGL(huff_hist_kernel<16>, grid, dim3(256), 0, st, a, nb, scr);
        else hipLaunchKernelGGL(huff_hist_kernel<8>, grid, dim3(256), 0, st, a, nb, scr);
        hipLaunchKernelGGL(huff_tables_kernel, dim3(n), dim3(64), 0, st, scr, kHuffLumaTables);
        if (bs == 16) hipLaunchKernelGGL((pack_huff_block_kernel<false, 16>), grid, dim3(256), 0, st, a, nb, cap, scr);
        else hipLaunchKernelGGL((pack_huff_block_kernel<false, 8>), grid, dim3(256), 0, st, a, nb, cap, scr);
        pack_scan_launch(a, n, nb, totals ? totals + f0 : nullptr, st);
        if (bs == 16) hipLaunchKernelGGL((pack_huff_block_kernel<true, 16>), grid, dim3(256), 0, st, a, nb, cap, scr);
        else hipLaunchKernelGGL((pack_huff_block_kernel<true, 8>), grid, dim3(256), 0, st, a, nb, cap, scr);
        (void)hipFreeAsync(scr, st);
    });
    return rc != SO_OK ? rc : all;
}

int pack_chroma_huff_frames_launch(const ChromaPackFrame* frames, int nframes, int nb, bool after,
                                   unsigned long long cap, uint32_t* totals, hipStream_t st) {
    int rc = SO_OK;
    const int all = for_frame_chunks<ChromaPackArgs>(
        frames, nframes, "pack chroma huff kernels", [&](const ChromaPackArgs& a, int n, int f0) {
            uint32_t* scr = nullptr;
            if (rc != SO_OK || (rc = huff_scratch(&scr, n, st)) != SO_OK) return;
            PackArgs sa{};   // the scan reads only `offs`
            for (int i = 0; i < n; ++i) sa.f[i].offs = a.f[i].offs;
            const dim3 grid = pack_grid(nb, n);
            uint32_t* const tot = totals ? totals + f0 : nullptr;
            uint32_t* const none = nullptr;
            hipLaunchKernelGGL(huff_chroma_hist_kernel, grid, dim3(256), 0, st, a, nb, scr);
            hipLaunchKernelGGL(huff_tables_kernel, dim3(n), dim3(64), 0, st, scr, kHuffChromaTables);
            hipLaunchKernelGGL((pack_chroma_huff_kernel<false>), grid, dim3(256), 0, st, a, nb, cap, none, scr);
            pack_scan_launch(sa, n, nb, after ? none : tot, st);
            if (after) hipLaunchKernelGGL((pack_chroma_huff_kernel<true, true>), grid, dim3(256), 0, st, a, nb, cap, tot, scr);
            else hipLaunchKernelGGL((pack_chroma_huff_kernel<true>), grid, dim3(256), 0, st, a, nb, cap, none, scr);
            (void)hipFreeAsync(scr, st);
        });
    return rc != SO_OK ? rc : all;
}

int unpack_huff_frames_launch(const UnpackFrame* frames, int nframes, int nb, int bs, int32_t* err, hipStream_t st) {
    return for_frame_chunks<UnpackArgs>(
        frames, nframes, "unpack_huff_block_kernel", [&](const UnpackArgs& a, int n, int) {
            const dim3 grid = unpack_grid(nb, n);
            if (bs == 16) hipLaunchKernelGGL(unpack_huff_block_kernel<16>, grid, dim3(256), 0, st, a, nb, err);
            else hipLaunchKernelGGL(unpack_huff_block_kernel<8>, grid, dim3(256), 0, st, a, nb, err);
        });
}

int unpack_chroma_huff_frames_launch(const ChromaUnpackFrame* frames, int nframes, int nb, int32_t* err,
                                     hipStream_t st) {
    return for_frame_chunks<ChromaUnpackArgs>(
        frames, nframes, "unpack_chroma_huff_kernel", [&](const ChromaUnpackArgs& a, int n, int) {
            hipLaunchKernelGGL(unpack_chroma_huff_kernel, unpack_grid(nb, n), dim3(256), 0, st, a, nb, err);
        });
}

}  // namespace so
