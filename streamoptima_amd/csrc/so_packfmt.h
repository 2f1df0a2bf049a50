// so_packfmt.h — the packed stream's format, stated once for its four device sources (so_pack.hip:
// luma, varints; so_packbits.hip: luma, Exp-Golomb bits; so_packchroma.hip: chroma, both codings;
// so_packhuff.hip: luma and chroma, per-frame Huffman tables) and for so_capi.hip.  The format itself is described at the top of those sources and is normative
// in include/streamoptima.h; this header holds what they share.
//
// Two layers:
//   * the plain layer -- C++17 with no device builtin beyond __builtin_clz*, every function SO_DEV:
//     the launch interface (frame structs, bounds, *_launch prototypes), the coding primitives, the
//     scan tables, and the strict decoders (two readers over a record's bytes, one token-list
//     parser, the luma and chroma record bodies; for "huff" the table rule, the expanded tables, the
//     reader through them and its two record bodies).  A host compiler can include it with SO_DEV
//     defined as `inline` (tests/host/unpack_check.cpp runs the decoders under sanitizers);
//   * the device layer (hipcc only) -- what the pack kernels share: the wave scan, the LDS stages,
//     the run machinery, the order-k choice, the load-ahead loop and the host loop over frames.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "so_common.h"

namespace so {

// =================================== plain layer ===============================================

// ---- launch interface ---------------------------------------------------------------------------
struct PackFrame {
    const uint8_t* split;
    const int16_t* mv;
    const int16_t* qtc;
    uint32_t* offs;        // [nb + 1] exclusive offsets (pass 1 writes counts)
    uint8_t* out;          // packed bytes
    int frame_type;
};
struct UnpackFrame {
    const uint8_t* in;
    const uint32_t* offs;
    uint8_t* split;
    int16_t* mv;
    int16_t* qtc;
    int frame_type;
};
struct ChromaPackFrame {
    const int16_t* qu;
    const int16_t* qv;
    uint32_t* offs;        // [nb + 1] exclusive offsets (pass 1 writes counts)
    uint8_t* out;
    const uint32_t* base;  // device word: the records go to out + *base + offs[b]; null: 0
};
struct ChromaUnpackFrame {
    const uint8_t* in;
    const uint32_t* offs;
    int16_t* qu;
    int16_t* qv;
};
constexpr int kPackMax = 32;   // frames a launch takes by value
struct PackArgs {
    PackFrame f[kPackMax];
};
struct UnpackArgs {
    UnpackFrame f[kPackMax];
};
struct ChromaPackArgs {
    ChromaPackFrame f[kPackMax];
};
struct ChromaUnpackArgs {
    ChromaUnpackFrame f[kPackMax];
};

// Worst case bytes of one luma block, varints: split + 4 x 3 mv varints + the token list of bs*bs
// coefficients (at most nn values + nn/2 + 1 run tokens, 3 bytes for any int16).
constexpr size_t pack_block_bound(int bs) { return 1 + 12 * 3 + (size_t)3 * (bs * bs + bs * bs / 2 + 4); }
constexpr int kPackStage = (int)pack_block_bound(16);
// Bits: split + k, 12 mv values of 33 bits, nn coefficients of 33 bits, and nn / 2 + 4 tokens of 19
// bits (|token| <= 256).  Loose on purpose, like pack_block_bound: no block has nn coefficients and
// that many tokens at once.
constexpr int pack_bits_block_bits(int bs) { return 3 + 12 * 33 + 33 * bs * bs + 19 * (bs * bs / 2 + 4); }
constexpr size_t pack_bits_block_bound(int bs) { return (size_t)(pack_bits_block_bits(bs) + 7) / 8; }
constexpr int kBitsStageWords = (pack_bits_block_bits(16) + 31) / 32;
// One chroma record, loose alike: two lists of 64 values, 32 run tokens and 4 more, 3 bytes each;
// 2 bits of k and two lists of 64 values of 33 bits and 36 tokens of 19 bits.
constexpr int kChromaBound = 2 * 3 * (64 + 32 + 4);                           // 600
constexpr int kChromaBitsBound = (2 + 2 * (33 * 64 + 19 * 36) + 7) / 8;       // 700
constexpr size_t pack_chroma_record_bound(bool bits) { return bits ? kChromaBitsBound : kChromaBound; }
constexpr int kChromaStageWords = (kChromaBitsBound + 3) / 4 + 1;

// Huffman coding ("huff"): 43 symbols per table, code lengths 1..15 in 4 bits each; luma has 15 tables
// (mv, tok0..6, coef0..6), chroma 14 (tok0..6, coef0..6), at the head of record 0.  A value is a code
// of at most 15 bits and at most 15 raw bits; a token (|token| <= 256, chroma 64) at most 15 + 9 (7).
constexpr int kHuffSyms = 43, kHuffMaxLen = 15, kHuffCtx = 7;
constexpr int kHuffLumaTables = 1 + 2 * kHuffCtx, kHuffChromaTables = 2 * kHuffCtx;
constexpr int huff_table_bytes(int ntab) { return (ntab * kHuffSyms + 1) / 2; }
constexpr int kHuffLumaTableBytes = huff_table_bytes(kHuffLumaTables);       // 323
constexpr int kHuffChromaTableBytes = huff_table_bytes(kHuffChromaTables);   // 301
constexpr int pack_huff_block_bits(int bs) { return 1 + 12 * 30 + 30 * bs * bs + 24 * (bs * bs / 2 + 4); }
constexpr size_t pack_huff_block_bound(int bs) { return (size_t)(pack_huff_block_bits(bs) + 7) / 8; }
constexpr int kHuffStageWords = (pack_huff_block_bits(16) + 31) / 32 + 1;
constexpr int kChromaHuffBound = (2 * (30 * 64 + 22 * 36) + 7) / 8;          // 678
constexpr int kChromaHuffStageWords = (kChromaHuffBound + 3) / 4 + 1;
// a frame's device scratch, in 32-bit words: the counts, the (length << 16 | code) entries, the table bytes
constexpr int kHuffTableWords = kHuffLumaTables * kHuffSyms;
constexpr int kHuffScratchWords = 2 * kHuffTableWords + (kHuffLumaTableBytes + 3) / 4 + 1;

// so_pack.hip
int pack_frames_launch(const PackFrame* frames, int nframes, int nb, int bs, unsigned long long cap, uint32_t* totals,
                       hipStream_t st);
int unpack_frames_launch(const UnpackFrame* frames, int nframes, int nb, int bs, int32_t* err, hipStream_t st);
// the one scan of per-record byte counts, for every coding: only `offs` of a.f[i] is read
void pack_scan_launch(const PackArgs& a, int nframes, int nb, uint32_t* totals, hipStream_t st);
// so_packbits.hip
int pack_bits_frames_launch(const PackFrame* frames, int nframes, int nb, int bs, unsigned long long cap,
                            uint32_t* totals, hipStream_t st);
int unpack_bits_frames_launch(const UnpackFrame* frames, int nframes, int nb, int bs, int32_t* err, hipStream_t st);
// so_packchroma.hip
int pack_chroma_frames_launch(const ChromaPackFrame* frames, int nframes, int nb, bool bits, bool after,
                              unsigned long long cap, uint32_t* totals, hipStream_t st);
int unpack_chroma_frames_launch(const ChromaUnpackFrame* frames, int nframes, int nb, bool bits, int32_t* err,
                                hipStream_t st);

// so_packhuff.hip
int pack_huff_frames_launch(const PackFrame* frames, int nframes, int nb, int bs, unsigned long long cap,
                            uint32_t* totals, hipStream_t st);
int unpack_huff_frames_launch(const UnpackFrame* frames, int nframes, int nb, int bs, int32_t* err, hipStream_t st);
int pack_chroma_huff_frames_launch(const ChromaPackFrame* frames, int nframes, int nb, bool after,
                                   unsigned long long cap, uint32_t* totals, hipStream_t st);
int unpack_chroma_huff_frames_launch(const ChromaUnpackFrame* frames, int nframes, int nb, int32_t* err,
                                     hipStream_t st);

// ---- coding primitives --------------------------------------------------------------------------
SO_DEV uint32_t zz(int v) { return ((uint32_t)v << 1) ^ (uint32_t)(v >> 31); }
SO_DEV int unzz(uint32_t z) { return (int)(z >> 1) ^ -(int)(z & 1u); }
// LEB128 length: floor((bit_length(z | 1) - 1) / 7) + 1, the division as (x * 37) >> 8 (exact
// for x < 32); no compares, so no VCC round trips per value
SO_DEV int vlen(uint32_t z) { return (((31 - __builtin_clz(z | 1u)) * 37) >> 8) + 1; }
// bits of ue(z), z <= 65535: 2 * bit_length(z + 1) - 1
SO_DEV int ue_len(uint32_t z) { return 63 - 2 * __builtin_clz(z + 1u); }

// ---- scan tables: scan position -> row-major index in an n x n block (anti-diagonal order,
// entropy_encoder_block, Encoder.py:1093-1123) ------------------------------------------------------
template <int N>
struct ScanTable {
    uint8_t t[N * N];
};
template <int N>
constexpr ScanTable<N> make_scan() {
    ScanTable<N> s{};
    int p = 0;
    for (int k = 0; k < 2 * N - 1; ++k) {
        int i = k < N ? 0 : k - N + 1, j = k < N ? k : N - 1;
        while (i < N && j >= 0) s.t[p++] = (uint8_t)(i * N + j), ++i, --j;
    }
    return s;
}
template <int N>
constexpr bool scan_inverts_scan_pos() {
    const ScanTable<N> s = make_scan<N>();
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j)
            if (s.t[scan_pos(N, i, j)] != i * N + j) return false;
    return true;
}
static_assert(scan_inverts_scan_pos<8>() && scan_inverts_scan_pos<16>(), "scan tables against so_common.h scan_pos");
#ifdef __HIPCC__
// initialised by a constant expression, so the tables arrive with the code object on every device
static __constant__ ScanTable<8> c_scan8 = make_scan<8>();
static __constant__ ScanTable<16> c_scan16 = make_scan<16>();
SO_DEV const uint8_t* scan_table(int n) { return n == 16 ? c_scan16.t : c_scan8.t; }
#else
constexpr ScanTable<8> k_scan8 = make_scan<8>();
constexpr ScanTable<16> k_scan16 = make_scan<16>();
SO_DEV const uint8_t* scan_table(int n) { return n == 16 ? k_scan16.t : k_scan8.t; }
#endif

// ---- the strict decoders ------------------------------------------------------------------------
// A reader walks one record's bytes [p, p + n) and never reads a byte outside them, whatever they
// hold; `bad` is set once the record is malformed and stays set.  Both readers offer split(),
// order(), se(k), finish(), so the record bodies below are written once for both codings.

// Varints.  A varint is 1-5 bytes.  Whatever its role, no value of a well-formed record leaves int16
// (split 0 / 1, |token| <= n*n <= 256, mv values and coefficients int16), i.e. zz < 2^16: the first
// three bytes carry 21 bits, any payload bit of the fourth and fifth byte (kept apart in `hi`, so
// none is shifted out) or of bits 16-20 makes the record malformed, and what is returned always
// fits the int16 it is stored to.
struct VarintReader {
    const uint8_t* p;
    const uint8_t* end;
    bool bad;
    SO_DEV VarintReader(const uint8_t* q, size_t n, bool bad0) : p(q), end(q + (bad0 ? 0 : n)), bad(bad0) {}
    SO_DEV int se(int /*k*/) {
        uint32_t z = 0, hi = 0;
        for (int sh = 0; sh < 35; sh += 7) {
            if (p >= end) break;
            const uint32_t c = *p++;
            if (sh < 21) z |= (c & 0x7Fu) << sh;
            else hi |= c & 0x7Fu;
            if (!(c & 0x80u)) {
                if (hi | (z >> 16)) break;
                return unzz(z);
            }
        }
        bad = true;
        return 0;
    }
    SO_DEV int split() { return se(0); }      // a number like any other: 0, or 1 at block size 16
    SO_DEV int order() { return 0; }          // varints have no order
    SO_DEV void finish() {                    // all the record's bytes must be consumed
        if (p != end) bad = true;
    }
};

// Bits, MSB first.  se(k): ue_k on zz(v) -- at most 16 prefix zeros, then 17 + k bits at most, 36 of
// the 41 that peek() returns; a longer prefix, a code running past the record's last byte or a
// z > 65535 is malformed.
struct BitReader {
    const uint8_t* p;
    unsigned long long nbytes, nbits, pos;
    bool bad;
    SO_DEV BitReader(const uint8_t* q, size_t n, bool bad0)
        : p(q), nbytes(bad0 ? 0ull : (unsigned long long)n), nbits(nbytes * 8), pos(0), bad(bad0) {}
    // the next 41+ bits at the top of a 64-bit word, zeros past the record's last byte
    SO_DEV unsigned long long peek() const {
        const unsigned long long by = pos >> 3;
        unsigned long long w = 0;
        for (int i = 0; i < 6; ++i) w = (w << 8) | (by + i < nbytes ? p[by + i] : 0u);
        return w << (16 + (int)(pos & 7));
    }
    SO_DEV uint32_t take(int n) {   // n plain bits, 1 <= n <= 8
        if (pos + n > nbits) {
            bad = true;
            return 0;
        }
        const uint32_t x = (uint32_t)(peek() >> (64 - n));
        pos += n;
        return x;
    }
    SO_DEV int se(int k) {
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
        return unzz(z);
    }
    SO_DEV int split() { return (int)take(1); }
    SO_DEV int order() { return (int)take(2); }
    SO_DEV void finish() {          // the pad: fewer than 8 bits left, all of them zero
        if (bad) return;
        const unsigned long long left = nbits - pos;
        if (left >= 8 || (left > 0 && (p[nbytes - 1] & ((1u << left) - 1u)) != 0)) bad = true;
    }
};

// One token list into the zeroed (sub-)block q of nn coefficients: a token -L needs 1 <= L <= nn - c
// and is followed by L values (order k), a token Z > 0 needs Z <= nn - c (c: the coefficients
// covered so far); a token 0 ends the list (the trailing zeros), and a list also ends at c == nn.
// Writes only q[scan[0 .. nn)].
template <typename Reader>
SO_DEV void unpack_token_list(int16_t* q, const uint8_t* scan, int nn, Reader& r, int k) {
    int c = 0;
    while (c < nn && !r.bad) {
        const int t = r.se(0);
        if (r.bad) break;
        if (t < 0) {
            if (-t > nn - c) { r.bad = true; break; }
            for (int i = 0; i < -t && !r.bad; ++i) q[scan[c + i]] = (int16_t)r.se(k);
            c -= t;
        } else if (t == 0) {
            break;
        } else {
            if (t > nn - c) { r.bad = true; break; }
            c += t;
        }
    }
}

// One luma record: split (0, or 1 at block size 16), the order (bits), the mv values (inter: dx, dy,
// ref; intra: dx; once, or 4x when split), then 1 list of BS x BS or 4 of 8 x 8.  mv: the block's
// 12 (inter) or 4 (intra) entries, those past the first of an unsplit block 0 on output; q: its
// BS * BS coefficients, zeroed by the caller.
template <int BS, typename Reader>
SO_DEV void unpack_luma_record(Reader& r, int inter, uint8_t* split, int16_t* mv, int16_t* q) {
    const int sp = r.split();
    const int k = r.order();
    if (sp != 0 && (sp != 1 || BS != 16)) r.bad = true;
    *split = (uint8_t)(sp == 1 && !r.bad);
    const int per = inter ? 3 : 1, nmv = (sp == 1 ? 4 : 1) * per;
    for (int j = 0; j < 4 * per; ++j) mv[j] = (int16_t)(j < nmv && !r.bad ? r.se(0) : 0);
    const int nsub = sp == 1 ? 4 : 1, n = sp == 1 ? 8 : BS, nn = n * n;
    const uint8_t* scan = scan_table(n);
    for (int j = 0; j < nsub && !r.bad; ++j) unpack_token_list(q + j * nn, scan, nn, r, k);
    r.finish();
}

// One chroma record: the order (bits), U's 8 x 8 list, then V's, into the zeroed qu / qv.
template <typename Reader>
SO_DEV void unpack_chroma_record(Reader& r, int16_t* qu, int16_t* qv) {
    const int k = r.order();
    unpack_token_list(qu, scan_table(8), 64, r, k);
    if (!r.bad) unpack_token_list(qv, scan_table(8), 64, r, k);
    r.finish();
}

// ---- the strict decoder of the "huff" coding ----------------------------------------------------
// The contexts: cls(p) = min(bit_length(p), 6).
SO_DEV int huff_cls(int p) { return p == 0 ? 0 : (32 - __builtin_clz((unsigned)p) < 6 ? 32 - __builtin_clz((unsigned)p) : 6); }

// A table as a decoder holds it: per length the first canonical code, the number of codes and where
// its symbols start in `sym` (the symbols by (length, symbol)).  Built from the transmitted lengths
// alone; any lengths whose Kraft sum is <= 1 are a valid table.
struct HuffDec {
    uint16_t first[kHuffMaxLen + 1];
    uint8_t cnt[kHuffMaxLen + 1], base[kHuffMaxLen + 1];
    uint8_t sym[kHuffSyms];
};

SO_DEV int huff_nibble(const uint8_t* bytes, int i) { return i & 1 ? bytes[i >> 1] & 15 : bytes[i >> 1] >> 4; }

// The frame-level rule, first half: record 0, n bytes at `bytes`, holds the table bytes of ntab tables
// and their spare nibble (luma: 645 nibbles in 323 bytes) is 0.  Reads the spare nibble's byte only
// when record 0 holds it.
SO_DEV bool huff_tables_head_ok(const uint8_t* bytes, unsigned long long n, int ntab) {
    if (n < (unsigned long long)huff_table_bytes(ntab)) return false;
    const int nnib = ntab * kHuffSyms;
    return !(nnib & 1) || huff_nibble(bytes, nnib) == 0;
}

// Second half: table t of the table bytes; false when its Kraft sum exceeds 1.  Reads the table's 43
// nibbles, writes d.
SO_DEV bool huff_dec_build(HuffDec& d, const uint8_t* bytes, int t) {
    for (int l = 0; l <= kHuffMaxLen; ++l) d.cnt[l] = 0;
    for (int s = 0; s < kHuffSyms; ++s) ++d.cnt[huff_nibble(bytes, t * kHuffSyms + s)];
    d.cnt[0] = 0;
    uint32_t kraft = 0, code = 0, at = 0;
    for (int l = 1; l <= kHuffMaxLen; ++l) {
        kraft += (uint32_t)d.cnt[l] << (kHuffMaxLen - l);
        d.first[l] = (uint16_t)code;
        d.base[l] = (uint8_t)at;
        code = (code + d.cnt[l]) << 1;
        at += d.cnt[l];
    }
    if (kraft > (1u << kHuffMaxLen)) return false;
    for (int l = 1, n = 0; l <= kHuffMaxLen; ++l)
        for (int s = 0; s < kHuffSyms && d.cnt[l]; ++s)
            if (huff_nibble(bytes, t * kHuffSyms + s) == l) d.sym[n++] = (uint8_t)s;
    return true;
}

// The bit reader with values read through the tables.  val(t): a bit pattern that matches no code of
// table t, or a code or its raw bits running past the record's last byte, is malformed.
struct HuffReader : BitReader {
    const HuffDec* tabs;
    SO_DEV HuffReader(const uint8_t* q, size_t n, bool bad0, const HuffDec* t) : BitReader(q, n, bad0), tabs(t) {}
    SO_DEV int val(int t) {
        const HuffDec& d = tabs[t];
        const unsigned long long W = peek();
        const uint32_t top = (uint32_t)(W >> (64 - kHuffMaxLen));
        int len = 1, s = -1;
        for (; len <= kHuffMaxLen; ++len) {
            const uint32_t c = (top >> (kHuffMaxLen - len)) - d.first[len];
            if (c < d.cnt[len]) {
                s = d.sym[d.base[len] + c];
                break;
            }
        }
        uint32_t z = (uint32_t)s;
        int nx = 0;
        if (s >= 32) {
            nx = s - 27;
            z = (1u << nx) | (uint32_t)((W << len) >> (64 - nx));
        }
        if (s < 0 || pos + len + nx > nbits) {
            bad = true;
            return 0;
        }
        pos += len + nx;
        return unzz(z);
    }
};

// unpack_token_list with the tables picked by position; TOK0: the first token table
template <int TOK0>
SO_DEV void unpack_huff_list(int16_t* q, const uint8_t* scan, int nn, HuffReader& r) {
    int c = 0;
    while (c < nn && !r.bad) {
        const int t = r.val(TOK0 + huff_cls(c));
        if (r.bad) break;
        if (t < 0) {
            if (-t > nn - c) { r.bad = true; break; }
            for (int i = 0; i < -t && !r.bad; ++i) q[scan[c + i]] = (int16_t)r.val(TOK0 + kHuffCtx + huff_cls(c + i));
            c -= t;
        } else if (t == 0) {
            break;
        } else {
            if (t > nn - c) { r.bad = true; break; }
            c += t;
        }
    }
}

// One luma record (record 0: what follows the table bytes): split (1 raw bit; 1 only at block size
// 16), the mv values through table 0, then 1 list of BS x BS or 4 of 8 x 8 through tok0..6 (tables
// 1..7) and coef0..6.  mv and q as unpack_luma_record.
template <int BS>
SO_DEV void unpack_huff_luma_record(HuffReader& r, int inter, uint8_t* split, int16_t* mv, int16_t* q) {
    const int sp = r.split();
    if (sp != 0 && BS != 16) r.bad = true;
    *split = (uint8_t)(sp == 1 && !r.bad);
    const int per = inter ? 3 : 1, nmv = (sp == 1 ? 4 : 1) * per;
    for (int j = 0; j < 4 * per; ++j) mv[j] = (int16_t)(j < nmv && !r.bad ? r.val(0) : 0);
    const int nsub = sp == 1 ? 4 : 1, n = sp == 1 ? 8 : BS, nn = n * n;
    const uint8_t* scan = scan_table(n);
    for (int j = 0; j < nsub && !r.bad; ++j) unpack_huff_list<1>(q + j * nn, scan, nn, r);
    r.finish();
}

// One chroma record: U's 8 x 8 list, then V's, through tok0..6 (tables 0..6) and coef0..6.
SO_DEV void unpack_huff_chroma_record(HuffReader& r, int16_t* qu, int16_t* qv) {
    unpack_huff_list<0>(qu, scan_table(8), 64, r);
    if (!r.bad) unpack_huff_list<0>(qv, scan_table(8), 64, r);
    r.finish();
}

// ---- what the fused decoders (so_decode.hip) add ------------------------------------------------
// A P-frame's reference indices are input like any other number of the record: true when every
// motion vector the block uses -- its first, or all four when split -- names a reference in
// [0, nref).  A decoder indexes its reference list only after this holds.
SO_DEV bool luma_mv_refs_ok(int split, const int16_t* mv, int nref) {
    bool ok = true;
    for (int j = 0; j < (split ? 4 : 1); ++j) ok = ok && mv[3 * j + 2] >= 0 && mv[3 * j + 2] < nref;
    return ok;
}

// The fused decoders parse a workgroup's records into an LDS tile, one record per lane, kDecodeTile
// records per workgroup.  A record's coefficients start decode_tile_stride int16 after the previous
// record's: 8 int16 (4 dwords) of padding keep the 16-byte row loads of the transform phase aligned
// and spread the parse lanes over 16 LDS banks instead of one.
constexpr int kDecodeTile = 64;
constexpr int decode_tile_stride(int ncoef) { return ncoef + 8; }

// One luma P record into its tile slot q (zeroed by the caller): unpack_luma_record, then the
// reference check.  Returns true when the record is malformed; split / mv / q are then unspecified
// and must not be used.
template <int BS, typename Reader>
SO_DEV bool decode_luma_p_record(Reader& r, int nref, uint8_t* split, int16_t* mv, int16_t* q) {
    unpack_luma_record<BS>(r, 1, split, mv, q);
    return r.bad || !luma_mv_refs_ok(*split, mv, nref);
}

// =================================== device layer ==============================================
#ifdef __HIPCC__

// accesses that reinterpret int16 storage: may_alias, so that type-based alias analysis keeps them
// in order with the int16 accesses to the same bytes
typedef uint32_t __attribute__((may_alias)) u32_alias;
typedef uint2 __attribute__((may_alias)) uint2_alias;
typedef uint4 __attribute__((may_alias)) uint4_alias;

// n int16 of an unpack output to zero, n a multiple of 8, q 16-byte aligned
template <int N>
SO_DEV void zero_i16(int16_t* q) {
#pragma unroll
    for (int i = 0; i < N / 8; ++i) reinterpret_cast<uint4_alias*>(q)[i] = make_uint4(0, 0, 0, 0);
}

SO_DEV void put_varint(uint8_t* p, int v) {
    uint32_t z = zz(v);
    do {
        *p++ = (uint8_t)(z & 0x7F) | (z > 0x7F ? 0x80 : 0);
        z >>= 7;
    } while (z);
}

// exclusive prefix sum over the wave; *total = the wave's sum.  T may pack independent fields whose
// wave sums stay below their widths, so that nothing carries from one into the next.
template <typename T>
SO_DEV T wave_excl_scan(T x, int lane, T* total) {
    T s = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(s, d);
        if (lane >= d) s += y;
    }
    *total = __shfl(s, 63);
    return s - x;
}

// The runs of a record, one wave: lane l owns the R consecutive scan positions R*l + j, whose values
// are v[]; the record is 64 * R positions in segments of S (a power of two; S = 64 * R: one list).
// A position starts a run when it opens a segment or its non-zero flag differs from the previous
// position's; a run's length is the distance to the next start (inside the lane, else the first
// start of the next lane that has one: one ballot and one shuffle).  tok[j] is the token position j
// would write -- it does write it when bit j of stb is set -- and nzb the non-zero flags.
template <int R>
struct PackRuns {
    int v[R], tok[R];
    unsigned nzb, stb;
};

template <int R>
SO_DEV PackRuns<R> pack_runs(const int (&v)[R], int S, int lane) {
    PackRuns<R> r;
    r.nzb = 0;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        r.v[j] = v[j];
        r.nzb |= (unsigned)(v[j] != 0) << j;
    }
    const unsigned prev_last = __shfl_up((r.nzb >> (R - 1)) & 1, 1);
    const unsigned prevb = ((r.nzb << 1) | (lane > 0 ? prev_last : 0u)) & ((1u << R) - 1);
    r.stb = r.nzb ^ prevb;
    if ((R * lane) % S == 0) r.stb |= 1u;         // a segment opens at this lane's first position
    const unsigned long long lanes_with_start = __ballot(r.stb != 0);
    const unsigned long long above = lane == 63 ? 0ull : lanes_with_start & (~0ull << (lane + 1));
    const int nl = above ? __builtin_ctzll(above) : lane;
    const int nfs = __shfl((int)__builtin_ctz(r.stb | 0x10u), nl);
    const int next_lane_start = above ? R * nl + nfs : 64 * R;
#pragma unroll
    for (int j = 0; j < R; ++j) {   // branch-free: every position computes its would-be token
        const unsigned later = r.stb & ~((2u << j) - 1);
        // the lane's next start after j; after j = R - 2 that can only be its last position
        const int in_lane = j == R - 2 ? R - 1 : __builtin_ctz(later | 0x10u);
        const int nxt = later ? R * lane + in_lane : next_lane_start;
        const int run = nxt - (R * lane + j);
        r.tok[j] = (r.nzb >> j) & 1 ? -run : ((nxt & (S - 1)) == 0 ? 0 : run);   // a trailing zero run is one 0
    }
    return r;
}

// a lane's varint bytes: its run tokens where it starts runs, its non-zero values
template <int R>
SO_DEV int varint_bytes(const PackRuns<R>& r) {
    int n = 0;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int nzj = (r.nzb >> j) & 1, stj = (r.stb >> j) & 1;
        n += (vlen(zz(r.tok[j])) & -stj) + (vlen(zz(r.v[j])) & -nzj);
    }
    return n;
}

template <int R>
SO_DEV void put_varints(uint8_t* p, const PackRuns<R>& r) {
#pragma unroll
    for (int j = 0; j < R; ++j) {
        if ((r.stb >> j) & 1) {
            put_varint(p, r.tok[j]);
            p += vlen(zz(r.tok[j]));
        }
        if (r.v[j] != 0) {
            put_varint(p, r.v[j]);
            p += vlen(zz(r.v[j]));
        }
    }
}

// ---- bits coding ------------------------------------------------------------------------------
// ue_k(z) is z + 2^k in 63 - k - 2 * clz(z + 2^k) bits, so a record's coefficient bits at order k are
// CNT * (63 - k) - 2 * C_k with CNT its non-zero values and C_k the sum of their clz(z + 2^k).  A
// lane sums the four clz of its values (16-bit fields of two words: <= 31 each, <= 7,936 per
// record) and its token bits tb; the orders are compared on the wave's sums.
template <int R>
struct BitsLane {
    uint32_t zt[R], zv[R];      // zz of the tokens and of the values
    uint32_t c01, c23, tb;
    SO_DEV unsigned long long clz_sums() const { return (unsigned long long)c23 << 32 | c01; }
};

template <int R>
SO_DEV BitsLane<R> bits_lane(const PackRuns<R>& r) {
    BitsLane<R> l;
    l.c01 = l.c23 = l.tb = 0;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const int nzj = (r.nzb >> j) & 1, stj = (r.stb >> j) & 1;
        l.zt[j] = zz(r.tok[j]);
        l.zv[j] = zz(r.v[j]);
        l.tb += (uint32_t)(ue_len(l.zt[j]) & -stj);
        const uint32_t m = (uint32_t)-nzj;
        l.c01 += (__builtin_clz(l.zv[j] + 1u) & m) + ((__builtin_clz(l.zv[j] + 2u) & m) << 16);
        l.c23 += (__builtin_clz(l.zv[j] + 4u) & m) + ((__builtin_clz(l.zv[j] + 8u) & m) << 16);
    }
    return l;
}

// bits of cnt values at order k, csum the (wave's, or a prefix's) packed clz sums
SO_DEV int order_bits(int cnt, unsigned long long csum, int k) {
    return cnt * (63 - k) - 2 * (int)((csum >> (16 * k)) & 0xFFFF);
}

// the order in 0..3 with the fewest coefficient bits, ties to the smallest; *bits = those bits
SO_DEV int pick_order(int cnt, unsigned long long ctot, int* bits) {
    int k = 0, best = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {               // strictly smaller only: ties go to the smallest k
        const int t = order_bits(cnt, ctot, c);
        if (c == 0 || t < best) best = t, k = c;
    }
    *bits = best;
    return k;
}

// The wave's LDS stage of WORDS 32-bit words, the stream's first bit the top bit of word 0.  Touched
// only through aligned 32-bit accesses.  Lanes merge their bits with an atomic OR per touched word
// into the zeroed stage: OR commutes, so the bytes do not depend on lane timing.
template <int WORDS>
SO_DEV void stage_or(uint32_t* stage, int w, uint32_t x) {
    if (x != 0 && w < WORDS)   // x != 0 only where the record has bits, i.e. inside its bound
        __hip_atomic_fetch_or(stage + w, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

SO_DEV void stage_zero(uint32_t* stage, int nbytes, int lane) {
    for (int i = lane; i < (nbytes + 3) >> 2; i += 64) stage[i] = 0;
}

// the stage's first nbytes out, consecutive lanes on consecutive bytes
SO_DEV void stage_store(uint8_t* out, const uint32_t* stage, int nbytes, int lane) {
    for (int i = lane; i < nbytes; i += 64) out[i] = (uint8_t)(stage[i >> 2] >> (24 - 8 * (i & 3)));
}

// A lane's consecutive codes, assembled into words before they are merged: `cur` holds the
// `fill` (< 32) bits of word w written so far, at its top.  A lane can own ~300 bits.
template <int WORDS>
struct BitAcc {
    uint32_t* stage;
    int w, fill;
    uint32_t cur;
    SO_DEV void put(uint32_t code, int len) {   // 1 <= len <= 33, code < 2^len
        const unsigned long long W = (unsigned long long)code << (64 - fill - len);   // shift in [0, 63]
        cur |= (uint32_t)(W >> 32);
        fill += len;                            // <= 64
        if (fill >= 32) {
            stage_or<WORDS>(stage, w++, cur);
            cur = (uint32_t)W;
            fill -= 32;
            if (fill == 32) {                   // 31 bits before a 33-bit code: two words complete
                stage_or<WORDS>(stage, w++, cur);
                cur = 0;
                fill = 0;
            }
        }
    }
    SO_DEV void finish() { stage_or<WORDS>(stage, w, cur); }
};

// a lane's codes from bit position pos on: its run tokens (se) where it starts runs, its non-zero
// values (se_k)
template <int WORDS, int R>
SO_DEV void put_codes(uint32_t* stage, int pos, const PackRuns<R>& r, const BitsLane<R>& l, int k) {
    BitAcc<WORDS> acc{stage, pos >> 5, pos & 31, 0u};
#pragma unroll
    for (int j = 0; j < R; ++j) {
        if ((r.stb >> j) & 1) acc.put(l.zt[j] + 1u, ue_len(l.zt[j]));
        const uint32_t code = l.zv[j] + (1u << k);
        if ((r.nzb >> j) & 1) acc.put(code, 63 - k - 2 * __builtin_clz(code));
    }
    acc.finish();
}

// ---- a luma block's inputs and runs (both codings) ---------------------------------------------
// A block's inputs, loaded one block ahead (every load of a block is independent of the others, so
// the wave pays one memory latency per block, not a chain of them).
struct PackIn {
    uint2 q;          // this lane's 4 coefficients (row-major)
    int sp;           // split flag
    int hv;           // mv value lane - 1 (lanes 1..nmv)
    uint32_t o0, o1;  // offs[b], offs[b + 1] (write pass)
};

template <bool WRITE, int bs>
SO_DEV PackIn pack_load(const PackFrame& f, int b, int nb, int lane) {
    // branch-free (b clamped, every lane loads) so the compiler can wait for exactly these
    // loads one block later instead of draining everything in flight
    b = b < nb ? b : nb - 1;
    constexpr int nn = bs * bs;
    const int nmv = f.frame_type == 1 ? 12 : 4;
    const int qi = lane * 4 < nn ? lane * 4 : 0;
    const int mi = lane >= 1 && lane <= nmv ? lane - 1 : 0;
    // the split byte's address goes through an opaque zero so that the load stays a vector
    // load (a uniform one becomes readfirstlane right after it, i.e. an immediate wait)
    int z;
    asm volatile("v_mov_b32 %0, 0" : "=v"(z));
    PackIn in;
    in.q = *reinterpret_cast<const uint2_alias*>(f.qtc + (size_t)b * nn + qi);
    in.sp = f.split[b + z];
    in.hv = f.mv[(size_t)b * nmv + mi];
    in.o0 = WRITE ? f.offs[b] : 0;
    in.o1 = WRITE ? f.offs[b + 1] : 0;
    return in;
}

// this lane's R = bs * bs / 64 scan positions as element indices of the row-major block, unsplit and
// split (4 segments of 8 x 8)
template <int bs>
struct LumaIdx {
    static constexpr int R = (bs * bs) >> 6;
    int whole[R], split[R];
    SO_DEV explicit LumaIdx(int lane) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int P = R * lane + j;
            whole[j] = bs == 16 ? c_scan16.t[P] : c_scan8.t[P];
            split[j] = (P & ~63) + c_scan8.t[P & 63];
        }
    }
};

// the block through the wave's LDS row into scan order, then its runs: one segment of bs * bs
// positions, or 4 of 64 when split
template <int bs>
SO_DEV PackRuns<LumaIdx<bs>::R> luma_runs(const PackIn& in, int sp, int lane, int16_t* __restrict__ sq,
                                          const LumaIdx<bs>& idx) {
    constexpr int nn = bs * bs, R = nn >> 6;
    if (lane * 4 < nn) *reinterpret_cast<uint2_alias*>(&sq[lane * 4]) = in.q;
    const int S = (sp && bs == 16) ? 64 : nn;   // segment length in scan positions
    __builtin_amdgcn_wave_barrier();   // LDS ops of one wave run in order; no fence (it would
                                       // also wait for the next block's loads in flight)
    int v[R];
#pragma unroll
    for (int j = 0; j < R; ++j) v[j] = sq[S == 64 && bs == 16 ? idx.split[j] : idx.whole[j]];
    return pack_runs<R>(v, S, lane);
}

// ---- a chroma record's inputs and runs (every coding) ------------------------------------------
// A record's inputs, loaded one record ahead: lanes 0..31 hold U's 64 coefficients (two each,
// row-major), lanes 32..63 V's.
struct ChromaIn {
    uint32_t q;
    uint32_t o0, o1;  // offs[b], offs[b + 1] (write pass)
};

// The write pass's view of a frame: `out` already moved to the frame's base, `cap` lowered by it
// (0 when the base alone passes it: no record of one byte or more fits).
struct ChromaDst {
    uint8_t* out;
    unsigned long long cap;
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
// and 2l + 1 of the U|V sequence, and the runs of its two lists (so_packfmt.h pack_runs at R = 2,
// S = 64).
SO_DEV PackRuns<2> chroma_runs(const ChromaIn& in, int lane, int16_t* __restrict__ sq, const int* idx) {
    reinterpret_cast<u32_alias*>(sq)[lane] = in.q;
    __builtin_amdgcn_wave_barrier();   // LDS ops of one wave run in order
    const int v[2] = {sq[idx[0]], sq[idx[1]]};
    return pack_runs<2>(v, 64, lane);
}

// ---- loops ---------------------------------------------------------------------------------------
// A wave's records b = w0, w0 + nw, ... < nb: two per iteration, each one's inputs loaded one record
// ahead, in two register sets (a loop-carried copy of a register still being loaded would wait for
// it).  load(b) must tolerate b >= nb (it clamps).
template <typename Load, typename One>
SO_DEV void pack_loop(int w0, int nw, int nb, Load load, One one) {
    auto x = load(w0);
    for (int b = w0; b < nb; b += 2 * nw) {
        const auto y = load(b + nw);
        one(b, x);
        if (b + nw >= nb) break;
        x = load(b + 2 * nw);
        one(b + nw, y);
    }
}

// host: the frames in chunks of kPackMax, each chunk by value in an Args; launch(a, n, f0) enqueues
// the chunk's kernels
template <typename Args, typename Frame, typename Launch>
int for_frame_chunks(const Frame* frames, int nframes, const char* what, Launch launch) {
    for (int f0 = 0; f0 < nframes; f0 += kPackMax) {
        const int n = nframes - f0 < kPackMax ? nframes - f0 : kPackMax;
        Args a{};
        for (int i = 0; i < n; ++i) a.f[i] = frames[f0 + i];
        launch(a, n, f0);
        const int rc = check_launch(what);
        if (rc != SO_OK) return rc;
    }
    return SO_OK;
}

// pack grid: 4 waves a workgroup, 8 records a wave; unpack grid: one thread a record
inline dim3 pack_grid(int nb, int n) { return dim3((nb + 31) / 32, n); }
inline dim3 unpack_grid(int nb, int n) { return dim3((nb + 255) / 256, n); }

#endif  // __HIPCC__

}  // namespace so
