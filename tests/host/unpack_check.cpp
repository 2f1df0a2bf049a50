// Host build of the packed stream's strict decoders (streamoptima_amd/csrc/so_packfmt.h, plain
// layer): the record bodies the unpack kernels run, here on the CPU under AddressSanitizer and
// UndefinedBehaviorSanitizer, so that "never reads outside the record's bytes, never writes outside
// the record's outputs, whatever the bytes" is checked and not only claimed.  Built and run by
// tests/test_host.py (CPU):
//   c++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all unpack_check.cpp
//   unpack_check IN OUT
// IN: records { u8 coding (0 varint, 1 bits, 2 huff), u8 kind (0 luma 16, 1 luma 8, 2 chroma), u8 frame
// type, u8 0, u32 n, n bytes }; huff: { ..., u32 n, u32 nt, nt bytes, n bytes }, the nt bytes what
// record 0 of the frame holds of the table bytes (all of them, or fewer when record 0 is shorter) and
// the n bytes the record (record 0's: what follows the tables).  Every record's bytes, the table
// bytes, the expanded tables and each output live in a heap allocation of exactly their size.
// OUT: per record { u8 bad, u8 split, i16 mv[12], i16 q[256] } (chroma: U in q[0..64), V in
// q[64..128); what a record does not have stays 0; huff with malformed tables: bad, nothing decoded).
#define SO_DEV inline
#include "../../streamoptima_amd/csrc/so_packfmt.h"

#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

struct Out {
    uint8_t bad, split;
    int16_t mv[12];
    int16_t q[256];
};
static_assert(sizeof(Out) == 2 + 24 + 512, "Out is written as it lies in memory");

template <int BS, typename Reader>
static void luma(const uint8_t* p, size_t n, int ftype, Out& o) {
    const int inter = ftype == 1, nmv = inter ? 12 : 4;
    std::unique_ptr<uint8_t[]> split(new uint8_t[1]());
    std::unique_ptr<int16_t[]> mv(new int16_t[nmv]());
    std::unique_ptr<int16_t[]> q(new int16_t[BS * BS]());
    Reader r(p, n, false);
    so::unpack_luma_record<BS>(r, inter, split.get(), mv.get(), q.get());
    o.bad = r.bad;
    o.split = split[0];
    memcpy(o.mv, mv.get(), sizeof(int16_t) * nmv);
    memcpy(o.q, q.get(), sizeof(int16_t) * BS * BS);
}

template <typename Reader>
static void chroma(const uint8_t* p, size_t n, Out& o) {
    std::unique_ptr<int16_t[]> qu(new int16_t[64]()), qv(new int16_t[64]());
    Reader r(p, n, false);
    so::unpack_chroma_record(r, qu.get(), qv.get());
    o.bad = r.bad;
    memcpy(o.q, qu.get(), 128);
    memcpy(o.q + 64, qv.get(), 128);
}

// huff: the frame's tables as the kernels' workgroup validates and expands them (the same two
// functions, the lanes' work in a loop), then the record body.  ntab: 15 luma, 14 chroma.
template <typename Body>
static void huff(const uint8_t* tb, size_t nt, int ntab, const uint8_t* p, size_t n, Out& o, Body body) {
    std::unique_ptr<so::HuffDec[]> tabs(new so::HuffDec[ntab]);
    bool ok = so::huff_tables_head_ok(tb, nt, ntab);
    for (int t = 0; ok && t < ntab; ++t) ok = so::huff_dec_build(tabs[t], tb, t);
    if (!ok) {
        o.bad = 1;
        return;
    }
    so::HuffReader r(p, n, false, tabs.get());
    body(r);
    o.bad = r.bad;
}

template <int BS>
static void huff_luma(const uint8_t* tb, size_t nt, const uint8_t* p, size_t n, int ftype, Out& o) {
    const int inter = ftype == 1, nmv = inter ? 12 : 4;
    std::unique_ptr<uint8_t[]> split(new uint8_t[1]());
    std::unique_ptr<int16_t[]> mv(new int16_t[nmv]());
    std::unique_ptr<int16_t[]> q(new int16_t[BS * BS]());
    huff(tb, nt, so::kHuffLumaTables, p, n, o,
         [&](so::HuffReader& r) { so::unpack_huff_luma_record<BS>(r, inter, split.get(), mv.get(), q.get()); });
    o.split = split[0];
    memcpy(o.mv, mv.get(), sizeof(int16_t) * nmv);
    memcpy(o.q, q.get(), sizeof(int16_t) * BS * BS);
}

static void huff_chroma(const uint8_t* tb, size_t nt, const uint8_t* p, size_t n, Out& o) {
    std::unique_ptr<int16_t[]> qu(new int16_t[64]()), qv(new int16_t[64]());
    huff(tb, nt, so::kHuffChromaTables, p, n, o,
         [&](so::HuffReader& r) { so::unpack_huff_chroma_record(r, qu.get(), qv.get()); });
    memcpy(o.q, qu.get(), 128);
    memcpy(o.q + 64, qv.get(), 128);
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    uint8_t h[8];
    long records = 0;
    while (fread(h, 1, 8, in) == 8) {
        uint32_t n;
        memcpy(&n, h + 4, 4);
        const int bits = h[0], kind = h[1], ftype = h[2];
        uint32_t nt = 0;
        if (bits == 2 && fread(&nt, 4, 1, in) != 1) return 2;
        std::unique_ptr<uint8_t[]> tb(new uint8_t[nt]);
        if (nt && fread(tb.get(), 1, nt, in) != nt) return 2;
        std::unique_ptr<uint8_t[]> bytes(new uint8_t[n]);   // exactly n: a read past the record is caught
        if (n && fread(bytes.get(), 1, n, in) != n) return 2;
        Out o;
        memset(&o, 0, sizeof o);
        if (bits == 2 && kind == 0) huff_luma<16>(tb.get(), nt, bytes.get(), n, ftype, o);
        else if (bits == 2 && kind == 1) huff_luma<8>(tb.get(), nt, bytes.get(), n, ftype, o);
        else if (bits == 2 && kind == 2) huff_chroma(tb.get(), nt, bytes.get(), n, o);
        else if (bits > 2) return 2;
        else if (kind == 0 && !bits) luma<16, so::VarintReader>(bytes.get(), n, ftype, o);
        else if (kind == 0) luma<16, so::BitReader>(bytes.get(), n, ftype, o);
        else if (kind == 1 && !bits) luma<8, so::VarintReader>(bytes.get(), n, ftype, o);
        else if (kind == 1) luma<8, so::BitReader>(bytes.get(), n, ftype, o);
        else if (kind == 2 && !bits) chroma<so::VarintReader>(bytes.get(), n, o);
        else if (kind == 2) chroma<so::BitReader>(bytes.get(), n, o);
        else return 2;
        if (fwrite(&o, sizeof o, 1, out) != 1) return 2;
        ++records;
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    printf("%ld records\n", records);
    return 0;
}
