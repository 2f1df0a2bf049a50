// Host build of what one parse lane of the fused luma decoder runs (streamoptima_amd/csrc/so_decode.hip
// phase 1: so_packfmt.h decode_luma_p_record = unpack_luma_record + luma_mv_refs_ok), on the CPU under
// AddressSanitizer and UndefinedBehaviorSanitizer.  The record is parsed into the middle slot of a
// three-slot coefficient tile with the kernel's padded stride (decode_tile_stride), the split and mv
// tiles alike, every allocation exactly sized; the neighbours' slots and the slot's own padding hold
// a pattern that must survive.  A reference array of exactly nref pointers is indexed -- and the
// plane behind the pointer read -- only after the check, as the kernel does.  Built and run by
// tests/test_decode_host.py (CPU):
//   c++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all decode_check.cpp
//   decode_check IN OUT
// IN: records { u8 coding (0 varint, 1 bits), u8 kind (0 luma 16, 1 luma 8), u8 nref, u8 0, u32 n,
// n bytes }.  OUT: per record { u8 bad, u8 split, u8 neighbours untouched, u8 reference bytes read,
// i16 mv[12], i16 q[256] }.
#define SO_DEV inline
#include "../../streamoptima_amd/csrc/so_packfmt.h"

#include <stdio.h>
#include <string.h>

#include <memory>
#include <vector>

struct Out {
    uint8_t bad, split, clean, fetched;
    int16_t mv[12];
    int16_t q[256];
};
static_assert(sizeof(Out) == 4 + 24 + 512, "Out is written as it lies in memory");

constexpr int16_t kPattern = 0x5A5A;

template <int BS, typename Reader>
static void one(const uint8_t* p, size_t n, int nref, Out& o) {
    constexpr int NN = BS * BS, STRIDE = so::decode_tile_stride(NN);
    static_assert(STRIDE == NN + 8, "the kernel's slot: the block and 4 dwords of padding");
    std::unique_ptr<int16_t[]> tile(new int16_t[3 * STRIDE]);
    std::unique_ptr<int16_t[]> mv(new int16_t[3 * 12]);
    std::unique_ptr<uint8_t[]> split(new uint8_t[3]);
    for (int i = 0; i < 3 * STRIDE; ++i) tile[i] = kPattern;
    for (int i = 0; i < NN; ++i) tile[STRIDE + i] = 0;          // what phase 0 zeroes for the record
    for (int i = 0; i < 36; ++i) mv[i] = kPattern;
    memset(split.get(), 0x5A, 3);
    // the frame's reference list: exactly nref pointers, each to a plane of one byte
    std::vector<std::unique_ptr<uint8_t[]>> planes;
    std::unique_ptr<const uint8_t*[]> refs(new const uint8_t*[nref]);
    for (int r = 0; r < nref; ++r) {
        planes.emplace_back(new uint8_t[1]);
        planes.back()[0] = (uint8_t)(r + 1);
        refs[r] = planes.back().get();
    }
    Reader r(p, n, false);
    const bool bad = so::decode_luma_p_record<BS>(r, nref, split.get() + 1, mv.get() + 12, tile.get() + STRIDE);
    o.bad = bad;
    o.fetched = 0;
    if (!bad) {   // phase 2 runs for this block: it indexes the list with the block's reference indices
        o.split = split[1];
        for (int j = 0; j < (split[1] ? 4 : 1); ++j) o.fetched += refs[mv[12 + 3 * j + 2]][0] != 0;
        memcpy(o.mv, mv.get() + 12, 24);
        memcpy(o.q, tile.get() + STRIDE, sizeof(int16_t) * NN);
    }
    bool clean = split[0] == 0x5A && split[2] == 0x5A;
    for (int i = 0; i < 12; ++i) clean = clean && mv[i] == kPattern && mv[24 + i] == kPattern;
    for (int i = 0; i < STRIDE; ++i) clean = clean && tile[i] == kPattern && tile[2 * STRIDE + i] == kPattern;
    for (int i = NN; i < STRIDE; ++i) clean = clean && tile[STRIDE + i] == kPattern;
    o.clean = clean;
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
        std::unique_ptr<uint8_t[]> bytes(new uint8_t[n]);   // exactly n: a read past the record is caught
        if (n && fread(bytes.get(), 1, n, in) != n) return 2;
        const int bits = h[0], kind = h[1], nref = h[2];
        if (nref < 1 || nref > 4 || kind > 1) return 2;
        Out o;
        memset(&o, 0, sizeof o);
        if (kind == 0 && !bits) one<16, so::VarintReader>(bytes.get(), n, nref, o);
        else if (kind == 0) one<16, so::BitReader>(bytes.get(), n, nref, o);
        else if (!bits) one<8, so::VarintReader>(bytes.get(), n, nref, o);
        else one<8, so::BitReader>(bytes.get(), n, nref, o);
        if (fwrite(&o, sizeof o, 1, out) != 1) return 2;
        ++records;
    }
    fclose(in);
    if (fclose(out) != 0) return 2;
    printf("%ld records\n", records);
    return 0;
}
