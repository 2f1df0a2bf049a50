// Host check of the scalar identities behind the packed tail of tq16_exact's FAST path
// (so_block.h: recon_row_bytes, sse_row_packed) and of the two forms that were built beside it
// and left out (the carry-free packed add as the byte add's alternative; the token count's row
// mask from the int16 pairs of the QTC store, measured level and not kept: DESIGN.md section 4).
// Stand-alone:
//
//     c++ -O1 -std=c++17 -Wall -Werror -fsanitize=address,undefined tools/check_recon_pack.cpp -o check && ./check
//
// Each model below performs the operations of the device code on plain integers:
//   1. the SDWA byte add (src0 byte e + src1 byte 3 -> dst byte e, the other bytes preserved)
//      against (pred + (gfix >> 24)) & 255 and against the former ((pred << 24) + gfix) >> 24,
//      for all 256 x 256 byte pairs, every byte index, random low bits and neighbours;
//   2. the carry-free packed byte add ((a & 7f..) + (b & 7f..)) ^ ((a ^ b) & 80..), the
//      alternative form of 1, over random dwords and the extremes;
//   3. c.c - 2 c.r + r.r in wrapping u32 against the sum of (c - r)^2, for all byte pairs and
//      for random and extreme 16-pixel rows through a model of v_dot4_u32_u8;
//   4. the row mask from packed int16 pairs (per-half unsigned min with 1, shift by 2 j, OR,
//      fold by 15) against the per-level compare, including -32768, -1, 0 and 1.
// Exit status 0 and "ok" when every identity holds; the first mismatch is printed otherwise.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {   // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static int fails = 0;
#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            if (fails++ < 10) {                   \
                std::printf("FAIL %s: ", #cond);  \
                std::printf(__VA_ARGS__);         \
                std::printf("\n");                \
            }                                     \
        }                                         \
    } while (0)

// v_add_u32_sdwa dst, src0, src1 dst_sel:BYTE_e dst_unused:UNUSED_PRESERVE src0_sel:BYTE_e src1_sel:BYTE_3
static uint32_t sdwa_add_byte(uint32_t dst, uint32_t src0, uint32_t src1, int e) {
    const uint32_t a = (src0 >> (8 * e)) & 255u, b = src1 >> 24;   // unsigned selects, zero-extended
    const uint32_t sum = a + b;                                    // the 32-bit add
    const uint32_t keep = dst & ~(255u << (8 * e));
    return keep | ((sum & 255u) << (8 * e));                       // the low byte of the result lands in byte e
}

// recon_row_bytes: the prediction dwords updated in place, byte e of pw[k] from g[4 k + e]
static void recon_row_bytes(uint32_t (&pw)[4], const uint32_t (&g)[16]) {
    for (int e = 0; e < 4; ++e)
        for (int k = 0; k < 4; ++k) pw[k] = sdwa_add_byte(pw[k], pw[k], g[4 * k + e], e);
}

static uint32_t packed_add_u8(uint32_t a, uint32_t b) {
    return ((a & 0x7f7f7f7fu) + (b & 0x7f7f7f7fu)) ^ ((a ^ b) & 0x80808080u);
}

// v_dot4_u32_u8 without clamp: acc + the four byte products, wrapping u32
static uint32_t udot4(uint32_t a, uint32_t b, uint32_t acc) {
    for (int e = 0; e < 4; ++e) acc += ((a >> (8 * e)) & 255u) * ((b >> (8 * e)) & 255u);
    return acc;
}

static uint32_t sse_row_packed(const uint32_t (&c)[4], const uint32_t (&r)[4]) {
    uint32_t sq = 0, cr = 0;
    for (int k = 0; k < 4; ++k) {
        sq = udot4(c[k], c[k], sq);
        sq = udot4(r[k], r[k], sq);
        cr = udot4(c[k], r[k], cr);
    }
    return sq - 2u * cr;
}

static uint32_t mask_from_pairs(const uint32_t (&p)[8]) {
    uint32_t a = 0;
    for (int j = 0; j < 8; ++j) {
        const uint32_t lo = p[j] & 0xFFFFu, hi = p[j] >> 16;
        const uint32_t t = (lo < 1u ? lo : 1u) | ((hi < 1u ? hi : 1u) << 16);   // v_pk_min_u16 with {1, 1}
        a |= t << (2 * j);
    }
    return (a | (a >> 15)) & 0xFFFFu;
}

static void check_byte_add() {
    for (int e = 0; e < 4; ++e)
        for (uint32_t pred = 0; pred < 256; ++pred)
            for (uint32_t top = 0; top < 256; ++top) {
                const uint32_t other = rnd() & ~(255u << (8 * e));
                const uint32_t pw = other | (pred << (8 * e));
                const uint32_t gfix = (top << 24) | (rnd() & 0xFFFFFFu);
                const uint32_t got = sdwa_add_byte(pw, pw, gfix, e);
                const uint32_t want = (pred + (gfix >> 24)) & 255u;
                const uint32_t former = (((pred << 24) + gfix) >> 24) & 255u;   // rec & 255 of the int form
                CHECK(((got >> (8 * e)) & 255u) == want, "e %d pred %u top %u", e, pred, top);
                CHECK(want == former, "former form: pred %u top %u", pred, top);
                CHECK((got & ~(255u << (8 * e))) == other, "neighbour bytes: e %d pred %u top %u", e, pred, top);
            }
    for (int it = 0; it < 200000; ++it) {   // whole rows
        uint32_t pw[4], p0[4], g[16];
        for (int k = 0; k < 4; ++k) p0[k] = pw[k] = it & 1 ? rnd() : (it & 2 ? 0u : 0xFFFFFFFFu);
        for (int c = 0; c < 16; ++c) g[c] = it & 4 ? rnd() : (rnd() & 0xFFFFFFu) | (it & 8 ? 0xFF000000u : 0x01000000u);
        recon_row_bytes(pw, g);
        for (int c = 0; c < 16; ++c) {
            const uint32_t pred = (p0[c >> 2] >> (8 * (c & 3))) & 255u;
            const uint32_t rec = (uint32_t)(int)((((pred) << 24) + g[c]) >> 24);
            CHECK(((pw[c >> 2] >> (8 * (c & 3))) & 255u) == (rec & 255u), "row it %d pixel %d", it, c);
        }
    }
}

static void check_packed_add() {
    const uint32_t ext[] = {0u, 0xFFFFFFFFu, 0x80808080u, 0x7F7F7F7Fu, 0x01010101u, 0xFF00FF00u, 0x00FF00FFu};
    const int ne = (int)(sizeof ext / sizeof ext[0]);
    for (int it = 0; it < 2000000 + ne * ne; ++it) {
        const uint32_t a = it < ne * ne ? ext[it / ne] : rnd(), b = it < ne * ne ? ext[it % ne] : rnd();
        uint32_t want = 0;
        for (int e = 0; e < 4; ++e) want |= ((((a >> (8 * e)) & 255u) + ((b >> (8 * e)) & 255u)) & 255u) << (8 * e);
        CHECK(packed_add_u8(a, b) == want, "a %08x b %08x", a, b);
    }
}

static void check_sse() {
    for (uint32_t c = 0; c < 256; ++c)
        for (uint32_t r = 0; r < 256; ++r) {
            const int d = (int)c - (int)r;
            CHECK(c * c - 2u * (c * r) + r * r == (uint32_t)(d * d), "bytes c %u r %u", c, r);
        }
    for (int it = 0; it < 500000; ++it) {
        uint32_t c[4], r[4];
        for (int k = 0; k < 4; ++k) {
            switch (it & 7) {   // the extremes: |c - r| = 255 on every pixel, both ways and alternating
                case 0: c[k] = 0u, r[k] = 0xFFFFFFFFu; break;
                case 1: c[k] = 0xFFFFFFFFu, r[k] = 0u; break;
                case 2: c[k] = 0xFF00FF00u, r[k] = 0x00FF00FFu; break;
                case 3: c[k] = r[k] = 0xFFFFFFFFu; break;
                default: c[k] = rnd(), r[k] = rnd();
            }
        }
        uint32_t want = 0;
        for (int p = 0; p < 16; ++p) {
            const int d = (int)((c[p >> 2] >> (8 * (p & 3))) & 255u) - (int)((r[p >> 2] >> (8 * (p & 3))) & 255u);
            want += (uint32_t)(d * d);
        }
        CHECK(sse_row_packed(c, r) == want, "row it %d", it);
        CHECK(want <= 16u * 255u * 255u, "row bound it %d", it);
    }
}

static void check_mask() {
    const int special[] = {-32768, -1, 0, 1, 32767, -32767, 2, -2, 256, -256};
    const int ns = (int)(sizeof special / sizeof special[0]);
    for (int it = 0; it < 1000000; ++it) {
        int q[16];
        for (int c = 0; c < 16; ++c) {
            const uint32_t v = rnd();
            switch (it & 3) {
                case 0: q[c] = special[v % ns]; break;
                case 1: q[c] = (v & 3) ? 0 : special[(v >> 2) % ns]; break;          // mostly zeros
                case 2: q[c] = (int)(int16_t)(v & 0xFFFFu); break;                    // any int16
                default: q[c] = (v & 1) ? 0 : (int)(int16_t)((v >> 1) & 0xFFFFu);
            }
        }
        if (it < 16) {   // single non-zero level at every position, both signs of the extremes
            for (int c = 0; c < 16; ++c) q[c] = 0;
            q[it] = it & 1 ? -32768 : -1;
        }
        uint32_t p[8], want = 0;
        for (int k = 0; k < 8; ++k) p[k] = (uint32_t)(uint16_t)q[2 * k] | ((uint32_t)q[2 * k + 1] << 16);
        for (int c = 0; c < 16; ++c) want |= (q[c] != 0 ? 1u : 0u) << c;
        CHECK(mask_from_pairs(p) == want, "mask it %d: got %04x want %04x", it, mask_from_pairs(p), want);
    }
}

int main() {
    check_byte_add();
    check_packed_add();
    check_sse();
    check_mask();
    if (fails) {
        std::printf("%d checks failed\n", fails);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
