// Host check of the fast transforms (so_dct.h: dct2_16_fast / dct3_16_fast) with tq16_exact's
// certificates and fallback against the pocketfft sequence alone: levels and reconstruction of
// every block of a corpus both ways, at QP 0-12.  Exits non-zero on any difference.
//   hipcc -O2 -ffp-contract=off -DSO_DEV=inline tools/check_dct_fast.cpp -o check_dct_fast -lpthread
//   ./check_dct_fast [--blocks N] [--file ties.bin]      (ties.bin: int16 [n][16][16] residual blocks)
// Prints the largest |fast - pocketfft| per direction with the derived bounds, the thresholds,
// and per QP the share of blocks flagged in each direction.
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../streamoptima_amd/csrc/so_dct.h"

namespace d = so::dct;

static constexpr double kRne = 0x1.8p52;
static inline int lo32(double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    return (int)(uint32_t)u;
}
static inline int q_exp(int row, int c, int qp) {
    const int s = row + c - 14;
    return qp + (s < 0 ? 0 : (s > 2 ? 2 : s));
}

struct Stats {
    double max_fwd = 0, max_inv = 0;
    long blocks[13] = {}, flag_fwd[13] = {}, flag_inv[13] = {}, inv_run[13] = {};
    long bad = 0, vectors = 0;
    void merge(const Stats& o) {
        max_fwd = std::fmax(max_fwd, o.max_fwd);
        max_inv = std::fmax(max_inv, o.max_inv);
        for (int i = 0; i < 13; ++i) {
            blocks[i] += o.blocks[i]; flag_fwd[i] += o.flag_fwd[i]; flag_inv[i] += o.flag_inv[i]; inv_run[i] += o.inv_run[i];
        }
        bad += o.bad;
        vectors += o.vectors;
    }
};

// 2-D transforms of integer rows, columns first (xform2d_rows / xform2d_fast)
template <bool INV, bool FAST>
static void xform2d(const int (&in)[16][16], double (&out)[16][16]) {
    double t[16][16];
    for (int l = 0; l < 16; ++l) {
        int x[16];
        double v[16];
        for (int r = 0; r < 16; ++r) x[r] = in[r][l];
        if (FAST) {
            if (INV) {
                for (int r = 0; r < 16; ++r) v[r] = (double)x[r];
                d::dct3_16_fast(v);
            } else {
                d::dct2_16_fast_i(x, v);
            }
        } else {
            if (INV) d::dct3_16_i(x, v); else d::dct2_16_i(x, v);
        }
        for (int r = 0; r < 16; ++r) t[r][l] = v[r];
    }
    for (int l = 0; l < 16; ++l) {
        double v[16];
        for (int c = 0; c < 16; ++c) v[c] = t[l][c];
        if (FAST) { if (INV) d::dct3_16_fast(v); else d::dct2_16_fast(v); }
        else { if (INV) d::dct3<16>(v); else d::dct2<16>(v); }
        for (int c = 0; c < 16; ++c) out[l][c] = v[c];
    }
}

static void quant(const double (&z)[16][16], int qp, int (&q)[16][16]) {
    for (int l = 0; l < 16; ++l)
        for (int c = 0; c < 16; ++c)
            q[l][c] = lo32(std::fma(std::nearbyint(z[l][c]), std::ldexp(1.0, -q_exp(l, c, qp)), kRne));
}

// one block at one QP: returns false on a difference
static bool check_block(const int (&res)[16][16], int qp, Stats& st) {
    double zp[16][16], zf[16][16];
    xform2d<false, false>(res, zp);
    xform2d<false, true>(res, zf);
    st.vectors += 64;
    int qa[16][16], qb[16][16];
    quant(zp, qp, qa);
    // the forward rule
    bool flag = false;
    for (int l = 0; l < 16; ++l)
        for (int c = 0; c < 16; ++c) {
            st.max_fwd = std::fmax(st.max_fwd, std::fabs(zf[l][c] - zp[l][c]));
            const double sc = std::ldexp(1.0, -q_exp(l, c, qp));
            const double r = std::nearbyint(zf[l][c]), dd = zf[l][c] - r;
            qb[l][c] = lo32(std::fma(r, sc, kRne));
            if (std::fabs(dd) >= 0.5 - d::kFastDeltaFwd) {
                const double r2 = r + std::copysign(1.0, dd);
                flag |= lo32(std::fma(r2, sc, kRne)) != qb[l][c];
            }
        }
    ++st.blocks[qp];
    if (flag) {
        ++st.flag_fwd[qp];
        std::memcpy(qb, qa, sizeof qa);   // the fallback: the pocketfft sequence's levels
    }
    bool ok = std::memcmp(qa, qb, sizeof qa) == 0;
    // inverse
    int dq[16][16];
    bool any = false;
    for (int l = 0; l < 16; ++l)
        for (int c = 0; c < 16; ++c) {
            dq[l][c] = (int)((uint32_t)qa[l][c] << q_exp(l, c, qp));
            any |= dq[l][c] != 0;
        }
    (void)any;
    double vp[16][16], vf[16][16];
    xform2d<true, false>(dq, vp);
    xform2d<true, true>(dq, vf);
    st.vectors += 64;
    ++st.inv_run[qp];
    constexpr double kFix = 0x1.8p28 + 0.5;
    bool iflag = false;
    int ra[16][16], rb[16][16];
    for (int l = 0; l < 16; ++l)
        for (int c = 0; c < 16; ++c) {
            st.max_inv = std::fmax(st.max_inv, std::fabs(vf[l][c] - vp[l][c]));
            ra[l][c] = lo32(vp[l][c] + kRne) & 255;
            const uint32_t g = (uint32_t)lo32(vf[l][c] + kFix);
            rb[l][c] = (int)(g >> 24);
            iflag |= ((g + 2u) << 8) <= (4u << 8);
        }
    if (iflag) {
        ++st.flag_inv[qp];
        std::memcpy(rb, ra, sizeof ra);
    }
    ok = ok && std::memcmp(ra, rb, sizeof ra) == 0;
    if (!ok) ++st.bad;
    return ok;
}

static void gen_block(std::mt19937_64& rng, long i, int (&res)[16][16]) {
    static const int lo[3] = {-128, 0, -255}, hi[3] = {127, 255, 0};   // tests/adversarial.py RANGES
    const int kind = (int)(i % 16);
    if (kind < 12) {            // seeded uniform residuals in the three ranges
        const int g = kind % 3;
        const int amp = kind < 6 ? hi[g] - lo[g] : 12;   // half of them low amplitude
        const int base = kind < 6 ? lo[g] : (lo[g] + hi[g]) / 2 - 6;
        for (auto& row : res) for (int& v : row) v = base + (int)(rng() % (uint64_t)(amp + 1));
    } else if (kind == 12) {    // constants at +-255 and small
        const int v0 = (rng() & 1) ? ((rng() & 1) ? 255 : -255) : (int)(rng() % 11) - 5;
        for (auto& row : res) for (int& v : row) v = v0;
    } else if (kind == 13) {    // alternating +-255 (checkerboard, columns, rows)
        const int m = (int)(rng() % 3), s = (rng() & 1) ? 255 : -255;
        for (int r = 0; r < 16; ++r)
            for (int c = 0; c < 16; ++c) res[r][c] = (((m == 0 ? r + c : (m == 1 ? c : r)) & 1) ? s : -s);
    } else if (kind == 14) {    // a single impulse at +-255
        for (auto& row : res) for (int& v : row) v = 0;
        res[rng() % 16][rng() % 16] = (rng() & 1) ? 255 : -255;
    } else {                    // a DC tie: the sum is 8 (mod 16)
        long sum = 0;
        for (auto& row : res) for (int& v : row) { v = (int)(rng() % 13) - 6; sum += v; }
        int need = (int)(((8 - sum) % 16 + 16) % 16);
        while (need--) res[rng() % 16][rng() % 16] += 1;
    }
}

int main(int argc, char** argv) {
    long nblocks = 1000000;
    std::string file;
    for (int i = 1; i < argc; ++i) {
        if (!std::strcmp(argv[i], "--blocks") && i + 1 < argc) nblocks = std::atol(argv[++i]);
        else if (!std::strcmp(argv[i], "--file") && i + 1 < argc) file = argv[++i];
        else { std::fprintf(stderr, "usage: %s [--blocks N] [--file ties.bin]\n", argv[0]); return 2; }
    }
    Stats total;
    if (!file.empty()) {   // blocks read from a file, each at every QP
        FILE* f = std::fopen(file.c_str(), "rb");
        if (!f) { std::perror(file.c_str()); return 2; }
        std::vector<int16_t> buf(256);
        long n = 0;
        while (std::fread(buf.data(), 2, 256, f) == 256) {
            int res[16][16];
            for (int k = 0; k < 256; ++k) {
                res[k / 16][k % 16] = buf[k];
                if (buf[k] < -255 || buf[k] > 255) { std::fprintf(stderr, "block %ld: residual out of range\n", n); return 2; }
            }
            for (int qp = 0; qp <= 12; ++qp) check_block(res, qp, total);
            ++n;
        }
        std::fclose(f);
        std::printf("file_blocks %ld\n", n);
    }
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt == 0 ? 1 : (nt > 16 ? 16 : nt);
    std::vector<Stats> part(nt);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; ++t)
        th.emplace_back([&, t]() {
            std::mt19937_64 rng(12345 + t);
            for (long i = t; i < nblocks; i += nt) {
                int res[16][16];
                gen_block(rng, i, res);
                check_block(res, (int)((i / 16) % 13), part[t]);
            }
        });
    for (auto& x : th) x.join();
    for (auto& p : part) total.merge(p);
    long nb = 0, ff = 0, fi = 0;
    for (int qp = 0; qp <= 12; ++qp) {
        nb += total.blocks[qp]; ff += total.flag_fwd[qp]; fi += total.flag_inv[qp];
        std::printf("qp %2d blocks %8ld flagged_fwd %.5f flagged_inv %.5f\n", qp, total.blocks[qp],
                    total.blocks[qp] ? (double)total.flag_fwd[qp] / total.blocks[qp] : 0.0,
                    total.blocks[qp] ? (double)total.flag_inv[qp] / total.blocks[qp] : 0.0);
    }
    std::printf("blocks %ld vectors %ld mismatches %ld\n", nb, total.vectors, total.bad);
    std::printf("fwd max_diff %.6e bound_fast %.6e bound_pocketfft %.6e delta %.6e accepted %ld fallback %ld\n", total.max_fwd,
                d::kFastBoundFwd, d::kPocketBoundFwd, d::kFastDeltaFwd, nb - ff, ff);
    std::printf("inv max_diff %.6e bound_fast %.6e bound_pocketfft %.6e delta %.6e accepted %ld fallback %ld\n", total.max_inv,
                d::kFastBoundInv, d::kPocketBoundInv, d::kFastDeltaInv, nb - fi, fi);
    return total.bad ? 1 : 0;
}
