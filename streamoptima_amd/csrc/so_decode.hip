// so_decode.hip — the fused decoders of the packed stream for gfx950: luma P-frames and chroma
// from their packed records straight to pixels (so_decode_p_frames, so_decode_chroma_frames;
// normative in include/streamoptima.h).  What so_unpack_frames(_bits) + so_inter_recon_ex and
// so_unpack_chroma_frames(_bits) + so_chroma_recon_frame compute, bit for bit, without the dense
// int16 coefficients in global memory (2 B per luma pixel written by one kernel and read back by
// the next).
//
// One launch per frame; stream order carries the frame-to-frame dependency (a frame's references
// are earlier launches' outputs).  A 256-thread workgroup takes kDecodeTile = 64 records:
//   0. every thread zeroes its share of the workgroup's int16 coefficient tile in LDS, and the
//      workgroup copies its records' bytes -- one contiguous range of the stream -- into LDS with
//      coalesced dword loads (into the transform scratch, idle until phase 2; a range that does not
//      fit it, or offsets that are not monotonic, leave the records in global memory);
//   1. the 64 lanes of wave 0 parse one record each into the tile -- so_packfmt.h's
//      unpack_luma_record / unpack_chroma_record, the bodies the unpack kernels run, at the same
//      one-record-per-lane utilisation -- and check the reference indices (luma_mv_refs_ok);
//      split, mv and the verdict go to LDS too;
//   2. after a workgroup barrier the 256 threads run the transform body of inter_recon_kernel
//      (so_tq.hip) / chroma_kernel<false> (so_chroma.hip) over the tile: 16 (8) lanes per block,
//      16 (32) blocks per round, 4 (2 at block size 8; 4 for chroma's 128 blocks) rounds -- the same
//      so_block.h functions in the same order, the coefficient rows read from LDS.
// A tile slot is decode_tile_stride() int16: the parse lanes work on 64 different slots at once,
// and a stride of 128 dwords would put all of them on one of the 64 LDS banks; 132 dwords spreads
// them over 16 banks and keeps the 16-byte row loads of phase 2 aligned (129 would spread them over
// all 64 but split every row load).  LDS per workgroup (DESIGN.md "Streaming decode"): 72.6 KB at
// block size 16, two workgroups per CU.  Measured there: a frame's workgroups all start together,
// so they parse together and then transform together; the kernel is slower than the unpack + recon
// pair on a whole run and level with it or faster a frame at a time, which is how the stream runs.
//
// A malformed record (everything the unpack kernels call malformed, and a reference index outside
// the frame's list) sets err[frame] = 1 + block and is skipped by phase 2: nothing is fetched
// through its motion vectors, its pixels are not written.  No thread leaves before the barriers.
#include "so_block.h"
#include "so_chroma.h"
#include "so_packfmt.h"

#include <vector>

namespace so {

// The workgroup's records, the bytes [src, src + total), into the LDS buffer `stage`: byte i of the
// range lands at stage[sh + i], sh = src's misalignment (returned), so that the range's interior
// moves as aligned dwords, consecutive lanes on consecutive words; its ragged ends move as single
// bytes, and nothing outside the range is read.  The parse lanes then walk their records at LDS
// latency instead of paying a global-memory round trip per dependent byte.
SO_DEV uint32_t stage_records(const uint8_t* src, uint32_t total, uint8_t* stage, int tid) {
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 3), end = sh + total;
    const uint8_t* base = src - sh;
    const uint32_t lo = sh ? 1 : 0, hi = end >> 2;   // the full words [lo, hi)
    for (uint32_t j = lo + tid; j < hi; j += 256)
        reinterpret_cast<u32_alias*>(stage)[j] = reinterpret_cast<const u32_alias*>(base)[j];
    if (tid < 8) {   // bytes of the first word, bytes of the word after the last full one
        const uint32_t i = tid < 4 ? (uint32_t)tid : hi * 4 + (uint32_t)(tid - 4);
        if (i >= sh && i < end && (i < 4 * lo || i >= 4 * hi)) stage[i] = base[i];
    }
    return sh;
}

// Whether the workgroup's nv records starting at block b0 can be parsed from LDS: they are the
// consecutive byte ranges of one range of at most `cap` - 3 bytes (offsets that are not
// monotonic, though each inside the stream's buffer, are parsed from global memory as the unpack
// kernels would).  All 256 threads call it; it is a workgroup barrier.  o0 / o1: this lane's record.
SO_DEV bool records_stageable(const uint32_t* __restrict__ offs, int b0, int nv, int tid, uint32_t cap,
                              uint32_t* first, uint32_t* o0, uint32_t* o1) {
    const uint32_t of = offs[b0], ol = offs[b0 + nv];
    bool ok = ol >= of && ol - of <= cap - 3;
    *first = of;
    *o0 = *o1 = 0;
    if (tid < nv) {
        *o0 = offs[b0 + tid];
        *o1 = offs[b0 + tid + 1];
        ok = ok && of <= *o0 && *o0 <= *o1 && *o1 <= ol;
    }
    return __syncthreads_and(ok) != 0;
}

struct DecodeLumaArgs {
    const uint8_t* packed;
    const uint32_t* offs;
    RefSet refs;
    int nref, H, W, qp;
    const int32_t* qp_row;
    const int32_t* qp_map;
    uint8_t* out_split;
    int16_t* out_mv;
    uint8_t* out_recon;
    int32_t* err;          // this frame's word
};

template <int BS, typename Reader>
__global__ void __launch_bounds__(256) decode_p_kernel(const DecodeLumaArgs a) {
    constexpr int NN = BS * BS, STRIDE = decode_tile_stride(NN), T = kDecodeTile;
    constexpr int G = BS, BPW = 256 / G, SB = BS / 2;
    constexpr int LDS_D = BS == 16 ? 288 : BS * (BS + 1);   // inter_recon_kernel's scratch per block
    static_assert((T * STRIDE) % 8 == 0 && (STRIDE * 2) % 16 == 0, "16-byte tile accesses");
    __shared__ alignas(16) int16_t tile[T * STRIDE];
    __shared__ alignas(16) int16_t s_mv[T * 12];
    __shared__ uint8_t s_split[T];
    __shared__ uint8_t s_bad[T];
    __shared__ double ldsd[BPW * LDS_D];
    const int tid = threadIdx.x;
    const int nbx = a.W / BS, nb = nbx * (a.H / BS);
    const int b0 = blockIdx.x * T;
    const int nv = nb - b0 < T ? nb - b0 : T;   // this workgroup's records

    for (int i = tid; i < T * STRIDE / 8; i += 256) reinterpret_cast<uint4_alias*>(tile)[i] = make_uint4(0, 0, 0, 0);
    // the records' bytes through the transform scratch, which phase 2 needs only after the parse
    uint8_t* stage = reinterpret_cast<uint8_t*>(ldsd);
    uint32_t first, o0, o1, sh = 0;
    const bool staged = records_stageable(a.offs, b0, nv, tid, (uint32_t)sizeof(ldsd), &first, &o0, &o1);
    if (staged) {
        sh = stage_records(a.packed + first, a.offs[b0 + nv] - first, stage, tid);
        __syncthreads();
    }
    if (tid < T) {
        bool bad = true;
        if (tid < nv) {
            auto parse = [&](const uint8_t* p) {
                Reader r(p, o1 - o0, o1 < o0);
                return decode_luma_p_record<BS>(r, a.nref, s_split + tid, s_mv + tid * 12, tile + tid * STRIDE);
            };
            bad = staged ? parse(stage + sh + (o0 - first)) : parse(a.packed + o0);
            if (bad) __hip_atomic_store(a.err, b0 + tid + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        s_bad[tid] = (uint8_t)bad;
    }
    __syncthreads();

    // the symbols out, consecutive lanes on consecutive words
    if (tid < nv) a.out_split[b0 + tid] = s_split[tid];
    for (int i = tid; i < nv * 6; i += 256)
        reinterpret_cast<u32_alias*>(a.out_mv + (size_t)b0 * 12)[i] = reinterpret_cast<const u32_alias*>(s_mv)[i];

    const int g = tid / G, l = tid % G;
    double* dl = ldsd + g * LDS_D;
    for (int rd = 0; rd < T / BPW; ++rd) {
        const int k = rd * BPW + g;   // slot; the whole lane group skips together, wave-scope exchange only
        if (k >= nv || s_bad[k]) continue;
        const int b = b0 + k;
        const int bx = b % nbx, by = b / nbx, x = bx * BS, y = by * BS;
        const int qpr = a.qp_map ? a.qp_map[b] : (a.qp_row ? a.qp_row[by] : a.qp);
        const int16_t* m = s_mv + k * 12;
        const int16_t* qt = tile + k * STRIDE;
        // inter_recon_kernel<BS, BS == 16, false>'s body from here on
        if (BS != 16 || !s_split[k]) {
            const int dx = m[0], dy = m[1], rf = m[2];
            int pred[BS], q[BS], dq[BS], rec[BS];
            const bool fast = (0 <= x + dx) && (x + dx < a.W - BS) && (0 <= y + dy) && (y + dy < a.H - BS);
            fetch_row<BS>(pick_ref(a.refs, rf), a.W, a.H, x + dx, y + dy + l, fast, pred);
            load_row_i16<BS>(qt + l * BS, q);
            dequant_row<BS>(q, l, qpr, dq);
            double r2[BS];
            xform2d_rows<BS, true>(dl, l, dq, r2);
#pragma unroll
            for (int c = 0; c < BS; ++c) rec[c] = pred[c] + (int)__builtin_rint(r2[c]);
            store_row_u8<BS>(a.out_recon, a.W, x, y + l, rec);
        } else if constexpr (BS == 16) {
            const int j = l >> 2, r0 = l & 3;
            const int qpm1 = qpr > 0 ? qpr - 1 : qpr;
            const int sdx = m[3 * j], sdy = m[3 * j + 1], sref = m[3 * j + 2];
            const int xs = x + (j & 1) * SB, ys = y + (j >> 1) * SB;
            const bool sfast = (0 <= xs + sdx) && (xs + sdx < a.W - SB) && (0 <= ys + sdy) && (ys + sdy < a.H - SB);
            int spred[2][8], sdq[2][8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                int qv[8];
                fetch_row<8>(pick_ref(a.refs, sref), a.W, a.H, xs + sdx, ys + sdy + r0 + 4 * h, sfast, spred[h]);
                load_row_i16<8>(qt + j * 64 + (r0 + 4 * h) * 8, qv);
                dequant_row<8>(qv, r0 + 4 * h, qpm1, sdq[h]);
            }
            double srd[2][8];
            xform2d_sub<true>(dl, l, sdq, srd);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                int rec[8];
#pragma unroll
                for (int c = 0; c < 8; ++c) rec[c] = spred[h][c] + (int)__builtin_rint(srd[h][c]);
                store_row_u8<8>(a.out_recon, a.W, xs, ys + r0 + 4 * h, rec);
            }
        }
    }
}

struct DecodeChromaArgs {
    const uint8_t* packed;
    const uint32_t* offs;
    RefSet refs[2];        // U, V (P-frames)
    uint8_t* recon[2];
    int nref, Hc, Wc, nbx, nb, frame_type;
    const uint8_t* split;  // the frame's luma symbols (P-frames)
    const int16_t* mv;
    int qp;
    const int32_t* qp_row;
    const int32_t* qp_map;
    int qp_offset;
    int32_t* err;          // this frame's word
};

// A record holds U's and V's block: slot k of the tile is U at [0, 64), V at [64, 128).  Phase 2's
// task t in [0, 128) is U of slot t (t < 64) or V of slot t - 64, 32 tasks a round.
template <typename Reader, int S>
__global__ void __launch_bounds__(256) decode_chroma_kernel(const DecodeChromaArgs a) {
    constexpr int N = 8, P = N + 1, GR = 256 / N, T = kDecodeTile, STRIDE = decode_tile_stride(128);
    static_assert((T * STRIDE) % 8 == 0 && (STRIDE * 2) % 16 == 0, "16-byte tile accesses");
    __shared__ alignas(16) int16_t tile[T * STRIDE];
    __shared__ uint8_t s_bad[T];
    __shared__ double lds[GR * N * P];
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * T;
    const int nv = a.nb - b0 < T ? a.nb - b0 : T;

    for (int i = tid; i < T * STRIDE / 8; i += 256) reinterpret_cast<uint4_alias*>(tile)[i] = make_uint4(0, 0, 0, 0);
    uint8_t* stage = reinterpret_cast<uint8_t*>(lds);   // as in decode_p_kernel
    uint32_t first, o0, o1, sh = 0;
    const bool staged = records_stageable(a.offs, b0, nv, tid, (uint32_t)sizeof(lds), &first, &o0, &o1);
    if (staged) {
        sh = stage_records(a.packed + first, a.offs[b0 + nv] - first, stage, tid);
        __syncthreads();
    }
    if (tid < T) {
        bool bad = true;
        if (tid < nv) {
            auto parse = [&](const uint8_t* p) {
                Reader r(p, o1 - o0, o1 < o0);
                unpack_chroma_record(r, tile + tid * STRIDE, tile + tid * STRIDE + 64);
                return r.bad;
            };
            bad = staged ? parse(stage + sh + (o0 - first)) : parse(a.packed + o0);
            if (bad) __hip_atomic_store(a.err, b0 + tid + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        s_bad[tid] = (uint8_t)bad;
    }
    __syncthreads();

    const int g = tid / N, l = tid % N;
    double* s = lds + g * N * P;
    for (int rd = 0; rd < 2 * T / GR; ++rd) {
        const int pi = rd >= T / GR ? 1 : 0, k = (rd - pi * (T / GR)) * GR + g;   // the plane is uniform in a round
        if (k >= nv || s_bad[k]) continue;   // the whole lane group skips; wave-scope exchange only
        const int b = b0 + k;
        const int bx = b % a.nbx, by = b / a.nbx, X = bx * N, Y = by * N + l;
        // chroma_kernel<false>'s body from here on
        const int base = a.qp_map ? a.qp_map[b] : (a.qp_row ? a.qp_row[by] : a.qp);
        const int qpc = clampi(base + a.qp_offset, 0, 20);
        int pred[N];
        if (a.frame_type == 0) {
#pragma unroll
            for (int c = 0; c < N; ++c) pred[c] = 128;
        } else {
            const int16_t* m = a.mv + (size_t)b * 12;
            const int q0 = a.split[b] ? 2 * (l >> 2) : 0, q1 = a.split[b] ? q0 + 1 : 0;   // Z order
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int16_t* mq = m + 3 * (h ? q1 : q0);
                const int dx = mq[0], dy = mq[1], r = clampi(mq[2], 0, a.nref - 1);
                chroma_pred4<S>(pick_ref(a.refs[pi], r), a.Wc, a.Hc, X + 4 * h, Y, dx, dy, pred + 4 * h);
            }
        }
        int q[N];
        load_row_i16<N>(tile + k * STRIDE + pi * 64 + l * N, q);
        double dq[N], r2[N];
        dequant_row_i<N>(q, l, qpc, dq);
        xform2d_rows<N, true>(s, l, dq, r2);
        int rec[N];
#pragma unroll
        for (int c = 0; c < N; ++c) rec[c] = pred[c] + (int)__builtin_rint(r2[c]);
        store_row_u8<N>(a.recon[pi], a.Wc, X, Y, rec);   // astype(uint8): mod 256
    }
}

// ---- validation shared by the two entry points ---------------------------------------------------
static int check_run(const char* fn, int nframes, int coding, int H, int W, int bs, int qp, int nref_max) {
    if (nframes < 0) {
        set_error("%s: nframes %d", fn, nframes);
        return SO_E_INVALID;
    }
    if (coding != 1 && coding != 2) {
        set_error("%s: coding %d (1 = varint, 2 = bits)", fn, coding);
        return SO_E_INVALID;
    }
    if (H <= 0 || W <= 0 || H % bs || W % bs || (long long)H * W > (1ll << 31)) {
        set_error("%s: frame %dx%d must be a positive multiple of block_size %d (pad with pad_hw)", fn, W, H, bs);
        return SO_E_INVALID;
    }
    if (qp < 0 || qp > 20) {
        set_error("%s: Qp %d outside [0, 20]", fn, qp);
        return SO_E_INVALID;
    }
    if (nref_max < 1 || nref_max > kMaxRef) {
        set_error("%s: nref_max %d outside [1, %d]", fn, nref_max, kMaxRef);
        return SO_E_INVALID;
    }
    return SO_OK;
}

// the last `n` planes of `list` as a RefSet, the unused entries repeating the first (never indexed:
// the kernels check or clamp the index against n)
static RefSet ref_set(const std::vector<const uint8_t*>& list, int n) {
    RefSet rs;
    const size_t first = list.size() - (size_t)n;
    for (int k = 0; k < kMaxRef; ++k) rs.p[k] = list[first + (size_t)(k < n ? k : 0)];
    return rs;
}

}  // namespace so

using namespace so;

extern "C" int so_decode_p_frames(int nframes, int coding, const uint8_t* const* packed, const uint32_t* const* offs,
                                  int H, int W, int bs, int qp, const int32_t* const* qp_row,
                                  const int32_t* const* qp_map, const uint8_t* const* refs0, int nref0, int nref_max,
                                  uint8_t* const* out_split, int16_t* const* out_mv, uint8_t* const* out_recon,
                                  int32_t* err, void* stream) {
    const char* fn = "so_decode_p_frames";
    if (bs != 16 && bs != 8) {
        set_error("%s: block_size %d not built (gfx950 kernels exist for 16 and 8)", fn, bs);
        return SO_E_UNSUPPORTED;
    }
    const int rc = check_run(fn, nframes, coding, H, W, bs, qp, nref_max);
    if (rc != SO_OK) return rc;
    if (nref0 < 1 || nref0 > nref_max) {
        set_error("%s: nref0 %d outside [1, nref_max %d]", fn, nref0, nref_max);
        return SO_E_INVALID;
    }
    if (nframes == 0) return SO_OK;
    SO_NEED(packed, fn); SO_NEED(offs, fn); SO_NEED(refs0, fn); SO_NEED(out_split, fn); SO_NEED(out_mv, fn);
    SO_NEED(out_recon, fn); SO_NEED(err, fn);
    std::vector<const uint8_t*> list;   // refs0, then the reconstructions, oldest first
    for (int k = 0; k < nref0; ++k) {
        SO_NEED(refs0[k], fn);
        list.push_back(refs0[k]);
    }
    for (int i = 0; i < nframes; ++i) {
        SO_NEED(packed[i], fn); SO_NEED(offs[i], fn); SO_NEED(out_split[i], fn); SO_NEED(out_mv[i], fn);
        SO_NEED(out_recon[i], fn);
        // rows move as 16-byte (8-byte at block size 8) vectors, the mv as dwords
        if (((uintptr_t)out_recon[i] & 15) || ((uintptr_t)out_mv[i] & 3)) {
            set_error("%s: out_recon[%d] must be 16-byte and out_mv[%d] 4-byte aligned", fn, i, i);
            return SO_E_INVALID;
        }
        for (const uint8_t* p : list)
            if (p == out_recon[i]) {
                set_error("%s: out_recon[%d] aliases a reference or another reconstruction", fn, i);
                return SO_E_INVALID;
            }
        list.push_back(out_recon[i]);
    }
    const int nb = (W / bs) * (H / bs);
    const dim3 grid((nb + kDecodeTile - 1) / kDecodeTile), blk(256);
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < nframes; ++i) {
        const int nref = nref0 + i < nref_max ? nref0 + i : nref_max;
        std::vector<const uint8_t*> upto(list.begin(), list.begin() + nref0 + i);
        DecodeLumaArgs a{packed[i], offs[i], ref_set(upto, nref), nref, H, W, qp, qp_row ? qp_row[i] : nullptr,
                         qp_map ? qp_map[i] : nullptr, out_split[i], out_mv[i], out_recon[i], err + i};
        if (bs == 16 && coding == 1) hipLaunchKernelGGL((decode_p_kernel<16, VarintReader>), grid, blk, 0, st, a);
        else if (bs == 16) hipLaunchKernelGGL((decode_p_kernel<16, BitReader>), grid, blk, 0, st, a);
        else if (coding == 1) hipLaunchKernelGGL((decode_p_kernel<8, VarintReader>), grid, blk, 0, st, a);
        else hipLaunchKernelGGL((decode_p_kernel<8, BitReader>), grid, blk, 0, st, a);
        const int lrc = check_launch("decode_p_kernel");
        if (lrc != SO_OK) return lrc;
    }
    return SO_OK;
}

// so_decode_chroma_frames and its _ex form: the base name passes mv_frac_bits 1 under its own name
static int decode_chroma_frames(const char* fn, int nframes, int coding, const int32_t* frame_types,
                                const uint8_t* const* packed, const uint32_t* const* offs, int H, int W, int bs,
                                const uint8_t* const* split, const int16_t* const* mv, int qp,
                                const int32_t* const* qp_row, const int32_t* const* qp_map, int qp_offset,
                                const uint8_t* const* refs0_u, const uint8_t* const* refs0_v, int nref0,
                                int nref_max, uint8_t* const* out_recon_u, uint8_t* const* out_recon_v,
                                int32_t* err, int mv_frac_bits, void* stream) {
    if (bs != 16) {
        set_error("%s: block_size %d not built (chroma follows 16x16 luma blocks)", fn, bs);
        return SO_E_UNSUPPORTED;
    }
    SO_TRY(check_mv_frac_bits(fn, mv_frac_bits));
    const int rc = check_run(fn, nframes, coding, H, W, bs, qp, nref_max);
    if (rc != SO_OK) return rc;
    if (qp_offset < -20 || qp_offset > 20) {
        set_error("%s: qp_offset %d outside [-20, 20]", fn, qp_offset);
        return SO_E_INVALID;
    }
    if (nref0 < 0 || nref0 > nref_max) {
        set_error("%s: nref0 %d outside [0, nref_max %d]", fn, nref0, nref_max);
        return SO_E_INVALID;
    }
    if (nframes == 0) return SO_OK;
    SO_NEED(frame_types, fn); SO_NEED(packed, fn); SO_NEED(offs, fn); SO_NEED(out_recon_u, fn);
    SO_NEED(out_recon_v, fn); SO_NEED(err, fn);
    if (nref0 > 0) {
        SO_NEED(refs0_u, fn); SO_NEED(refs0_v, fn);
    }
    std::vector<const uint8_t*> lu, lv, all;   // the current lists, and every plane seen (aliasing)
    for (int k = 0; k < nref0; ++k) {
        SO_NEED(refs0_u[k], fn); SO_NEED(refs0_v[k], fn);
        if (((uintptr_t)refs0_u[k] | (uintptr_t)refs0_v[k]) & 7) {
            set_error("%s: planes must be 8-byte aligned", fn);
            return SO_E_INVALID;
        }
        lu.push_back(refs0_u[k]); lv.push_back(refs0_v[k]);
        all.push_back(refs0_u[k]); all.push_back(refs0_v[k]);
    }
    std::vector<DecodeChromaArgs> args((size_t)nframes);
    for (int i = 0; i < nframes; ++i) {
        const int ft = frame_types[i];
        if (ft != 0 && ft != 1) {
            set_error("%s: frame_types[%d] = %d", fn, i, ft);
            return SO_E_INVALID;
        }
        SO_NEED(packed[i], fn); SO_NEED(offs[i], fn); SO_NEED(out_recon_u[i], fn); SO_NEED(out_recon_v[i], fn);
        if (((uintptr_t)out_recon_u[i] | (uintptr_t)out_recon_v[i]) & 7) {
            set_error("%s: planes must be 8-byte aligned", fn);
            return SO_E_INVALID;
        }
        if (out_recon_u[i] == out_recon_v[i]) {
            set_error("%s: out_recon_u[%d] aliases out_recon_v[%d]", fn, i, i);
            return SO_E_INVALID;
        }
        for (const uint8_t* p : all)
            if (p == out_recon_u[i] || p == out_recon_v[i]) {
                set_error("%s: a reconstruction of frame %d aliases a reference or another reconstruction", fn, i);
                return SO_E_INVALID;
            }
        if (ft == 0) {   // an I-frame clears the list
            lu.clear(); lv.clear();
        } else {
            if (lu.empty()) {
                set_error("%s: frame %d is a P-frame with an empty reference list", fn, i);
                return SO_E_INVALID;
            }
            SO_NEED(split, fn); SO_NEED(mv, fn); SO_NEED(split[i], fn); SO_NEED(mv[i], fn);
        }
        DecodeChromaArgs& a = args[(size_t)i];
        a = DecodeChromaArgs{};
        a.packed = packed[i]; a.offs = offs[i];
        a.nref = ft == 1 ? (int)lu.size() : 1;
        if (ft == 1) {
            a.refs[0] = ref_set(lu, a.nref); a.refs[1] = ref_set(lv, a.nref);
            a.split = split[i]; a.mv = mv[i];
        }
        a.recon[0] = out_recon_u[i]; a.recon[1] = out_recon_v[i];
        a.Hc = H / 2; a.Wc = W / 2; a.nbx = W / 16; a.nb = (W / 16) * (H / 16);
        a.frame_type = ft;
        a.qp = qp; a.qp_row = qp_row ? qp_row[i] : nullptr; a.qp_map = qp_map ? qp_map[i] : nullptr;
        a.qp_offset = qp_offset;
        a.err = err + i;
        // every reconstruction is appended, the oldest dropped at nref_max
        if ((int)lu.size() >= nref_max) {
            lu.erase(lu.begin()); lv.erase(lv.begin());
        }
        lu.push_back(out_recon_u[i]); lv.push_back(out_recon_v[i]);
        all.push_back(out_recon_u[i]); all.push_back(out_recon_v[i]);
    }
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < nframes; ++i) {
        const DecodeChromaArgs& a = args[(size_t)i];
        const dim3 grid((a.nb + kDecodeTile - 1) / kDecodeTile), blk(256);
        if (mv_frac_bits == 2) {
            if (coding == 1) hipLaunchKernelGGL((decode_chroma_kernel<VarintReader, 2>), grid, blk, 0, st, a);
            else hipLaunchKernelGGL((decode_chroma_kernel<BitReader, 2>), grid, blk, 0, st, a);
        } else if (coding == 1) {
            hipLaunchKernelGGL((decode_chroma_kernel<VarintReader, 1>), grid, blk, 0, st, a);
        } else {
            hipLaunchKernelGGL((decode_chroma_kernel<BitReader, 1>), grid, blk, 0, st, a);
        }
        const int lrc = check_launch("decode_chroma_kernel");
        if (lrc != SO_OK) return lrc;
    }
    return SO_OK;
}

extern "C" int so_decode_chroma_frames(int nframes, int coding, const int32_t* frame_types,
                                       const uint8_t* const* packed, const uint32_t* const* offs, int H, int W, int bs,
                                       const uint8_t* const* split, const int16_t* const* mv, int qp,
                                       const int32_t* const* qp_row, const int32_t* const* qp_map, int qp_offset,
                                       const uint8_t* const* refs0_u, const uint8_t* const* refs0_v, int nref0,
                                       int nref_max, uint8_t* const* out_recon_u, uint8_t* const* out_recon_v,
                                       int32_t* err, void* stream) {
    return decode_chroma_frames("so_decode_chroma_frames", nframes, coding, frame_types, packed, offs, H, W, bs, split,
                                mv, qp, qp_row, qp_map, qp_offset, refs0_u, refs0_v, nref0, nref_max, out_recon_u,
                                out_recon_v, err, 1, stream);
}

extern "C" int so_decode_chroma_frames_ex(int nframes, int coding, const int32_t* frame_types,
                                          const uint8_t* const* packed, const uint32_t* const* offs, int H, int W,
                                          int bs, const uint8_t* const* split, const int16_t* const* mv, int qp,
                                          const int32_t* const* qp_row, const int32_t* const* qp_map, int qp_offset,
                                          const uint8_t* const* refs0_u, const uint8_t* const* refs0_v, int nref0,
                                          int nref_max, uint8_t* const* out_recon_u, uint8_t* const* out_recon_v,
                                          int32_t* err, int mv_frac_bits, void* stream) {
    return decode_chroma_frames("so_decode_chroma_frames_ex", nframes, coding, frame_types, packed, offs, H, W, bs,
                                split, mv, qp, qp_row, qp_map, qp_offset, refs0_u, refs0_v, nref0, nref_max,
                                out_recon_u, out_recon_v, err, mv_frac_bits, stream);
}
