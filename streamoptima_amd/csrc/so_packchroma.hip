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
//
// so_pack_chroma_frames_after / _bits_after: the same passes with the write pass alone knowing a
// per-frame base, *f.base, a device word that earlier work on the stream wrote (the luma scan's
// offs[nb]): record b lands at out + base + offs[b], guarded by base + offs[b + 1] <= cap, and the
// write pass, not the scan, stores totals[i] = base + offs[nb].  offs stays relative.  A record may
// thus start at any byte: both store paths write single bytes (out[i] = stage[i], stage_store).
#include "so_packfmt.h"

namespace so {

// ---- varint coding -------------------------------------------------------------------------------
template <bool WRITE>
SO_DEV void pack_chroma_one(const ChromaPackFrame& f, int b, const ChromaDst& d, int lane, const ChromaIn& in,
                            int16_t* __restrict__ sq, uint8_t* __restrict__ stage, const int* idx) {
    const PackRuns<2> r = chroma_runs(in, lane, sq, idx);
    int total;
    const int ex = wave_excl_scan(varint_bytes(r), lane, &total);
    if (!WRITE) {
        if (lane == 0) f.offs[b] = (uint32_t)total;
        return;
    }
    if (in.o1 > d.cap) return;
    // bytes into the wave's LDS stage, then out with consecutive lanes on consecutive bytes
    put_varints(stage + ex, r);
    __builtin_amdgcn_wave_barrier();
    uint8_t* out = d.out + in.o0;
    for (int i = lane; i < total; i += 64) out[i] = stage[i];
}

// ---- bits coding ---------------------------------------------------------------------------------
// The order k is picked over both lists (so_packfmt.h pick_order); it is the record's first two bits.
template <bool WRITE>
SO_DEV void pack_chroma_bits_one(const ChromaPackFrame& f, int b, const ChromaDst& d, int lane,
                                 const ChromaIn& in, int16_t* __restrict__ sq, uint32_t* __restrict__ stage,
                                 const int* idx) {
    const PackRuns<2> r = chroma_runs(in, lane, sq, idx);
    const BitsLane<2> l = bits_lane(r);
    // one scan of the clz sums (16-bit fields: <= 31 * 128), one of count (10 bits: <= 128) | token bits
    // (a token is at most 15 bits, |token| <= 64; their sum stays below 3 * 128 + 4 < 2^12)
    unsigned long long ctot;
    const unsigned long long cex = wave_excl_scan(l.clz_sums(), lane, &ctot);
    int mtot;
    const int mex = wave_excl_scan(__builtin_popcount(r.nzb) | (int)(l.tb << 10), lane, &mtot);
    int best;
    const int k = pick_order(mtot & 0x3FF, ctot, &best);
    const int total_bits = 2 + (mtot >> 10) + best;
    const int nbytes = (total_bits + 7) >> 3;
    if (!WRITE) {
        if (lane == 0) f.offs[b] = (uint32_t)nbytes;
        return;
    }
    if (in.o1 > d.cap) return;
    stage_zero(stage, nbytes, lane);
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) stage_or<kChromaStageWords>(stage, 0, (uint32_t)k << 30);
    const int pos = 2 + (mex >> 10) + order_bits(mex & 0x3FF, cex, k);
    put_codes<kChromaStageWords>(stage, pos, r, l, k);
    __builtin_amdgcn_wave_barrier();
    stage_store(d.out + in.o0, stage, nbytes, lane);
}

// Each wave packs records b = wave, wave + nwaves, ... of its frame (blockIdx.y), the next
// record's inputs loaded before the current one is packed (so_packfmt.h pack_loop).  AFTER (the
// write pass of the _after entries): the frame's base is read once (one uniform load; a null
// pointer is base 0) and, given `totals`, the frame's first thread stores base + offs[nb] there at
// system scope.  The plain entries' instantiations know no base, leave the totals to the scan and
// pass null.
template <bool WRITE, bool BITS, bool AFTER = false>
__global__ void __launch_bounds__(256) pack_chroma_kernel(const ChromaPackArgs a, int nb, unsigned long long cap,
                                                          uint32_t* totals) {
    __shared__ alignas(4) int16_t sq[4][128];
    __shared__ uint32_t stage[WRITE ? 4 : 1][WRITE ? (BITS ? kChromaStageWords : kChromaBound / 4 + 2) : 1];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int w0 = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wv), nw = gridDim.x * 4;
    const ChromaPackFrame f = a.f[blockIdx.y];   // a copy: its pointers stay in SGPRs
    ChromaDst d{f.out, cap};
    if constexpr (WRITE && AFTER) {
        const uint32_t base = f.base ? *f.base : 0u;
        d.out += base;
        d.cap = cap > base ? cap - base : 0ull;
        if (totals && blockIdx.x == 0 && threadIdx.x == 0)
            __hip_atomic_store(totals + blockIdx.y, base + f.offs[nb], __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    // this lane's two scan positions as int16 indices into the staged record (U at 0, V at 64)
    int idx[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int P = 2 * lane + j;
        idx[j] = (P & 64) + c_scan8.t[P & 63];
    }
    pack_loop(
        w0, nw, nb, [&](int b) { return chroma_load<WRITE>(f, b, nb, lane); },
        [&](int b, const ChromaIn& in) {
            if constexpr (BITS)
                pack_chroma_bits_one<WRITE>(f, b, d, lane, in, sq[wv], stage[WRITE ? wv : 0], idx);
            else   // the varint stage is bytes: character accesses alias anything
                pack_chroma_one<WRITE>(f, b, d, lane, in, sq[wv], reinterpret_cast<uint8_t*>(stage[WRITE ? wv : 0]),
                                       idx);
        });
}

// ---- unpack: one thread per record ---------------------------------------------------------------
// Each thread zeroes both 8x8 blocks and parses U's list then V's from its bytes
// [offs[b], offs[b+1]), never reading outside them.  Malformed input (the rules in
// include/streamoptima.h; also offs[b + 1] < offs[b]) sets *err = 1 + the record's index.
template <typename Reader>
__global__ void __launch_bounds__(256) unpack_chroma_kernel(const ChromaUnpackArgs a, int nb, int32_t* __restrict__ err) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    const ChromaUnpackFrame& f = a.f[blockIdx.y];
    const uint32_t o0 = f.offs[b], o1 = f.offs[b + 1];
    int16_t* qu = f.qu + (size_t)b * 64;
    int16_t* qv = f.qv + (size_t)b * 64;
    zero_i16<64>(qu);
    zero_i16<64>(qv);
    Reader r(f.in + o0, o1 - o0, o1 < o0);
    unpack_chroma_record(r, qu, qv);
    if (r.bad) __hip_atomic_store(err, b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// after: the frames carry a base; the totals then come from the write pass (base + offs[nb]), not
// from the scan
int pack_chroma_frames_launch(const ChromaPackFrame* frames, int nframes, int nb, bool bits, bool after,
                              unsigned long long cap, uint32_t* totals, hipStream_t st) {
    return for_frame_chunks<ChromaPackArgs>(
        frames, nframes, "pack chroma kernels", [&](const ChromaPackArgs& a, int n, int f0) {
            PackArgs sa{};   // the scan reads only `offs`
            for (int i = 0; i < n; ++i) sa.f[i].offs = a.f[i].offs;
            const dim3 grid = pack_grid(nb, n);
            uint32_t* const tot = totals ? totals + f0 : nullptr;
            uint32_t* const none = nullptr;
            if (bits) hipLaunchKernelGGL((pack_chroma_kernel<false, true>), grid, dim3(256), 0, st, a, nb, cap, none);
            else hipLaunchKernelGGL((pack_chroma_kernel<false, false>), grid, dim3(256), 0, st, a, nb, cap, none);
            pack_scan_launch(sa, n, nb, after ? none : tot, st);
            if (!after) {
                if (bits) hipLaunchKernelGGL((pack_chroma_kernel<true, true>), grid, dim3(256), 0, st, a, nb, cap, none);
                else hipLaunchKernelGGL((pack_chroma_kernel<true, false>), grid, dim3(256), 0, st, a, nb, cap, none);
            } else if (bits) {
                hipLaunchKernelGGL((pack_chroma_kernel<true, true, true>), grid, dim3(256), 0, st, a, nb, cap, tot);
            } else {
                hipLaunchKernelGGL((pack_chroma_kernel<true, false, true>), grid, dim3(256), 0, st, a, nb, cap, tot);
            }
        });
}

int unpack_chroma_frames_launch(const ChromaUnpackFrame* frames, int nframes, int nb, bool bits, int32_t* err,
                                hipStream_t st) {
    return for_frame_chunks<ChromaUnpackArgs>(
        frames, nframes, "unpack chroma kernels", [&](const ChromaUnpackArgs& a, int n, int) {
            const dim3 grid = unpack_grid(nb, n);
            if (bits) hipLaunchKernelGGL(unpack_chroma_kernel<BitReader>, grid, dim3(256), 0, st, a, nb, err);
            else hipLaunchKernelGGL(unpack_chroma_kernel<VarintReader>, grid, dim3(256), 0, st, a, nb, err);
        });
}

}  // namespace so
