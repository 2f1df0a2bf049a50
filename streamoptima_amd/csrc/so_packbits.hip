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
#include "so_packfmt.h"

namespace so {

// One header code of 1..33 bits at bit position pos.
SO_DEV void stage_put(uint32_t* stage, int pos, uint32_t code, int len) {
    const unsigned long long W = (unsigned long long)code << (64 - (pos & 31) - len);
    stage_or<kBitsStageWords>(stage, pos >> 5, (uint32_t)(W >> 32));
    stage_or<kBitsStageWords>(stage, (pos >> 5) + 1, (uint32_t)W);
}

// One block by one wave; lane l owns the R = nn / 64 consecutive scan positions R*l + j, runs and
// tokens by so_packfmt.h luma_runs.  A position's bits are its run token (se) if it starts a run,
// then its value (se_k) if non-zero; two wave scans of the lanes' sums give the block's totals at
// the four orders -- which pick k -- and every lane's bit offset at the chosen order.  The
// header sits on lanes 0..H-1: split and k (3 bits) on lane 0, the mv values after it.
template <bool WRITE, int bs>
SO_DEV void pack_bits_one_block(const PackFrame& f, int b, unsigned long long cap, int lane, const PackIn& in,
                                int16_t* __restrict__ sq, uint32_t* __restrict__ stage, const LumaIdx<bs>& idx) {
    const int sp = in.sp != 0;
    const int inter = f.frame_type == 1, H = 1 + (sp ? 4 : 1) * (inter ? 3 : 1);
    const auto r = luma_runs<bs>(in, sp, lane, sq, idx);
    const auto l = bits_lane(r);
    // one scan of the clz sums, one of header bits (10 bits: <= 399) | count (10: <= 256) | token bits
    // (12: <= 768); no field's wave sum reaches its width
    const int hb = lane == 0 ? 3 : (lane < H ? ue_len(zz(in.hv)) : 0);
    unsigned long long ctot;
    const unsigned long long cex = wave_excl_scan(l.clz_sums(), lane, &ctot);
    int mtot;
    const int mex = wave_excl_scan(hb | __builtin_popcount(r.nzb) << 10 | (int)(l.tb << 20), lane, &mtot);
    const int cnt = (mtot >> 10) & 0x3FF, hsum = mtot & 0x3FF;
    int best;
    const int k = pick_order(cnt, ctot, &best);
    const int total_bits = hsum + (int)((unsigned)mtot >> 20) + best;
    const int nbytes = (total_bits + 7) >> 3;
    if (!WRITE) {
        if (lane == 0) f.offs[b] = (uint32_t)nbytes;
        return;
    }
    if (in.o1 > cap) return;
    stage_zero(stage, nbytes, lane);
    __builtin_amdgcn_wave_barrier();
    if (lane < H) stage_put(stage, mex & 0x3FF, lane == 0 ? (uint32_t)(sp << 2 | k) : zz(in.hv) + 1u, hb);
    const int pos = hsum + (int)((unsigned)mex >> 20) + order_bits((mex >> 10) & 0x3FF, cex, k);
    put_codes<kBitsStageWords>(stage, pos, r, l, k);
    __builtin_amdgcn_wave_barrier();
    stage_store(f.out + in.o0, stage, nbytes, lane);
}

// Each wave packs blocks b = wave, wave + nwaves, ... of its frame (blockIdx.y), the next
// block's inputs loaded before the current one is packed (so_packfmt.h pack_loop).
template <bool WRITE, int bs>
__global__ void __launch_bounds__(256) pack_bits_block_kernel(const PackArgs a, int nb, unsigned long long cap) {
    __shared__ alignas(16) int16_t sq[4][256];
    __shared__ uint32_t stage[WRITE ? 4 : 1][WRITE ? kBitsStageWords : 1];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int w0 = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wv), nw = gridDim.x * 4;
    const PackFrame f = a.f[blockIdx.y];
    const LumaIdx<bs> idx(lane);
    pack_loop(
        w0, nw, nb, [&](int b) { return pack_load<WRITE, bs>(f, b, nb, lane); },
        [&](int b, const PackIn& in) {
            pack_bits_one_block<WRITE, bs>(f, b, cap, lane, in, sq[wv], stage[WRITE ? wv : 0], idx);
        });
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
    int16_t* q = f.qtc + (size_t)b * (BS * BS);
    zero_i16<BS * BS>(q);
    const int inter = f.frame_type == 1;
    BitReader r(f.in + o0, o1 - o0, o1 < o0);
    unpack_luma_record<BS>(r, inter, f.split + b, f.mv + (size_t)b * (inter ? 12 : 4), q);
    if (r.bad) __hip_atomic_store(err, b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

int unpack_bits_frames_launch(const UnpackFrame* frames, int nframes, int nb, int bs, int32_t* err, hipStream_t st) {
    return for_frame_chunks<UnpackArgs>(
        frames, nframes, "unpack_bits_block_kernel", [&](const UnpackArgs& a, int n, int) {
            const dim3 grid = unpack_grid(nb, n);
            if (bs == 16) hipLaunchKernelGGL(unpack_bits_block_kernel<16>, grid, dim3(256), 0, st, a, nb, err);
            else hipLaunchKernelGGL(unpack_bits_block_kernel<8>, grid, dim3(256), 0, st, a, nb, err);
        });
}

int pack_bits_frames_launch(const PackFrame* frames, int nframes, int nb, int bs, unsigned long long cap,
                            uint32_t* totals, hipStream_t st) {
    return for_frame_chunks<PackArgs>(frames, nframes, "pack bits kernels", [&](const PackArgs& a, int n, int f0) {
        const dim3 grid = pack_grid(nb, n);
        if (bs == 16) hipLaunchKernelGGL((pack_bits_block_kernel<false, 16>), grid, dim3(256), 0, st, a, nb, cap);
        else hipLaunchKernelGGL((pack_bits_block_kernel<false, 8>), grid, dim3(256), 0, st, a, nb, cap);
        pack_scan_launch(a, n, nb, totals ? totals + f0 : nullptr, st);
        if (bs == 16) hipLaunchKernelGGL((pack_bits_block_kernel<true, 16>), grid, dim3(256), 0, st, a, nb, cap);
        else hipLaunchKernelGGL((pack_bits_block_kernel<true, 8>), grid, dim3(256), 0, st, a, nb, cap);
    });
}

}  // namespace so
