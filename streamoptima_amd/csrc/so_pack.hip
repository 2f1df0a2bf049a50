// so_pack.hip — the symbols of a frame as one packed byte stream on the device, so a host
// caller downloads the bitstream's content (symbols out of the timed region)
// instead of the dense int16 QTC planes (2 B per pixel).
//
// The content is exactly what the reference's two text lines carry per frame: the block's
// split flag and motion vectors (differential_encoder_frame, Encoder.py:1419-1520, before its
// differencing) and the RLE token list of every (sub-)block (entropy_encoder_block,
// :1086-1131, which entropy_encoder_frame joins, :1522-1542).  Per block, in raster order:
//     split | mv values | tokens of each (sub-)block
// every number a zigzag LEB128 varint (zz(v) = 2v for v >= 0, -2v-1 for v < 0; 7 bits per
// byte, high bit = more).  mv values: inter (dx, dy, ref) once, or 4x in Z order when split;
// intra dx once or 4x.  A (sub-)block's token list is self-delimiting: "-L" and L values
// cover L coefficients, "Z" (> 0) covers Z zeros, "0" ends the block (the trailing zero
// run), and a list ends after n*n coefficients otherwise.  bitstream.unpack_frame restores
// the lists and MVs on the host.
//
// What a decoder (unpack_block_kernel, bitstream.unpack_frame) takes as malformed -- the
// specification is tests/packref.py unpack_block_strict:
//   * a varint is 1-5 bytes, decoded with no bits dropped and then un-zigzagged; a sixth
//     continuation byte, or a varint running off the end of the block's bytes, is malformed;
//   * split is 0, or 1 at block size 16; anything else is malformed;
//   * every mv value and every coefficient lies in [-32768, 32767], else malformed;
//   * a token -L needs 1 <= L <= nn - k, a token Z > 0 needs Z <= nn - k (k: the coefficients
//     of the (sub-)block covered so far, nn its size); a token 0 ends the (sub-)block, and a
//     list also ends at k == nn;
//   * all the block's bytes must be consumed.
// Accepted though not canonical (unambiguous, never written by so_pack_frames):
//   * an over-long varint of up to 5 bytes whose value fits;
//   * a 0 value inside a -L list;
//   * a zero run that reaches exactly nn written as Z instead of 0.
// mv entries past the first of an unsplit block are 0 on output.
//
// Two passes over the frame (one wave per block): byte counts, an exclusive scan per frame
// (one workgroup), then the bytes at their offsets.  HBM-bound: the dense QTC read once per
// pass (2 B/px) against the packed stream written once.  A block whose bytes would pass the
// caller's capacity is not written (the caller compares offs[nb] with it).
#include "so_packfmt.h"

namespace so {

// One block by one wave; lane l owns the R = nn / 64 consecutive scan positions P = R*l + j.
// The block goes through LDS into scan order and into runs (so_packfmt.h luma_runs: a segment is
// 256 positions unsplit, 4 x 64 split, 64 for 8x8).  A position's bytes are its run token if it
// starts a run, then its value if non-zero.  The header (split, then the mv values) sits on lanes
// 0..H-1; one wave prefix sum of (header bytes << 16 | token bytes) places both.  WRITE = false
// stores the byte count.
template <bool WRITE, int bs>
SO_DEV void pack_one_block(const PackFrame& f, int b, unsigned long long cap, int lane, const PackIn& in,
                           int16_t* __restrict__ sq, uint8_t* __restrict__ stage, const LumaIdx<bs>& idx) {
    const int sp = in.sp;
    const int inter = f.frame_type == 1, H = 1 + (sp ? 4 : 1) * (inter ? 3 : 1);
    const auto r = luma_runs<bs>(in, sp, lane, sq, idx);
    const int nbytes = varint_bytes(r);
    const int hv = lane == 0 ? sp : in.hv;
    const int hb = lane < H ? vlen(zz(hv)) : 0;
    int tot;
    const int ex = wave_excl_scan((hb << 16) | nbytes, lane, &tot);
    const int hsum = tot >> 16, total = hsum + (tot & 0xFFFF);
    if (!WRITE) {
        if (lane == 0) f.offs[b] = (uint32_t)total;
        return;
    }
    if (in.o1 > cap) return;
    // bytes into the wave's LDS stage, then out with consecutive lanes on consecutive bytes
    if (lane < H) put_varint(stage + (ex >> 16), hv);
    put_varints(stage + hsum + (ex & 0xFFFF), r);
    __builtin_amdgcn_wave_barrier();
    uint8_t* out = f.out + in.o0;
    for (int i = lane; i < total; i += 64) out[i] = stage[i];
}

// Each wave packs blocks b = wave, wave + nwaves, ... of its frame (blockIdx.y), loading the
// next block's inputs before packing the current one (so_packfmt.h pack_loop).
template <bool WRITE, int bs>
__global__ void __launch_bounds__(256) pack_block_kernel(const PackArgs a, int nb, unsigned long long cap) {
    __shared__ alignas(16) int16_t sq[4][256];
    __shared__ uint8_t stage[WRITE ? 4 : 1][WRITE ? kPackStage : 1];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int w0 = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + wv), nw = gridDim.x * 4;
    const PackFrame f = a.f[blockIdx.y];   // a copy: its pointers stay in SGPRs
    const LumaIdx<bs> idx(lane);
    pack_loop(
        w0, nw, nb, [&](int b) { return pack_load<WRITE, bs>(f, b, nb, lane); },
        [&](int b, const PackIn& in) {
            pack_one_block<WRITE, bs>(f, b, cap, lane, in, sq[wv], stage[WRITE ? wv : 0], idx);
        });
}

// exclusive scan of offs[0..nb) in place, total in offs[nb] (and in totals[blockIdx.x] when
// given -- host-mapped memory: a system-scope store): one 1024-thread workgroup per frame,
// the counts in tiles of 8192 -- loaded and stored coalesced (consecutive lanes on
// consecutive counts) through LDS, scanned 8 consecutive counts per thread (one wave scan of
// the threads' sums, one of the 16 wave totals), the tile's total carried into the next.
// Round 6: replaces a chunk-per-thread scan whose lanes read 128 B apart (52 us for a 2-frame
// P-run chunk, on the host-stream region's critical path at its end).
constexpr int kScanTile = 8192;
__global__ void __launch_bounds__(1024) pack_scan_kernel(const PackArgs a, int nb, uint32_t* totals) {
    __shared__ alignas(16) uint32_t tile[kScanTile];
    __shared__ uint32_t wtot[16];
    uint32_t* offs = a.f[blockIdx.x].offs;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    uint32_t carry = 0;
    for (int base = 0; base < nb; base += kScanTile) {
        const int n = nb - base < kScanTile ? nb - base : kScanTile;
#pragma unroll
        for (int i = 0; i < kScanTile / 1024; ++i) {
            const int e = t + 1024 * i;
            tile[e] = e < n ? offs[base + e] : 0u;
        }
        __syncthreads();
        const uint4 lo = reinterpret_cast<const uint4*>(tile)[2 * t];
        const uint4 hi = reinterpret_cast<const uint4*>(tile)[2 * t + 1];
        const uint32_t s = lo.x + lo.y + lo.z + lo.w + hi.x + hi.y + hi.z + hi.w;
        int wsum;
        const uint32_t wex = (uint32_t)wave_excl_scan((int)s, lane, &wsum);
        if (lane == 0) wtot[wv] = (uint32_t)wsum;
        __syncthreads();
        uint32_t before = carry, all = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const uint32_t v = wtot[w];
            before += w < wv ? v : 0u;
            all += v;
        }
        uint32_t r = before + wex;
        uint4 o0, o1;
        o0.x = r; r += lo.x; o0.y = r; r += lo.y; o0.z = r; r += lo.z; o0.w = r; r += lo.w;
        o1.x = r; r += hi.x; o1.y = r; r += hi.y; o1.z = r; r += hi.z; o1.w = r;
        reinterpret_cast<uint4*>(tile)[2 * t] = o0;
        reinterpret_cast<uint4*>(tile)[2 * t + 1] = o1;
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kScanTile / 1024; ++i) {
            const int e = t + 1024 * i;
            if (e < n) offs[base + e] = tile[e];
        }
        carry += all;
        __syncthreads();   // the tile and wave totals are reused
    }
    if (t == 0) {
        offs[nb] = carry;
        if (totals) __hip_atomic_store(totals + blockIdx.x, carry, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// the scan, also for the other codings of the stream (so_packbits.hip, so_packchroma.hip)
void pack_scan_launch(const PackArgs& a, int nframes, int nb, uint32_t* totals, hipStream_t st) {
    hipLaunchKernelGGL(pack_scan_kernel, dim3(nframes), dim3(1024), 0, st, a, nb, totals);
}

// ---- unpack (so_unpack_frames): the packed stream back to split / mv / qtc ----------------
// One thread per block parses its bytes [offs[b], offs[b+1]) sequentially: the header, then
// each (sub-)block's tokens -- "-L" and L values, "Z" zeros, "0" the trailing zeros -- into
// the zeroed block in scan order.  Malformed input (the rules at the top of this file; also
// offs[b + 1] < offs[b]) sets *err = 1 + that block's index.  Offsets that point outside the
// stream's buffer are the caller's to exclude (packedfile.read does).
template <int BS>
__global__ void __launch_bounds__(256) unpack_block_kernel(const UnpackArgs a, int nb, int32_t* __restrict__ err) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nb) return;
    const UnpackFrame& f = a.f[blockIdx.y];
    const uint32_t o0 = f.offs[b], o1 = f.offs[b + 1];
    int16_t* q = f.qtc + (size_t)b * (BS * BS);
    zero_i16<BS * BS>(q);
    const int inter = f.frame_type == 1;
    VarintReader r(f.in + o0, o1 - o0, o1 < o0);
    unpack_luma_record<BS>(r, inter, f.split + b, f.mv + (size_t)b * (inter ? 12 : 4), q);
    if (r.bad) __hip_atomic_store(err, b + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

int unpack_frames_launch(const UnpackFrame* frames, int nframes, int nb, int bs, int32_t* err, hipStream_t st) {
    return for_frame_chunks<UnpackArgs>(frames, nframes, "unpack_block_kernel", [&](const UnpackArgs& a, int n, int) {
        if (bs == 16) hipLaunchKernelGGL(unpack_block_kernel<16>, unpack_grid(nb, n), dim3(256), 0, st, a, nb, err);
        else hipLaunchKernelGGL(unpack_block_kernel<8>, unpack_grid(nb, n), dim3(256), 0, st, a, nb, err);
    });
}

int pack_frames_launch(const PackFrame* frames, int nframes, int nb, int bs, unsigned long long cap, uint32_t* totals,
                       hipStream_t st) {
    return for_frame_chunks<PackArgs>(frames, nframes, "pack kernels", [&](const PackArgs& a, int n, int f0) {
        const dim3 grid = pack_grid(nb, n);
        if (bs == 16) hipLaunchKernelGGL((pack_block_kernel<false, 16>), grid, dim3(256), 0, st, a, nb, cap);
        else hipLaunchKernelGGL((pack_block_kernel<false, 8>), grid, dim3(256), 0, st, a, nb, cap);
        pack_scan_launch(a, n, nb, totals ? totals + f0 : nullptr, st);
        if (bs == 16) hipLaunchKernelGGL((pack_block_kernel<true, 16>), grid, dim3(256), 0, st, a, nb, cap);
        else hipLaunchKernelGGL((pack_block_kernel<true, 8>), grid, dim3(256), 0, st, a, nb, cap);
    });
}

}  // namespace so
