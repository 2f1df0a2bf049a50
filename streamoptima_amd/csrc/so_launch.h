// so_launch.h — the launchers so_capi.hip calls that have no unit header of their own, declared
// once and included by the boundary and by every defining unit, so a drifted signature is a
// compile error in the unit that drifted.  (The persistent runs: so_run.h; chroma, colour,
// scaling and the packed stream: so_chroma.h, so_colour.h, so_scale.h, so_packfmt.h.)
#pragma once
#include "so_common.h"

namespace so {

// ---- so_me.hip -------------------------------------------------------------------------------
int me_launch(const uint8_t* cur, const RefSet& refs, int nref, int H, int W, int bs, int sr, int by0, int by1,
              int32_t* out_best, int32_t* out_sub, hipStream_t st);
int me_generic_launch(const uint8_t* cur, const RefSet& refs, const uint8_t* planes, size_t pstride, int nref, int H,
                      int W, int bs, int sr, int by0, int by1, int32_t* out_best, int32_t* out_sub, hipStream_t st);
int me_fme_launch(const uint8_t* cur, const uint8_t* planes, size_t pstride, int nref, int H, int W, int by0, int by1,
                  int32_t* out_best, int32_t* out_sub, hipStream_t st);
int fme_planes_launch(const uint8_t* ref, int H, int W, int wrap, uint8_t* out, size_t pstride, hipStream_t st);
int p_tile_launch(const uint8_t* cur, const RefSet& refs, int H, int W, int by0, int by1, int qp_rd,
                  const int32_t* qp_row, const int32_t* qp_map, int32_t* out_best, uint8_t* out_split,
                  int16_t* out_mv, int16_t* out_qtc, int32_t* out_tokens, int32_t* out_mae, uint8_t* out_recon,
                  int32_t* out_sse, hipStream_t st, bool tokens_only = false, const int16_t* prev_mv = nullptr);
int stripe_halo_push_launch(const uint8_t* plane, int W, int by0, int by1, uint8_t* up, uint8_t* dn,
                            uint32_t* up_flags, uint32_t* dn_flags, int gf, uint32_t epoch, hipStream_t st);
int frame_push_launch(const uint8_t* plane, int H, int W, uint8_t* dst, uint32_t* flags, uint32_t epoch,
                      hipStream_t st);

// ---- so_fastme.hip ---------------------------------------------------------------------------
int me_fastpred_launch(const uint8_t* cur, const uint8_t* const* ptrs, int nptr, int nref, int H, int W, int bs,
                       int fme, int by0, int by1, int serial, int32_t* out_best, int32_t* out_sub, int32_t* seg_ws,
                       hipStream_t st);
constexpr size_t kFastSegWords = 2 * 4096 * 6;   // the speculated chain's segment records

// ---- so_tq.hip -------------------------------------------------------------------------------
int inter_tq_launch(const uint8_t* cur, const RefSet& refs, const uint8_t* planes, size_t pstride, int H, int W,
                    int bs, int by0, int by1, const int32_t* best, const int32_t* sub, int qp_rd,
                    const int32_t* qp_row, const int32_t* qp_map, int vbs, double lam, uint8_t* out_split,
                    int16_t* out_mv, int16_t* out_qtc, int32_t* out_tokens, int32_t* out_mae, uint8_t* out_recon,
                    int32_t* out_sse, hipStream_t st);
int inter_tq_2pass_launch(const uint8_t* cur, const RefSet& refs, int H, int W, const int32_t* best, const int32_t* t1,
                          int qp_rd, const int32_t* qp_row, const int32_t* roi, int qp_lo, int qp_hi,
                          int32_t* out_qpmap, uint8_t* out_split, int16_t* out_mv, int16_t* out_qtc,
                          int32_t* out_tokens, int32_t* out_mae, uint8_t* out_recon, int32_t* out_sse,
                          hipStream_t st);
int inter_recon_launch(const RefSet& refs, const uint8_t* planes, size_t pstride, int H, int W, int bs, int qp,
                       const int32_t* qp_row, const int32_t* qp_map, const uint8_t* split, const int16_t* mv,
                       const int16_t* qtc, uint8_t* out_recon, hipStream_t st);

// ---- so_intra.hip ----------------------------------------------------------------------------
int intra_encode_launch(const uint8_t* cur, int H, int W, int bs, int sr, int by0, int by1, int qp_rd,
                        const int32_t* qp_row, const int32_t* qp_map, int vbs, double lam, uint8_t* out_split,
                        int16_t* out_mv, int16_t* out_qtc, int32_t* out_tokens, int32_t* out_mae, uint8_t* out_recon,
                        int32_t* out_sse, uint8_t* idres, hipStream_t st);
int intra_recon_launch(int H, int W, int bs, int sr, int qp, const int32_t* qp_row, const int32_t* qp_map,
                       const uint8_t* split, const int16_t* mv, const int16_t* qtc, uint8_t* out_recon, uint8_t* idres,
                       hipStream_t st);

// ---- so_ssim.hip -----------------------------------------------------------------------------
size_t ssim_tiles(int H, int W, int win);
int ssim_launch(const uint8_t* const* a, const uint8_t* const* b, int nframes, int H, int W, size_t pitch_a,
                size_t pitch_b, int win, double* out, double* ws, hipStream_t st);

// ---- so_reduce.hip ---------------------------------------------------------------------------
constexpr int kSumMax = 64;   // arrays per sum_rows_launch (kernel-argument table)
// int64 sum of `len` int32 values of each of rows[0 .. n), n <= kSumMax, into out[0 .. n)
int sum_rows_launch(const int32_t* const* rows, int n, int len, int64_t* out, hipStream_t st);
// *out += the sum of squared differences of n bytes (a, b 16-byte aligned)
int sse_launch(const uint8_t* a, const uint8_t* b, int64_t n, uint64_t* out, hipStream_t st);
// the per-block QPs of block rows [by0, by1), nbx blocks each (qp_map_kernel's rule)
int qp_map_launch(const int32_t* tokens, int nbx, int by0, int by1, int qp_rd, const int32_t* qp_row,
                  const int32_t* roi, int qp_lo, int qp_hi, int32_t* out, hipStream_t st);

}  // namespace so
