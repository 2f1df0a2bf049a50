/*
 * streamoptima.h — C-ABI of libstreamoptima_hip.so, the MI355X (gfx950) per-block
 * encode path of a StreamOptima-compatible block video encoder.
 *
 * The reference (Suyashagarw/StreamOptima) is pure Python and has no FFI: its drop-in
 * boundary is the Y_Video_codec / decoder Python API.  Each entry point below replaces
 * the reference functions cited next to it; the Python facade in streamoptima_amd/
 * (Encoder.py, decoder.py) keeps the reference's method names and calls these through
 * ctypes (see INTEGRATION.md for the binding).
 *
 * Conventions
 *  - Frames are uint8, row-major, pitch == width, resident in device (HBM) memory; every
 *    frame buffer must be readable for 16 bytes past its last pixel.
 *  - H and W are the encoded frame size and must be multiples of bs (the reference's
 *    pad_hw, Encoder.py:140-155, is applied by the caller; see DESIGN.md for 1080p).
 *  - Blocks are numbered in raster order, nb = (H/bs) * (W/bs).
 *  - All pointers except `refs` (a HOST array of device pointers) are device pointers
 *    allocated by the caller (PyTorch tensors in the facade).  The library never
 *    allocates device memory; all calls are asynchronous on `stream` (a hipStream_t).
 *  - Return 0 (SO_OK) on success, SO_E_* (< 0) for bad arguments, or a positive
 *    hipError_t.  so_last_error() returns a thread-local message for the last failure.
 *  - No C++ exception crosses this boundary.
 *
 * Canonical output layout (shared with tests/golden and the CPU oracle):
 *   split[nb]            uint8   1 = variable-block-size split (4 sub-blocks, Z order)
 *   inter mv[nb][4][3]   int16   (dx, dy, ref) per sub-block; unsplit => entry 0 only
 *   intra mv[nb][4]      int16   dx per sub-block (-1 for blocks at x == 0)
 *   qtc[nb][bs*bs]       int16   quantised coefficients; split => 4 x (bs/2)^2 Z order
 *   tokens[nb]           int32   len(entropy_encoder_block(...)) summed over sub-blocks
 *   mae_num[nb]          int32   block MAE * bs*bs (an integer SAD), -1 = inf
 */
#ifndef STREAMOPTIMA_H
#define STREAMOPTIMA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SO_OK 0
#define SO_E_INVALID (-1)      /* bad argument (message in so_last_error) */
#define SO_E_UNSUPPORTED (-2)  /* valid in the reference but not built for gfx950 yet */
#define SO_MAX_REF 4           /* nRefFrames supported by the kernels */
#define SO_ABI_VERSION 1

/* library identification / diagnostics */
int so_abi_version(void);
const char* so_last_error(void);

/*
 * Full-search integer-pel motion estimation for every bs x bs block of `cur`.
 * Replaces find_best_match + compute_mae + is_better_mv (Encoder.py:678-717, 314-315,
 * 771-773) as called from inter_prediction (Encoder.py:505-562).
 *   refs[nref]   host array of device pointers to H x W reference frames
 *   sr           search range (dx, dy in [-sr, sr]); candidate valid iff
 *                0 <= x+dx < W-bs and 0 <= y+dy < H-bs (strict, like the reference)
 *   out_best     int32 [nb][4]: (dx, dy, ref, sad); sad = -1 if no candidate is valid
 *   out_sub      optional int32 [nb][4][4]: the same for the four (bs/2) sub-blocks of
 *                every block (VBSEnable, Encoder.py:512-544); NULL to skip
 */
int so_me_full_search(const uint8_t* cur, const uint8_t* const* refs, int nref, int H,
                      int W, int bs, int sr, int32_t* out_best, int32_t* out_sub,
                      void* stream);

/*
 * Residual, DCT, quantisation, token count, VBS rate-distortion split decision,
 * dequantisation, IDCT and reconstruction for every block of a P-frame.
 * Replaces calculate_inter_frame_residual (Encoder.py:432-460), apply_2d_dct (:779),
 * quantize_TC (:787), entropy_encoder_block's length (:1086), calculate_RD_cost (:1133)
 * and the split decision (:564-578), the per-block loop of complete_inter_flow
 * (:1665-1697) and reconstruct_frame / reconstruct_block (:824-932).
 *   best/sub     outputs of so_me_full_search (sub may be NULL when vbs == 0)
 *   qp_rd        QP in effect during inter_prediction (used for the RD decision)
 *   qp_row       device int32 [H/bs] per-row QP (rate control), or NULL => qp_rd
 *   lam          lambda of calculate_RD_cost
 *   out_recon    H x W uint8 reconstruction (may not alias any ref)
 *   out_sse      optional int32 [nb]: per-block sum of (cur - recon)^2, for the PSNR of
 *                calculate_metrics (Encoder.py:934) without a separate frame pass; NULL to skip
 */
int so_inter_tq_recon(const uint8_t* cur, const uint8_t* const* refs, int nref, int H,
                      int W, int bs, const int32_t* best, const int32_t* sub, int qp_rd,
                      const int32_t* qp_row, int vbs, double lam, uint8_t* out_split,
                      int16_t* out_mv, int16_t* out_qtc, int32_t* out_tokens,
                      int32_t* out_mae_num, uint8_t* out_recon, int32_t* out_sse, void* stream);

/* int32 elements of scratch so_encode_p_frame needs: nb*4 (+ nb*16 with vbs), + 49,152 for the
 * segment records of the speculated fast-ME predictor chain (so_encode_p_rows_ex) */
size_t so_p_frame_scratch_elems(int H, int W, int bs, int vbs);

/*
 * One P-frame of complete_inter_flow (Encoder.py:1644-1709): so_me_full_search then
 * so_inter_tq_recon, with `scratch` (device int32, so_p_frame_scratch_elems) between.
 */
int so_encode_p_frame(const uint8_t* cur, const uint8_t* const* refs, int nref, int H,
                      int W, int bs, int sr, int qp_rd, const int32_t* qp_row, int vbs,
                      double lam, uint8_t* out_split, int16_t* out_mv, int16_t* out_qtc,
                      int32_t* out_tokens, int32_t* out_mae_num, uint8_t* out_recon,
                      int32_t* out_sse, int32_t* scratch, void* stream);

/*
 * Stripe variant of so_encode_p_frame for multi-GPU sharding: encodes only
 * the block rows [by0, by1) of the frame.  cur, refs and out_recon are still the FULL
 * H x W planes (the search reads the whole reference; only the stripe's pixel rows of
 * out_recon are written).  Symbol outputs (split, mv, qtc, tokens, mae_num, sse) and the
 * scratch are STRIPE-LOCAL: block (bx, by) is record (by - by0) * (W/bs) + bx.  qp_row is
 * the full-frame [H/bs] array.  Concatenating the stripes of by0 = 0 .. H/bs in order
 * reproduces so_encode_p_frame exactly.  so_p_frame_scratch_elems(H, W, ...) suffices.
 */
int so_encode_p_rows(const uint8_t* cur, const uint8_t* const* refs, int nref, int H, int W,
                     int bs, int sr, int by0, int by1, int qp_rd, const int32_t* qp_row,
                     int vbs, double lam, uint8_t* out_split, int16_t* out_mv,
                     int16_t* out_qtc, int32_t* out_tokens, int32_t* out_mae_num,
                     uint8_t* out_recon, int32_t* out_sse, int32_t* scratch, void* stream);

/*
 * Process-wide options of the library (explicit calls, not environment variables; the A/B
 * knobs of the development tools exist only in -DSO_AB builds).  Set them before enqueueing
 * the work they affect; they are read on the host when a call enqueues its launches.
 *   SO_OPT_RUN_2PASS_FUSED   so_encode_p_run_2pass runs both passes of every frame in ONE
 *                            persistent launch (1, default: measured faster, DESIGN.md section 5;
 *                            frames of three or more 32-row tile rows) or as the per-frame kernel
 *                            sequence (0)
 *   SO_OPT_FASTME_SERIAL     fast_me under ParallelMode 0: the one-wavefront serial walk of the
 *                            predictor chain (1) instead of the speculated segments (0, default)
 *   SO_OPT_FASTME_SEGMENT    blocks per speculated segment (default 32, >= 1)
 *   SO_OPT_FASTME_WARMUP     blocks a segment's guess runs ahead of it (default 32, >= 0)
 *   SO_OPT_COUNT_SAD_OPS     the one-GPU persistent runs (so_encode_p_run / _runs) count their
 *                            searches' SAD byte operations into workspace words 66..67 (1; default
 *                            0: a separate test-hook kernel instantiation runs while it is set,
 *                            so the product kernels carry no counting code)
 *   SO_OPT_RUN_ZERO_SKIP     the one-GPU plain run (so_encode_p_run / _runs, VBS off) launches the
 *                            instantiation whose waves skip the IDCT when all their blocks
 *                            quantised to zero (1; exact either way: an all-zero block's inverse
 *                            is zero).  Faster where most blocks are zero (flat content), a
 *                            little slower elsewhere; default 0.  The Python engine sets it per
 *                            run from the previous run's share of all-zero blocks.
 *   SO_OPT_RUN_TALL_TILES    the tile of the one-GPU plain run (so_encode_p_run / _runs, VBS off, no
 *                            test hook set): 128 x 48 px (24 blocks: six of the workgroup's eight
 *                            waves transform, and a tile's window halo is smaller) or the
 *                            128 x 32 px of every other run.  -1 (default, "unset"): 48 rows when
 *                            the frames in flight offer at least as many 48-row tiles as the
 *                            grid has resident workgroups (4K: yes; 1080p: no, it stays on the
 *                            32-row tile, whose tile step is shorter); 0: never; 1: always.
 *                            Exact either way.  so_p_run_tile_rows reports the choice.
 * so_set_option returns SO_E_INVALID for an unknown option or a value out of range.
 */
#define SO_OPT_RUN_2PASS_FUSED 1
#define SO_OPT_FASTME_SERIAL 2
#define SO_OPT_FASTME_SEGMENT 3
#define SO_OPT_FASTME_WARMUP 4
#define SO_OPT_COUNT_SAD_OPS 5
/* TEST ONLY -- never set it around work whose output is used.  SO_OPT_TEST_LOSE_FLAG = k > 0:
 * the next one-GPU run never sets the done flag of its task k - 1, so the tiles that wait on it
 * time out (50 ms each) and record themselves, and that run's symbols are WRONG (the wait
 * diagnostics' test, tests/test_gpu_waits.py).  It is read when a run is enqueued, so a run
 * captured into a graph would stay broken on every replay: a one-GPU run enqueued on a
 * capturing stream while it is set fails with SO_E_INVALID.  Both this option and
 * SO_OPT_COUNT_SAD_OPS select a separate test-hook instantiation of the one-GPU run kernel; the
 * product kernels carry neither hook. */
#define SO_OPT_TEST_LOSE_FLAG 6
#define SO_OPT_RUN_ZERO_SKIP 7
#define SO_OPT_RUN_TALL_TILES 8
int so_set_option(int option, int value);
int so_get_option(int option);

/*
 * A run of consecutive P-frames (the GOP loop's P-frames between two I-frames,
 * Encoder.py:1839-1867 with nRefFrames 1): frame i predicts from frame i-1's
 * reconstruction (out_recon[i-1]), frame 0 from ref0.  Output is identical to
 * so_encode_p_frame called per frame.  Covers bs 16 / sr 16 with W a multiple of 128 (whole
 * cache lines per tile row); anything else is SO_E_UNSUPPORTED (call so_encode_p_frame per
 * frame).  vbs / lam: VBSEnable and calculate_RD_cost's lambda (Encoder.py:512-578,
 * :1133-1158) -- the block and sub-block search and the RD split run inside the launch
 * (vbs 0: lam unused).
 *
 * One persistent launch per 32 frames: workgroups take (frame, tile) tasks in frame-major
 * raster order, and a tile of frame i starts once the 3x3 tiles of frame i-1 its +-16 px
 * window reads are done (device-scope flags in `workspace`; reconstructions are
 * stored write-through), so consecutive frames overlap on the device with no host
 * round trip.  curs / out_* are host arrays of nframes device pointers; out_sse may be
 * NULL.  workspace: caller-owned uint32 [so_p_run_workspace_elems(H, W)], ZEROED ONCE by the
 * caller before its first use and then only passed back: each launch leaves its counters
 * at 0 and its epoch in the workspace (done flags are compared with the launch's epoch, so
 * nothing is reset between launches).  One workspace serves one stream at a time.  Word 32
 * (SO_P_RUN_TIMEOUT_WORD) is the timeout count: the caller reads it after the run (or after a
 * whole GOP of runs) and clears it (with words 33..35 and the record at 96..127).
 * Nonzero means a dependency wait polled for 50 ms (2 s for another rank's flags; intervals in
 * which the waiting wave was descheduled are not counted) and the run's symbols may be wrong;
 * the facade raises with the record of the first such wait (Engine.check_run).  Consumers poll
 * the flags and then take an agent-scope acquire before reading the reference rows.
 */
#define SO_P_RUN_TIMEOUT_WORD 32
/* Word 64: the number of blocks whose exact SEA search took the dense fallback (more than 192
 * candidates survived the 4x4-cell bound: flat or noise-like content), summed over launches
 * like the timeout count until the caller clears it (a content statistic, not an error). */
#define SO_P_RUN_FALLBACK_WORD 64
/* Words 66..67 (uint64, little endian; with SO_OPT_COUNT_SAD_OPS set): SAD byte operations the
 * searches executed (every
 * v_sad_u8 / v_sad_hi_u8 lane instruction counts its 4 bytes: byte sums, bounds, survivor and
 * dense SADs), summed like word 64.  The dense-equivalent count of the reference's full scan
 * (Encoder.py:688-715) is (valid candidates) x 256 per P-frame; this is what ran. */
#define SO_P_RUN_SAD_OPS_WORD 66
/* Words 68, 69: wavefronts (four blocks each) of the plain one-GPU run whose fast forward /
 * inverse transform could not certify a rounding and re-ran the pocketfft sequence, summed like
 * word 64 (a content statistic: exact ties of the rational coefficients, low QPs). */
#define SO_P_RUN_TQ_FALLBACK_WORD 68
/* Wait health, accumulated like the timeout count ("Waits"):
 * word 33: waits whose relaxed flag polls kept missing a flag for 1 ms of polling that an
 *          atomic read then found set (the wait completes with atomic reads; not an error);
 * word 34: poll intervals longer than 1 ms (the waiting wave was descheduled: compute-queue
 *          preemption), excluded from the wait's bound (not an error). */
#define SO_P_RUN_STALE_WORD 33
#define SO_P_RUN_GAP_WORD 34
/* Words 96..127: the record of the first wait that timed out since word 35 was cleared (all
 * zero: none).  [0] magic 0x534F0001, [1] task, [2] frame (in the launch), [3] dep frame,
 * [4] tile, [5] the launch's epoch (local flags), [6] the GOP epoch (another rank's flags),
 * [7] mode | vbs << 4 | pass << 8 | escalated << 12, [8] lanes waited on (bit l), [9] lanes
 * polling another rank's flags, [10] polling time (100 MHz ticks, gaps excluded), [11] wall
 * ticks, [12] longest poll gap, [13] polls, [14] ticks from the timeout until every awaited
 * flag read set (0xFFFFFFFF: not within 50 ms more), [15] HW_ID, [16] XCC_ID, [17] blockIdx.x,
 * [18] gridDim.x, [19] lanes whose flag an atomic read found set at the timeout,
 * [20 + l] the last value lane l read (l < 12). */
#define SO_P_RUN_DIAG_WORD 96
#define SO_P_RUN_DIAG_MAGIC 0x534F0001u
size_t so_p_run_workspace_elems(int H, int W);
/* The workgroups the persistent run kernel keeps resident on the calling thread's current
 * device (CUs x workgroups per CU; vbs: the VBSEnable kernel): the grid of an uncapped launch.
 * Several ranks' runs sharing ONE device (in-process tests, time-shared rehearsals) must keep
 * the sum of their grids (max_wg of the stripe / frame-pipeline entry points) within it: a
 * launch that cannot become resident would leave the others waiting on its tasks (DESIGN.md
 * section 6, "Forward progress").  SO_E_INVALID if the device query fails. */
int so_p_run_resident_workgroups(int vbs);
/* The same for ONE run kind: mode 0 the one-GPU run (so_encode_p_run / _runs), 1 the stripe
 * run, 2 the frame pipeline, 3 the fused two-pass run, 4 the two-pass frame pipeline (vbs: modes
 * 0 and 2).  so_p_run_resident_workgroups(vbs) is the smallest of these, so a claim sized by it
 * fits whichever kernel a rank launches.  SO_E_INVALID for another mode or a failed query. */
int so_p_run_mode_resident_workgroups(int mode, int vbs);
/* Block rows per tile, 2 or 3, that a one-GPU plain run of H x W frames with `conc` independent
 * runs interleaved (so_encode_p_run: 1) would use on the calling thread's current device under
 * the current SO_OPT_RUN_TALL_TILES.  SO_E_INVALID for a bad shape or a failed device query. */
int so_p_run_tile_rows(int H, int W, int conc);
int so_encode_p_run(const uint8_t* const* curs, int nframes, const uint8_t* ref0, int H, int W,
                    int bs, int sr, int qp_rd, const int32_t* qp_row, int vbs, double lam,
                    uint8_t* const* out_split,
                    int16_t* const* out_mv, int16_t* const* out_qtc, int32_t* const* out_tokens,
                    int32_t* const* out_mae_num, uint8_t* const* out_recon, int32_t* const* out_sse,
                    uint32_t* workspace, void* stream);

/*
 * A run of P-frames with two-pass rate control (build extension, RCFlag 3)
 * in one call: per frame, pass 1 at the rate-control row QP (qp_row, or qp_rd)
 * gives each block's token count t, the per-block QP is clamp(row QP + delta + roi, qp_lo,
 * qp_hi) with delta = [t n >= 2m] + [t n >= 4m] - [2 t n < m] - [4 t n < m] (m = the block
 * row's pass-1 token sum over its n blocks; so_qp_map's rule), and pass 2 re-runs the
 * transforms at those QPs on pass 1's motion vectors.  Identical to the per-frame sequence
 * so_encode_p_rows_ex (pass 1) + so_qp_map + so_encode_p_rows_ex(SO_REUSE_ME) (pass 2);
 * out_qp_map[i] (int32 [nb]) receives frame i's QPs.  roi: int32 [nb] offsets or NULL.  By
 * default both passes run in ONE persistent launch (each task the pass 2 of one tile, then the
 * pass 1 of the tile tiles_x + 1 positions later; a pass 2 waits for its tile row's pass 1);
 * with so_set_option(SO_OPT_RUN_2PASS_FUSED, 0), or for frames of fewer than three 32-row tile
 * rows, the library enqueues the per-frame kernel sequence itself instead (pass 1 tokens-only,
 * pass 2 with the QP map; the ME records kept in the workspace).  Frame i predicts from frame i-1's
 * pass-2 reconstruction, frame 0 from ref0.  Same coverage and workspace as so_encode_p_run
 * (W <= 8192).
 */
/*
 * 1 when so_encode_p_run_2pass runs an H x W frame (bs 16) in the one persistent launch (the
 * option SO_OPT_RUN_2PASS_FUSED is on and the frame has three 32-row tile rows or more, which
 * the merged schedule's deadlock-freedom needs), 0 when it enqueues the per-frame sequence.
 */
int so_p_run_2pass_fused(int H, int W);

int so_encode_p_run_2pass(const uint8_t* const* curs, int nframes, const uint8_t* ref0, int H, int W,
                          int bs, int sr, int qp_rd, const int32_t* qp_row, const int32_t* roi,
                          int qp_lo, int qp_hi, uint8_t* const* out_split, int16_t* const* out_mv,
                          int16_t* const* out_qtc, int32_t* const* out_tokens,
                          int32_t* const* out_mae_num, uint8_t* const* out_recon,
                          int32_t* const* out_sse, int32_t* const* out_qp_map, uint32_t* workspace,
                          void* stream);

/*
 * Several independent runs of P-frames in ONE persistent launch (the P-frames of several
 * GOPs, or of the runs between a GOP's I-frames): frame i predicts from out_recon[j] when
 * ref_frame[i] = j (j < i, a frame of this list: its tiles are waited for inside the launch
 * as in so_encode_p_run) and from refs[i] when ref_frame[i] = -1 (a plane complete before
 * the call, e.g. an I-frame's reconstruction).  Frames are taken in list order, so
 * interleaving the runs (A1 B1 A2 B2 ...) keeps the tiles of one frame of every run in flight
 * at once: where one frame has fewer tiles than the GPU's resident workgroups (1080p), the
 * runs fill the GPU that one run's frame-to-frame dependency leaves idle.  Each run's
 * output is identical to so_encode_p_run of that run alone (the reference's loop,
 * Encoder.py:1839-1867, per GOP).  refs: host array of nframes device pointers (entries with
 * ref_frame >= 0 are ignored); ref_frame: host int32[nframes]; the rest as so_encode_p_run.
 */
int so_encode_p_runs(const uint8_t* const* curs, int nframes, const uint8_t* const* refs,
                     const int32_t* ref_frame, int H, int W, int bs, int sr, int qp_rd,
                     const int32_t* qp_row, int vbs, double lam, uint8_t* const* out_split,
                     int16_t* const* out_mv,
                     int16_t* const* out_qtc, int32_t* const* out_tokens, int32_t* const* out_mae_num,
                     uint8_t* const* out_recon, int32_t* const* out_sse, uint32_t* workspace,
                     void* stream);

/*
 * ONE GOP across the GPUs of a node (BASELINE configs[3]): rank r encodes the block rows
 * [by0, by1) of every P-frame of a run with the persistent kernel of so_encode_p_run, and the
 * stripes hand their boundary rows to each other inside the launch -- the reference's frame
 * dependency (Encoder.py:1864-1867, P(i) searches recon(i-1)) extended across GPUs:
 *   * each rank's reconstruction planes live in UNCACHED device memory (so_alloc_uncached),
 *     addressed by "virtual" full-frame bases (row y of frame gf at base_gf + y * W; the
 *     allocation holds rows [16 by0 - 16, 16 by1 + 32));
 *   * a tile of the stripe's first (last) tile row also stores its top (bottom) 16 rows into
 *     the up (down) neighbour's plane of the frame -- peer memory mapped with so_ipc_open,
 *     reached over xGMI -- with system-scope write-through stores and, once they have drained,
 *     sets the neighbour's flag [gf * tiles_x + tx] (tiles_x = W / 128) to `epoch`;
 *   * a first- (last-) row tile waits, besides its own 3x3 tiles of the frame before, for
 *     my_up_flags (my_dn_flags) [(gf - 1) * tiles_x + tx - 1 .. tx + 1] == epoch.
 * curs: the frames (full H x W planes, only the stripe rows are read); out_recon[i]: virtual
 * bases of the stripe's planes; ref0: the virtual base of frame gbase - 1; symbol outputs are
 * stripe-local as in so_encode_p_rows.  peer_up0 / peer_dn0: the neighbours' virtual bases
 * of frame 0 as mapped here (frame gf at + gf * stride); any of the four neighbour pointers
 * NULL = no neighbour on that side.  epoch: a per-GOP value the flags are compared with
 * (they are never reset).  max_wg > 0 caps the resident grid (ranks sharing one GPU).
 * gbase >= 1 (frame 0 is the GOP's I-frame).
 */
int so_encode_p_run_stripe(const uint8_t* const* curs, int nframes, const uint8_t* ref0, int H, int W,
                           int bs, int sr, int by0, int by1, int qp_rd, const int32_t* qp_row,
                           uint8_t* const* out_split, int16_t* const* out_mv, int16_t* const* out_qtc,
                           int32_t* const* out_tokens, int32_t* const* out_mae_num,
                           uint8_t* const* out_recon, int32_t* const* out_sse, uint32_t* workspace,
                           int gbase, uint8_t* peer_up0, uint8_t* peer_dn0, long long stride,
                           const uint32_t* my_up_flags, const uint32_t* my_dn_flags,
                           uint32_t* peer_up_flags, uint32_t* peer_dn_flags, uint32_t epoch, int max_wg,
                           void* stream);

/* The I-frame's hand-off: rows [16 by0, 16 by0 + 16) of `plane` (a virtual base) to peer_up,
 * rows [16 by1 - 16, 16 by1) to peer_dn (the neighbours' virtual bases of frame gf), then
 * their flags [gf * tiles_x + tx] = epoch.  NULL peer = no neighbour on that side. */
int so_stripe_halo_push(const uint8_t* plane, int H, int W, int by0, int by1, int gf, uint8_t* peer_up,
                        uint8_t* peer_dn, uint32_t* peer_up_flags, uint32_t* peer_dn_flags,
                        uint32_t epoch, void* stream);

/*
 * One GOP across GPUs, consecutive frames on consecutive ranks (the frame pipeline of
 * DESIGN.md §6; north_star "frames within a GOP shard across the GPUs").  Rank g of N encodes
 * the frames k = g + N*j; frame k predicts from frame k-1, encoded by rank g-1 (mod N).  Each
 * rank owns uncached landing planes (so_alloc_uncached; slot j at land0 + j * stride, at least
 * H*W bytes + 16) with one flag word per 128x32 tile (land_flags + j * ntiles, ntiles =
 * (W/128) * ceil(H/32)): slot j holds the reconstruction of frame k-1 for its frame j, flagged
 * tile by tile == epoch as it arrives.  The persistent run of the rank's frames [slot0,
 * slot0 + nframes) waits per tile for the 3x3 arrived tiles of its reference, and stores every
 * tile's reconstruction both into out_recon[i] (local) and, system-scope write-through over
 * xGMI, into the landing plane its push code names before setting that rank's flag to epoch:
 * push_to[i] = 2 * slot + peer puts frame i's reconstruction into slot `slot` of peer_land0
 * (peer 0, flags peer_flags) or of peer2_land0 (peer 1, flags peer2_flags) -- the two ring
 * neighbours, so the ring direction can alternate per block of N frames -- and -1 pushes
 * nothing (the GOP's last frame).  Slots at or past nslots (every rank's slot count) are
 * rejected, as is slot0 + nframes > nslots.  Epochs are never reset (a new GOP uses a new
 * epoch).  vbs / lam as so_encode_p_run.  The symbols are those of so_encode_p_run over the
 * same frames.  so_frame_push sends a finished frame (the I-frame) the same way.  workspace:
 * so_p_run_workspace_elems(H, W), as so_encode_p_run.  max_wg > 0 caps the grid.
 */
int so_encode_p_run_fpipe2(const uint8_t* const* curs, int nframes, int H, int W, int bs, int sr,
                           int qp_rd, const int32_t* qp_row, int vbs, double lam,
                           uint8_t* const* out_split,
                           int16_t* const* out_mv, int16_t* const* out_qtc, int32_t* const* out_tokens,
                           int32_t* const* out_mae_num, uint8_t* const* out_recon,
                           int32_t* const* out_sse, uint32_t* workspace, const uint8_t* land0,
                           const uint32_t* land_flags, int slot0, uint8_t* peer_land0,
                           uint32_t* peer_flags, uint8_t* peer2_land0, uint32_t* peer2_flags,
                           const int32_t* push_to, int nslots, long long stride, uint32_t epoch,
                           int max_wg, void* stream);
/*
 * The frame pipeline with two-pass rate control and ROI (BASELINE configs[4] across GPUs;
 * build extension): each of the rank's frames runs pass 1, the per-block
 * QP map and pass 2 exactly as so_encode_p_run_2pass (roi, qp_lo, qp_hi, out_qp_map as there),
 * tile by tile inside ONE persistent launch (a tile's pass 2 starts once its tile row finished
 * pass 1), and pass 2 pushes the final reconstruction into the next frame's rank as
 * so_encode_p_run_fpipe2 does (same landing planes, flags, push codes, nslots and epochs).
 * A rank owns whole frames, so the row-local QP statistics never cross ranks.  The symbols
 * and QP maps are those of the one-GPU two-pass sequence over the same frames.  A tile row's
 * pass-2 tasks are queued about one grid's worth of tile rows after its pass-1 tasks; p2lag > 0
 * caps that lag (consecutive frames across ranks trail each other by ~lag + 2 tile rows, so
 * more ranks want a shorter one: pipeline.fpipe_p2lag); 0 = no cap.
 */
int so_encode_p_run_fpipe_2pass(const uint8_t* const* curs, int nframes, int H, int W, int bs, int sr,
                                int qp_rd, const int32_t* qp_row, const int32_t* roi, int qp_lo,
                                int qp_hi, uint8_t* const* out_split, int16_t* const* out_mv,
                                int16_t* const* out_qtc, int32_t* const* out_tokens,
                                int32_t* const* out_mae_num, uint8_t* const* out_recon,
                                int32_t* const* out_sse, int32_t* const* out_qp_map, uint32_t* workspace,
                                const uint8_t* land0, const uint32_t* land_flags, int slot0,
                                uint8_t* peer_land0, uint32_t* peer_flags, uint8_t* peer2_land0,
                                uint32_t* peer2_flags, const int32_t* push_to, int nslots, long long stride,
                                uint32_t epoch, int max_wg, int p2lag, void* stream);
int so_frame_push(const uint8_t* plane, int H, int W, uint8_t* peer_plane, uint32_t* peer_flags,
                  uint32_t epoch, void* stream);

/* Device memory the ranks share.  The one exception to "the library never allocates": the
 * landing planes and flags of the cross-GPU hand-off must be uncached
 * (hipExtMallocWithFlags(hipDeviceMallocUncached)), which PyTorch cannot allocate. */
#define SO_IPC_HANDLE_BYTES 64
int so_alloc_uncached(size_t bytes, void** out);
int so_free_device(void* p);
int so_ipc_export(void* p, uint8_t* out_handle);            /* hipIpcGetMemHandle */
int so_ipc_open(const uint8_t* handle, void** out);         /* hipIpcOpenMemHandle */
int so_ipc_close(void* p);
/* stream-ordered copies / fills of such memory (torch cannot wrap it) */
int so_copy_d2d(void* dst, const void* src, size_t bytes, void* stream);
int so_memset_d8(void* dst, int value, size_t bytes, void* stream);

/* int32 elements of scratch so_encode_i_frame / so_intra_recon need: nb*(bs*bs) + nb*8 */
size_t so_i_frame_scratch_elems(int H, int W, int bs);

/*
 * One I-frame of complete_intra_flow, intra_mode 0 (Encoder.py:1582-1642):
 * intra_prediction (:1238-1347, horizontal search intra_find_best_match_horizontal
 * :1010-1045, canvas generalised from the hard-coded 288x352 to H x W), per-block
 * DCT/quant/tokens/VBS-RD, and reconstruct_frame_intra (:1350-1417; unclipped canvas,
 * final astype(uint8) == mod-256 wrap).  out_mv is int16 [nb][4].  out_sse: optional
 * int32 [H] per PIXEL ROW sum of (cur - recon)^2 (the recon is produced row-parallel).
 */
int so_encode_i_frame(const uint8_t* cur, int H, int W, int bs, int sr, int qp_rd,
                      const int32_t* qp_row, int vbs, double lam, uint8_t* out_split,
                      int16_t* out_mv, int16_t* out_qtc, int32_t* out_tokens,
                      int32_t* out_mae_num, uint8_t* out_recon, int32_t* out_sse,
                      int32_t* scratch, void* stream);

/*
 * Stripe variant of so_encode_i_frame: block rows [by0, by1), same conventions as
 * so_encode_p_rows; out_sse is [(by1 - by0) * bs] per pixel row of the stripe.  Intra
 * mode 0 reads only original pixels and its reconstruction is row-local, so stripes need
 * no halo.
 */
int so_encode_i_rows(const uint8_t* cur, int H, int W, int bs, int sr, int by0, int by1,
                     int qp_rd, const int32_t* qp_row, int vbs, double lam, uint8_t* out_split,
                     int16_t* out_mv, int16_t* out_qtc, int32_t* out_tokens,
                     int32_t* out_mae_num, uint8_t* out_recon, int32_t* out_sse,
                     int32_t* scratch, void* stream);

/*
 * ---- ME variants: fast_me and FMEEnable (Encoder.py:388-406, 678-742, 1644-1651) -----------
 *
 * me_mode:
 *   SO_ME_FULL      find_best_match, exhaustive +-sr (the default path above);
 *   SO_ME_FAST      fast_me, serial branch of inter_prediction (:462-585): the 3x3
 *                   neighbourhood of a predictor that is the previous block's mv in raster
 *                   order (starting at (0,0,0)); a serial chain -- ONE wavefront walks the
 *                   frame, so stripes (by0 > 0) are rejected;
 *   SO_ME_FAST_PAR  fast_me under ParallelMode 2 (inter_prediction_parallel :587-676):
 *                   predictor (0,0,0) for every block and nRefFrames 1 (VBS is rejected: the
 *                   reference raises NameError there).
 * fast_me's MAE is the chosen reference INDEX (:742): the ME record's last field is then
 * ref * n^2 (and 0 when no candidate was valid, with mv = the predictor).
 * fme: search the frac frame frac_me_reference_frame(refs) ((2H-1) x (2W-1)) at (2x, 2y) over
 *   half-pel offsets in [-2sr, 2sr]; MVs are in half-pel units.  The library builds the
 *   frame as four phase planes P_ab[i][j] = F[2i+a][2j+b] into the caller's workspace
 *   `fme_planes` (so_fme_workspace_bytes) on every call, with
 *   fme_wrap = 1 when every reference is a uint8 reconstruction (the reference's
 *   `row + np.roll(row, -1)` then wraps mod 256), 0 while the list still holds the float64
 *   all-128 start frame (Encoder.py:1798).
 */
#define SO_ME_FULL 0
#define SO_ME_FAST 1
#define SO_ME_FAST_PAR 2

/* bytes of the FME workspace for nref references: nref * 4 planes of so_fme_plane_stride */
size_t so_fme_plane_stride(int H, int W);
size_t so_fme_workspace_bytes(int H, int W, int nref);

/* The four phase planes of one reference's frac frame (frac_me_reference_frame,
 * Encoder.py:388-403 / decoder.py:468-483) into out_planes (4 x so_fme_plane_stride). */
int so_fme_planes(const uint8_t* ref, int H, int W, int wrap, uint8_t* out_planes, void* stream);

/* so_me_full_search generalised by me_mode / fme (fme_planes: workspace, NULL unless fme). */
int so_me_search_ex(const uint8_t* cur, const uint8_t* const* refs, int nref, int H, int W, int bs,
                    int sr, int me_mode, int fme, int fme_wrap, uint8_t* fme_planes,
                    int32_t* out_best, int32_t* out_sub, void* stream);

/*
 * so_encode_p_rows generalised by me_mode / fme, a per-block QP map and flags; the same
 * outputs and scratch.
 *   qp_map  device int32 [H/bs * W/bs] per-block QP (full-frame, raster) or NULL; it
 *           replaces qp_row / qp_rd for the quantisation and reconstruction of each block
 *           (the VBS RD decision keeps qp_rd, like the reference's); see so_qp_map
 *   flags   SO_REUSE_ME: skip the ME; `scratch` (and fme_planes) still hold the ME records
 *           of a previous call on the same cur / refs / rows (pass 2 of two-pass RC)
 *           SO_TOKENS_ONLY: pass 1 of two-pass RC -- only out_tokens and the ME records in
 *           `scratch` are guaranteed (the fused full-search path skips the rest of the
 *           transform); the other outputs are left for the SO_REUSE_ME pass to write
 */
#define SO_REUSE_ME 1
#define SO_TOKENS_ONLY 2
int so_encode_p_rows_ex(const uint8_t* cur, const uint8_t* const* refs, int nref, int H, int W,
                        int bs, int sr, int by0, int by1, int qp_rd, const int32_t* qp_row,
                        const int32_t* qp_map, int vbs, double lam, int me_mode, int fme,
                        int fme_wrap, uint8_t* fme_planes, int flags, uint8_t* out_split,
                        int16_t* out_mv,
                        int16_t* out_qtc, int32_t* out_tokens, int32_t* out_mae_num,
                        uint8_t* out_recon, int32_t* out_sse, int32_t* scratch, void* stream);

/* Decoder P-frame reconstruction with FMEEnable (decoder.py:97-211 FME branches) and a
 * per-block QP map (NULL: qp_row / qp). */
int so_inter_recon_ex(const uint8_t* const* refs, int nref, int H, int W, int bs, int qp,
                      const int32_t* qp_row, const int32_t* qp_map, int fme, int fme_wrap,
                      uint8_t* fme_planes,
                      const uint8_t* split, const int16_t* mv, const int16_t* qtc,
                      uint8_t* out_recon, void* stream);

/* so_encode_i_rows / so_intra_recon with a per-block QP map (NULL: qp_row / qp_rd). */
int so_encode_i_rows_ex(const uint8_t* cur, int H, int W, int bs, int sr, int by0, int by1,
                        int qp_rd, const int32_t* qp_row, const int32_t* qp_map, int vbs,
                        double lam, uint8_t* out_split, int16_t* out_mv, int16_t* out_qtc,
                        int32_t* out_tokens, int32_t* out_mae_num, uint8_t* out_recon,
                        int32_t* out_sse, int32_t* scratch, void* stream);
int so_intra_recon_ex(int H, int W, int bs, int qp, const int32_t* qp_row, const int32_t* qp_map,
                      const uint8_t* split, const int16_t* mv, const int16_t* qtc,
                      uint8_t* out_recon, int32_t* scratch, void* stream);

/*
 * ROI and two-pass rate control (BASELINE configs[4]; a build extension -- the reference
 * computes per-row stats in complete_*_flow and discards them, Encoder.py:1627-1640,
 * 1696-1707, and has no ROI).  Writes the per-block QP map of block rows [by0, by1):
 *   qp = clamp(base + delta + roi, qp_lo, qp_hi),  base = qp_row[by] or qp_rd,
 *   delta in [-2, 2] from the block's pass-1 token count t against its row's sum m over n
 *   blocks: [t n >= 2m] + [t n >= 4m] - [2 t n < m] - [4 t n < m]  (0 when tokens == NULL).
 *   tokens  device int32 stripe-local pass-1 token counts (so_encode_*_rows out_tokens), or NULL
 *   roi     device int32 [H/bs * W/bs] QP offsets (negative = finer), or NULL
 *   out_qp_map  device int32 [H/bs * W/bs] (rows outside [by0, by1) untouched)
 */
int so_qp_map(const int32_t* tokens, int H, int W, int bs, int by0, int by1, int qp_rd,
              const int32_t* qp_row, const int32_t* roi, int qp_lo, int qp_hi,
              int32_t* out_qp_map, void* stream);

/* Decoder: P-frame reconstruction from symbols (decoder.py:97-211). */
int so_inter_recon(const uint8_t* const* refs, int nref, int H, int W, int bs, int qp,
                   const int32_t* qp_row, const uint8_t* split, const int16_t* mv,
                   const int16_t* qtc, uint8_t* out_recon, void* stream);

/* Decoder: I-frame reconstruction from symbols (decoder.py:330-432, mode 0). */
int so_intra_recon(int H, int W, int bs, int qp, const int32_t* qp_row,
                   const uint8_t* split, const int16_t* mv, const int16_t* qtc,
                   uint8_t* out_recon, int32_t* scratch, void* stream);

/*
 * Batched per-block transforms for the reference's per-block public methods (the drop-in
 * surface): n blocks of N x N doubles (N = 16 or 8), row-major [n][N][N].
 *   inverse 0: out_tc = np.round(DCT-II 2-D)     -- apply_2d_dct (Encoder.py:779-784)
 *              with qp >= 0 also out_q = np.round(TC / Q(N, qp)) -- quantize_TC (:787-789)
 *              and out_tokens[n] = len(entropy_encoder_block(QTC)) (:1086-1131), the
 *              per-block terms of calculate_RD_cost (:1133-1158)
 *   inverse 1: out_tc = np.round(DCT-III 2-D)    -- apply_2d_idct (:810-817), the transform
 *              inside reconstruct_block (:824-827); out_q / out_tokens must be NULL
 * Outputs are device int32 [n][N][N] / [n] (each may be NULL).  Same FP64 operation order as
 * the frame kernels (pocketfft replica, bitwise equal to scipy.fftpack).
 */
int so_block_xform(const double* in, int n, int N, int inverse, int qp, int32_t* out_tc,
                   int32_t* out_q, int32_t* out_tokens, void* stream);

/*
 * Sum of squared differences of two uint8 planes of n pixels, ADDED into *out_sse
 * (device uint64; zero it first).  PSNR per frame (calculate_metrics, Encoder.py:934)
 * is 10*log10(255^2 / (sse / n)) on the host.
 */
int so_sse_u8(const uint8_t* a, const uint8_t* b, int64_t n, uint64_t* out_sse,
              void* stream);

/*
 * SSIM of nframes pairs of uint8 planes (calculate_metrics, Encoder.py:934-935:
 * skimage.metrics.structural_similarity(a, b, win_size=win) on uint8 frames): data range 255,
 * uniform win x win window, sample covariance, K1 0.01, K2 0.03, and the mean of S over the
 * (H - win + 1) x (W - win + 1) windows that lie fully inside the picture (skimage crops a border
 * of (win - 1) / 2).  With NP = win^2 and the exact integer window sums sx, sy, sxx, syy, sxy:
 *   ux = sx / NP, uy = sy / NP, vx = (NP sxx - sx^2) / (NP (NP - 1)), vy and vxy alike,
 *   S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),  C1 = 2.55^2, C2 = 7.65^2,
 * evaluated in FP64.
 *   a, b       HOST arrays of nframes device pointers; pair i is a[i] against b[i].  Planes need no
 *              alignment; row y of a plane starts pitch bytes after row y - 1 (pitch_a / pitch_b
 *              >= W, in bytes), so the H x W picture area of a padded plane is measured alone
 *   win        odd, 3..15 (the reference uses 11); H >= win and W >= win
 *   out        nframes device doubles
 *   workspace  device doubles [so_ssim_workspace_elems(nframes, H, W, win)] (0 for a geometry
 *              so_ssim_u8 rejects): one partial per tile, every one written before it is read
 *              (no zeroing needed).  One workspace serves one stream at a time.
 * A frame's partials are added in a fixed order with no floating-point atomics: its value has
 * the same bits from run to run and whether it is computed alone or inside a batch.  Identical
 * planes give exactly 1.0.  nframes == 0 returns SO_OK.
 */
size_t so_ssim_workspace_elems(int nframes, int H, int W, int win);
int so_ssim_u8(const uint8_t* const* a, const uint8_t* const* b, int nframes, int H, int W,
               size_t pitch_a, size_t pitch_b, int win, double* out, double* workspace, void* stream);

/*
 * Chroma 4:2:0 (build extension: the reference codes luma only; DESIGN.md "Chroma 4:2:0").  U and V
 * of one frame, encoded from the LUMA frame's motion: luma block b = (bx, by) of the 16x16 grid
 * owns the 8x8 block at (8 bx, 8 by) of each chroma plane (H/2 x W/2, pitch W/2; H, W: the padded
 * luma size), one launch for both planes, asynchronous on `stream`.
 *   prediction   frame_type 0: every sample 128.  frame_type 1: the block's luma MV mv[b][0] =
 *                (dx, dy, r) -- mv[b][j] for its 4x4 quadrant j (Z order) when split[b] -- in
 *                half-sample units: ix = dx >> 1, fx = dx & 1, x0 = clamp(X + ix, 0, W/2 - 1),
 *                x1 = clamp(X + ix + fx, 0, W/2 - 1), y alike,
 *                P = (R[y0][x0] + R[y0][x1] + R[y1][x0] + R[y1][x1] + 2) >> 2 on the chroma plane R
 *                of reference clamp(r, 0, nref - 1): total for any MV, exact integers
 *   transform    one 8x8 per block, the reference's per-block functions at N = 8: apply_2d_dct
 *                (Encoder.py:779), quantize_TC with generate_Q_matrix(8, qpc) (:787, :938),
 *                len(entropy_encoder_block) (:1086), rescale_QTC, apply_2d_idct (:810),
 *                (P + idct).astype(uint8) (:824, mod-256 wrap)
 *   qpc          clamp(base + qp_offset, 0, 20), base = qp_map[b] if qp_map, else qp_row[by] if
 *                qp_row, else qp -- the values the luma frame was given (no -1 for split blocks)
 *   cur_u/v      the frame's chroma planes;  refs_u/v: HOST arrays of nref device pointers, the
 *                chroma reconstructions in the luma reference list's order (frame_type 1 only;
 *                ignored, with nref, for frame_type 0, as are split and mv)
 *   split, mv    the luma frame's symbols (uint8 [nb], int16 [nb][4][3])
 *   out_qtc_u/v  int16 [nb][64] row-major;  out_tokens, out_sse: int32 [2][nb] (U then V), the
 *                token count and the sum of (cur - recon)^2 of every block
 * Planes must be 8-byte aligned and qtc arrays 16-byte aligned; nothing outside a plane is read.
 * bs != 16 is SO_E_UNSUPPORTED; H or W not a multiple of 16, a frame_type other than 0 / 1, nref
 * outside 1..SO_MAX_REF on a P-frame, a NULL required pointer or a reconstruction that aliases a
 * reference (or the other reconstruction) is SO_E_INVALID, before any launch.
 * so_chroma_recon_frame is the decoder: the same prediction and inverse path from qtc_u / qtc_v.
 *
 * so_chroma_encode_frame_ex / so_chroma_recon_frame_ex take one more argument, mv_frac_bits = s: the
 * number of fractional bits of the luma vector seen from the chroma plane -- 1 when the luma vectors
 * are full-sample (the two functions above, which forward with 1 and report under their own names),
 * 2 when they are half-sample (FMEEnable).  Only the P-frame prediction depends on it.  With
 * D = 1 << s, for the sample at (X, Y) with vector (dx, dy, r):
 *     ix = dx >> s (arithmetic, floor)      fx = dx & (D - 1)         iy, fy alike
 *     x0 = clamp(X + ix, 0, W/2 - 1)        x1 = clamp(X + ix + (fx != 0), 0, W/2 - 1)      y0, y1 alike
 *     P  = ((D-fx)(D-fy) R[y0][x0] + fx (D-fy) R[y0][x1] + (D-fx) fy R[y1][x0] + fx fy R[y1][x1]
 *           + (1 << (2s - 1))) >> 2s
 * on the chroma plane R of reference clamp(r, 0, nref - 1).  Exact integers; the weights sum to D^2,
 * so P is in 0..255, and the clamps keep it total for any int16 vector.  At s = 1 (fx, fy in {0, 1})
 * the weights are 4, 2 + 2 or 1 + 1 + 1 + 1 over 4 and x1 = clamp(X + ix + fx): the formula above, bit
 * for bit.  A multiple of D moves whole samples.  mv_frac_bits other than 1 / 2 is SO_E_INVALID
 * before any launch (checked after bs); every other rule is that of the base function.
 */
int so_chroma_encode_frame(const uint8_t* cur_u, const uint8_t* cur_v, const uint8_t* const* refs_u,
                           const uint8_t* const* refs_v, int nref, int H, int W, int bs, int frame_type,
                           const uint8_t* split, const int16_t* mv, int qp, const int32_t* qp_row,
                           const int32_t* qp_map, int qp_offset, int16_t* out_qtc_u, int16_t* out_qtc_v,
                           int32_t* out_tokens, uint8_t* out_recon_u, uint8_t* out_recon_v, int32_t* out_sse,
                           void* stream);
int so_chroma_recon_frame(const uint8_t* const* refs_u, const uint8_t* const* refs_v, int nref, int H, int W,
                          int bs, int frame_type, const uint8_t* split, const int16_t* mv, int qp,
                          const int32_t* qp_row, const int32_t* qp_map, int qp_offset, const int16_t* qtc_u,
                          const int16_t* qtc_v, uint8_t* out_recon_u, uint8_t* out_recon_v, void* stream);
int so_chroma_encode_frame_ex(const uint8_t* cur_u, const uint8_t* cur_v, const uint8_t* const* refs_u,
                              const uint8_t* const* refs_v, int nref, int H, int W, int bs, int frame_type,
                              const uint8_t* split, const int16_t* mv, int qp, const int32_t* qp_row,
                              const int32_t* qp_map, int qp_offset, int16_t* out_qtc_u, int16_t* out_qtc_v,
                              int32_t* out_tokens, uint8_t* out_recon_u, uint8_t* out_recon_v,
                              int32_t* out_sse, int mv_frac_bits, void* stream);
int so_chroma_recon_frame_ex(const uint8_t* const* refs_u, const uint8_t* const* refs_v, int nref, int H,
                             int W, int bs, int frame_type, const uint8_t* split, const int16_t* mv, int qp,
                             const int32_t* qp_row, const int32_t* qp_map, int qp_offset,
                             const int16_t* qtc_u, const int16_t* qtc_v, uint8_t* out_recon_u,
                             uint8_t* out_recon_v, int mv_frac_bits, void* stream);

/*
 * Colour conversion (build extension; DESIGN.md "Colour conversion"): 8-bit RGB to and from the
 * padded 4:2:0 planes the chroma path codes, exact integers, one launch for a batch of frames,
 * asynchronous on `stream`, no host synchronisation.  tests/colourref.py restates it in numpy.
 *   matrix      SO_COLOUR_BT601 (Kr 0.299, Kb 0.114) or SO_COLOUR_BT709 (Kr 0.2126, Kb 0.0722)
 *   full_range  1: Y and C in 0..255, yoff 0;  0: Y in 16..235, C in 16..240, yoff 16
 *   arithmetic  int32 with 16 fractional bits; >> is the arithmetic shift (floor)
 *   forward tables  F = rint(coef * 65536), then the G entry of each row takes what makes the Y row
 *               sum to rint(ys * 65536) (ys = 1 or 219/255) and the chroma rows to 0.  Rows Y, Cb, Cr;
 *               columns R, G, B:
 *                 601 full     [19595, 38470, 7471] [-11058, -21710, 32768] [32768, -27439, -5329]
 *                 601 limited  [16829, 33039, 6416] [-9714, -19070, 28784] [28784, -24103, -4681]
 *                 709 full     [13933, 46871, 4732] [-7509, -25259, 32768] [32768, -29763, -3005]
 *                 709 limited  [11966, 40254, 4064] [-6596, -22188, 28784] [28784, -26145, -2639]
 *   forward     Y = clip((F_Y . (R, G, B) + (yoff << 16) + 32768) >> 16, 0, 255) per pixel.  The chroma
 *               sample of the 2 x 2 luma cell at (2i, 2j) comes from the cell's sums SR, SG, SB, sited
 *               at the cell's centre, with one rounding:
 *                 C = clip((F_C . (SR, SG, SB) + (128 << 18) + (1 << 17)) >> 18, 0, 255)
 *               (the clip matters: at full range pure red and pure blue reach 256).  Y goes to an
 *               Hp x Wp plane of pitch Wp, U and V to Hp/2 x Wp/2 planes of pitch Wp/2, and every
 *               sample outside the h x w picture area is written as 128 by the same launch.
 *   inverse tables  J = rint(M * 65536), unadjusted, M the inverse of the real forward matrix
 *               (255/219 and 255/224 included at limited range).  Rows R, G, B; columns Y - yoff,
 *               U - 128, V - 128:
 *                 601 full     [65536, 0, 91881] [65536, -22553, -46802] [65536, 116130, 0]
 *                 601 limited  [76309, 0, 104597] [76309, -25675, -53279] [76309, 132201, 0]
 *                 709 full     [65536, 0, 103206] [65536, -12276, -30679] [65536, 121609, 0]
 *                 709 limited  [76309, 0, 117489] [76309, -13975, -34925] [76309, 138438, 0]
 *   inverse     each chroma sample serves its 2 x 2 luma samples (replication, the adjoint of the
 *               forward average):
 *                 out_c = clip((J[c][0] (Y - yoff) + J[c][1] (U - 128) + J[c][2] (V - 128) + 32768) >> 16, 0, 255)
 *               The picture area of the padded planes is read; h x w pixels are written.
 *   int32       forward: |F| <= 46871 and a cell's sums are <= 1020, so |F_C . S| <= 3 * 46871 * 1020
 *               < 2^28 and the offsets add < 2^26; the Y sum is below 2^25.  Inverse: |J| <= 138438 <
 *               2^18 and |Y - yoff|, |U - 128|, |V - 128| <= 255, so the three products sum to less
 *               than 3 * 2^26 < 2^28.  No intermediate leaves int32.
 *   layouts     SO_LAYOUT_HWC: interleaved, pixel (y, x) at rgb + y * pitch + 3 x (pitch >= 3 w);
 *               SO_LAYOUT_CHW: planar, channel c of pixel (y, x) at rgb + c * plane_stride + y * pitch
 *               + x (pitch >= w; plane_stride is ignored for HWC).  Bytes, any alignment: a row
 *               segment whose address is not a multiple of 4 is moved byte by byte, so a cropped view
 *               of a larger picture converts in place.
 *   rgb, y, u, v  HOST arrays of nframes device pointers.  Only the picture area of a source is read;
 *               only the planes (forward) or the picture area of rgb (inverse) are written.
 * SO_E_INVALID before any launch, the argument named in so_last_error: h or w odd or not positive; Hp
 * or Wp odd or smaller than the picture; a pitch smaller than a row; a matrix, full_range or layout
 * outside the values above; nframes < 0; a NULL pointer; a destination that overlaps another
 * destination or a source.  nframes == 0 with valid scalars returns SO_OK.
 */
#define SO_COLOUR_BT601 0
#define SO_COLOUR_BT709 1
#define SO_LAYOUT_HWC 0
#define SO_LAYOUT_CHW 1
int so_rgb_to_yuv420(const uint8_t* const* rgb, int nframes, int h, int w, int layout, size_t pitch,
                     size_t plane_stride, int matrix, int full_range, int Hp, int Wp, uint8_t* const* y,
                     uint8_t* const* u, uint8_t* const* v, void* stream);
int so_yuv420_to_rgb(const uint8_t* const* y, const uint8_t* const* u, const uint8_t* const* v, int nframes,
                     int Hp, int Wp, int h, int w, int matrix, int full_range, int layout, uint8_t* const* rgb,
                     size_t pitch, size_t plane_stride, void* stream);

/*
 * Scaling (build extension; DESIGN.md "Scaling"): a separable polyphase resampler for 8-bit 4:2:0
 * pictures, exact integers, one launch for Y, U and V of a batch of frames, asynchronous on
 * `stream`, no host synchronisation.  tests/scaleref.py restates it in numpy.
 *   tables      one per axis and plane kind (luma horizontal yh, luma vertical yv, chroma horizontal
 *               ch, chroma vertical cv), each as coef int16 [n_dst][taps], first int32 [n_dst] and
 *               taps (1..32), in DEVICE memory.  streamoptima_amd.scale.taps builds them: the centre
 *               of output j is (j + 0.5) n_src / n_dst - 0.5 (cell centres, the siting of the colour
 *               conversion's chroma), the kernel function (bilinear; Catmull-Rom bicubic, a = -0.5;
 *               lanczos3) is stretched by max(1, n_src / n_dst), the weights at the integer positions
 *               strictly inside its support are normalised, multiplied by 16384 and rounded, and the
 *               largest tap takes what makes the row sum exactly 16384; sum |coef| <= 32768 per row.
 *               first[j] + t may lie outside the source: the index is clamped (edge replication).
 *   arithmetic  per plane, >> the arithmetic shift (floor), horizontal first, then vertical:
 *                 hsum(y, j) = sum_t coef_h[j][t] * src[y][clamp(first_h[j] + t, 0, ws - 1)]
 *                 mid(y, j)  = clamp((hsum + 128) >> 8, -32768, 32767)      int16, 6 fractional bits
 *                 vsum(i, j) = sum_t coef_v[i][t] * mid(clamp(first_v[i] + t, 0, hs - 1), j)
 *                 out(i, j)  = clip((vsum + (1 << 19)) >> 20, 0, 255)
 *   int32       with tables as above |hsum| <= 255 * 32768 < 2^23, |mid| <= 255 * 2 * 64 = 32640 (the
 *               int16 clamp never acts), |vsum| <= 32640 * 32768 < 2^30, and 2^19 more stays in int32.
 *               A constant plane maps to the same constant; n_src == n_dst gives taps = 1, coef =
 *               16384, first[j] = j, an exact copy.  The final clip does act (ringing on hard edges).
 *               The tables are not validated: for any contents the kernel stays inside its buffers
 *               (both clamps above) and sums with wrapping unsigned arithmetic; results are
 *               specified only for tables built as above.
 *   source      sy, su, sv: HOST arrays of nframes device pointers to the top-left sample of hs x ws
 *               luma and hs/2 x ws/2 chroma pictures, rows pitch_y and pitch_c bytes apart (any
 *               alignment: the picture area of padded planes, or a cropped view).  Only the picture
 *               area is read.
 *   destination dy, du, dv: dense Hp x Wp luma planes (pitch Wp) and Hp/2 x Wp/2 chroma planes (pitch
 *               Wp/2).  The hd x wd picture is written top-left; every other sample of the planes is
 *               written as 128 by the same launch (the padding so_rgb_to_yuv420 writes).
 *   luma only   su == sv == du == dv == NULL scales luma alone (the chroma tables are ignored); a
 *               partial set is invalid.
 * SO_E_INVALID before any launch, the argument named in so_last_error: a size that is not positive,
 * or with chroma odd; Hp or Wp smaller than the picture, or with chroma odd; a pitch shorter than a
 * row; taps outside 1..32; nframes < 0; a NULL pointer or table; a destination that overlaps a source
 * or another destination.  nframes == 0 with valid scalars returns SO_OK.  SO_E_UNSUPPORTED: a ratio
 * so extreme that no tile of it fits the LDS (far beyond what 32 taps resample).
 */
int so_scale_yuv420(const uint8_t* const* sy, const uint8_t* const* su, const uint8_t* const* sv, int nframes,
                    int hs, int ws, size_t pitch_y, size_t pitch_c, uint8_t* const* dy, uint8_t* const* du,
                    uint8_t* const* dv, int hd, int wd, int Hp, int Wp, const int16_t* coef_yh,
                    const int32_t* first_yh, int taps_yh, const int16_t* coef_yv, const int32_t* first_yv,
                    int taps_yv, const int16_t* coef_ch, const int32_t* first_ch, int taps_ch,
                    const int16_t* coef_cv, const int32_t* first_cv, int taps_cv, void* stream);

/*
 * Deblocking (build extension; DESIGN.md "Deblocking"): a display-side post-filter over the edges of
 * the transform grid of decoded 8-bit 4:2:0 planes.  It is NOT in the coding loop: the sources (the
 * reconstructions, which stay the references) are only read, separate planes are written.  Exact
 * integers, >> the arithmetic shift (floor), one launch for Y, U and V of a batch of frames,
 * asynchronous on `stream`, no host synchronisation, no allocation.  tests/deblockref.py restates it
 * in numpy.
 *   planes      dense H x W luma (H, W multiples of bs) and H/2 x W/2 chroma planes.  The whole padded
 *               plane is filtered; callers crop afterwards.  Samples no edge touches are copied: the
 *               output is a complete plane.
 *   cells       every plane is a grid of 8 x 8 cells.  blockqp(b) = qp_map[b] if a map is given, else
 *               qp_row[by] if rows are given, else qp, clamped to 0..20 (maps and rows are device
 *               memory nobody validated: a bad entry gives a wrong picture and nothing worse).
 *               Luma cell in block b: cellqp = blockqp(b), and where split[b] != 0, blockqp(b) - 1
 *               (0 stays 0): the rule split sub-blocks are dequantised by.  bs 16: a block is 2 x 2
 *               cells; bs 8: one cell.  Chroma cell, one per luma block:
 *               cellqp = clamp(blockqp(b) + chroma_qp_offset, 0, 20); split does not enter.
 *   edges       between two horizontally or vertically adjacent cells of a plane that belong to
 *               different blocks, or (luma, bs 16) to one block with split[b] != 0.  None on the plane's
 *               border.  q = clamp(max(cellqp_P, cellqp_Q) + strength, 0, 20), s = 1 << q,
 *               alpha = min(s, 255), beta = min((3 * s) >> 3, 255), tc = min(s >> 2, 255),
 *               tc1 = tc >> 1.  For q < 2, tc is 0 and the filter is the identity.
 *   one line    across an edge, p2 p1 p0 | q0 q1 q2 with p0, q0 adjacent to it:
 *                 d   = q0 - p0
 *                 on  = |d| < alpha and |p1 - p0| < beta and |q1 - q0| < beta
 *                 ap  = |p2 - p0| < beta            aq = |q2 - q0| < beta
 *                 dl  = clip3(-tc, tc, (4 * d + (p1 - q1) + 4) >> 3)
 *                 avg = (p0 + q0 + 1) >> 1                        (from the unfiltered p0, q0)
 *                 if on:       p0' = clip(p0 + dl, 0, 255)    q0' = clip(q0 - dl, 0, 255)
 *                 if on && ap: p1' = p1 + clip3(-tc1, tc1, (p2 + avg - 2 * p1) >> 1)
 *                 if on && aq: q1' = q1 + clip3(-tc1, tc1, (q2 + avg - 2 * q1) >> 1)
 *               p2 and q2 are never written; p1' and q1' stay inside 0..255 by construction.
 *   order       pass 1 filters every vertical edge (lines along rows) from the input, pass 2 every
 *               horizontal edge (lines along columns) from pass 1's result.  Inside a pass the edges
 *               are independent: 8 apart, a line writes two samples a side and reads three.
 *   arrays      sy .. dv, split, qp_row, qp_map: HOST arrays of nframes device pointers.  split (uint8
 *               [nb]), qp_row (int32 [H / bs]) and qp_map (int32 [nb]) may be NULL as a whole or hold
 *               NULL for single frames: no splits; no map -> rows -> qp.
 *   luma only   su == sv == du == dv == NULL filters luma alone; a partial set is invalid.
 * SO_E_INVALID before any launch, the argument named in so_last_error, in this order: nframes < 0; bs
 * not 8 or 16; H or W not a positive multiple of bs, or H * W above 2^31 samples (one rule, the
 * bound every frame geometry of this library has); qp outside 0..20; chroma_qp_offset outside
 * -20..20; strength outside -3..3; (nframes == 0 returns SO_OK here;) sy or dy NULL or holding a NULL
 * plane; a partial chroma set or a NULL chroma plane; a destination plane that overlaps a source or
 * another destination of the call.  SO_E_UNSUPPORTED: chroma with bs 8; a non-NULL split entry with
 * bs 8 (4-sample sub-blocks: the lines of a pass would overlap).
 */
int so_deblock_yuv420(const uint8_t* const* sy, const uint8_t* const* su, const uint8_t* const* sv,
                      int nframes, int H, int W, int bs, const uint8_t* const* split, int qp,
                      const int32_t* const* qp_row, const int32_t* const* qp_map,
                      int chroma_qp_offset, int strength,
                      uint8_t* const* dy, uint8_t* const* du, uint8_t* const* dv, void* stream);

/*
 * out[i] = sum of rows[i][0..len) (int32 -> int64) for i < n: the per-frame SSE of a GOP from
 * the encode kernels' per-block / per-row out_sse arrays (rows: a HOST array of device
 * pointers), one launch.
 */
int so_sum_i32_rows(const int32_t* const* rows, int n, int len, int64_t* out, void* stream);

/*
 * Packed symbol stream: the content of the reference's two text lines per frame
 * (differential_encoder_frame's MVs before differencing, Encoder.py:1419-1520, and
 * entropy_encoder_block's RLE token lists, :1086-1131 / :1522-1542) as zigzag LEB128
 * varints, per block in raster order:  split | mv values | token lists of its (sub-)blocks.
 * Replaces downloading the dense int16 QTC (2 B/px) when symbols leave the GPU
 * (transmit_bitstream, :1544-1580).  Format: so_pack.hip; host decoder: bitstream.unpack_frame.
 *
 * so_pack_bound: the worst-case bytes of a frame of nb blocks (a capacity that never
 *   overflows).
 * so_pack_frames: for frame i (frame_types: a HOST array, 0 = intra, 1 = inter; split / mv /
 *   qtc: device arrays in the canonical symbol layout) writes offs[i][0..nb) = each block's byte offset, offs[i][nb] =
 *   the frame's total, and the stream into out[i][0..total).  Blocks that would pass `cap`
 *   bytes are not written: the caller checks offs[i][nb] <= cap before using out[i].
 *   Stream-ordered, no host synchronisation.
 * so_pack_frames_ex: the same, and totals[i] = offs[i][nb] (totals: nframes uint32, device
 *   memory or page-locked host memory the device can address -- stored at system scope, so a
 *   host that has waited for the stream reads them without a copy; NULL = none).  A host
 *   streaming the packed bytes out learns each frame's length from it without a gather and a
 *   copy per chunk (hoststream.HostStreamEncoder).
 */
size_t so_pack_bound(int nb, int block_size);
int so_pack_frames(int nframes, const int32_t* frame_types, const uint8_t* const* split,
                   const int16_t* const* mv, const int16_t* const* qtc, int nb, int block_size,
                   uint32_t* const* offs, uint8_t* const* out, unsigned long long cap,
                   void* stream);
int so_pack_frames_ex(int nframes, const int32_t* frame_types, const uint8_t* const* split,
                      const int16_t* const* mv, const int16_t* const* qtc, int nb, int block_size,
                      uint32_t* const* offs, uint8_t* const* out, unsigned long long cap,
                      uint32_t* totals, void* stream);

/*
 * The inverse (the decoder side of the packed stream): frame i's bytes packed[i] with the
 * block offsets offs[i][0..nb] so_pack_frames wrote, back to split / mv / qtc in the canonical
 * layout (mv entries past the first of an unsplit block are 0 on output).  frame_types: HOST
 * array.  Malformed input sets the device int32 *err to 1 + a bad block's index (zero it
 * first); a bad block's outputs are unspecified.  Block b is decoded from exactly its bytes
 * [offs[b], offs[b+1]); offs[b+1] < offs[b] is malformed, and within the block:
 *   * a varint is 1-5 bytes, decoded with no bits dropped and then un-zigzagged; a sixth
 *     continuation byte, or a varint running off the end of the block's bytes, is malformed;
 *   * split is 0, or 1 at block size 16; anything else is malformed;
 *   * every mv value and every coefficient lies in [-32768, 32767], else malformed;
 *   * a token -L needs 1 <= L <= nn - k, a token Z > 0 needs Z <= nn - k (k: the coefficients
 *     of the (sub-)block covered so far, nn its size); a token 0 ends the (sub-)block, and a
 *     list also ends at k == nn;
 *   * all the block's bytes must be consumed.
 * Accepted though not canonical (unambiguous, never written by so_pack_frames):
 *   * an over-long varint of up to 5 bytes whose value fits;
 *   * a 0 value inside a -L list;
 *   * a zero run that reaches exactly nn written as Z instead of 0.
 * Offsets that point outside packed[i]'s buffer are a caller precondition, not checked here
 * (packedfile.read rejects files whose lengths do not add up).
 */
int so_unpack_frames(int nframes, const int32_t* frame_types, const uint8_t* const* packed,
                     const uint32_t* const* offs, int nb, int block_size, uint8_t* const* split,
                     int16_t* const* mv, int16_t* const* qtc, int32_t* err, void* stream);

/*
 * The same stream in the "bits" coding: the same symbols per block, in the same order, as
 * bit-granular Exp-Golomb codes instead of varints (about half the bytes).  Blocks stay
 * byte-aligned, so the offsets, the totals, the capacity guard and the parallel decode work as
 * above.  The format (the model is tests/packbitsref.py):
 *
 * Bits are written MSB-first within each byte.  With zz(v) = 2v for v >= 0 and -2v-1 otherwise:
 *   ue(z):    let m = z + 1 and n = bit_length(m); n - 1 zero bits, then m in n bits.
 *   ue_k(z):  ue(z >> k) followed by the low k bits of z.
 *   se(v) = ue(zz(v)),  se_k(v) = ue_k(zz(v)).
 *   -32768 is the longest value at 33 bits: code lengths cross 32 and, accumulated, 64 bits.
 * One block, in raster order:
 *   1. split: 1 bit.
 *   2. k: 2 bits, the order of this block's coefficient codes.
 *   3. The mv values, se each; the same values and order as the varint format: inter
 *      (dx, dy, ref) once, or 4x in Z order when split; intra dx once or 4x.
 *   4. Each (sub-)block's token list exactly as in the varint format ("-L" then L values, "Z",
 *      a trailing "0").  Tokens are se, coefficient values se_k.
 *   5. Zero bits up to the next byte boundary.
 * Canonical k (what so_pack_frames_bits writes): the k in 0..3 that minimises the block's
 * total coefficient bits; ties go to the smallest k; a block with no coefficient writes 0.
 * Malformed to a decoder (so_unpack_frames_bits, bitstream.unpack_frame_bits):
 *   * a ue prefix of more than 16 zero bits;
 *   * a decoded z > 65535 (so every mv value and coefficient lies in int16);
 *   * a code running past the block's last byte;
 *   * split = 1 at block size 8;
 *   * the token rules as above (-L needs 1 <= L <= nn - k', Z > 0 needs Z <= nn - k', 0 ends
 *     the list, a list also ends at nn; k': the coefficients covered so far);
 *   * after the last list, 8 or more bits left, or any set bit among them;
 *   * offs[b+1] < offs[b].
 * Accepted though never written: a non-minimal k; k != 0 with no coefficients; a 0 value
 * inside a -L list; a zero run reaching exactly nn written as Z.
 * mv entries past the first of an unsplit block are 0 on output.
 *
 * so_pack_bits_bound(nb, bs) = nb * ceil((3 + 12*33 + 33*nn + 19*(nn/2 + 4)) / 8), nn = bs^2;
 *   0 for nb <= 0 or bs other than 8 or 16.  Loose on purpose, like so_pack_bound; at bs 16
 *   about 1.4 KB per block, so a block's length fits a container's u16.
 * so_pack_frames_bits: arguments and behaviour of so_pack_frames_ex (totals may be NULL).
 * so_unpack_frames_bits: arguments and behaviour of so_unpack_frames.
 */
size_t so_pack_bits_bound(int nb, int block_size);
int so_pack_frames_bits(int nframes, const int32_t* frame_types, const uint8_t* const* split,
                        const int16_t* const* mv, const int16_t* const* qtc, int nb, int block_size,
                        uint32_t* const* offs, uint8_t* const* out, unsigned long long cap,
                        uint32_t* totals, void* stream);
int so_unpack_frames_bits(int nframes, const int32_t* frame_types, const uint8_t* const* packed,
                          const uint32_t* const* offs, int nb, int block_size,
                          uint8_t* const* split, int16_t* const* mv, int16_t* const* qtc,
                          int32_t* err, void* stream);

/*
 * The chroma coefficients (so_chroma_encode_frame's qtc_u / qtc_v, device int16 [nb][64] each,
 * row-major) as a packed stream, in both codings of the luma stream.  The models are in
 * tests/packchromaref.py; host decoders: bitstream.unpack_chroma_frame / unpack_chroma_frame_bits.
 *
 * One record per luma block b, in raster order: the token list of U's 8x8 block b, then the
 * token list of V's block b.  A list is exactly a (sub-)block list of the luma format: scan in
 * scan_order(8); "-L" is followed by L values; "Z" > 0 is a run of Z zeros; "0" is the trailing
 * zero run; a list also ends after 64 coefficients.  No split flag and no motion vectors.
 *
 * Coding "varint" (so_pack_chroma_frames): every number a zigzag LEB128 varint; the shortest
 * record is 2 bytes.  Malformed to a decoder (k: the coefficients of the list covered so far):
 *   * a varint running past 5 bytes or off the end of the record;
 *   * a decoded zigzag value of 2^16 or more;
 *   * a token -L with L < 1 or L > 64 - k;  a token Z > 64 - k;
 *   * bytes left after V's list;
 *   * offs[b+1] < offs[b].
 * Accepted though never written: an over-long varint of up to 5 bytes whose value fits; a 0
 * value inside a -L list; a run reaching exactly 64 written as Z.
 *
 * Coding "bits" (so_pack_chroma_frames_bits): bits MSB-first; first k in 2 bits, the order of
 * this record's coefficient codes, shared by both lists; then U's list, then V's, tokens se and
 * coefficient values se_k (defined above); then zero bits up to the byte boundary.  Canonical
 * k: the k in 0..3 that minimises the record's total coefficient bits over both lists; ties go
 * to the smallest k; a record with no coefficient writes 0.  Malformed to a decoder:
 *   * a ue prefix of more than 16 zero bits;  a decoded z > 65535;
 *   * a code running past the record's last byte;
 *   * a token breaking the token rules above;
 *   * 8 or more bits left after V's list, or any set bit among the bits left;
 *   * offs[b+1] < offs[b].
 * Accepted though never written: a non-minimal k; k != 0 with no coefficient; a 0 value inside
 * a -L list; a run reaching exactly 64 written as Z.
 *
 * so_pack_chroma_bound(nb) = nb * 600 (two lists of 3 * (64 + 32 + 4) bytes) and
 * so_pack_chroma_bits_bound(nb) = nb * ceil((2 + 2 * (33*64 + 19*36)) / 8) = nb * 700: loose on
 *   purpose, like the luma bounds; a record's length fits a container's u16.  0 for nb <= 0.
 * so_pack_chroma_frames / _bits: offs, out, cap and totals exactly as so_pack_frames_ex
 *   (exclusive offsets with the total in offs[i][nb]; a record that would pass `cap` is not
 *   written; totals, which may be NULL, stored at system scope).  A NULL required pointer or
 *   nb <= 0 is SO_E_INVALID; nframes = 0 is SO_OK.  Stream-ordered, no host synchronisation.
 * so_pack_chroma_frames_after / _bits_after: the same records placed behind bytes that are already
 *   in out[i] (a frame's luma stream), so that one buffer holds the frame's whole payload.
 *   base[i] points at one device uint32 -- typically the luma stream's offs[i] + nb, written by
 *   so_pack_frames_ex earlier on the same stream; it is read on the device by the write pass and
 *   never on the host.  Record b of frame i goes to out[i] + *base[i] + offs[i][b]; offs stays
 *   relative (the exclusive scan of the chroma record lengths, the chroma total in offs[i][nb]),
 *   so the unpackers and a container's chroma lengths read it unchanged.  A record is written
 *   only if *base[i] + offs[i][b+1] <= cap.  totals[i] = *base[i] + offs[i][nb] (may be NULL;
 *   stored at system scope).  Bytes before *base[i] and after the written records are not
 *   touched.  A NULL base or base[i] is SO_E_INVALID, as for the other required pointers.
 * so_unpack_chroma_frames / _bits: the inverse, as so_unpack_frames: every record decoded from
 *   exactly its bytes [offs[b], offs[b+1]) into the zeroed blocks; malformed input sets the
 *   device int32 *err to 1 + a bad record's index (zero it first); a bad record's outputs are
 *   unspecified.  Offsets that point outside packed[i]'s buffer are a caller precondition.
 */
size_t so_pack_chroma_bound(int nb);
size_t so_pack_chroma_bits_bound(int nb);
int so_pack_chroma_frames(int nframes, const int16_t* const* qtc_u, const int16_t* const* qtc_v,
                          int nb, uint32_t* const* offs, uint8_t* const* out,
                          unsigned long long cap, uint32_t* totals, void* stream);
int so_pack_chroma_frames_bits(int nframes, const int16_t* const* qtc_u,
                               const int16_t* const* qtc_v, int nb, uint32_t* const* offs,
                               uint8_t* const* out, unsigned long long cap, uint32_t* totals,
                               void* stream);
int so_pack_chroma_frames_after(int nframes, const int16_t* const* qtc_u,
                                const int16_t* const* qtc_v, int nb, uint32_t* const* offs,
                                uint8_t* const* out, const uint32_t* const* base,
                                unsigned long long cap, uint32_t* totals, void* stream);
int so_pack_chroma_frames_bits_after(int nframes, const int16_t* const* qtc_u,
                                     const int16_t* const* qtc_v, int nb, uint32_t* const* offs,
                                     uint8_t* const* out, const uint32_t* const* base,
                                     unsigned long long cap, uint32_t* totals, void* stream);
int so_unpack_chroma_frames(int nframes, const uint8_t* const* packed, const uint32_t* const* offs,
                            int nb, int16_t* const* qtc_u, int16_t* const* qtc_v, int32_t* err,
                            void* stream);
int so_unpack_chroma_frames_bits(int nframes, const uint8_t* const* packed,
                                 const uint32_t* const* offs, int nb, int16_t* const* qtc_u,
                                 int16_t* const* qtc_v, int32_t* err, void* stream);

/*
 * Both streams in the "huff" coding (so_packhuff.hip; container coding 3): the symbols of the
 * "bits" coding, in the same order, as canonical Huffman codes from tables built per frame.
 * Records stay byte-aligned, so the offsets, the totals, the capacity guard, the _after placement
 * and the parallel decode work as above.  The model is tests/packhuffref.py; host decoders:
 * bitstream.unpack_frame_huff / unpack_chroma_frame_huff.
 *
 * Bits are written MSB-first within each byte.
 * A value v (mv value, token or coefficient alike): z = zz(v), 0 <= z <= 65535.
 *   z < 32:   symbol z, no extra bits.
 *   else:     n = bit_length(z) (6..16); symbol 32 + n - 6, then the low n - 1 bits of z, raw.
 *   43 symbols.  Code lengths are 1..15 (0: the symbol is absent), so a code and its extra bits
 *   are at most 30 bits.
 * Contexts: cls(p) = min(bit_length(p), 6), p the scan position inside the (sub-)block: for a
 *   token the number of coefficients covered before it, for a coefficient its own position.
 *   Luma has 15 tables per frame, in this order: mv, tok0..tok6, coef0..coef6; chroma 14, shared by
 *   U and V: tok0..tok6, coef0..coef6.  An mv value is coded with table mv, a token with
 *   tok[cls(p)], a coefficient with coef[cls(p)].
 * One luma block: split, 1 raw bit; the mv values (the values and order of the other codings);
 *   each (sub-)block's token list ("-L" then L values, "Z", a trailing "0"); zero bits up to the
 *   next byte boundary.  There is no k field.
 * One chroma record: U's list, V's list (nn = 64), zero bits up to the next byte boundary.
 * Tables: codes are canonical -- ordered by (length, symbol), the first code of a length being
 *   (the previous length's first code + its number of codes) << 1, starting from 0 at length 1.
 *   A table is transmitted as its 43 lengths, 4 bits each, high nibble first; the frame's tables
 *   follow each other in the order above: 645 nibbles in 323 bytes for luma, 602 in 301 for chroma,
 *   the last nibble of the luma bytes 0.  They are the first bytes of record 0 of the frame:
 *   record 0 is the table bytes, then its codes; offs and the per-record lengths count them in.
 *   A decoder reads them from packed + offs[0] before any record.
 * Canonical lengths (what so_pack_frames_huff / so_pack_chroma_frames_huff write): Huffman's
 *   algorithm on the frame's symbol counts per table.  The nodes are numbered: the leaf of symbol
 *   s is node s, merged nodes are 43, 44, ... in the order they are made.  Each step removes the two
 *   smallest nodes by (weight, node number) and makes a node of their summed weight; only symbols
 *   with a non-zero count take part.  A symbol's length is its leaf's depth.  A table with one
 *   used symbol gives it length 1; unused symbols get 0.  If the longest code exceeds 15, every
 *   non-zero count c is replaced by (c + 1) >> 1 and the table is rebuilt, until it fits.
 * A decoder depends on the transmitted lengths only and accepts any table whose Kraft sum
 *   (the sum of 2^-length over the non-zero lengths) is <= 1.
 * Malformed to a decoder (so_unpack_frames_huff, so_unpack_chroma_frames_huff and the host
 *   decoders), besides the rules of the "bits" coding that still apply (a code running past the
 *   record's last byte; split = 1 at block size 8; the token rules; after the last list 8 or more
 *   bits left or a set bit among them; offs[b+1] < offs[b]):
 *   * a table whose Kraft sum exceeds 1, or a non-zero last nibble (luma), reported as record 0;
 *   * record 0 shorter than the table bytes, reported as record 0;
 *   * a bit pattern that matches no code of the table in force.
 *   When the tables are malformed no record of the frame is decoded.
 * Accepted though never written: lengths that are not the canonical ones; a 0 value inside a -L
 *   list; a zero run reaching exactly nn written as Z.
 *
 * so_pack_huff_bound(nb, bs) = nb * ceil((1 + 12*30 + 30*nn + 24*(nn/2 + 4)) / 8) + 323, nn = bs^2:
 *   the argument of so_pack_bits_bound value by value -- 12 mv values and nn coefficients of at
 *   most 30 bits, nn/2 + 4 tokens (|token| <= 256: a code and 9 extra bits) -- plus the table
 *   bytes.  0 for nb <= 0 or bs other than 8 or 16.  Record 0 at bs 16 is at most 1,725 bytes, so
 *   every length fits a container's u16.
 * so_pack_chroma_huff_bound(nb) = nb * ceil(2 * (30*64 + 22*36) / 8) + 301 = nb * 678 + 301.
 * so_pack_frames_huff, so_unpack_frames_huff, so_pack_chroma_frames_huff, _huff_after,
 *   so_unpack_chroma_frames_huff: arguments, behaviour and refusals of their _bits twins.  The
 *   packers take the frames' counters and tables from the device's stream-ordered memory pool
 *   and return them there: stream-ordered like everything else, no host synchronisation.  A
 *   frame's symbol counts must stay below 2^32 in total.
 * so_decode_p_frames / so_decode_chroma_frames do not take coding 3: a "huff" stream is decoded
 *   with the unpack entry points followed by the reconstruction entry points.
 */
size_t so_pack_huff_bound(int nb, int block_size);
int so_pack_frames_huff(int nframes, const int32_t* frame_types, const uint8_t* const* split,
                        const int16_t* const* mv, const int16_t* const* qtc, int nb, int block_size,
                        uint32_t* const* offs, uint8_t* const* out, unsigned long long cap,
                        uint32_t* totals, void* stream);
int so_unpack_frames_huff(int nframes, const int32_t* frame_types, const uint8_t* const* packed,
                          const uint32_t* const* offs, int nb, int block_size,
                          uint8_t* const* split, int16_t* const* mv, int16_t* const* qtc,
                          int32_t* err, void* stream);
size_t so_pack_chroma_huff_bound(int nb);
int so_pack_chroma_frames_huff(int nframes, const int16_t* const* qtc_u,
                               const int16_t* const* qtc_v, int nb, uint32_t* const* offs,
                               uint8_t* const* out, unsigned long long cap, uint32_t* totals,
                               void* stream);
int so_pack_chroma_frames_huff_after(int nframes, const int16_t* const* qtc_u,
                                     const int16_t* const* qtc_v, int nb, uint32_t* const* offs,
                                     uint8_t* const* out, const uint32_t* const* base,
                                     unsigned long long cap, uint32_t* totals, void* stream);
int so_unpack_chroma_frames_huff(int nframes, const uint8_t* const* packed,
                                 const uint32_t* const* offs, int nb, int16_t* const* qtc_u,
                                 int16_t* const* qtc_v, int32_t* err, void* stream);

/* ---- fused decode: packed records straight to pixels (so_decode.hip) -------------------------
 * The receiving side's hot path.  Both entry points compute exactly what the unpack entry points
 * followed by the reconstruction entry points compute, without the dense int16 coefficients in
 * global memory: a workgroup parses 64 records into LDS and transforms them from there.  All
 * pointer arrays (packed, offs, qp_row, qp_map, refs0*, split, mv, out_*) are HOST arrays of
 * device pointers; `coding` is the container's number: 1 varint (so_pack_frames), 2 bits
 * (so_pack_frames_bits).  One kernel launch per frame, enqueued in order on `stream`: stream order
 * carries the dependency of a frame on the reconstructions before it.  No host synchronisation.
 *
 * so_decode_p_frames: a run of nframes consecutive luma P-frames.  Frame i is decoded from
 *   packed[i] with the block offsets offs[i][0..nb] (nb = (H / bs) * (W / bs); the formats
 *   so_unpack_frames / so_unpack_frames_bits read, frame type 1) into out_split[i] (uint8 [nb]),
 *   out_mv[i] (int16 [nb][4][3], entries past the first of an unsplit block 0) and the plane
 *   out_recon[i] (uint8 [H][W]).  qp, and qp_row[i] (int32 [H / bs]) / qp_map[i] (int32 [nb]) as
 *   so_inter_recon_ex takes them; qp_row, qp_map or single entries may be NULL.
 *   Reference list of frame i: the last min(nref_max, nref0 + i) planes of refs0[0..nref0)
 *   followed by out_recon[0..i), oldest first -- the list decoder.decode_symbols hands to
 *   so_inter_recon_ex for that frame.
 *   Result: bit for bit that of so_unpack_frames(_bits) + so_inter_recon_ex(fme = 0) per frame,
 *   for block size 16 (split blocks included) and 8, any H, W that are multiples of bs.
 *   Malformed input: whatever so_unpack_frames(_bits) calls malformed, and -- new here -- a
 *   reference index outside [0, the frame's list length) in any motion vector the block uses (its
 *   first; all four when split).  A malformed block sets err[i] = 1 + its index (err: device int32
 *   [nframes], zeroed by the caller), its own pixels, split and mv are unspecified, and nothing is
 *   read or written outside the buffers given: the reference list is indexed only after the check,
 *   and dx / dy need none (every sample outside the plane's interior is bounded one by one).
 *   Every other block of the frame is decoded as usual, later frames run on whatever that left,
 *   and the call returns SO_OK: the caller reads err.  Offsets that point outside packed[i]'s
 *   buffer are a caller precondition, as for the unpack entry points.
 *   Before any launch: SO_E_UNSUPPORTED for a bs other than 16 / 8; SO_E_INVALID for nframes < 0, a
 *   coding other than 1 / 2, H or W not a positive multiple of bs, qp outside 0..20, nref_max
 *   outside 1..SO_MAX_REF, nref0 outside 1..nref_max, a NULL required pointer, an out_recon[i]
 *   that is not 16-byte aligned (out_mv[i]: 4-byte) or that aliases a refs0 plane or another
 *   out_recon.  nframes == 0 with valid scalars is SO_OK.
 *
 * so_decode_chroma_frames: U and V of a run of frames of either type (frame_types[i]: 0 intra,
 *   1 inter).  Frame i is decoded from its chroma records packed[i] / offs[i][0..nb] (the formats
 *   of so_unpack_chroma_frames / _bits) and the luma split[i] / mv[i] of the same frame --
 *   so_decode_p_frames' outputs, or an I-frame's unpacked ones; for a type-0 frame they are not
 *   read and may be NULL (as may split / mv themselves when no frame is type 1).  qp, qp_row,
 *   qp_map, qp_offset as so_chroma_recon_frame takes them.
 *   Reference lists (U and V alike), the rule of decoder._chroma_loop: they start as refs0_u /
 *   refs0_v[0..nref0); a P-frame predicts from the current list, an I-frame clears it first; every
 *   reconstruction is then appended, the oldest dropped when the list holds nref_max.  nref0 may
 *   be 0 only if frame 0 is type 0.
 *   Result: bit for bit that of so_unpack_chroma_frames(_bits) + so_chroma_recon_frame per frame.
 *   The reference index is clamped to the list, as so_chroma_recon_frame does.  A malformed record
 *   sets err[i] = 1 + its index; its two blocks are not written.
 *   Before any launch: SO_E_UNSUPPORTED for bs != 16; SO_E_INVALID as above, and for a frame type
 *   other than 0 / 1, qp_offset outside -20..20, nref0 outside 0..nref_max, a P-frame whose list
 *   is empty, planes that are not 8-byte aligned, an out_recon_u[i] equal to out_recon_v[i], or a
 *   reconstruction that aliases a refs0 plane or another reconstruction.
 *   so_decode_chroma_frames_ex adds mv_frac_bits as so_chroma_recon_frame_ex takes it (mv[i] then
 *   being the half-sample vectors of a luma frame decoded under FME); so_decode_chroma_frames
 *   forwards with 1 under its own name.  A value other than 1 / 2 is SO_E_INVALID, checked after bs.
 */
int so_decode_p_frames(int nframes, int coding, const uint8_t* const* packed,
                       const uint32_t* const* offs, int H, int W, int bs, int qp,
                       const int32_t* const* qp_row, const int32_t* const* qp_map,
                       const uint8_t* const* refs0, int nref0, int nref_max,
                       uint8_t* const* out_split, int16_t* const* out_mv, uint8_t* const* out_recon,
                       int32_t* err, void* stream);
int so_decode_chroma_frames(int nframes, int coding, const int32_t* frame_types,
                            const uint8_t* const* packed, const uint32_t* const* offs, int H, int W,
                            int bs, const uint8_t* const* split, const int16_t* const* mv, int qp,
                            const int32_t* const* qp_row, const int32_t* const* qp_map,
                            int qp_offset, const uint8_t* const* refs0_u,
                            const uint8_t* const* refs0_v, int nref0, int nref_max,
                            uint8_t* const* out_recon_u, uint8_t* const* out_recon_v, int32_t* err,
                            void* stream);
int so_decode_chroma_frames_ex(int nframes, int coding, const int32_t* frame_types,
                               const uint8_t* const* packed, const uint32_t* const* offs, int H, int W,
                               int bs, const uint8_t* const* split, const int16_t* const* mv, int qp,
                               const int32_t* const* qp_row, const int32_t* const* qp_map,
                               int qp_offset, const uint8_t* const* refs0_u,
                               const uint8_t* const* refs0_v, int nref0, int nref_max,
                               uint8_t* const* out_recon_u, uint8_t* const* out_recon_v, int32_t* err,
                               int mv_frac_bits, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STREAMOPTIMA_H */
