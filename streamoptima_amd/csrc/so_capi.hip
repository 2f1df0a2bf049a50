// so_capi.hip — the extern "C" boundary of libstreamoptima_hip.so (include/streamoptima.h).
// Argument validation, thread-local error text, launches; no device allocation, no host
// synchronisation (every entry point is capturable into a hipGraph).
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include <hip/hip_ext.h>

#include "so_chroma.h"
#include "so_colour.h"
#include "so_common.h"
#include "so_deblock.h"
#include "so_launch.h"
#include "so_packfmt.h"
#include "so_run.h"
#include "so_scale.h"

namespace so {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

// so_set_option / so_get_option (SO_OPT_*): index = option id
// SO_OPT_RUN_2PASS_FUSED on by default, SO_OPT_RUN_TALL_TILES unset (-1: chosen per launch)
static std::atomic<int> g_opt[9] = {0, 1, 0, 32, 32, 0, 0, 0, -1};

int option(int id) {
    return (id > 0 && id < 9) ? g_opt[id].load(std::memory_order_relaxed) : 0;
}

#ifdef SO_AB
// A/B builds only (not in the header): tools that set the SO_AB environment knobs
// (tools/ab_guard.py) check for this symbol, so a knob can never silently measure the default path
extern "C" int so_debug_ab_build(void) { return 1; }
#endif

// The fused search + transform tile kernel (so_me.hip p_tile_kernel) covers the headline
// configuration: bs 16, sr 16, full search, no VBS / FME, one reference.  SO_FUSED=0 or an
// SO_ME_IMPL A/B selection keeps the two-launch path (ME kernel + inter_tq_kernel).
static bool use_fused(int bs, int sr, int vbs, int nref) {
    if (bs != 16 || sr != 16 || vbs || nref != 1) return false;
#ifdef SO_AB   // A/B builds only
    const char* f = getenv("SO_FUSED");
    if (f && strcmp(f, "0") == 0) return false;
    const char* impl = getenv("SO_ME_IMPL");
    return impl == nullptr || impl[0] == 0;
#else
    return true;
#endif
}

// ---- validation ------------------------------------------------------------------------------
// VBSEnable flag and calculate_RD_cost's lambda (Encoder.py:1133-1158)
static int check_vbs(const char* fn, int vbs, double lam) {
    if (vbs != 0 && vbs != 1) {
        set_error("%s: vbs must be 0 or 1", fn);
        return SO_E_INVALID;
    }
    if (vbs && !(lam >= 0.0 && lam < 1e300)) {
        set_error("%s: lambda %g (VBSEnable needs a finite lambda >= 0)", fn, lam);
        return SO_E_INVALID;
    }
    return SO_OK;
}

static int check_geom(const char* fn, int H, int W, int bs, int vbs) {
    if (bs != 16 && bs != 8) {
        set_error("%s: block_size %d not built (gfx950 kernels exist for 16 and 8)", fn, bs);
        return SO_E_UNSUPPORTED;
    }
    if (vbs && bs != 16) {
        set_error("%s: VBSEnable needs block_size 16 (8x8 sub-blocks)", fn);
        return SO_E_UNSUPPORTED;
    }
    if (H <= 0 || W <= 0 || H % bs || W % bs) {
        set_error("%s: frame %dx%d must be a positive multiple of block_size %d (pad with pad_hw)", fn, W, H, bs);
        return SO_E_INVALID;
    }
    if ((long long)H * W > (1ll << 31)) {
        set_error("%s: frame too large", fn);
        return SO_E_INVALID;
    }
    return SO_OK;
}

static int check_sr(const char* fn, int sr) {
    if (sr < 0 || sr > 64) {
        set_error("%s: search_range %d outside [0, 64]", fn, sr);
        return SO_E_UNSUPPORTED;
    }
    return SO_OK;
}

static int check_intra_width(const char* fn, int W) {
    if (W > 8192) {   // intra_recon_kernel keeps one pixel row (12 B/px) in LDS
        set_error("%s: intra frames wider than 8192 px are not built", fn);
        return SO_E_UNSUPPORTED;
    }
    return SO_OK;
}

static int check_rows(const char* fn, int H, int bs, int by0, int by1) {
    if (by0 < 0 || by1 < by0 || by1 > H / bs) {
        set_error("%s: block-row range [%d, %d) outside [0, %d]", fn, by0, by1, H / bs);
        return SO_E_INVALID;
    }
    return SO_OK;
}

static int check_qp(const char* fn, int qp) {
    if (qp < 0 || qp > 20) {
        set_error("%s: Qp %d outside [0, 20]", fn, qp);
        return SO_E_INVALID;
    }
    return SO_OK;
}

static int make_refs(const char* fn, const uint8_t* const* refs, int nref, RefSet* rs) {
    if (refs == nullptr || nref < 1 || nref > kMaxRef) {
        set_error("%s: nref %d outside [1, %d]", fn, nref, kMaxRef);
        return SO_E_INVALID;
    }
    for (int i = 0; i < kMaxRef; ++i) rs->p[i] = i < nref ? refs[i] : refs[0];
    for (int i = 0; i < nref; ++i)
        if (!refs[i]) {
            set_error("%s: refs[%d] is NULL", fn, i);
            return SO_E_INVALID;
        }
    return SO_OK;
}

// after make_refs: the reconstruction may be none of the planes it is predicted from
static int check_recon_not_ref(const char* fn, const uint8_t* const* refs, int nref, const uint8_t* out_recon) {
    for (int i = 0; i < nref; ++i)
        if (refs[i] == out_recon) {
            set_error("%s: out_recon aliases refs[%d]", fn, i);
            return SO_E_INVALID;
        }
    return SO_OK;
}

static int check_qp_clamp(const char* fn, int qp_lo, int qp_hi) {
    if (qp_lo < 0 || qp_hi > 20 || qp_lo > qp_hi) {
        set_error("%s: QP clamp [%d, %d] outside [0, 20]", fn, qp_lo, qp_hi);
        return SO_E_INVALID;
    }
    return SO_OK;
}

// a HIP runtime call's status as an entry point's return code, with the runtime's own text
static int hip_status(const char* fn, hipError_t e) {
    if (e == hipSuccess) return SO_OK;
    set_error("%s: %s", fn, hipGetErrorString(e));
    return (int)e;
}

// ---- the persistent runs' shared checks (so_encode_p_run*, the frame pipeline) ----------------
// The scalar arguments.  The run kernels cover one configuration; `tail` is the caller's end of
// that sentence; a two-pass run is built for W <= 8192 only.
static int check_run(const char* fn, int H, int W, int bs, int sr, int qp_rd, int vbs, double lam, bool two_pass,
                     const char* tail) {
    SO_TRY(check_geom(fn, H, W, bs, vbs));
    SO_TRY(check_vbs(fn, vbs, lam));
    SO_TRY(check_sr(fn, sr));
    SO_TRY(check_qp(fn, qp_rd));
    if (bs != 16 || sr != 16 || W % 128 != 0 || (two_pass && W > 8192)) {
        set_error("%s: covers bs 16 / sr 16 / W %% 128 == 0%s", fn, tail);
        return SO_E_UNSUPPORTED;
    }
    return SO_OK;
}

// The arrays of per-frame pointers a run takes ([nframes] each; out_sse optional, out_qp_map
// two-pass runs only).
struct RunArrays {
    const uint8_t* const* curs;
    uint8_t* const* out_split;
    int16_t* const* out_mv;
    int16_t* const* out_qtc;
    int32_t* const* out_tokens;
    int32_t* const* out_mae_num;
    uint8_t* const* out_recon;
    int32_t* const* out_sse;
    int32_t* const* out_qp_map;
};

static int need_run_outputs(const char* fn, const RunArrays& a) {
    const auto& [curs, out_split, out_mv, out_qtc, out_tokens, out_mae_num, out_recon, out_sse, out_qp_map] = a;
    SO_NEED(out_split, fn); SO_NEED(out_mv, fn); SO_NEED(out_qtc, fn); SO_NEED(out_tokens, fn);
    SO_NEED(out_mae_num, fn); SO_NEED(out_recon, fn);
    return SO_OK;
}

// Frame by frame: no NULL entry, then the caller's own rule for frame i (`each`: aliasing,
// landing planes, dependencies), then the kernels' record of the frame's outputs.
template <class Each>
static int run_frames(const char* fn, const RunArrays& a, int nframes, std::vector<PFrameOut>* outs, Each each) {
    const auto& [curs, out_split, out_mv, out_qtc, out_tokens, out_mae_num, out_recon, out_sse, out_qp_map] = a;
    outs->resize((size_t)nframes);
    for (int i = 0; i < nframes; ++i) {
        SO_NEED(curs[i], fn); SO_NEED(out_split[i], fn); SO_NEED(out_mv[i], fn); SO_NEED(out_qtc[i], fn);
        SO_NEED(out_tokens[i], fn); SO_NEED(out_mae_num[i], fn); SO_NEED(out_recon[i], fn);
        if (out_qp_map) SO_NEED(out_qp_map[i], fn);
        SO_TRY(each(i));
        (*outs)[(size_t)i] = PFrameOut{out_split[i], out_mv[i], out_qtc[i], out_tokens[i], out_mae_num[i], out_recon[i],
                                       out_sse ? out_sse[i] : nullptr, out_qp_map ? out_qp_map[i] : nullptr};
    }
    return SO_OK;
}

// a chain from ref0: frame i's reconstruction is neither ref0 nor an earlier frame's
static int check_chain_alias(const char* fn, const uint8_t* ref0, uint8_t* const* out_recon, int i) {
    for (int j = -1; j < i; ++j)
        if (out_recon[i] == (j < 0 ? ref0 : out_recon[j])) {
            set_error("%s: out_recon[%d] aliases ref0 or another frame's reconstruction", fn, i);
            return SO_E_INVALID;
        }
    return SO_OK;
}

// ---- aliasing of pictures given as address spans (colour conversion, scaling) -----------------
struct Span {
    uintptr_t lo, hi;   // [lo, hi)
    bool dst;
    const char* what;
    int frame;
};

// A destination may share no byte with a source or another destination; sources may repeat.
// dst_vs_dst false leaves destination against destination to the caller (whose destinations may
// interleave inside one span).
static int check_spans(const char* fn, std::vector<Span>& spans, bool dst_vs_dst) {
    std::sort(spans.begin(), spans.end(), [](const Span& a, const Span& b) { return a.lo < b.lo; });
    // the furthest end so far of a source, of a destination, and which span it belongs to
    const Span *far_src = nullptr, *far_dst = nullptr;
    for (const Span& s : spans) {
        const Span* hit = nullptr;
        if (far_dst && s.lo < far_dst->hi && (!s.dst || dst_vs_dst)) hit = far_dst;
        if (!hit && s.dst && far_src && s.lo < far_src->hi) hit = far_src;
        if (hit) {
            set_error("%s: %s[%d] aliases %s[%d] (a destination overlaps a source or another destination)", fn,
                      s.what, s.frame, hit->what, hit->frame);
            return SO_E_INVALID;
        }
        const Span*& far = s.dst ? far_dst : far_src;
        if (!far || s.hi > far->hi) far = &s;
    }
    return SO_OK;
}

}  // namespace so

using namespace so;

extern "C" {

int so_abi_version(void) { return SO_ABI_VERSION; }

int so_set_option(int opt, int value) {
    const bool ok = (opt == SO_OPT_RUN_2PASS_FUSED || opt == SO_OPT_FASTME_SERIAL || opt == SO_OPT_COUNT_SAD_OPS ||
                     opt == SO_OPT_RUN_ZERO_SKIP)
                        ? (value == 0 || value == 1)
                    : opt == SO_OPT_RUN_TALL_TILES                               ? (value >= -1 && value <= 1)
                    : opt == SO_OPT_FASTME_SEGMENT                               ? value >= 1
                    : opt == SO_OPT_FASTME_WARMUP || opt == SO_OPT_TEST_LOSE_FLAG ? value >= 0
                                                                                 : false;
    if (!ok) {
        set_error("so_set_option: option %d value %d is unknown or out of range", opt, value);
        return SO_E_INVALID;
    }
    g_opt[opt].store(value, std::memory_order_relaxed);
    return SO_OK;
}

int so_get_option(int opt) { return option(opt); }

const char* so_last_error(void) { return g_err; }

int so_me_full_search(const uint8_t* cur, const uint8_t* const* refs, int nref, int H, int W, int bs,
                      int sr, int32_t* out_best, int32_t* out_sub, void* stream) {
    const char* fn = "so_me_full_search";
    SO_TRY(check_geom(fn, H, W, bs, out_sub != nullptr));
    SO_TRY(check_sr(fn, sr));
    SO_NEED(cur, fn);
    SO_NEED(out_best, fn);
    RefSet rs;
    SO_TRY(make_refs(fn, refs, nref, &rs));
    return me_launch(cur, rs, nref, H, W, bs, sr, 0, H / bs, out_best, out_sub, (hipStream_t)stream);
}

int so_inter_tq_recon(const uint8_t* cur, const uint8_t* const* refs, int nref, int H, int W, int bs,
                      const int32_t* best, const int32_t* sub, int qp_rd, const int32_t* qp_row, int vbs,
                      double lam, uint8_t* out_split, int16_t* out_mv, int16_t* out_qtc, int32_t* out_tokens,
                      int32_t* out_mae_num, uint8_t* out_recon, int32_t* out_sse, void* stream) {
    const char* fn = "so_inter_tq_recon";
    SO_TRY(check_geom(fn, H, W, bs, vbs));
    SO_TRY(check_qp(fn, qp_rd));
    SO_NEED(cur, fn); SO_NEED(best, fn); SO_NEED(out_split, fn); SO_NEED(out_mv, fn);
    SO_NEED(out_qtc, fn); SO_NEED(out_tokens, fn); SO_NEED(out_mae_num, fn); SO_NEED(out_recon, fn);
    if (vbs) SO_NEED(sub, fn);
    RefSet rs;
    SO_TRY(make_refs(fn, refs, nref, &rs));
    SO_TRY(check_recon_not_ref(fn, refs, nref, out_recon));
    return inter_tq_launch(cur, rs, nullptr, 0, H, W, bs, 0, H / bs, best, vbs ? sub : nullptr, qp_rd, qp_row, nullptr, vbs, lam,
                           out_split, out_mv, out_qtc, out_tokens, out_mae_num, out_recon, out_sse,
                           (hipStream_t)stream);
}

size_t so_p_frame_scratch_elems(int H, int W, int bs, int vbs) {
    if (bs <= 0) return 0;
    const size_t nb = (size_t)(W / bs) * (size_t)(H / bs);
    return nb * 4 + (vbs ? nb * 16 : 0) + kFastSegWords;
}

int so_encode_p_frame(const uint8_t* cur, const uint8_t* const* refs, int nref, int H, int W, int bs, int sr,
                      int qp_rd, const int32_t* qp_row, int vbs, double lam, uint8_t* out_split,
                      int16_t* out_mv, int16_t* out_qtc, int32_t* out_tokens, int32_t* out_mae_num,
                      uint8_t* out_recon, int32_t* out_sse, int32_t* scratch, void* stream) {
    if (bs <= 0) {
        set_error("so_encode_p_frame: block_size %d", bs);
        return SO_E_UNSUPPORTED;
    }
    return so_encode_p_rows(cur, refs, nref, H, W, bs, sr, 0, H / bs, qp_rd, qp_row, vbs, lam, out_split, out_mv,
                            out_qtc, out_tokens, out_mae_num, out_recon, out_sse, scratch, stream);
}

// ---- P-frame runs: one persistent launch (so_me.hip p_run_kernel) -----------------------
size_t so_p_run_workspace_elems(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    return p_run_workspace_words(H, W);
}

int so_p_run_resident_workgroups(int vbs) {
    const int n = p_run_capacity(vbs ? 1 : 0);
    if (n <= 0) {
        set_error("so_p_run_resident_workgroups: device query failed");
        return SO_E_INVALID;
    }
    return n;
}

int so_p_run_tile_rows(int H, int W, int conc) {
    if (H < 16 || W < 128 || H % 16 != 0 || W % 128 != 0 || conc < 1) {
        set_error("so_p_run_tile_rows: H %d W %d conc %d (H a multiple of 16, W of 128, conc >= 1)", H, W, conc);
        return SO_E_INVALID;
    }
    const int n = p_run_tile_rows(H, W, conc);
    if (n <= 0) {
        set_error("so_p_run_tile_rows: device query failed");
        return SO_E_INVALID;
    }
    return n;
}

int so_p_run_2pass_fused(int H, int W) {
    return H > 0 && W > 0 && option(SO_OPT_RUN_2PASS_FUSED) == 1 && p_run_2pass_fused_ok(H, W) ? 1 : 0;
}

int so_p_run_mode_resident_workgroups(int mode, int vbs) {
    if (mode < 0 || mode > 4 || (vbs && mode != 0 && mode != 2)) {
        set_error("so_p_run_mode_resident_workgroups: mode %d%s", mode, vbs ? " with vbs (modes 0, 2)" : " (0..4)");
        return SO_E_INVALID;
    }
    const int n = p_run_capacity(vbs ? 1 : 0, mode);
    if (n <= 0) {
        set_error("so_p_run_mode_resident_workgroups: device query failed");
        return SO_E_INVALID;
    }
    return n;
}

int so_encode_p_run(const uint8_t* const* curs, int nframes, const uint8_t* ref0, int H, int W, int bs, int sr,
                    int qp_rd, const int32_t* qp_row, int vbs, double lam, uint8_t* const* out_split,
                    int16_t* const* out_mv, int16_t* const* out_qtc, int32_t* const* out_tokens,
                    int32_t* const* out_mae_num, uint8_t* const* out_recon, int32_t* const* out_sse,
                    uint32_t* workspace, void* stream) {
    const char* fn = "so_encode_p_run";
    SO_TRY(check_run(fn, H, W, bs, sr, qp_rd, vbs, lam, false, " (call so_encode_p_frame per frame)"));
    if (nframes <= 0) return SO_OK;
    const RunArrays a{curs, out_split, out_mv, out_qtc, out_tokens, out_mae_num, out_recon, out_sse, nullptr};
    SO_NEED(curs, fn); SO_NEED(ref0, fn);
    SO_TRY(need_run_outputs(fn, a));
    SO_NEED(workspace, fn);
    std::vector<PFrameOut> outs;
    SO_TRY(run_frames(fn, a, nframes, &outs, [&](int i) { return check_chain_alias(fn, ref0, out_recon, i); }));
    return p_run_launch(curs, nframes, ref0, H, W, qp_rd, qp_row, vbs, lam, outs.data(), workspace,
                        (hipStream_t)stream);
}

int so_encode_p_runs(const uint8_t* const* curs, int nframes, const uint8_t* const* refs, const int32_t* ref_frame,
                     int H, int W, int bs, int sr, int qp_rd, const int32_t* qp_row, int vbs, double lam,
                     uint8_t* const* out_split, int16_t* const* out_mv, int16_t* const* out_qtc,
                     int32_t* const* out_tokens, int32_t* const* out_mae_num, uint8_t* const* out_recon,
                     int32_t* const* out_sse, uint32_t* workspace, void* stream) {
    const char* fn = "so_encode_p_runs";
    SO_TRY(check_run(fn, H, W, bs, sr, qp_rd, vbs, lam, false, " (call so_encode_p_frame per frame)"));
    if (nframes <= 0) return SO_OK;
    const RunArrays a{curs, out_split, out_mv, out_qtc, out_tokens, out_mae_num, out_recon, out_sse, nullptr};
    SO_NEED(curs, fn); SO_NEED(refs, fn); SO_NEED(ref_frame, fn);
    SO_TRY(need_run_outputs(fn, a));
    SO_NEED(workspace, fn);
    std::vector<PFrameOut> outs;
    std::vector<int> deps((size_t)nframes);
    int conc = 0;   // runs starting from a plane outside the list: interleaved chains
    SO_TRY(run_frames(fn, a, nframes, &outs, [&](int i) {
        const int d = ref_frame[i];
        if (d >= i || d < -1) {
            set_error("%s: ref_frame[%d] = %d (must be -1 or an earlier frame of the list)", fn, i, d);
            return SO_E_INVALID;
        }
        if (d < 0) {
            SO_NEED(refs[i], fn);
            ++conc;
        }
        deps[(size_t)i] = d;
        for (int j = 0; j < nframes; ++j)
            if ((j != i && out_recon[i] == out_recon[j]) || (ref_frame[j] < 0 && out_recon[i] == refs[j])) {
                set_error("%s: out_recon[%d] aliases a reference plane or another frame's reconstruction", fn, i);
                return SO_E_INVALID;
            }
        return SO_OK;
    }));
    return p_runs_launch(curs, nframes, refs, deps.data(), conc, H, W, qp_rd, qp_row, vbs, lam, outs.data(), workspace,
                         (hipStream_t)stream);
}

int so_encode_p_run_2pass(const uint8_t* const* curs, int nframes, const uint8_t* ref0, int H, int W, int bs, int sr,
                          int qp_rd, const int32_t* qp_row, const int32_t* roi, int qp_lo, int qp_hi,
                          uint8_t* const* out_split, int16_t* const* out_mv, int16_t* const* out_qtc,
                          int32_t* const* out_tokens, int32_t* const* out_mae_num, uint8_t* const* out_recon,
                          int32_t* const* out_sse, int32_t* const* out_qp_map, uint32_t* workspace, void* stream) {
    const char* fn = "so_encode_p_run_2pass";
    SO_TRY(check_run(fn, H, W, bs, sr, qp_rd, 0, 0.0, true, ", W <= 8192 (encode per frame otherwise)"));
    SO_TRY(check_qp_clamp(fn, qp_lo, qp_hi));
    if (nframes <= 0) return SO_OK;
    const RunArrays a{curs, out_split, out_mv, out_qtc, out_tokens, out_mae_num, out_recon, out_sse, out_qp_map};
    SO_NEED(curs, fn); SO_NEED(ref0, fn);
    SO_TRY(need_run_outputs(fn, a));
    SO_NEED(out_qp_map, fn); SO_NEED(workspace, fn);
    std::vector<PFrameOut> outs;
    SO_TRY(run_frames(fn, a, nframes, &outs, [&](int i) { return check_chain_alias(fn, ref0, out_recon, i); }));
    hipStream_t st = (hipStream_t)stream;
    // default: both passes of every frame in one persistent launch (each task the pass 2 of one
    // tile and the pass 1 of another), for frames of three tile rows or
    // more; otherwise, or with SO_OPT_RUN_2PASS_FUSED = 0, the per-frame sequence below
    if (so_p_run_2pass_fused(H, W))
        return p_run_2pass_launch(curs, nframes, ref0, H, W, qp_rd, qp_row, roi, qp_lo, qp_hi, outs.data(), workspace,
                                  st);
    // per frame, pass 1 (fused search + tokens only) and pass 2 (the QP map from pass 1's token
    // counts, then the transforms on pass 1's ME records, kept in the workspace), enqueued from
    // here with no host round trip per frame
    // the workspace's pass-1 region (kRunMax >= 5 blocks' words per block): the ME records
    // (4 words per block), then the pass-1 token counts (1 word per block)
    int32_t* best = p_run_t1_region(workspace, H, W);
    const int nbx = W / 16, nby = H / 16;
    int32_t* t1 = best + (size_t)4 * nbx * nby;
    static_assert(kRunMax >= 5, "the pass-1 region holds 4 + 1 words per block");
    for (int i = 0; i < nframes; ++i) {
        RefSet rs{};
        rs.p[0] = i ? out_recon[i - 1] : ref0;
        const PFrameOut& o = outs[(size_t)i];
        // pass 1 with the previous frame's (final) motion records as the search's U hint
        SO_TRY(p_tile_launch(curs[i], rs, H, W, 0, nby, qp_rd, qp_row, nullptr, best, o.split, o.mv, o.qtc, t1,
                             o.mae, o.recon, o.sse, st, true, i ? out_mv[i - 1] : nullptr));
        // pass 2 derives the QP map from the pass-1 tokens itself (qp_map_kernel's rule) and
        // stores it: no separate QP-map launch per frame
        SO_TRY(inter_tq_2pass_launch(curs[i], rs, H, W, best, t1, qp_rd, qp_row, roi, qp_lo, qp_hi, o.qpmap, o.split,
                                     o.mv, o.qtc, o.tokens, o.mae, o.recon, o.sse, st));
    }
    return SO_OK;
}

// ---- one GOP across GPUs: a rank's stripe of every frame (so_me.hip PRunStripe) -------------
int so_encode_p_run_stripe(const uint8_t* const* curs, int nframes, const uint8_t* ref0, int H, int W, int bs, int sr,
                           int by0, int by1, int qp_rd, const int32_t* qp_row, uint8_t* const* out_split,
                           int16_t* const* out_mv, int16_t* const* out_qtc, int32_t* const* out_tokens,
                           int32_t* const* out_mae_num, uint8_t* const* out_recon, int32_t* const* out_sse,
                           uint32_t* workspace, int gbase, uint8_t* peer_up0, uint8_t* peer_dn0, long long stride,
                           const uint32_t* my_up_flags, const uint32_t* my_dn_flags, uint32_t* peer_up_flags,
                           uint32_t* peer_dn_flags, uint32_t epoch, int max_wg, void* stream) {
    const char* fn = "so_encode_p_run_stripe";
    SO_TRY(check_run(fn, H, W, bs, sr, qp_rd, 0, 0.0, false, ""));
    if (by0 < 0 || by1 > H / 16 || by1 <= by0 || gbase < 1) {
        set_error("%s: bad stripe [%d, %d) of %d block rows or gbase %d", fn, by0, by1, H / 16, gbase);
        return SO_E_INVALID;
    }
    if ((peer_up0 != nullptr) != (peer_up_flags != nullptr) || (peer_dn0 != nullptr) != (peer_dn_flags != nullptr) ||
        (peer_up0 != nullptr) != (my_up_flags != nullptr) || (peer_dn0 != nullptr) != (my_dn_flags != nullptr) ||
        (peer_up0 && by0 == 0) || (peer_dn0 && by1 == H / 16)) {
        set_error("%s: a neighbour needs its plane, its flags and mine, and none past the frame edge", fn);
        return SO_E_INVALID;
    }
    if (nframes <= 0) return SO_OK;
    const RunArrays a{curs, out_split, out_mv, out_qtc, out_tokens, out_mae_num, out_recon, out_sse, nullptr};
    SO_NEED(curs, fn); SO_NEED(ref0, fn);
    SO_TRY(need_run_outputs(fn, a));
    SO_NEED(workspace, fn);
    std::vector<PFrameOut> outs;
    SO_TRY(run_frames(fn, a, nframes, &outs, [](int) { return SO_OK; }));
    PRunStripe sp{by0, by1, peer_up0, peer_dn0, stride, my_up_flags, my_dn_flags, peer_up_flags, peer_dn_flags,
                  epoch, gbase, nullptr};
    return p_run_stripe_launch(curs, nframes, ref0, H, W, qp_rd, qp_row, outs.data(), workspace, sp, max_wg,
                               (hipStream_t)stream);
}

int so_stripe_halo_push(const uint8_t* plane, int H, int W, int by0, int by1, int gf, uint8_t* peer_up,
                        uint8_t* peer_dn, uint32_t* peer_up_flags, uint32_t* peer_dn_flags, uint32_t epoch,
                        void* stream) {
    const char* fn = "so_stripe_halo_push";
    SO_TRY(check_geom(fn, H, W, 16, 0));
    if (W % 128 != 0 || by0 < 0 || by1 > H / 16 || by1 <= by0 || gf < 0 || by1 - by0 < 1) {
        set_error("%s: bad stripe [%d, %d) / frame %d", fn, by0, by1, gf);
        return SO_E_INVALID;
    }
    if ((peer_up != nullptr) != (peer_up_flags != nullptr) || (peer_dn != nullptr) != (peer_dn_flags != nullptr)) {
        set_error("%s: a neighbour plane needs its flags", fn);
        return SO_E_INVALID;
    }
    SO_NEED(plane, fn);
    if (!peer_up && !peer_dn) return SO_OK;
    return stripe_halo_push_launch(plane, W, by0, by1, peer_up, peer_dn, peer_up_flags, peer_dn_flags, gf, epoch,
                                   (hipStream_t)stream);
}

// ---- one GOP across GPUs: consecutive frames on consecutive ranks (so_me.hip kRunFPipe) -----
// The frame pipeline's argument checks and launch, with (two_pass) or without two-pass RC.
static int fpipe_run(const char* fn, bool two_pass, const uint8_t* const* curs, int nframes, int H, int W, int bs,
                     int sr, int qp_rd, const int32_t* qp_row, int vbs, double lam, const int32_t* roi, int qp_lo,
                     int qp_hi,
                     uint8_t* const* out_split, int16_t* const* out_mv, int16_t* const* out_qtc,
                     int32_t* const* out_tokens, int32_t* const* out_mae_num, uint8_t* const* out_recon,
                     int32_t* const* out_sse, int32_t* const* out_qp_map, uint32_t* workspace, const uint8_t* land0,
                     const uint32_t* land_flags, int slot0, uint8_t* peer_land0, uint32_t* peer_flags,
                     uint8_t* peer2_land0, uint32_t* peer2_flags, const int32_t* push_to, int nslots, long long stride,
                     uint32_t epoch, int max_wg, int p2lag, void* stream) {
    // two-pass RC with VBSEnable is not built for the frame pipeline: its entry point takes no vbs
    SO_TRY(check_run(fn, H, W, bs, sr, qp_rd, vbs, lam, two_pass, two_pass ? ", W <= 8192" : ""));
    if (two_pass) SO_TRY(check_qp_clamp(fn, qp_lo, qp_hi));
    // every rank owns `nslots` landing slots: this run reads slots [slot0, slot0 + nframes) and
    // writes (system scope, over xGMI) only slots below nslots of its peers
    if (p2lag < 0) {
        set_error("%s: p2lag %d < 0", fn, p2lag);
        return SO_E_INVALID;
    }
    if (slot0 < 0 || nslots < 1 || slot0 + nframes > nslots || stride < (long long)H * W) {
        set_error("%s: slot0 %d + %d frames / nslots %d / stride %lld", fn, slot0, nframes, nslots, stride);
        return SO_E_INVALID;
    }
    if (nframes <= 0) return SO_OK;
    const RunArrays a{curs, out_split, out_mv, out_qtc, out_tokens, out_mae_num, out_recon, out_sse,
                      two_pass ? out_qp_map : nullptr};
    SO_NEED(curs, fn);
    SO_TRY(need_run_outputs(fn, a));
    SO_NEED(workspace, fn); SO_NEED(land0, fn);
    SO_NEED(land_flags, fn); SO_NEED(peer_land0, fn); SO_NEED(peer_flags, fn); SO_NEED(peer2_land0, fn);
    SO_NEED(peer2_flags, fn); SO_NEED(push_to, fn);
    if (two_pass) SO_NEED(out_qp_map, fn);
    std::vector<PFrameOut> outs;
    std::vector<int> push((size_t)nframes);
    const uint8_t* land_end = land0 + (long long)(slot0 + nframes) * stride;
    SO_TRY(run_frames(fn, a, nframes, &outs, [&](int i) {
        if (out_recon[i] >= land0 && out_recon[i] < land_end) {
            set_error("%s: out_recon[%d] lies in the landing planes", fn, i);
            return SO_E_INVALID;
        }
        if (push_to[i] < -1 || (push_to[i] >> 1) >= nslots) {   // -1: nothing follows, no push
            set_error("%s: push_to[%d] = %d (nslots %d)", fn, i, push_to[i], nslots);
            return SO_E_INVALID;
        }
        push[(size_t)i] = push_to[i];
        return SO_OK;
    }));
    PRunStripe sp{0, H / 16, peer2_land0, peer_land0, stride, nullptr, land_flags, peer2_flags, peer_flags,
                  epoch, slot0, land0};
    if (two_pass) {
        sp.roi = roi;
        sp.qp_lo = qp_lo;
        sp.qp_hi = qp_hi;
        sp.p2lag = p2lag;
        return p_run_fpipe_2pass_launch(curs, nframes, H, W, qp_rd, qp_row, outs.data(), workspace, sp, max_wg,
                                        (hipStream_t)stream, push.data());
    }
    return p_run_fpipe_launch(curs, nframes, H, W, qp_rd, qp_row, vbs, lam, outs.data(), workspace, sp, max_wg,
                              (hipStream_t)stream, push.data());
}

int so_encode_p_run_fpipe2(const uint8_t* const* curs, int nframes, int H, int W, int bs, int sr, int qp_rd,
                           const int32_t* qp_row, int vbs, double lam, uint8_t* const* out_split, int16_t* const* out_mv,
                           int16_t* const* out_qtc, int32_t* const* out_tokens, int32_t* const* out_mae_num,
                           uint8_t* const* out_recon, int32_t* const* out_sse, uint32_t* workspace,
                           const uint8_t* land0, const uint32_t* land_flags, int slot0, uint8_t* peer_land0,
                           uint32_t* peer_flags, uint8_t* peer2_land0, uint32_t* peer2_flags, const int32_t* push_to,
                           int nslots, long long stride, uint32_t epoch, int max_wg, void* stream) {
    return fpipe_run("so_encode_p_run_fpipe2", false, curs, nframes, H, W, bs, sr, qp_rd, qp_row, vbs, lam, nullptr, 0, 0,
                     out_split, out_mv, out_qtc, out_tokens, out_mae_num, out_recon, out_sse, nullptr, workspace, land0,
                     land_flags, slot0, peer_land0, peer_flags, peer2_land0, peer2_flags, push_to, nslots, stride, epoch,
                     max_wg, 0, stream);
}

int so_encode_p_run_fpipe_2pass(const uint8_t* const* curs, int nframes, int H, int W, int bs, int sr, int qp_rd,
                                const int32_t* qp_row, const int32_t* roi, int qp_lo, int qp_hi,
                                uint8_t* const* out_split, int16_t* const* out_mv, int16_t* const* out_qtc,
                                int32_t* const* out_tokens, int32_t* const* out_mae_num, uint8_t* const* out_recon,
                                int32_t* const* out_sse, int32_t* const* out_qp_map, uint32_t* workspace,
                                const uint8_t* land0, const uint32_t* land_flags, int slot0, uint8_t* peer_land0,
                                uint32_t* peer_flags, uint8_t* peer2_land0, uint32_t* peer2_flags,
                                const int32_t* push_to, int nslots, long long stride, uint32_t epoch, int max_wg,
                                int p2lag, void* stream) {
    return fpipe_run("so_encode_p_run_fpipe_2pass", true, curs, nframes, H, W, bs, sr, qp_rd, qp_row, 0, 0.0, roi, qp_lo,
                     qp_hi,
                     out_split, out_mv, out_qtc, out_tokens, out_mae_num, out_recon, out_sse, out_qp_map, workspace,
                     land0, land_flags, slot0, peer_land0, peer_flags, peer2_land0, peer2_flags, push_to, nslots, stride,
                     epoch, max_wg, p2lag, stream);
}

int so_frame_push(const uint8_t* plane, int H, int W, uint8_t* peer_plane, uint32_t* peer_flags, uint32_t epoch,
                  void* stream) {
    const char* fn = "so_frame_push";
    SO_TRY(check_geom(fn, H, W, 16, 0));
    if (W % 128 != 0) {
        set_error("%s: W %% 128 != 0", fn);
        return SO_E_UNSUPPORTED;
    }
    SO_NEED(plane, fn); SO_NEED(peer_plane, fn); SO_NEED(peer_flags, fn);
    return frame_push_launch(plane, H, W, peer_plane, peer_flags, epoch, (hipStream_t)stream);
}

// ---- memory the ranks share (uncached landing planes, IPC) ----------------------------------
int so_alloc_uncached(size_t bytes, void** out) {
    if (!out || bytes == 0) {
        set_error("so_alloc_uncached: bad arguments");
        return SO_E_INVALID;
    }
    const hipError_t e = hipExtMallocWithFlags(out, bytes, hipDeviceMallocUncached);
    if (e != hipSuccess) {
        set_error("so_alloc_uncached(%zu): %s", bytes, hipGetErrorString(e));
        return (int)e;
    }
    return SO_OK;
}

int so_free_device(void* p) {
    return hip_status("so_free_device", hipFree(p));
}

int so_ipc_export(void* p, uint8_t* out_handle) {
    static_assert(sizeof(hipIpcMemHandle_t) <= SO_IPC_HANDLE_BYTES, "IPC handle size");
    if (!p || !out_handle) {
        set_error("so_ipc_export: bad arguments");
        return SO_E_INVALID;
    }
    hipIpcMemHandle_t h;
    SO_TRY(hip_status("so_ipc_export", hipIpcGetMemHandle(&h, p)));
    memset(out_handle, 0, SO_IPC_HANDLE_BYTES);
    memcpy(out_handle, &h, sizeof(h));
    return SO_OK;
}

int so_ipc_open(const uint8_t* handle, void** out) {
    if (!handle || !out) {
        set_error("so_ipc_open: bad arguments");
        return SO_E_INVALID;
    }
    hipIpcMemHandle_t h;
    memcpy(&h, handle, sizeof(h));
    return hip_status("so_ipc_open", hipIpcOpenMemHandle(out, h, hipIpcMemLazyEnablePeerAccess));
}

int so_copy_d2d(void* dst, const void* src, size_t bytes, void* stream) {
    if ((!dst || !src) && bytes) {
        set_error("so_copy_d2d: bad arguments");
        return SO_E_INVALID;
    }
    return hip_status("so_copy_d2d", hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
}

int so_memset_d8(void* dst, int value, size_t bytes, void* stream) {
    return hip_status("so_memset_d8", hipMemsetAsync(dst, value, bytes, (hipStream_t)stream));
}

int so_ipc_close(void* p) {
    return hip_status("so_ipc_close", hipIpcCloseMemHandle(p));
}

size_t so_i_frame_scratch_elems(int H, int W, int bs) {
    if (bs <= 0) return 0;
    const size_t nb = (size_t)(W / bs) * (size_t)(H / bs);
    return nb * (size_t)bs * bs + nb * 8;
}

// ---- the base entry points and their _ex forms (per-block QP map, ME variants, FME) ---------
static int i_rows(const char* fn, const uint8_t* cur, int H, int W, int bs, int sr, int by0, int by1, int qp_rd,
                  const int32_t* qp_row, const int32_t* qp_map, int vbs, double lam, uint8_t* out_split,
                  int16_t* out_mv, int16_t* out_qtc, int32_t* out_tokens, int32_t* out_mae_num, uint8_t* out_recon,
                  int32_t* out_sse, int32_t* scratch, void* stream) {
    SO_TRY(check_geom(fn, H, W, bs, vbs));
    SO_TRY(check_intra_width(fn, W));
    SO_TRY(check_sr(fn, sr));
    SO_TRY(check_qp(fn, qp_rd));
    SO_TRY(check_rows(fn, H, bs, by0, by1));
    SO_NEED(cur, fn); SO_NEED(out_split, fn); SO_NEED(out_mv, fn); SO_NEED(out_qtc, fn);
    SO_NEED(out_tokens, fn); SO_NEED(out_mae_num, fn); SO_NEED(out_recon, fn); SO_NEED(scratch, fn);
    return intra_encode_launch(cur, H, W, bs, sr, by0, by1, qp_rd, qp_row, qp_map, vbs, lam, out_split, out_mv,
                               out_qtc, out_tokens, out_mae_num, out_recon, out_sse, reinterpret_cast<uint8_t*>(scratch),
                               (hipStream_t)stream);
}

int so_encode_i_rows(const uint8_t* cur, int H, int W, int bs, int sr, int by0, int by1, int qp_rd,
                     const int32_t* qp_row, int vbs, double lam, uint8_t* out_split, int16_t* out_mv,
                     int16_t* out_qtc, int32_t* out_tokens, int32_t* out_mae_num, uint8_t* out_recon,
                     int32_t* out_sse, int32_t* scratch, void* stream) {
    return i_rows("so_encode_i_rows", cur, H, W, bs, sr, by0, by1, qp_rd, qp_row, nullptr, vbs, lam, out_split, out_mv,
                  out_qtc, out_tokens, out_mae_num, out_recon, out_sse, scratch, stream);
}

int so_encode_i_rows_ex(const uint8_t* cur, int H, int W, int bs, int sr, int by0, int by1, int qp_rd,
                        const int32_t* qp_row, const int32_t* qp_map, int vbs, double lam, uint8_t* out_split,
                        int16_t* out_mv, int16_t* out_qtc, int32_t* out_tokens, int32_t* out_mae_num,
                        uint8_t* out_recon, int32_t* out_sse, int32_t* scratch, void* stream) {
    return i_rows("so_encode_i_rows_ex", cur, H, W, bs, sr, by0, by1, qp_rd, qp_row, qp_map, vbs, lam, out_split,
                  out_mv, out_qtc, out_tokens, out_mae_num, out_recon, out_sse, scratch, stream);
}

int so_encode_i_frame(const uint8_t* cur, int H, int W, int bs, int sr, int qp_rd, const int32_t* qp_row,
                      int vbs, double lam, uint8_t* out_split, int16_t* out_mv, int16_t* out_qtc,
                      int32_t* out_tokens, int32_t* out_mae_num, uint8_t* out_recon, int32_t* out_sse,
                      int32_t* scratch, void* stream) {
    if (bs <= 0) {
        set_error("so_encode_i_frame: block_size %d", bs);
        return SO_E_UNSUPPORTED;
    }
    return so_encode_i_rows(cur, H, W, bs, sr, 0, H / bs, qp_rd, qp_row, vbs, lam, out_split, out_mv, out_qtc,
                            out_tokens, out_mae_num, out_recon, out_sse, scratch, stream);
}

static int inter_recon(const char* fn, const uint8_t* const* refs, int nref, int H, int W, int bs, int qp,
                       const int32_t* qp_row, const int32_t* qp_map, int fme, int fme_wrap, uint8_t* fme_planes,
                       const uint8_t* split, const int16_t* mv, const int16_t* qtc, uint8_t* out_recon, void* stream) {
    SO_TRY(check_geom(fn, H, W, bs, 0));
    SO_TRY(check_qp(fn, qp));
    SO_NEED(split, fn); SO_NEED(mv, fn); SO_NEED(qtc, fn); SO_NEED(out_recon, fn);
    if (fme) SO_NEED(fme_planes, fn);
    RefSet rs;
    SO_TRY(make_refs(fn, refs, nref, &rs));
    const size_t ps = so_fme_plane_stride(H, W);   // read by the FME kernels only
    hipStream_t st = (hipStream_t)stream;
    if (fme)
        for (int r = 0; r < nref; ++r)
            SO_TRY(fme_planes_launch(refs[r], H, W, fme_wrap, fme_planes + (size_t)r * 4 * ps, ps, st));
    return inter_recon_launch(rs, fme ? fme_planes : nullptr, ps, H, W, bs, qp, qp_row, qp_map, split, mv, qtc,
                              out_recon, st);
}

int so_inter_recon(const uint8_t* const* refs, int nref, int H, int W, int bs, int qp, const int32_t* qp_row,
                   const uint8_t* split, const int16_t* mv, const int16_t* qtc, uint8_t* out_recon, void* stream) {
    return inter_recon("so_inter_recon", refs, nref, H, W, bs, qp, qp_row, nullptr, 0, 0, nullptr, split, mv, qtc,
                       out_recon, stream);
}

int so_inter_recon_ex(const uint8_t* const* refs, int nref, int H, int W, int bs, int qp, const int32_t* qp_row,
                      const int32_t* qp_map, int fme, int fme_wrap, uint8_t* fme_planes, const uint8_t* split, const int16_t* mv,
                      const int16_t* qtc, uint8_t* out_recon, void* stream) {
    return inter_recon("so_inter_recon_ex", refs, nref, H, W, bs, qp, qp_row, qp_map, fme, fme_wrap, fme_planes, split,
                       mv, qtc, out_recon, stream);
}

static int intra_recon(const char* fn, int H, int W, int bs, int qp, const int32_t* qp_row, const int32_t* qp_map,
                       const uint8_t* split, const int16_t* mv, const int16_t* qtc, uint8_t* out_recon,
                       int32_t* scratch, void* stream) {
    SO_TRY(check_geom(fn, H, W, bs, 0));
    SO_TRY(check_intra_width(fn, W));
    SO_TRY(check_qp(fn, qp));
    SO_NEED(split, fn); SO_NEED(mv, fn); SO_NEED(qtc, fn); SO_NEED(out_recon, fn); SO_NEED(scratch, fn);
    // the recon kernel only needs sr to size its ring: the largest reachable offset is 64
    return intra_recon_launch(H, W, bs, 64, qp, qp_row, qp_map, split, mv, qtc, out_recon,
                              reinterpret_cast<uint8_t*>(scratch), (hipStream_t)stream);
}

int so_intra_recon(int H, int W, int bs, int qp, const int32_t* qp_row, const uint8_t* split, const int16_t* mv,
                   const int16_t* qtc, uint8_t* out_recon, int32_t* scratch, void* stream) {
    return intra_recon("so_intra_recon", H, W, bs, qp, qp_row, nullptr, split, mv, qtc, out_recon, scratch, stream);
}

int so_intra_recon_ex(int H, int W, int bs, int qp, const int32_t* qp_row, const int32_t* qp_map,
                      const uint8_t* split, const int16_t* mv, const int16_t* qtc, uint8_t* out_recon,
                      int32_t* scratch, void* stream) {
    return intra_recon("so_intra_recon_ex", H, W, bs, qp, qp_row, qp_map, split, mv, qtc, out_recon, scratch, stream);
}

size_t so_fme_plane_stride(int H, int W) {
    if (H <= 0 || W <= 0) return 0;
    return (((size_t)H * W + 64) + 255) & ~(size_t)255;   // 64 B of slack for aligned row reads
}

size_t so_fme_workspace_bytes(int H, int W, int nref) {
    return nref <= 0 ? 0 : (size_t)nref * 4 * so_fme_plane_stride(H, W);
}

int so_fme_planes(const uint8_t* ref, int H, int W, int wrap, uint8_t* out_planes, void* stream) {
    const char* fn = "so_fme_planes";
    SO_NEED(ref, fn); SO_NEED(out_planes, fn);
    if (H <= 1 || W <= 1 || W % 4) {
        set_error("%s: frame %dx%d (W must be a multiple of 4)", fn, W, H);
        return SO_E_INVALID;
    }
    return fme_planes_launch(ref, H, W, wrap, out_planes, so_fme_plane_stride(H, W), (hipStream_t)stream);
}

// shared validation + dispatch of the ME variants into best / sub
static int me_ex(const char* fn, const uint8_t* cur, const uint8_t* const* refs, int nref, const RefSet& rs, int H,
                 int W, int bs, int sr, int by0, int by1, int me_mode, int fme, int fme_wrap, uint8_t* planes,
                 int32_t* best, int32_t* sub, hipStream_t st, int32_t* seg_ws = nullptr) {
    if (me_mode < SO_ME_FULL || me_mode > SO_ME_FAST_PAR) {
        set_error("%s: me_mode %d", fn, me_mode);
        return SO_E_INVALID;
    }
    if (me_mode == SO_ME_FAST_PAR && sub) {
        set_error("%s: fast_me under ParallelMode 2 with VBSEnable (the reference raises NameError, "
                  "Encoder.py:609)", fn);
        return SO_E_UNSUPPORTED;
    }
    if (me_mode == SO_ME_FAST && by0 != 0) {
        set_error("%s: fast_me's predictor chain runs over the whole frame (no stripes)", fn);
        return SO_E_UNSUPPORTED;
    }
    const size_t ps = so_fme_plane_stride(H, W);
    if (fme) {
        SO_NEED(planes, fn);
        if (me_mode == SO_ME_FULL && sr > 63) {
            set_error("%s: FME search_range %d > 63", fn, sr);
            return SO_E_UNSUPPORTED;
        }
        for (int r = 0; r < nref; ++r)
            SO_TRY(fme_planes_launch(refs[r], H, W, fme_wrap, planes + (size_t)r * 4 * ps, ps, st));
    }
    if (me_mode == SO_ME_FULL) {
        if (!fme) return me_launch(cur, rs, nref, H, W, bs, sr, by0, by1, best, sub, st);
        if (bs == 16 && sr == 16) return me_fme_launch(cur, planes, ps, nref, H, W, by0, by1, best, sub, st);
        return me_generic_launch(cur, rs, planes, ps, nref, H, W, bs, sr, by0, by1, best, sub, st);
    }
    const uint8_t* ptrs[4 * kMaxRef];
    const int nfast = me_mode == SO_ME_FAST_PAR ? 1 : nref;
    int nptr = 0;
    for (int r = 0; r < nfast; ++r) {
        if (fme)
            for (int p = 0; p < 4; ++p) ptrs[nptr++] = planes + (size_t)(4 * r + p) * ps;
        else
            ptrs[nptr++] = refs[r];
    }
    return me_fastpred_launch(cur, ptrs, nptr, nfast, H, W, bs, fme, by0, by1, me_mode == SO_ME_FAST, best, sub, seg_ws,
                              st);
}

int so_me_search_ex(const uint8_t* cur, const uint8_t* const* refs, int nref, int H, int W, int bs, int sr,
                    int me_mode, int fme, int fme_wrap, uint8_t* fme_planes, int32_t* out_best, int32_t* out_sub,
                    void* stream) {
    const char* fn = "so_me_search_ex";
    SO_TRY(check_geom(fn, H, W, bs, out_sub != nullptr));
    SO_TRY(check_sr(fn, sr));
    SO_NEED(cur, fn);
    SO_NEED(out_best, fn);
    RefSet rs;
    SO_TRY(make_refs(fn, refs, nref, &rs));
    return me_ex(fn, cur, refs, nref, rs, H, W, bs, sr, 0, H / bs, me_mode, fme, fme_wrap, fme_planes, out_best,
                 out_sub, (hipStream_t)stream);
}

// `fn` names the entry point refusals are reported under
static int p_rows(const char* fn, const uint8_t* cur, const uint8_t* const* refs, int nref, int H, int W, int bs, int sr,
                  int by0, int by1, int qp_rd, const int32_t* qp_row, const int32_t* qp_map, int vbs, double lam,
                  int me_mode, int fme, int fme_wrap, uint8_t* fme_planes, int flags, uint8_t* out_split,
                  int16_t* out_mv, int16_t* out_qtc, int32_t* out_tokens, int32_t* out_mae_num, uint8_t* out_recon,
                  int32_t* out_sse, int32_t* scratch, void* stream) {
    SO_TRY(check_geom(fn, H, W, bs, vbs));
    SO_TRY(check_sr(fn, sr));
    SO_TRY(check_qp(fn, qp_rd));
    SO_TRY(check_rows(fn, H, bs, by0, by1));
    SO_NEED(cur, fn); SO_NEED(scratch, fn); SO_NEED(out_split, fn); SO_NEED(out_mv, fn);
    SO_NEED(out_qtc, fn); SO_NEED(out_tokens, fn); SO_NEED(out_mae_num, fn); SO_NEED(out_recon, fn);
    RefSet rs;
    SO_TRY(make_refs(fn, refs, nref, &rs));
    SO_TRY(check_recon_not_ref(fn, refs, nref, out_recon));
    const size_t nbs = (size_t)(W / bs) * (size_t)(by1 - by0);
    int32_t* best = scratch;
    int32_t* sub = vbs ? scratch + nbs * 4 : nullptr;
    hipStream_t st = (hipStream_t)stream;
    if (flags & SO_REUSE_ME) {
        // pass 2 of two-pass RC: the ME records (and FME planes) of the previous call stay
        if (fme) SO_NEED(fme_planes, fn);
    } else if (me_mode == SO_ME_FULL && !fme && use_fused(bs, sr, vbs, nref)) {
        return p_tile_launch(cur, rs, H, W, by0, by1, qp_rd, qp_row, qp_map, best, out_split, out_mv, out_qtc,
                             out_tokens, out_mae_num, out_recon, out_sse, st, (flags & SO_TOKENS_ONLY) != 0);
    } else {
        SO_TRY(me_ex(fn, cur, refs, nref, rs, H, W, bs, sr, by0, by1, me_mode, fme, fme_wrap, fme_planes, best, sub,
                     st, scratch + nbs * 4 + (vbs ? nbs * 16 : 0)));
    }
    return inter_tq_launch(cur, rs, fme ? fme_planes : nullptr, so_fme_plane_stride(H, W), H, W, bs, by0, by1, best,
                           sub, qp_rd, qp_row, qp_map, vbs, lam, out_split, out_mv, out_qtc, out_tokens, out_mae_num, out_recon,
                           out_sse, st);
}

int so_encode_p_rows(const uint8_t* cur, const uint8_t* const* refs, int nref, int H, int W, int bs, int sr,
                     int by0, int by1, int qp_rd, const int32_t* qp_row, int vbs, double lam, uint8_t* out_split,
                     int16_t* out_mv, int16_t* out_qtc, int32_t* out_tokens, int32_t* out_mae_num,
                     uint8_t* out_recon, int32_t* out_sse, int32_t* scratch, void* stream) {
    return p_rows("so_encode_p_rows", cur, refs, nref, H, W, bs, sr, by0, by1, qp_rd, qp_row, nullptr, vbs, lam,
                  SO_ME_FULL, 0, 0, nullptr, 0, out_split, out_mv, out_qtc, out_tokens, out_mae_num, out_recon, out_sse,
                  scratch, stream);
}

int so_encode_p_rows_ex(const uint8_t* cur, const uint8_t* const* refs, int nref, int H, int W, int bs, int sr,
                        int by0, int by1, int qp_rd, const int32_t* qp_row, const int32_t* qp_map, int vbs, double lam,
                        int me_mode, int fme, int fme_wrap, uint8_t* fme_planes, int flags, uint8_t* out_split, int16_t* out_mv, int16_t* out_qtc,
                        int32_t* out_tokens, int32_t* out_mae_num, uint8_t* out_recon, int32_t* out_sse,
                        int32_t* scratch, void* stream) {
    // with nothing of the _ex form asked for this is so_encode_p_rows, and reports under that name
    const bool plain = me_mode == SO_ME_FULL && !fme && !qp_map && !(flags & (SO_REUSE_ME | SO_TOKENS_ONLY));
    return p_rows(plain ? "so_encode_p_rows" : "so_encode_p_rows_ex", cur, refs, nref, H, W, bs, sr, by0, by1, qp_rd,
                  qp_row, qp_map, vbs, lam, me_mode, fme, fme_wrap, fme_planes, flags, out_split, out_mv, out_qtc,
                  out_tokens, out_mae_num, out_recon, out_sse, scratch, stream);
}

int so_qp_map(const int32_t* tokens, int H, int W, int bs, int by0, int by1, int qp_rd, const int32_t* qp_row,
              const int32_t* roi, int qp_lo, int qp_hi, int32_t* out_qp_map, void* stream) {
    const char* fn = "so_qp_map";
    if (bs <= 0 || H <= 0 || W <= 0 || H % bs || W % bs) {
        set_error("%s: bad geometry", fn);
        return SO_E_INVALID;
    }
    SO_TRY(check_rows(fn, H, bs, by0, by1));
    SO_NEED(out_qp_map, fn);
    SO_TRY(check_qp_clamp(fn, qp_lo, qp_hi));
    if (by1 <= by0) return SO_OK;
    return qp_map_launch(tokens, W / bs, by0, by1, qp_rd, qp_row, roi, qp_lo, qp_hi, out_qp_map, (hipStream_t)stream);
}

int so_sum_i32_rows(const int32_t* const* rows, int n, int len, int64_t* out, void* stream) {
    const char* fn = "so_sum_i32_rows";
    if (n < 0 || len < 0) {
        set_error("%s: n %d / len %d", fn, n, len);
        return SO_E_INVALID;
    }
    if (n == 0) return SO_OK;
    SO_NEED(rows, fn); SO_NEED(out, fn);
    for (int i0 = 0; i0 < n; i0 += kSumMax) {
        const int m = n - i0 < kSumMax ? n - i0 : kSumMax;
        for (int i = 0; i < m; ++i) SO_NEED(rows[i0 + i], fn);
        SO_TRY(sum_rows_launch(rows + i0, m, len, out + i0, (hipStream_t)stream));
    }
    return SO_OK;
}

int so_sse_u8(const uint8_t* a, const uint8_t* b, int64_t n, uint64_t* out_sse, void* stream) {
    const char* fn = "so_sse_u8";
    SO_NEED(a, fn); SO_NEED(b, fn); SO_NEED(out_sse, fn);
    if (n < 0) {
        set_error("%s: n < 0", fn);
        return SO_E_INVALID;
    }
    if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 15) {
        set_error("%s: planes must be 16-byte aligned", fn);
        return SO_E_INVALID;
    }
    return sse_launch(a, b, n, out_sse, (hipStream_t)stream);
}

// ---- SSIM (so_ssim.hip) -----------------------------------------------------------------------
size_t so_ssim_workspace_elems(int nframes, int H, int W, int win) {
    if (nframes <= 0 || (long long)H * W > (1ll << 31)) return 0;
    return (size_t)nframes * ssim_tiles(H, W, win);
}

int so_ssim_u8(const uint8_t* const* a, const uint8_t* const* b, int nframes, int H, int W, size_t pitch_a,
               size_t pitch_b, int win, double* out, double* workspace, void* stream) {
    const char* fn = "so_ssim_u8";
    if (win < 3 || win > 15 || win % 2 == 0) {
        set_error("%s: win %d (odd, 3..15)", fn, win);
        return SO_E_INVALID;
    }
    if (H < win || W < win) {
        set_error("%s: picture %dx%d is smaller than the %d-pixel window", fn, W, H, win);
        return SO_E_INVALID;
    }
    if ((long long)H * W > (1ll << 31)) {
        set_error("%s: frame too large", fn);
        return SO_E_INVALID;
    }
    if (pitch_a < (size_t)W || pitch_b < (size_t)W) {
        set_error("%s: pitch %zu / %zu below the width %d", fn, pitch_a, pitch_b, W);
        return SO_E_INVALID;
    }
    if (nframes < 0) {
        set_error("%s: nframes %d", fn, nframes);
        return SO_E_INVALID;
    }
    if (nframes == 0) return SO_OK;
    SO_NEED(a, fn); SO_NEED(b, fn); SO_NEED(out, fn); SO_NEED(workspace, fn);
    for (int i = 0; i < nframes; ++i) {
        SO_NEED(a[i], fn); SO_NEED(b[i], fn);
    }
    return ssim_launch(a, b, nframes, H, W, pitch_a, pitch_b, win, out, workspace, (hipStream_t)stream);
}

// ---- colour conversion (so_colour.hip) ------------------------------------------------------------
namespace {
// two h-row views of `row` bytes per row and one pitch: does a byte belong to both?
bool colour_views_overlap(uintptr_t a, uintptr_t b, size_t pitch, size_t row, int h) {
    const uintptr_t d = a < b ? b - a : a - b;
    const size_t q = d / pitch, r = d % pitch;
    return (r < row && q < (size_t)h) || (r + row > pitch && q + 1 < (size_t)h);
}

// the scalar checks both directions share; fills g
int colour_geom(const char* fn, int nframes, int h, int w, int Hp, int Wp, int layout, size_t pitch,
                size_t plane_stride, int matrix, int full_range, bool forward, ColourGeom* g) {
    if (h <= 0 || w <= 0 || h % 2 || w % 2) {
        set_error("%s: h %d, w %d (a 4:2:0 picture is positive and even both ways)", fn, h, w);
        return SO_E_INVALID;
    }
    if (Hp < h || Wp < w || Hp % 2 || Wp % 2) {
        set_error("%s: Hp %d, Wp %d (even, and at least the picture's %d x %d)", fn, Hp, Wp, h, w);
        return SO_E_INVALID;
    }
    if ((long long)Hp * Wp > (1ll << 31)) {
        set_error("%s: Hp %d x Wp %d: frame too large", fn, Hp, Wp);
        return SO_E_INVALID;
    }
    if (layout != SO_LAYOUT_HWC && layout != SO_LAYOUT_CHW) {
        set_error("%s: layout %d (SO_LAYOUT_HWC or SO_LAYOUT_CHW)", fn, layout);
        return SO_E_INVALID;
    }
    const size_t row = layout == SO_LAYOUT_HWC ? 3 * (size_t)w : (size_t)w;
    if (pitch < row) {
        set_error("%s: pitch %zu below a row's %zu bytes", fn, pitch, row);
        return SO_E_INVALID;
    }
    if (layout == SO_LAYOUT_CHW && plane_stride == 0) {
        set_error("%s: plane_stride 0 (the three planes of a CHW picture are apart)", fn);
        return SO_E_INVALID;
    }
    if (matrix != SO_COLOUR_BT601 && matrix != SO_COLOUR_BT709) {
        set_error("%s: matrix %d (SO_COLOUR_BT601 or SO_COLOUR_BT709)", fn, matrix);
        return SO_E_INVALID;
    }
    if (full_range != 0 && full_range != 1) {
        set_error("%s: full_range %d (0 or 1)", fn, full_range);
        return SO_E_INVALID;
    }
    if (nframes < 0) {
        set_error("%s: nframes %d", fn, nframes);
        return SO_E_INVALID;
    }
    g->h = h; g->w = w; g->Hp = Hp; g->Wp = Wp;
    g->pitch = pitch;
    g->plane = layout == SO_LAYOUT_CHW ? plane_stride : 0;
    const int32_t* t = (forward ? kColourFwd : kColourInv)[2 * matrix + (full_range ? 0 : 1)];
    for (int i = 0; i < 9; ++i) g->c[i] = t[i];
    g->yoff = full_range ? 0 : 16;
    return SO_OK;
}

// Pointers and aliasing.  The planes are dense; an RGB picture is h rows of `row` bytes `pitch`
// apart (three such views plane_stride apart for CHW).  A destination may share no byte with a
// source or another destination.  Sources may repeat.
int colour_alias(const char* fn, const uint8_t* const* rgb, const uint8_t* const* y, const uint8_t* const* u,
                 const uint8_t* const* v, int nframes, const ColourGeom& g, int layout, bool forward) {
    const size_t row = layout == SO_LAYOUT_HWC ? 3 * (size_t)g.w : (size_t)g.w;
    const size_t view = (size_t)(g.h - 1) * g.pitch + row;
    const size_t ny = (size_t)g.Hp * g.Wp, nc = ny / 4;
    const int nviews = layout == SO_LAYOUT_HWC ? 1 : 3;
    std::vector<Span> spans;
    spans.reserve((size_t)nframes * 6);
    for (int i = 0; i < nframes; ++i) {
        const uintptr_t py = reinterpret_cast<uintptr_t>(y[i]), pu = reinterpret_cast<uintptr_t>(u[i]),
                        pv = reinterpret_cast<uintptr_t>(v[i]), pr = reinterpret_cast<uintptr_t>(rgb[i]);
        spans.push_back({py, py + ny, forward, "y", i});
        spans.push_back({pu, pu + nc, forward, "u", i});
        spans.push_back({pv, pv + nc, forward, "v", i});
        for (int c = 0; c < nviews; ++c)
            spans.push_back({pr + c * g.plane, pr + c * g.plane + view, !forward, "rgb", i});
    }
    SO_TRY(check_spans(fn, spans, forward));   // inverse: destination against destination below
    if (!forward) {
        // RGB destinations may interleave row by row (crops of one canvas): an exact test, pair by pair
        std::vector<uintptr_t> views;
        for (int i = 0; i < nframes; ++i)
            for (int c = 0; c < nviews; ++c) views.push_back(reinterpret_cast<uintptr_t>(rgb[i]) + c * g.plane);
        for (size_t a = 0; a < views.size(); ++a)
            for (size_t b = a + 1; b < views.size(); ++b)
                if (colour_views_overlap(views[a], views[b], g.pitch, row, g.h)) {
                    set_error("%s: rgb[%d] aliases rgb[%d] (two destination pictures share bytes)", fn,
                              (int)(a / nviews), (int)(b / nviews));
                    return SO_E_INVALID;
                }
    }
    return SO_OK;
}

int colour_pointers(const char* fn, const uint8_t* const* rgb, const uint8_t* const* y, const uint8_t* const* u,
                    const uint8_t* const* v, int nframes) {
    SO_NEED(rgb, fn); SO_NEED(y, fn); SO_NEED(u, fn); SO_NEED(v, fn);
    for (int i = 0; i < nframes; ++i)
        if (!rgb[i] || !y[i] || !u[i] || !v[i]) {
            set_error("%s: %s[%d] is NULL", fn, !rgb[i] ? "rgb" : !y[i] ? "y" : !u[i] ? "u" : "v", i);
            return SO_E_INVALID;
        }
    return SO_OK;
}
}  // namespace

int so_rgb_to_yuv420(const uint8_t* const* rgb, int nframes, int h, int w, int layout, size_t pitch,
                     size_t plane_stride, int matrix, int full_range, int Hp, int Wp, uint8_t* const* y,
                     uint8_t* const* u, uint8_t* const* v, void* stream) {
    const char* fn = "so_rgb_to_yuv420";
    ColourGeom g{};
    SO_TRY(colour_geom(fn, nframes, h, w, Hp, Wp, layout, pitch, plane_stride, matrix, full_range, true, &g));
    if (nframes == 0) return SO_OK;
    SO_TRY(colour_pointers(fn, rgb, y, u, v, nframes));
    SO_TRY(colour_alias(fn, rgb, y, u, v, nframes, g, layout, true));
    return colour_forward_launch(layout, rgb, y, u, v, nframes, g, (hipStream_t)stream);
}

int so_yuv420_to_rgb(const uint8_t* const* y, const uint8_t* const* u, const uint8_t* const* v, int nframes,
                     int Hp, int Wp, int h, int w, int matrix, int full_range, int layout, uint8_t* const* rgb,
                     size_t pitch, size_t plane_stride, void* stream) {
    const char* fn = "so_yuv420_to_rgb";
    ColourGeom g{};
    SO_TRY(colour_geom(fn, nframes, h, w, Hp, Wp, layout, pitch, plane_stride, matrix, full_range, false, &g));
    if (nframes == 0) return SO_OK;
    SO_TRY(colour_pointers(fn, rgb, y, u, v, nframes));
    SO_TRY(colour_alias(fn, rgb, y, u, v, nframes, g, layout, false));
    return colour_inverse_launch(layout, y, u, v, rgb, nframes, g, (hipStream_t)stream);
}

// ---- scaling (so_scale.hip) -----------------------------------------------------------------------
namespace {
int scale_table(const char* fn, const char* what, const int16_t* coef, const int32_t* first, int taps,
                ScaleTable* t) {
    if (taps < 1 || taps > kScaleMaxTaps) {
        set_error("%s: taps_%s %d outside [1, %d]", fn, what, taps, kScaleMaxTaps);
        return SO_E_INVALID;
    }
    if (!coef || !first) {
        set_error("%s: %s_%s is NULL", fn, !coef ? "coef" : "first", what);
        return SO_E_INVALID;
    }
    t->coef = coef; t->first = first; t->taps = taps;
    return SO_OK;
}
}  // namespace

int so_scale_yuv420(const uint8_t* const* sy, const uint8_t* const* su, const uint8_t* const* sv, int nframes,
                    int hs, int ws, size_t pitch_y, size_t pitch_c, uint8_t* const* dy, uint8_t* const* du,
                    uint8_t* const* dv, int hd, int wd, int Hp, int Wp, const int16_t* coef_yh,
                    const int32_t* first_yh, int taps_yh, const int16_t* coef_yv, const int32_t* first_yv,
                    int taps_yv, const int16_t* coef_ch, const int32_t* first_ch, int taps_ch,
                    const int16_t* coef_cv, const int32_t* first_cv, int taps_cv, void* stream) {
    const char* fn = "so_scale_yuv420";
    const int nchroma = (su != nullptr) + (sv != nullptr) + (du != nullptr) + (dv != nullptr);
    if (nchroma != 0 && nchroma != 4) {
        set_error("%s: %s is NULL (su, sv, du and dv are all given, or all NULL for luma only)", fn,
                  !su ? "su" : !sv ? "sv" : !du ? "du" : "dv");
        return SO_E_INVALID;
    }
    const bool chroma = nchroma == 4;
    if (hs <= 0 || ws <= 0 || (chroma && (hs % 2 || ws % 2))) {
        set_error("%s: hs %d, ws %d (a source picture is positive%s)", fn, hs, ws,
                  chroma ? ", and even both ways with chroma" : "");
        return SO_E_INVALID;
    }
    if (hd <= 0 || wd <= 0 || (chroma && (hd % 2 || wd % 2))) {
        set_error("%s: hd %d, wd %d (a destination picture is positive%s)", fn, hd, wd,
                  chroma ? ", and even both ways with chroma" : "");
        return SO_E_INVALID;
    }
    if (Hp < hd || Wp < wd || (chroma && (Hp % 2 || Wp % 2))) {
        set_error("%s: Hp %d, Wp %d (at least the picture's %d x %d%s)", fn, Hp, Wp, hd, wd,
                  chroma ? ", and even with chroma" : "");
        return SO_E_INVALID;
    }
    if ((long long)Hp * Wp > (1ll << 31) || (long long)hs * ws > (1ll << 31)) {
        set_error("%s: %d x %d -> %d x %d: frame too large", fn, hs, ws, Hp, Wp);
        return SO_E_INVALID;
    }
    if (pitch_y < (size_t)ws) {
        set_error("%s: pitch_y %zu below a row's %d bytes", fn, pitch_y, ws);
        return SO_E_INVALID;
    }
    if (chroma && pitch_c < (size_t)(ws / 2)) {
        set_error("%s: pitch_c %zu below a row's %d bytes", fn, pitch_c, ws / 2);
        return SO_E_INVALID;
    }
    if (nframes < 0) {
        set_error("%s: nframes %d", fn, nframes);
        return SO_E_INVALID;
    }
    ScaleGeom g{};
    g.nplanes = chroma ? 3 : 1;
    g.p[0].hs = hs; g.p[0].ws = ws; g.p[0].hd = hd; g.p[0].wd = wd; g.p[0].Hp = Hp; g.p[0].Wp = Wp;
    g.p[0].spitch = pitch_y;
    SO_TRY(scale_table(fn, "yh", coef_yh, first_yh, taps_yh, &g.p[0].h));
    SO_TRY(scale_table(fn, "yv", coef_yv, first_yv, taps_yv, &g.p[0].v));
    if (chroma) {
        g.p[1].hs = hs / 2; g.p[1].ws = ws / 2; g.p[1].hd = hd / 2; g.p[1].wd = wd / 2;
        g.p[1].Hp = Hp / 2; g.p[1].Wp = Wp / 2;
        g.p[1].spitch = pitch_c;
        SO_TRY(scale_table(fn, "ch", coef_ch, first_ch, taps_ch, &g.p[1].h));
        SO_TRY(scale_table(fn, "cv", coef_cv, first_cv, taps_cv, &g.p[1].v));
    }
    if (!scale_tiles(&g)) {
        set_error("%s: %d x %d -> %d x %d with %d / %d taps: no tile of this ratio fits the LDS", fn, hs, ws, hd,
                  wd, taps_yh, taps_yv);
        return SO_E_UNSUPPORTED;
    }
    if (nframes == 0) return SO_OK;
    SO_NEED(sy, fn); SO_NEED(dy, fn);

    // A source is hs rows of ws bytes a pitch apart (taken as one span), a destination a dense plane.
    // A destination may share no byte with a source or another destination; sources may repeat.
    const uint8_t* const* srcs[3] = {sy, su, sv};
    uint8_t* const* dsts[3] = {dy, du, dv};
    static const char* const sname[3] = {"sy", "su", "sv"};
    static const char* const dname[3] = {"dy", "du", "dv"};
    std::vector<Span> spans;
    spans.reserve((size_t)nframes * 6);
    for (int i = 0; i < nframes; ++i)
        for (int k = 0; k < g.nplanes; ++k) {
            const ScalePlane& p = g.p[k != 0];
            if (!srcs[k][i] || !dsts[k][i]) {
                set_error("%s: %s[%d] is NULL", fn, !srcs[k][i] ? sname[k] : dname[k], i);
                return SO_E_INVALID;
            }
            const uintptr_t ps = reinterpret_cast<uintptr_t>(srcs[k][i]), pd = reinterpret_cast<uintptr_t>(dsts[k][i]);
            spans.push_back({ps, ps + (size_t)(p.hs - 1) * p.spitch + p.ws, false, sname[k], i});
            spans.push_back({pd, pd + (size_t)p.Hp * p.Wp, true, dname[k], i});
        }
    SO_TRY(check_spans(fn, spans, true));

    for (int f0 = 0; f0 < nframes; f0 += kScaleBatch) {
        const int m = nframes - f0 < kScaleBatch ? nframes - f0 : kScaleBatch;
        ScalePtrs p{};
        for (int i = 0; i < m; ++i)
            for (int k = 0; k < g.nplanes; ++k) {
                p.s[k][i] = srcs[k][f0 + i];
                p.d[k][i] = dsts[k][f0 + i];
            }
        SO_TRY(scale_launch(p, m, g, (hipStream_t)stream));
    }
    return SO_OK;
}

// ---- deblocking post-filter (so_deblock.hip) -----------------------------------------------------
int so_deblock_yuv420(const uint8_t* const* sy, const uint8_t* const* su, const uint8_t* const* sv, int nframes,
                      int H, int W, int bs, const uint8_t* const* split, int qp, const int32_t* const* qp_row,
                      const int32_t* const* qp_map, int chroma_qp_offset, int strength, uint8_t* const* dy,
                      uint8_t* const* du, uint8_t* const* dv, void* stream) {
    const char* fn = "so_deblock_yuv420";
    if (nframes < 0) {
        set_error("%s: nframes %d", fn, nframes);
        return SO_E_INVALID;
    }
    if (bs != 8 && bs != 16) {
        set_error("%s: bs %d (the cells are 8 x 8: block size 8 or 16)", fn, bs);
        return SO_E_INVALID;
    }
    if (H <= 0 || W <= 0 || H % bs || W % bs || (long long)H * W > (1ll << 31)) {
        set_error("%s: H %d, W %d (positive multiples of bs %d, at most 2^31 samples)", fn, H, W, bs);
        return SO_E_INVALID;
    }
    if (qp < 0 || qp > 20) {
        set_error("%s: qp %d outside [0, 20]", fn, qp);
        return SO_E_INVALID;
    }
    if (chroma_qp_offset < -20 || chroma_qp_offset > 20) {
        set_error("%s: chroma_qp_offset %d outside [-20, 20]", fn, chroma_qp_offset);
        return SO_E_INVALID;
    }
    if (strength < -3 || strength > 3) {
        set_error("%s: strength %d outside [-3, 3]", fn, strength);
        return SO_E_INVALID;
    }
    if (nframes == 0) return SO_OK;
    SO_NEED(sy, fn); SO_NEED(dy, fn);
    for (int i = 0; i < nframes; ++i)
        if (!sy[i] || !dy[i]) {
            set_error("%s: %s[%d] is NULL", fn, !sy[i] ? "sy" : "dy", i);
            return SO_E_INVALID;
        }
    const int nchroma = (su != nullptr) + (sv != nullptr) + (du != nullptr) + (dv != nullptr);
    if (nchroma != 0 && nchroma != 4) {
        set_error("%s: %s is NULL (su, sv, du and dv are all given, or all NULL for luma only)", fn,
                  !su ? "su" : !sv ? "sv" : !du ? "du" : "dv");
        return SO_E_INVALID;
    }
    const bool chroma = nchroma == 4;
    const uint8_t* const* srcs[3] = {sy, su, sv};
    uint8_t* const* dsts[3] = {dy, du, dv};
    static const char* const sname[3] = {"sy", "su", "sv"};
    static const char* const dname[3] = {"dy", "du", "dv"};
    for (int i = 0; chroma && i < nframes; ++i)
        for (int k = 1; k < 3; ++k)
            if (!srcs[k][i] || !dsts[k][i]) {
                set_error("%s: %s[%d] is NULL", fn, !srcs[k][i] ? sname[k] : dname[k], i);
                return SO_E_INVALID;
            }
    // A destination may share no byte with a source or another destination; sources may repeat.
    std::vector<Span> spans;
    spans.reserve((size_t)nframes * 6);
    for (int i = 0; i < nframes; ++i)
        for (int k = 0; k < (chroma ? 3 : 1); ++k) {
            const size_t bytes = k ? (size_t)(H / 2) * (W / 2) : (size_t)H * W;
            const uintptr_t ps = reinterpret_cast<uintptr_t>(srcs[k][i]), pd = reinterpret_cast<uintptr_t>(dsts[k][i]);
            spans.push_back({ps, ps + bytes, false, sname[k], i});
            spans.push_back({pd, pd + bytes, true, dname[k], i});
        }
    SO_TRY(check_spans(fn, spans, true));
    if (chroma && bs == 8) {
        set_error("%s: chroma needs bs 16 (the 4:2:0 codec is built for 16 x 16 blocks)", fn);
        return SO_E_UNSUPPORTED;
    }
    for (int i = 0; bs == 8 && split && i < nframes; ++i)
        if (split[i]) {
            set_error("%s: split[%d] with bs 8 (4-sample sub-blocks: the lines of a pass would overlap)", fn, i);
            return SO_E_UNSUPPORTED;
        }

    DeblockGeom g{};
    g.H = H; g.W = W; g.bs = bs; g.nplanes = chroma ? 3 : 1;
    g.qp = qp; g.chroma_qp_offset = chroma_qp_offset; g.strength = strength;
    deblock_tiles(&g);
    for (int f0 = 0; f0 < nframes; f0 += kDeblockBatch) {
        const int m = nframes - f0 < kDeblockBatch ? nframes - f0 : kDeblockBatch;
        DeblockPtrs p{};
        for (int i = 0; i < m; ++i) {
            for (int k = 0; k < g.nplanes; ++k) {
                p.s[k][i] = srcs[k][f0 + i];
                p.d[k][i] = dsts[k][f0 + i];
            }
            p.split[i] = split ? split[f0 + i] : nullptr;
            p.qp_row[i] = qp_row ? qp_row[f0 + i] : nullptr;
            p.qp_map[i] = qp_map ? qp_map[f0 + i] : nullptr;
        }
        SO_TRY(deblock_launch(p, m, g, (hipStream_t)stream));
    }
    return SO_OK;
}

// ---- chroma 4:2:0 (so_chroma.hip) ----------------------------------------------------------------
// so_chroma_encode_frame / so_chroma_recon_frame and their _ex forms: one function, the base
// names passing mv_frac_bits 1 under their own name
static int chroma_frame(const char* fn, bool encode, const uint8_t* cur_u, const uint8_t* cur_v,
                        const uint8_t* const* refs_u, const uint8_t* const* refs_v, int nref, int H, int W, int bs,
                        int frame_type, const uint8_t* split, const int16_t* mv, int qp, const int32_t* qp_row,
                        const int32_t* qp_map, int qp_offset, int16_t* qtc_u, int16_t* qtc_v, int32_t* out_tokens,
                        uint8_t* out_recon_u, uint8_t* out_recon_v, int32_t* out_sse, int mv_frac_bits,
                        void* stream) {
    if (bs != 16) {
        set_error("%s: block_size %d not built (chroma follows 16x16 luma blocks)", fn, bs);
        return SO_E_UNSUPPORTED;
    }
    SO_TRY(check_mv_frac_bits(fn, mv_frac_bits));
    if (H <= 0 || W <= 0 || H % 16 || W % 16) {
        set_error("%s: luma frame %dx%d must be a positive multiple of 16 (pad with pad_hw)", fn, W, H);
        return SO_E_INVALID;
    }
    if ((long long)H * W > (1ll << 31)) {
        set_error("%s: frame too large", fn);
        return SO_E_INVALID;
    }
    if (frame_type != 0 && frame_type != 1) {
        set_error("%s: frame_type %d (0 = intra, 1 = inter)", fn, frame_type);
        return SO_E_INVALID;
    }
    SO_TRY(check_qp(fn, qp));
    if (qp_offset < -20 || qp_offset > 20) {
        set_error("%s: qp_offset %d outside [-20, 20]", fn, qp_offset);
        return SO_E_INVALID;
    }
    ChromaArgs a{};
    if (frame_type == 1) {
        if (nref < 1 || nref > kMaxRef) {
            set_error("%s: nref %d outside [1, %d]", fn, nref, kMaxRef);
            return SO_E_INVALID;
        }
        SO_TRY(make_refs(fn, refs_u, nref, &a.pl[0].refs));
        SO_TRY(make_refs(fn, refs_v, nref, &a.pl[1].refs));
        SO_NEED(split, fn); SO_NEED(mv, fn);
    }
    if (encode) {
        SO_NEED(cur_u, fn); SO_NEED(cur_v, fn); SO_NEED(out_tokens, fn); SO_NEED(out_sse, fn);
    }
    SO_NEED(qtc_u, fn); SO_NEED(qtc_v, fn); SO_NEED(out_recon_u, fn); SO_NEED(out_recon_v, fn);
    if (out_recon_u == out_recon_v) {
        set_error("%s: out_recon_u aliases out_recon_v", fn);
        return SO_E_INVALID;
    }
    // rows move as 8-byte vectors and the prediction reads aligned dwords of the planes
    const uintptr_t planes_or = (uintptr_t)cur_u | (uintptr_t)cur_v | (uintptr_t)out_recon_u | (uintptr_t)out_recon_v;
    uintptr_t refs_or = 0;
    if (frame_type == 1)
        for (int i = 0; i < nref; ++i) {
            refs_or |= (uintptr_t)refs_u[i] | (uintptr_t)refs_v[i];
            if (refs_u[i] == out_recon_u || refs_u[i] == out_recon_v || refs_v[i] == out_recon_u ||
                refs_v[i] == out_recon_v) {
                set_error("%s: a reconstruction aliases refs[%d]", fn, i);
                return SO_E_INVALID;
            }
        }
    if (((planes_or | refs_or) & 7) || (((uintptr_t)qtc_u | (uintptr_t)qtc_v) & 15)) {
        set_error("%s: planes must be 8-byte aligned and qtc 16-byte aligned", fn);
        return SO_E_INVALID;
    }
    a.pl[0].cur = cur_u; a.pl[1].cur = cur_v;
    a.pl[0].qtc = qtc_u; a.pl[1].qtc = qtc_v;
    a.pl[0].recon = out_recon_u; a.pl[1].recon = out_recon_v;
    a.nref = frame_type == 1 ? nref : 1;
    a.Hc = H / 2; a.Wc = W / 2; a.nbx = W / 16; a.nb = (W / 16) * (H / 16);
    a.frame_type = frame_type;
    a.split = split; a.mv = mv;
    a.qp = qp; a.qp_row = qp_row; a.qp_map = qp_map; a.qp_offset = qp_offset;
    a.tokens = out_tokens; a.sse = out_sse;
    a.mv_frac_bits = mv_frac_bits;
    return chroma_launch(a, encode, (hipStream_t)stream);
}

int so_chroma_encode_frame(const uint8_t* cur_u, const uint8_t* cur_v, const uint8_t* const* refs_u,
                           const uint8_t* const* refs_v, int nref, int H, int W, int bs, int frame_type,
                           const uint8_t* split, const int16_t* mv, int qp, const int32_t* qp_row,
                           const int32_t* qp_map, int qp_offset, int16_t* out_qtc_u, int16_t* out_qtc_v,
                           int32_t* out_tokens, uint8_t* out_recon_u, uint8_t* out_recon_v, int32_t* out_sse,
                           void* stream) {
    return chroma_frame("so_chroma_encode_frame", true, cur_u, cur_v, refs_u, refs_v, nref, H, W, bs, frame_type,
                        split, mv, qp, qp_row, qp_map, qp_offset, out_qtc_u, out_qtc_v, out_tokens, out_recon_u,
                        out_recon_v, out_sse, 1, stream);
}

int so_chroma_encode_frame_ex(const uint8_t* cur_u, const uint8_t* cur_v, const uint8_t* const* refs_u,
                              const uint8_t* const* refs_v, int nref, int H, int W, int bs, int frame_type,
                              const uint8_t* split, const int16_t* mv, int qp, const int32_t* qp_row,
                              const int32_t* qp_map, int qp_offset, int16_t* out_qtc_u, int16_t* out_qtc_v,
                              int32_t* out_tokens, uint8_t* out_recon_u, uint8_t* out_recon_v, int32_t* out_sse,
                              int mv_frac_bits, void* stream) {
    return chroma_frame("so_chroma_encode_frame_ex", true, cur_u, cur_v, refs_u, refs_v, nref, H, W, bs, frame_type,
                        split, mv, qp, qp_row, qp_map, qp_offset, out_qtc_u, out_qtc_v, out_tokens, out_recon_u,
                        out_recon_v, out_sse, mv_frac_bits, stream);
}

int so_chroma_recon_frame(const uint8_t* const* refs_u, const uint8_t* const* refs_v, int nref, int H, int W, int bs,
                          int frame_type, const uint8_t* split, const int16_t* mv, int qp, const int32_t* qp_row,
                          const int32_t* qp_map, int qp_offset, const int16_t* qtc_u, const int16_t* qtc_v,
                          uint8_t* out_recon_u, uint8_t* out_recon_v, void* stream) {
    return chroma_frame("so_chroma_recon_frame", false, nullptr, nullptr, refs_u, refs_v, nref, H, W, bs, frame_type,
                        split, mv, qp, qp_row, qp_map, qp_offset, const_cast<int16_t*>(qtc_u),
                        const_cast<int16_t*>(qtc_v), nullptr, out_recon_u, out_recon_v, nullptr, 1, stream);
}

int so_chroma_recon_frame_ex(const uint8_t* const* refs_u, const uint8_t* const* refs_v, int nref, int H, int W,
                             int bs, int frame_type, const uint8_t* split, const int16_t* mv, int qp,
                             const int32_t* qp_row, const int32_t* qp_map, int qp_offset, const int16_t* qtc_u,
                             const int16_t* qtc_v, uint8_t* out_recon_u, uint8_t* out_recon_v, int mv_frac_bits,
                             void* stream) {
    return chroma_frame("so_chroma_recon_frame_ex", false, nullptr, nullptr, refs_u, refs_v, nref, H, W, bs,
                        frame_type, split, mv, qp, qp_row, qp_map, qp_offset, const_cast<int16_t*>(qtc_u),
                        const_cast<int16_t*>(qtc_v), nullptr, out_recon_u, out_recon_v, nullptr, mv_frac_bits, stream);
}

// ---- packed symbol stream (so_pack.hip) -----------------------------------------------------
size_t so_pack_bound(int nb, int bs) {
    if (nb <= 0 || (bs != 16 && bs != 8)) return 0;
    return (size_t)nb * pack_block_bound(bs);
}

int so_pack_frames(int nframes, const int32_t* frame_types, const uint8_t* const* split, const int16_t* const* mv,
                   const int16_t* const* qtc, int nb, int bs, uint32_t* const* offs, uint8_t* const* out,
                   unsigned long long cap, void* stream) {
    return so_pack_frames_ex(nframes, frame_types, split, mv, qtc, nb, bs, offs, out, cap, nullptr, stream);
}

// the block size and counts of every pack / unpack entry point (chroma passes its fixed 16)
static int check_pack_counts(const char* fn, int bs, int nb, int nframes) {
    if (bs != 16 && bs != 8) {
        set_error("%s: block_size %d not built", fn, bs);
        return SO_E_UNSUPPORTED;
    }
    if (nb <= 0 || nframes < 0) {
        set_error("%s: nb %d / nframes %d", fn, nb, nframes);
        return SO_E_INVALID;
    }
    return SO_OK;
}

// validation and launch of every coding of the stream (bits: so_packbits.hip, huff: so_packhuff.hip)
enum PackCoding { kVarint = 0, kBits = 1, kHuff = 2 };
static int pack_frames_any(const char* fn, int bits, int nframes, const int32_t* frame_types,
                           const uint8_t* const* split, const int16_t* const* mv, const int16_t* const* qtc, int nb,
                           int bs, uint32_t* const* offs, uint8_t* const* out, unsigned long long cap,
                           uint32_t* totals, void* stream) {
    SO_TRY(check_pack_counts(fn, bs, nb, nframes));
    if (nframes == 0) return SO_OK;
    SO_NEED(frame_types, fn); SO_NEED(split, fn); SO_NEED(mv, fn); SO_NEED(qtc, fn); SO_NEED(offs, fn); SO_NEED(out, fn);
    std::vector<PackFrame> fr((size_t)nframes);
    for (int i = 0; i < nframes; ++i) {
        SO_NEED(split[i], fn); SO_NEED(mv[i], fn); SO_NEED(qtc[i], fn); SO_NEED(offs[i], fn); SO_NEED(out[i], fn);
        if (frame_types[i] != 0 && frame_types[i] != 1) {
            set_error("%s: frame_types[%d] = %d", fn, i, frame_types[i]);
            return SO_E_INVALID;
        }
        fr[i] = PackFrame{split[i], mv[i], qtc[i], offs[i], out[i], frame_types[i]};
    }
    if (bits == kHuff) return pack_huff_frames_launch(fr.data(), nframes, nb, bs, cap, totals, (hipStream_t)stream);
    return bits ? pack_bits_frames_launch(fr.data(), nframes, nb, bs, cap, totals, (hipStream_t)stream)
                : pack_frames_launch(fr.data(), nframes, nb, bs, cap, totals, (hipStream_t)stream);
}

static int unpack_frames_any(const char* fn, int bits, int nframes, const int32_t* frame_types,
                             const uint8_t* const* packed, const uint32_t* const* offs, int nb, int bs,
                             uint8_t* const* split, int16_t* const* mv, int16_t* const* qtc, int32_t* err,
                             void* stream) {
    SO_TRY(check_pack_counts(fn, bs, nb, nframes));
    if (nframes == 0) return SO_OK;
    SO_NEED(frame_types, fn); SO_NEED(packed, fn); SO_NEED(offs, fn); SO_NEED(split, fn); SO_NEED(mv, fn);
    SO_NEED(qtc, fn); SO_NEED(err, fn);
    std::vector<UnpackFrame> fr((size_t)nframes);
    for (int i = 0; i < nframes; ++i) {
        SO_NEED(packed[i], fn); SO_NEED(offs[i], fn); SO_NEED(split[i], fn); SO_NEED(mv[i], fn); SO_NEED(qtc[i], fn);
        if (frame_types[i] != 0 && frame_types[i] != 1) {
            set_error("%s: frame_types[%d] = %d", fn, i, frame_types[i]);
            return SO_E_INVALID;
        }
        fr[i] = UnpackFrame{packed[i], offs[i], split[i], mv[i], qtc[i], frame_types[i]};
    }
    if (bits == kHuff) return unpack_huff_frames_launch(fr.data(), nframes, nb, bs, err, (hipStream_t)stream);
    return bits ? unpack_bits_frames_launch(fr.data(), nframes, nb, bs, err, (hipStream_t)stream)
                : unpack_frames_launch(fr.data(), nframes, nb, bs, err, (hipStream_t)stream);
}

int so_pack_frames_ex(int nframes, const int32_t* frame_types, const uint8_t* const* split, const int16_t* const* mv,
                      const int16_t* const* qtc, int nb, int bs, uint32_t* const* offs, uint8_t* const* out,
                      unsigned long long cap, uint32_t* totals, void* stream) {
    return pack_frames_any("so_pack_frames", false, nframes, frame_types, split, mv, qtc, nb, bs, offs, out, cap, totals,
                           stream);
}

int so_unpack_frames(int nframes, const int32_t* frame_types, const uint8_t* const* packed, const uint32_t* const* offs,
                     int nb, int bs, uint8_t* const* split, int16_t* const* mv, int16_t* const* qtc, int32_t* err,
                     void* stream) {
    return unpack_frames_any("so_unpack_frames", false, nframes, frame_types, packed, offs, nb, bs, split, mv, qtc, err,
                             stream);
}

// ---- the same stream in the "bits" coding (so_packbits.hip) ---------------------------------
size_t so_pack_bits_bound(int nb, int bs) {
    if (nb <= 0 || (bs != 16 && bs != 8)) return 0;
    return (size_t)nb * pack_bits_block_bound(bs);
}

int so_pack_frames_bits(int nframes, const int32_t* frame_types, const uint8_t* const* split,
                        const int16_t* const* mv, const int16_t* const* qtc, int nb, int bs, uint32_t* const* offs,
                        uint8_t* const* out, unsigned long long cap, uint32_t* totals, void* stream) {
    return pack_frames_any("so_pack_frames_bits", true, nframes, frame_types, split, mv, qtc, nb, bs, offs, out, cap,
                           totals, stream);
}

int so_unpack_frames_bits(int nframes, const int32_t* frame_types, const uint8_t* const* packed,
                          const uint32_t* const* offs, int nb, int bs, uint8_t* const* split, int16_t* const* mv,
                          int16_t* const* qtc, int32_t* err, void* stream) {
    return unpack_frames_any("so_unpack_frames_bits", true, nframes, frame_types, packed, offs, nb, bs, split, mv, qtc,
                             err, stream);
}

// ---- the same stream in the "huff" coding (so_packhuff.hip) ---------------------------------
size_t so_pack_huff_bound(int nb, int bs) {
    if (nb <= 0 || (bs != 16 && bs != 8)) return 0;
    return (size_t)nb * pack_huff_block_bound(bs) + kHuffLumaTableBytes;
}

int so_pack_frames_huff(int nframes, const int32_t* frame_types, const uint8_t* const* split,
                        const int16_t* const* mv, const int16_t* const* qtc, int nb, int bs, uint32_t* const* offs,
                        uint8_t* const* out, unsigned long long cap, uint32_t* totals, void* stream) {
    return pack_frames_any("so_pack_frames_huff", kHuff, nframes, frame_types, split, mv, qtc, nb, bs, offs, out, cap,
                           totals, stream);
}

int so_unpack_frames_huff(int nframes, const int32_t* frame_types, const uint8_t* const* packed,
                          const uint32_t* const* offs, int nb, int bs, uint8_t* const* split, int16_t* const* mv,
                          int16_t* const* qtc, int32_t* err, void* stream) {
    return unpack_frames_any("so_unpack_frames_huff", kHuff, nframes, frame_types, packed, offs, nb, bs, split, mv, qtc,
                             err, stream);
}

// ---- the chroma coefficients as a packed stream, every coding (so_packchroma.hip, so_packhuff.hip)
size_t so_pack_chroma_bound(int nb) { return nb <= 0 ? 0 : (size_t)nb * pack_chroma_record_bound(false); }
size_t so_pack_chroma_bits_bound(int nb) { return nb <= 0 ? 0 : (size_t)nb * pack_chroma_record_bound(true); }

size_t so_pack_chroma_huff_bound(int nb) {
    return nb <= 0 ? 0 : (size_t)nb * kChromaHuffBound + kHuffChromaTableBytes;
}

static int pack_chroma_any(const char* fn, int bits, int nframes, const int16_t* const* qtc_u,
                           const int16_t* const* qtc_v, int nb, uint32_t* const* offs, uint8_t* const* out,
                           bool after, const uint32_t* const* base, unsigned long long cap, uint32_t* totals,
                           void* stream) {
    SO_TRY(check_pack_counts(fn, 16, nb, nframes));
    if (nframes == 0) return SO_OK;
    SO_NEED(qtc_u, fn); SO_NEED(qtc_v, fn); SO_NEED(offs, fn); SO_NEED(out, fn);
    if (after) SO_NEED(base, fn);
    std::vector<ChromaPackFrame> fr((size_t)nframes);
    for (int i = 0; i < nframes; ++i) {
        SO_NEED(qtc_u[i], fn); SO_NEED(qtc_v[i], fn); SO_NEED(offs[i], fn); SO_NEED(out[i], fn);
        if (after) SO_NEED(base[i], fn);
        fr[i] = ChromaPackFrame{qtc_u[i], qtc_v[i], offs[i], out[i], after ? base[i] : nullptr};
    }
    if (bits == kHuff)
        return pack_chroma_huff_frames_launch(fr.data(), nframes, nb, after, cap, totals, (hipStream_t)stream);
    return pack_chroma_frames_launch(fr.data(), nframes, nb, bits, after, cap, totals, (hipStream_t)stream);
}

static int unpack_chroma_any(const char* fn, int bits, int nframes, const uint8_t* const* packed,
                             const uint32_t* const* offs, int nb, int16_t* const* qtc_u, int16_t* const* qtc_v,
                             int32_t* err, void* stream) {
    SO_TRY(check_pack_counts(fn, 16, nb, nframes));
    if (nframes == 0) return SO_OK;
    SO_NEED(packed, fn); SO_NEED(offs, fn); SO_NEED(qtc_u, fn); SO_NEED(qtc_v, fn); SO_NEED(err, fn);
    std::vector<ChromaUnpackFrame> fr((size_t)nframes);
    for (int i = 0; i < nframes; ++i) {
        SO_NEED(packed[i], fn); SO_NEED(offs[i], fn); SO_NEED(qtc_u[i], fn); SO_NEED(qtc_v[i], fn);
        fr[i] = ChromaUnpackFrame{packed[i], offs[i], qtc_u[i], qtc_v[i]};
    }
    if (bits == kHuff) return unpack_chroma_huff_frames_launch(fr.data(), nframes, nb, err, (hipStream_t)stream);
    return unpack_chroma_frames_launch(fr.data(), nframes, nb, bits, err, (hipStream_t)stream);
}

int so_pack_chroma_frames(int nframes, const int16_t* const* qtc_u, const int16_t* const* qtc_v, int nb,
                          uint32_t* const* offs, uint8_t* const* out, unsigned long long cap, uint32_t* totals,
                          void* stream) {
    return pack_chroma_any("so_pack_chroma_frames", false, nframes, qtc_u, qtc_v, nb, offs, out, false, nullptr, cap,
                           totals, stream);
}

int so_pack_chroma_frames_bits(int nframes, const int16_t* const* qtc_u, const int16_t* const* qtc_v, int nb,
                               uint32_t* const* offs, uint8_t* const* out, unsigned long long cap, uint32_t* totals,
                               void* stream) {
    return pack_chroma_any("so_pack_chroma_frames_bits", true, nframes, qtc_u, qtc_v, nb, offs, out, false, nullptr,
                           cap, totals, stream);
}

int so_pack_chroma_frames_after(int nframes, const int16_t* const* qtc_u, const int16_t* const* qtc_v, int nb,
                                uint32_t* const* offs, uint8_t* const* out, const uint32_t* const* base,
                                unsigned long long cap, uint32_t* totals, void* stream) {
    return pack_chroma_any("so_pack_chroma_frames_after", false, nframes, qtc_u, qtc_v, nb, offs, out, true, base, cap,
                           totals, stream);
}

int so_pack_chroma_frames_bits_after(int nframes, const int16_t* const* qtc_u, const int16_t* const* qtc_v, int nb,
                                     uint32_t* const* offs, uint8_t* const* out, const uint32_t* const* base,
                                     unsigned long long cap, uint32_t* totals, void* stream) {
    return pack_chroma_any("so_pack_chroma_frames_bits_after", true, nframes, qtc_u, qtc_v, nb, offs, out, true, base,
                           cap, totals, stream);
}

int so_unpack_chroma_frames(int nframes, const uint8_t* const* packed, const uint32_t* const* offs, int nb,
                            int16_t* const* qtc_u, int16_t* const* qtc_v, int32_t* err, void* stream) {
    return unpack_chroma_any("so_unpack_chroma_frames", false, nframes, packed, offs, nb, qtc_u, qtc_v, err, stream);
}

int so_unpack_chroma_frames_bits(int nframes, const uint8_t* const* packed, const uint32_t* const* offs, int nb,
                                 int16_t* const* qtc_u, int16_t* const* qtc_v, int32_t* err, void* stream) {
    return unpack_chroma_any("so_unpack_chroma_frames_bits", true, nframes, packed, offs, nb, qtc_u, qtc_v, err,
                             stream);
}

int so_pack_chroma_frames_huff(int nframes, const int16_t* const* qtc_u, const int16_t* const* qtc_v, int nb,
                               uint32_t* const* offs, uint8_t* const* out, unsigned long long cap, uint32_t* totals,
                               void* stream) {
    return pack_chroma_any("so_pack_chroma_frames_huff", kHuff, nframes, qtc_u, qtc_v, nb, offs, out, false, nullptr,
                           cap, totals, stream);
}

int so_pack_chroma_frames_huff_after(int nframes, const int16_t* const* qtc_u, const int16_t* const* qtc_v, int nb,
                                     uint32_t* const* offs, uint8_t* const* out, const uint32_t* const* base,
                                     unsigned long long cap, uint32_t* totals, void* stream) {
    return pack_chroma_any("so_pack_chroma_frames_huff_after", kHuff, nframes, qtc_u, qtc_v, nb, offs, out, true, base,
                           cap, totals, stream);
}

int so_unpack_chroma_frames_huff(int nframes, const uint8_t* const* packed, const uint32_t* const* offs, int nb,
                                 int16_t* const* qtc_u, int16_t* const* qtc_v, int32_t* err, void* stream) {
    return unpack_chroma_any("so_unpack_chroma_frames_huff", kHuff, nframes, packed, offs, nb, qtc_u, qtc_v, err,
                             stream);
}

}  // extern "C"
