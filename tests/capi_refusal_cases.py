"""The refusal matrix of the C boundary: for every validating entry point of so_capi.hip, and for
so_decode_p_frames / so_decode_chroma_frames, calls that are refused on the host -- one per check,
plus the orderings a call with several faults must keep.  Addresses are made up: no case may get
as far as a launch (tests/golden/record_capi_refusals.py refuses to record one that does).

cases() returns [(id, function name, ctypes arguments)].  Every entry point has a valid base call
(`_BASE`); a case is that call with some arguments replaced.
"""
import ctypes

N = 2                  # frames per call
H, W = 64, 128         # 4 x 8 blocks of 16
NB = (H // 16) * (W // 16)
STRIDE = H * W
LAND0 = 0x40000000     # the frame pipeline's landing planes
BIG = (65536, 32896)   # H x W beyond 2^31 samples, multiples of 128


def P(k):
    """A made-up 256-byte aligned device address, distinct per k and 16 MiB apart."""
    return 0x1000000 * (k + 1)


class A(list):
    """A host array of pointers (None: NULL)."""


class I(list):   # noqa: E742
    """A host array of int32."""


def _c(v):
    if isinstance(v, A):
        return (ctypes.c_void_p * max(len(v), 1))(*v)
    if isinstance(v, I):
        return (ctypes.c_int32 * max(len(v), 1))(*v)
    return v


def _pp(k):
    return A([P(k), P(k) + 0x400000])


def _outs(k0):
    """The seven per-frame output arrays of a run, from address k0."""
    return [("out_split", _pp(k0)), ("out_mv", _pp(k0 + 1)), ("out_qtc", _pp(k0 + 2)), ("out_tokens", _pp(k0 + 3)),
            ("out_mae_num", _pp(k0 + 4)), ("out_recon", _pp(k0 + 5)), ("out_sse", _pp(k0 + 6))]


def _out1(k0):
    return [("out_split", P(k0)), ("out_mv", P(k0 + 1)), ("out_qtc", P(k0 + 2)), ("out_tokens", P(k0 + 3)),
            ("out_mae_num", P(k0 + 4)), ("out_recon", P(k0 + 5)), ("out_sse", P(k0 + 6))]


_GEOM = [("H", H), ("W", W), ("bs", 16)]
_LAND = [("land0", LAND0), ("land_flags", P(40)), ("slot0", 0), ("peer_land0", P(41)), ("peer_flags", P(42)),
         ("peer2_land0", P(43)), ("peer2_flags", P(44)), ("push_to", I([0, 2])), ("nslots", 3), ("stride", STRIDE),
         ("epoch", 1), ("max_wg", 0)]
_TABLES = [(f"{k}_{t}", v) for t, p in (("yh", 50), ("yv", 53), ("ch", 56), ("cv", 59))
           for k, v in (("coef", P(p)), ("first", P(p + 1)), ("taps", 4))]
_PACK = [("nframes", N), ("frame_types", I([0, 1])), ("split", _pp(1)), ("mv", _pp(2)), ("qtc", _pp(3)), ("nb", NB),
         ("bs", 16), ("offs", _pp(4)), ("out", _pp(5)), ("cap", 1 << 20)]
_UNPACK = [("nframes", N), ("frame_types", I([0, 1])), ("packed", _pp(1)), ("offs", _pp(2)), ("nb", NB), ("bs", 16),
           ("split", _pp(3)), ("mv", _pp(4)), ("qtc", _pp(5)), ("err", P(6)), ("stream", None)]
_CPACK = [("nframes", N), ("qtc_u", _pp(1)), ("qtc_v", _pp(2)), ("nb", NB), ("offs", _pp(3)), ("out", _pp(4))]
_CUNPACK = [("nframes", N), ("packed", _pp(1)), ("offs", _pp(2)), ("nb", NB), ("qtc_u", _pp(3)), ("qtc_v", _pp(4)),
            ("err", P(5)), ("stream", None)]
_CHROMA = [("refs_u", A([P(2)])), ("refs_v", A([P(3)])), ("nref", 1), *_GEOM, ("frame_type", 1), ("split", P(4)),
           ("mv", P(5)), ("qp", 4), ("qp_row", None), ("qp_map", None), ("qp_offset", 0)]

_BASE = {
    "so_set_option": [("opt", 1), ("value", 1)],
    "so_me_full_search": [("cur", P(0)), ("refs", A([P(1)])), ("nref", 1), *_GEOM, ("sr", 16), ("out_best", P(2)),
                          ("out_sub", None), ("stream", None)],
    "so_inter_tq_recon": [("cur", P(0)), ("refs", A([P(1)])), ("nref", 1), *_GEOM, ("best", P(2)), ("sub", None),
                          ("qp_rd", 4), ("qp_row", None), ("vbs", 0), ("lam", 0.0), *_out1(10), ("stream", None)],
    "so_encode_p_frame": [("cur", P(0)), ("refs", A([P(1)])), ("nref", 1), *_GEOM, ("sr", 16), ("qp_rd", 4),
                          ("qp_row", None), ("vbs", 0), ("lam", 0.0), *_out1(10), ("scratch", P(3)), ("stream", None)],
    "so_encode_p_rows": [("cur", P(0)), ("refs", A([P(1)])), ("nref", 1), *_GEOM, ("sr", 16), ("by0", 0), ("by1", 4),
                         ("qp_rd", 4), ("qp_row", None), ("vbs", 0), ("lam", 0.0), *_out1(10), ("scratch", P(3)),
                         ("stream", None)],
    "so_encode_p_rows_ex": [("cur", P(0)), ("refs", A([P(1)])), ("nref", 1), *_GEOM, ("sr", 16), ("by0", 0),
                            ("by1", 4), ("qp_rd", 4), ("qp_row", None), ("qp_map", P(4)), ("vbs", 0), ("lam", 0.0),
                            ("me_mode", 0), ("fme", 0), ("fme_wrap", 1), ("fme_planes", None), ("flags", 0),
                            *_out1(10), ("scratch", P(3)), ("stream", None)],
    "so_me_search_ex": [("cur", P(0)), ("refs", A([P(1)])), ("nref", 1), *_GEOM, ("sr", 16), ("me_mode", 0),
                        ("fme", 0), ("fme_wrap", 1), ("fme_planes", None), ("out_best", P(2)), ("out_sub", None),
                        ("stream", None)],
    "so_p_run_tile_rows": [("H", H), ("W", W), ("conc", 1)],
    "so_p_run_mode_resident_workgroups": [("mode", 0), ("vbs", 0)],
    "so_encode_p_run": [("curs", _pp(0)), ("nframes", N), ("ref0", P(1)), *_GEOM, ("sr", 16), ("qp_rd", 4),
                        ("qp_row", None), ("vbs", 0), ("lam", 0.0), *_outs(10), ("workspace", P(3)),
                        ("stream", None)],
    "so_encode_p_runs": [("curs", _pp(0)), ("nframes", N), ("refs", A([P(1), None])), ("ref_frame", I([-1, 0])),
                         *_GEOM, ("sr", 16), ("qp_rd", 4), ("qp_row", None), ("vbs", 0), ("lam", 0.0), *_outs(10),
                         ("workspace", P(3)), ("stream", None)],
    "so_encode_p_run_2pass": [("curs", _pp(0)), ("nframes", N), ("ref0", P(1)), *_GEOM, ("sr", 16), ("qp_rd", 4),
                              ("qp_row", None), ("roi", None), ("qp_lo", 0), ("qp_hi", 12), *_outs(10),
                              ("out_qp_map", _pp(17)), ("workspace", P(3)), ("stream", None)],
    "so_encode_p_run_stripe": [("curs", _pp(0)), ("nframes", N), ("ref0", P(1)), *_GEOM, ("sr", 16), ("by0", 1),
                               ("by1", 3), ("qp_rd", 4), ("qp_row", None), *_outs(10), ("workspace", P(3)),
                               ("gbase", 1), ("peer_up0", P(30)), ("peer_dn0", P(31)), ("stride", STRIDE),
                               ("my_up_flags", P(32)), ("my_dn_flags", P(33)), ("peer_up_flags", P(34)),
                               ("peer_dn_flags", P(35)), ("epoch", 1), ("max_wg", 0), ("stream", None)],
    "so_stripe_halo_push": [("plane", P(0)), ("H", H), ("W", W), ("by0", 1), ("by1", 3), ("gf", 0), ("peer_up", P(1)),
                            ("peer_dn", P(2)), ("peer_up_flags", P(3)), ("peer_dn_flags", P(4)), ("epoch", 1),
                            ("stream", None)],
    "so_encode_p_run_fpipe2": [("curs", _pp(0)), ("nframes", N), *_GEOM, ("sr", 16), ("qp_rd", 4), ("qp_row", None),
                               ("vbs", 0), ("lam", 0.0), *_outs(10), ("workspace", P(3)), *_LAND, ("stream", None)],
    "so_encode_p_run_fpipe_2pass": [("curs", _pp(0)), ("nframes", N), *_GEOM, ("sr", 16), ("qp_rd", 4),
                                    ("qp_row", None), ("roi", None), ("qp_lo", 0), ("qp_hi", 12), *_outs(10),
                                    ("out_qp_map", _pp(17)), ("workspace", P(3)), *_LAND, ("p2lag", 0),
                                    ("stream", None)],
    "so_frame_push": [("plane", P(0)), ("H", H), ("W", W), ("peer_plane", P(1)), ("peer_flags", P(2)), ("epoch", 1),
                      ("stream", None)],
    "so_alloc_uncached": [("bytes", 4096), ("out", ctypes.pointer(ctypes.c_void_p()))],
    "so_ipc_export": [("p", P(0)), ("out_handle", P(1))],
    "so_ipc_open": [("handle", P(0)), ("out", ctypes.pointer(ctypes.c_void_p()))],
    "so_copy_d2d": [("dst", P(0)), ("src", P(1)), ("bytes", 16), ("stream", None)],
    "so_encode_i_frame": [("cur", P(0)), *_GEOM, ("sr", 16), ("qp_rd", 4), ("qp_row", None), ("vbs", 0), ("lam", 0.0),
                          *_out1(10), ("scratch", P(3)), ("stream", None)],
    "so_encode_i_rows": [("cur", P(0)), *_GEOM, ("sr", 16), ("by0", 0), ("by1", 4), ("qp_rd", 4), ("qp_row", None),
                         ("vbs", 0), ("lam", 0.0), *_out1(10), ("scratch", P(3)), ("stream", None)],
    "so_encode_i_rows_ex": [("cur", P(0)), *_GEOM, ("sr", 16), ("by0", 0), ("by1", 4), ("qp_rd", 4), ("qp_row", None),
                            ("qp_map", P(4)), ("vbs", 0), ("lam", 0.0), *_out1(10), ("scratch", P(3)),
                            ("stream", None)],
    "so_inter_recon": [("refs", A([P(1)])), ("nref", 1), *_GEOM, ("qp", 4), ("qp_row", None), ("split", P(2)),
                       ("mv", P(3)), ("qtc", P(4)), ("out_recon", P(5)), ("stream", None)],
    "so_inter_recon_ex": [("refs", A([P(1)])), ("nref", 1), *_GEOM, ("qp", 4), ("qp_row", None), ("qp_map", P(6)),
                          ("fme", 0), ("fme_wrap", 1), ("fme_planes", None), ("split", P(2)), ("mv", P(3)),
                          ("qtc", P(4)), ("out_recon", P(5)), ("stream", None)],
    "so_intra_recon": [*_GEOM, ("qp", 4), ("qp_row", None), ("split", P(2)), ("mv", P(3)), ("qtc", P(4)),
                       ("out_recon", P(5)), ("scratch", P(6)), ("stream", None)],
    "so_intra_recon_ex": [*_GEOM, ("qp", 4), ("qp_row", None), ("qp_map", P(7)), ("split", P(2)), ("mv", P(3)),
                          ("qtc", P(4)), ("out_recon", P(5)), ("scratch", P(6)), ("stream", None)],
    "so_fme_planes": [("ref", P(0)), ("H", H), ("W", W), ("wrap", 1), ("out_planes", P(1)), ("stream", None)],
    "so_qp_map": [("tokens", P(0)), *_GEOM, ("by0", 0), ("by1", 4), ("qp_rd", 4), ("qp_row", None), ("roi", None),
                  ("qp_lo", 0), ("qp_hi", 12), ("out_qp_map", P(1)), ("stream", None)],
    "so_sum_i32_rows": [("rows", _pp(0)), ("n", N), ("len", 32), ("out", P(1)), ("stream", None)],
    "so_sse_u8": [("a", P(0)), ("b", P(1)), ("n", 4096), ("out_sse", P(2)), ("stream", None)],
    "so_ssim_u8": [("a", _pp(0)), ("b", _pp(1)), ("nframes", N), ("H", H), ("W", W), ("pitch_a", W), ("pitch_b", W),
                   ("win", 11), ("out", P(2)), ("workspace", P(3)), ("stream", None)],
    "so_rgb_to_yuv420": [("rgb", _pp(0)), ("nframes", N), ("h", 60), ("w", 120), ("layout", 0), ("pitch", 360),
                         ("plane_stride", 0), ("matrix", 0), ("full_range", 0), ("Hp", H), ("Wp", W), ("y", _pp(1)),
                         ("u", _pp(2)), ("v", _pp(3)), ("stream", None)],
    "so_yuv420_to_rgb": [("y", _pp(1)), ("u", _pp(2)), ("v", _pp(3)), ("nframes", N), ("Hp", H), ("Wp", W), ("h", 60),
                         ("w", 120), ("matrix", 0), ("full_range", 0), ("layout", 0), ("rgb", _pp(0)), ("pitch", 360),
                         ("plane_stride", 0), ("stream", None)],
    "so_scale_yuv420": [("sy", _pp(0)), ("su", _pp(1)), ("sv", _pp(2)), ("nframes", N), ("hs", 120), ("ws", 240),
                        ("pitch_y", 240), ("pitch_c", 120), ("dy", _pp(3)), ("du", _pp(4)), ("dv", _pp(5)),
                        ("hd", 60), ("wd", 120), ("Hp", H), ("Wp", W), *_TABLES, ("stream", None)],
    "so_chroma_encode_frame": [("cur_u", P(0)), ("cur_v", P(1)), *_CHROMA, ("out_qtc_u", P(6)), ("out_qtc_v", P(7)),
                               ("out_tokens", P(8)), ("out_recon_u", P(9)), ("out_recon_v", P(10)), ("out_sse", P(11)),
                               ("stream", None)],
    "so_chroma_recon_frame": [*_CHROMA, ("qtc_u", P(6)), ("qtc_v", P(7)), ("out_recon_u", P(9)), ("out_recon_v", P(10)),
                              ("stream", None)],
    "so_pack_frames": [*_PACK, ("stream", None)],
    "so_pack_frames_ex": [*_PACK, ("totals", None), ("stream", None)],
    "so_pack_frames_bits": [*_PACK, ("totals", None), ("stream", None)],
    "so_unpack_frames": _UNPACK,
    "so_unpack_frames_bits": _UNPACK,
    "so_pack_chroma_frames": [*_CPACK, ("cap", 1 << 20), ("totals", None), ("stream", None)],
    "so_pack_chroma_frames_bits": [*_CPACK, ("cap", 1 << 20), ("totals", None), ("stream", None)],
    "so_pack_chroma_frames_after": [*_CPACK, ("base", _pp(5)), ("cap", 1 << 20), ("totals", None), ("stream", None)],
    "so_pack_chroma_frames_bits_after": [*_CPACK, ("base", _pp(5)), ("cap", 1 << 20), ("totals", None),
                                         ("stream", None)],
    "so_unpack_chroma_frames": _CUNPACK,
    "so_unpack_chroma_frames_bits": _CUNPACK,
    "so_decode_p_frames": [("nframes", N), ("coding", 1), ("packed", _pp(0)), ("offs", _pp(1)), *_GEOM, ("qp", 4),
                           ("qp_row", None), ("qp_map", None), ("refs0", A([P(2)])), ("nref0", 1), ("nref_max", 2),
                           ("out_split", _pp(3)), ("out_mv", _pp(4)), ("out_recon", _pp(5)), ("err", P(6)),
                           ("stream", None)],
    "so_decode_chroma_frames": [("nframes", N), ("coding", 1), ("frame_types", I([1, 1])), ("packed", _pp(0)),
                                ("offs", _pp(1)), *_GEOM, ("split", _pp(2)), ("mv", _pp(3)), ("qp", 4),
                                ("qp_row", None), ("qp_map", None), ("qp_offset", 0), ("refs0_u", A([P(4)])),
                                ("refs0_v", A([P(5)])), ("nref0", 1), ("nref_max", 2), ("out_recon_u", _pp(6)),
                                ("out_recon_v", _pp(7)), ("err", P(8)), ("stream", None)],
}

_RUNS = ("so_encode_p_run", "so_encode_p_runs", "so_encode_p_run_2pass", "so_encode_p_run_stripe",
         "so_encode_p_run_fpipe2", "so_encode_p_run_fpipe_2pass")


def _ptr_names(fn):
    """(scalar pointers, pointer arrays) of fn's base call that are given."""
    scal = [k for k, v in _BASE[fn] if isinstance(v, int) and not isinstance(v, bool) and v >= 0x1000000]
    arrs = [k for k, v in _BASE[fn] if isinstance(v, A)]
    return scal, arrs


def _with(arr, i, v):
    out = type(arr)(arr)
    out[i] = v
    return out


def _table():
    """[(function, label, {argument: value})]"""
    t = []

    def add(fn, label, **over):
        t.append((fn, label, over))

    # every pointer NULL in turn, and for an array its first and its last entry
    for fn in _BASE:
        if fn in ("so_set_option", "so_p_run_tile_rows", "so_p_run_mode_resident_workgroups"):
            continue
        base = dict(_BASE[fn])
        scal, arrs = _ptr_names(fn)
        optional = {"qp_map"}   # arguments that may be NULL
        if fn not in ("so_chroma_encode_frame", "so_sse_u8"):
            optional.add("out_sse")
        if fn == "so_qp_map":
            optional.add("tokens")
        for k in scal:
            if k not in optional:
                add(fn, f"null {k}", **{k: None})
        for k, v in base.items():
            if isinstance(v, I):
                add(fn, f"null {k}", **{k: None})
        for k in arrs:
            if k in optional:
                continue
            add(fn, f"null {k}", **{k: None})
            add(fn, f"null {k}[0]", **{k: _with(base[k], 0, None)})
            if len(base[k]) > 1 and base[k][-1] is not None:
                add(fn, f"null {k}[last]", **{k: _with(base[k], len(base[k]) - 1, None)})

    # geometry, search range, QP, VBS: each caller of the shared checks
    for fn in _BASE:
        names = [k for k, _ in _BASE[fn]]

        def add(fn, label, names=names, **over):   # noqa: F811  (only what the entry point takes)
            if set(over) <= set(names):
                t.append((fn, label, over))
        if "bs" in names:
            add(fn, "bs 12", bs=12)
            add(fn, "bs 0", bs=0)
            add(fn, "H 60", H=60)
            add(fn, "W 0", W=0)
            if fn != "so_qp_map":   # which has a geometry rule of its own, and no QP check
                add(fn, "too large", H=BIG[0], W=BIG[1])
        if "sr" in names:
            add(fn, "sr 65", sr=65)
            add(fn, "sr -1", sr=-1)
        for q in ("qp_rd", "qp"):
            if q in names and fn != "so_qp_map":
                add(fn, f"{q} 21", **{q: 21})
                add(fn, f"{q} -1", **{q: -1})
        if "vbs" in names:
            add(fn, "vbs bs 8", vbs=1, bs=8)
        if "vbs" in names and fn in _RUNS:   # only the runs check the flag and lambda
            add(fn, "vbs 2", vbs=2)
            add(fn, "vbs lambda nan", vbs=1, lam=float("nan"))
            add(fn, "vbs lambda inf", vbs=1, lam=float("inf"))
            add(fn, "vbs lambda < 0", vbs=1, lam=-1.0)
        if "by0" in names and "gbase" not in names and "gf" not in names:
            add(fn, "by0 -1", by0=-1)
            add(fn, "by1 < by0", by0=2, by1=1)
            add(fn, "by1 past", by1=5)
        if fn in _RUNS:   # the one configuration the run kernels cover
            add(fn, "bs 8", bs=8)
            add(fn, "sr 8", sr=8)
            add(fn, "W 96", W=96)
            if "qp_lo" in names:
                add(fn, "W 8320", W=8320)
        if "qp_lo" in names:
            add(fn, "clamp lo > hi", qp_lo=5, qp_hi=3)
            add(fn, "clamp lo < 0", qp_lo=-1)
            add(fn, "clamp hi > 20", qp_hi=21)
        if "nref" in names:
            add(fn, "nref 0", nref=0)
            add(fn, "nref 5", nref=5)
        if "nframes" in names:
            add(fn, "nframes -1", nframes=-1)

    def add(fn, label, **over):   # noqa: F811
        t.append((fn, label, over))

    # the orderings the run entry points keep
    for fn in _RUNS:
        base = dict(_BASE[fn])
        names = list(base)
        nulls = {k: None for k, v in base.items() if isinstance(v, (A, I)) or (isinstance(v, int) and v >= 0x1000000)}
        add(fn, "order: geometry before QP", H=60, qp_rd=21)
        if "vbs" in names:
            add(fn, "order: vbs 2 before search range", vbs=2, sr=65)
        if "qp_lo" in names:
            add(fn, "order: width before clamp", W=96, qp_lo=5, qp_hi=3)
            add(fn, "order: two-pass width before clamp", W=8320, qp_lo=5, qp_hi=3)
        add(fn, "order: search range before QP", sr=65, qp_rd=21)
        add(fn, "order: QP before covers", qp_rd=21, W=96)
        add(fn, "nframes 0, all NULL", nframes=0, **nulls)
        add(fn, "nframes 0, bad geometry", nframes=0, H=60, **nulls)
        add(fn, "order: frame 0 NULL before frame 1 NULL", out_mv=_with(base["out_mv"], 0, None),
            out_split=_with(base["out_split"], 1, None))
        add(fn, "order: out_split before workspace", out_split=None, workspace=None)
        add(fn, "order: curs before out_recon", curs=None, out_recon=None)
    for fn in ("so_encode_p_run", "so_encode_p_run_2pass"):
        rec = dict(_BASE[fn])["out_recon"]
        add(fn, "recon[0] aliases ref0", out_recon=_with(rec, 0, P(1)))
        add(fn, "recon[1] aliases ref0", out_recon=_with(rec, 1, P(1)))
        add(fn, "recon[1] aliases recon[0]", out_recon=A([rec[0], rec[0]]))
        add(fn, "order: frame 0 alias before frame 1 NULL", out_recon=_with(rec, 0, P(1)),
            out_split=_with(dict(_BASE[fn])["out_split"], 1, None))
        add(fn, "order: ref0 before out_split", ref0=None, out_split=None)
    add("so_encode_p_run_2pass", "order: out_qp_map before workspace", out_qp_map=None, workspace=None)
    add("so_encode_p_run_fpipe_2pass", "order: workspace before out_qp_map", out_qp_map=None, workspace=None)
    add("so_encode_p_run_fpipe_2pass", "order: push_to before out_qp_map", out_qp_map=None, push_to=None)

    fn = "so_encode_p_runs"
    rec = dict(_BASE[fn])["out_recon"]
    add(fn, "ref_frame later", ref_frame=I([-1, 1]))
    add(fn, "ref_frame -2", ref_frame=I([-2, 0]))
    add(fn, "ref_frame[1] -1 without refs[1]", ref_frame=I([-1, -1]))
    add(fn, "recon[0] aliases refs[0]", out_recon=_with(rec, 0, P(1)))
    add(fn, "recon[1] aliases refs[0]", out_recon=_with(rec, 1, P(1)))
    add(fn, "recon[0] aliases recon[1]", out_recon=A([rec[1], rec[1]]))
    add(fn, "order: frame 0 alias before frame 1 NULL", out_recon=_with(rec, 0, P(1)),
        out_split=_with(dict(_BASE[fn])["out_split"], 1, None))
    add(fn, "order: refs before ref_frame", refs=None, ref_frame=None)
    add(fn, "order: ref_frame before out_split", ref_frame=None, out_split=None)

    fn = "so_encode_p_run_stripe"
    add(fn, "by0 -1", by0=-1)
    add(fn, "by1 past", by1=5)
    add(fn, "by1 == by0", by0=2, by1=2)
    add(fn, "gbase 0", gbase=0)
    add(fn, "peer_up0 without flags", peer_up_flags=None)
    add(fn, "peer_dn0 without my flags", my_dn_flags=None)
    add(fn, "up neighbour at the top edge", by0=0)
    add(fn, "down neighbour at the bottom edge", by1=4)
    add(fn, "order: stripe before nframes 0", nframes=0, by0=-1)
    add(fn, "order: curs[0] before curs[1]", curs=A([None, None]))

    fn = "so_stripe_halo_push"
    add(fn, "W 96", W=96)
    add(fn, "by0 -1", by0=-1)
    add(fn, "by1 past", by1=5)
    add(fn, "by1 == by0", by0=2, by1=2)
    add(fn, "gf -1", gf=-1)
    add(fn, "H 60", H=60)
    add(fn, "peer_up without flags", peer_up_flags=None)
    add(fn, "flags without peer_dn", peer_dn=None)
    add(fn, "no peers", peer_up=None, peer_dn=None, peer_up_flags=None, peer_dn_flags=None)

    for fn in ("so_encode_p_run_fpipe2", "so_encode_p_run_fpipe_2pass"):
        rec = dict(_BASE[fn])["out_recon"]
        add(fn, "stride short", stride=STRIDE - 1)
        add(fn, "slot0 -1", slot0=-1)
        add(fn, "nslots 0", nslots=0)
        add(fn, "run past the slots", slot0=2)
        add(fn, "push_to[0] -2", push_to=I([-2, 2]))
        add(fn, "push_to[1] -2", push_to=I([0, -2]))
        add(fn, "push_to[1] past the slots", push_to=I([0, 6]))
        add(fn, "recon[0] in the landing planes", out_recon=_with(rec, 0, LAND0))
        add(fn, "recon[1] in the landing planes", out_recon=_with(rec, 1, LAND0 + STRIDE))
        add(fn, "order: slots before nframes 0", nframes=0, slot0=-1)
        add(fn, "order: landing before push_to", out_recon=_with(rec, 0, LAND0), push_to=I([-2, 2]))
        add(fn, "order: frame 0 landing before frame 1 NULL", out_recon=_with(rec, 0, LAND0),
            out_split=_with(dict(_BASE[fn])["out_split"], 1, None))
    add("so_encode_p_run_fpipe_2pass", "p2lag -1", p2lag=-1)
    add("so_encode_p_run_fpipe_2pass", "order: clamp before p2lag", p2lag=-1, qp_lo=5, qp_hi=3)
    add("so_encode_p_run_fpipe_2pass", "order: p2lag before slots", p2lag=-1, slot0=-1)

    add("so_frame_push", "H 60", H=60)
    add("so_frame_push", "W 96", W=96)
    add("so_set_option", "unknown option", opt=99)
    add("so_set_option", "option 0", opt=0)
    add("so_set_option", "value 2", value=2)
    add("so_set_option", "tall tiles -2", opt=8, value=-2)
    add("so_set_option", "segment 0", opt=3, value=0)
    add("so_set_option", "warmup -1", opt=4, value=-1)
    add("so_p_run_tile_rows", "H 8", H=8)
    add("so_p_run_tile_rows", "W 96", W=96)
    add("so_p_run_tile_rows", "conc 0", conc=0)
    add("so_p_run_mode_resident_workgroups", "mode 5", mode=5)
    add("so_p_run_mode_resident_workgroups", "mode -1", mode=-1)
    add("so_p_run_mode_resident_workgroups", "mode 1 with vbs", mode=1, vbs=1)
    add("so_alloc_uncached", "bytes 0", bytes=0)
    add("so_alloc_uncached", "null out", out=None)
    add("so_ipc_open", "null out", out=None)

    # the reconstruction against the references, and the _ex pairs
    for fn in ("so_inter_tq_recon", "so_encode_p_rows", "so_encode_p_rows_ex", "so_encode_p_frame"):
        add(fn, "recon aliases refs[0]", out_recon=P(1))
        add(fn, "recon aliases refs[1]", refs=A([P(1), P(5)]), nref=2, out_recon=P(5))
        add(fn, "order: refs[1] NULL before alias", refs=A([P(1), None]), nref=2, out_recon=P(1))
    add("so_inter_tq_recon", "vbs without sub", vbs=1, lam=1.0)
    add("so_me_full_search", "sub with bs 8", out_sub=P(3), bs=8)
    add("so_encode_p_rows_ex", "defaults, bs 12: reported as so_encode_p_rows", qp_map=None, bs=12)
    add("so_encode_p_rows_ex", "defaults, null cur", qp_map=None, cur=None)
    add("so_encode_p_rows_ex", "defaults, recon aliases refs[0]", qp_map=None, out_recon=P(1))
    add("so_encode_p_rows_ex", "tokens only, bs 12", qp_map=None, flags=2, bs=12)
    add("so_encode_p_rows_ex", "reuse with fme, no planes", flags=1, fme=1)
    add("so_encode_p_rows_ex", "me_mode 3", me_mode=3)
    add("so_encode_p_rows_ex", "me_mode -1", me_mode=-1)
    add("so_encode_p_rows_ex", "fast parallel with vbs", me_mode=2, vbs=1, lam=1.0)
    add("so_encode_p_rows_ex", "fast in a stripe", me_mode=1, by0=1)
    add("so_encode_p_rows_ex", "fme without planes", fme=1, sr=8)
    add("so_encode_p_rows_ex", "fme sr 64", fme=1, fme_planes=P(6), sr=64)
    add("so_me_search_ex", "me_mode 3", me_mode=3)
    add("so_me_search_ex", "fast parallel with sub", me_mode=2, out_sub=P(3))
    add("so_me_search_ex", "fme without planes", fme=1)
    add("so_me_search_ex", "fme sr 64", fme=1, fme_planes=P(6), sr=64)
    add("so_inter_recon_ex", "fme without planes", fme=1)
    for fn in ("so_encode_i_rows", "so_encode_i_rows_ex", "so_encode_i_frame", "so_intra_recon", "so_intra_recon_ex"):
        add(fn, "W 8208", W=8208)
        add(fn, "order: geometry before width", W=8200)
    add("so_fme_planes", "H 1", H=1)
    add("so_fme_planes", "W 126", W=126)
    add("so_fme_planes", "order: NULL before geometry", ref=None, W=126)

    fn = "so_qp_map"
    add(fn, "order: geometry before rows", H=60, by1=9)
    add(fn, "order: rows before out_qp_map", by1=5, out_qp_map=None)
    add(fn, "order: out_qp_map before clamp", out_qp_map=None, qp_lo=5, qp_hi=3)
    add(fn, "no rows", by0=2, by1=2)
    add("so_sum_i32_rows", "n -1", n=-1)
    add("so_sum_i32_rows", "len -1", len=-1)
    add("so_sum_i32_rows", "n 0", n=0, rows=None, out=None)
    add("so_sse_u8", "n -1", n=-1)
    add("so_sse_u8", "a unaligned", a=P(0) + 8)
    add("so_sse_u8", "b unaligned", b=P(1) + 1)
    fn = "so_ssim_u8"
    add(fn, "win 2", win=2)
    add(fn, "win 12", win=12)
    add(fn, "win 17", win=17)
    add(fn, "H below win", H=8)
    add(fn, "too large", H=BIG[0], W=BIG[1], pitch_a=BIG[1], pitch_b=BIG[1])
    add(fn, "pitch_a short", pitch_a=W - 1)
    add(fn, "pitch_b short", pitch_b=W - 1)
    add(fn, "nframes 0", nframes=0, a=None, b=None, out=None, workspace=None)

    # colour: the scalar checks, then the alias sweep
    y = dict(_BASE["so_rgb_to_yuv420"])["y"]
    rgb = dict(_BASE["so_rgb_to_yuv420"])["rgb"]
    ny, view = H * W, 59 * 360 + 360
    for fn in ("so_rgb_to_yuv420", "so_yuv420_to_rgb"):
        fwd = fn == "so_rgb_to_yuv420"
        add(fn, "h odd", h=59)
        add(fn, "w 0", w=0)
        add(fn, "Hp below h", Hp=32)
        add(fn, "Wp odd", Wp=129)
        add(fn, "too large", Hp=BIG[0], Wp=BIG[1])
        add(fn, "layout 2", layout=2)
        add(fn, "pitch short", pitch=359)
        add(fn, "chw without plane stride", layout=1, pitch=120)
        add(fn, "matrix 2", matrix=2)
        add(fn, "full_range 2", full_range=2)
        add(fn, "nframes 0", nframes=0, rgb=None, y=None, u=None, v=None)
        add(fn, "order: geometry before nframes 0", nframes=0, h=59)
        # sources may repeat: accepted up to the NULL check that follows cannot be shown without a
        # launch, so the repeated source comes with a NULL that is found first in argument order
        if fwd:
            add(fn, "repeated source then NULL v[1]", rgb=A([rgb[0], rgb[0]]), v=A([P(3), None]))
            add(fn, "y[1] over rgb[0]", y=_with(y, 1, rgb[0] + 100))
            add(fn, "rgb[1] ends inside y[0]", rgb=_with(rgb, 1, y[0] - view + 1))
            add(fn, "y[1] over y[0]", y=A([y[0], y[0] + ny - 1]))
            add(fn, "u[0] over v[1]", u=_with(dict(_BASE[fn])["u"], 0, dict(_BASE[fn])["v"][1] + ny // 4 - 1))
            add(fn, "y[1] touches y[0]", y=A([y[0], y[0] + ny]), v=A([P(3), None]))
        else:
            add(fn, "repeated source then NULL v[1]", y=A([y[0], y[0]]), v=A([P(3), None]))
            add(fn, "rgb[1] over y[0]", rgb=_with(rgb, 1, y[0] + 100))
            add(fn, "rgb[0] over rgb[1], same rows", rgb=A([rgb[0], rgb[0] + 359]))
            add(fn, "rgb[0] over rgb[1], a row apart", rgb=A([rgb[0], rgb[0] + 360 + 10]), pitch=720)
            add(fn, "chw planes overlap", layout=1, pitch=120, plane_stride=60 * 120 - 1)
            add(fn, "crops interleave, then NULL v[1]", rgb=A([rgb[0], rgb[0] + 360]), pitch=720, v=A([P(3), None]))
            add(fn, "crops interleave and overlap by a byte", rgb=A([rgb[0], rgb[0] + 359]), pitch=720)

    fn = "so_scale_yuv420"
    b = dict(_BASE[fn])
    add(fn, "su only NULL", su=None)
    add(fn, "dv only NULL", dv=None)
    add(fn, "luma only, null sy[1]", su=None, sv=None, du=None, dv=None, sy=_with(b["sy"], 1, None))
    add(fn, "luma only, odd sizes, null dy", su=None, sv=None, du=None, dv=None, hs=119, ws=239, hd=59, wd=119,
        Hp=61, Wp=127, dy=None)
    add(fn, "hs odd", hs=119)
    add(fn, "ws 0", ws=0)
    add(fn, "hd odd", hd=59)
    add(fn, "wd 0", wd=0)
    add(fn, "Hp below hd", Hp=32)
    add(fn, "Wp odd", Wp=129)
    add(fn, "too large", Hp=BIG[0], Wp=BIG[1])
    add(fn, "source too large", hs=BIG[0], ws=BIG[1], pitch_y=BIG[1], pitch_c=BIG[1] // 2)
    add(fn, "pitch_y short", pitch_y=239)
    add(fn, "pitch_c short", pitch_c=119)
    for tname in ("yh", "yv", "ch", "cv"):
        add(fn, f"taps_{tname} 0", **{f"taps_{tname}": 0})
        add(fn, f"taps_{tname} 999", **{f"taps_{tname}": 999})
    add(fn, "luma only ignores chroma tables", su=None, sv=None, du=None, dv=None, coef_ch=None, taps_cv=0, sy=None)
    add(fn, "order: nframes -1 before tables", nframes=-1, taps_yh=0)
    add(fn, "nframes 0", nframes=0, sy=None, su=None, sv=None, dy=None, du=None, dv=None)
    add(fn, "nframes 0, all chroma arrays", nframes=0, sy=None, dy=None)
    sy, dy = b["sy"], b["dy"]
    sview, dplane = 119 * 240 + 240, H * W
    add(fn, "repeated source then NULL dv[1]", sy=A([sy[0], sy[0]]), dv=_with(b["dv"], 1, None))
    add(fn, "dy[1] over sy[0]", dy=_with(dy, 1, sy[0] + sview - 1))
    add(fn, "sy[1] ends inside dy[0]", sy=_with(sy, 1, dy[0] - sview + 1))
    add(fn, "dy[1] over dy[0]", dy=A([dy[0], dy[0] + dplane - 1]))
    add(fn, "du[0] over dv[1]", du=_with(b["du"], 0, b["dv"][1] + dplane // 4 - 1))
    add(fn, "order: NULL in frame 1 before alias in frame 0", dy=_with(dy, 0, sy[0]), sv=_with(b["sv"], 1, None))

    for fn in ("so_chroma_encode_frame", "so_chroma_recon_frame"):
        add(fn, "bs 8", bs=8)
        add(fn, "frame_type 2", frame_type=2)
        add(fn, "qp_offset 21", qp_offset=21)
        add(fn, "qp_offset -21", qp_offset=-21)
        add(fn, "intra ignores refs", frame_type=0, refs_u=None, refs_v=None, nref=0, split=None, mv=None,
            out_recon_u=None)
        add(fn, "recon_u is recon_v", out_recon_v=P(9))
        add(fn, "recon_u aliases refs_v[0]", out_recon_u=P(3))
        add(fn, "recon_v aliases refs_u[0]", out_recon_v=P(2))
        add(fn, "recon_u unaligned", out_recon_u=P(9) + 4)
        add(fn, "refs_v[0] unaligned", refs_v=A([P(3) + 4]))
        add(fn, "order: alias before alignment", out_recon_u=P(3), out_recon_v=P(10) + 4)
        add(fn, "order: frame_type before qp", frame_type=2, qp=21)
    add("so_chroma_encode_frame", "qtc_u unaligned", out_qtc_u=P(6) + 8)
    add("so_chroma_encode_frame", "cur_v unaligned", cur_v=P(1) + 4)
    add("so_chroma_recon_frame", "qtc_v unaligned", qtc_v=P(7) + 8)

    for fn in ("so_pack_frames", "so_pack_frames_ex", "so_pack_frames_bits", "so_unpack_frames",
               "so_unpack_frames_bits"):
        add(fn, "nb 0", nb=0)
        add(fn, "frame_types[0] 2", frame_types=I([2, 1]))
        add(fn, "frame_types[1] -1", frame_types=I([0, -1]))
        add(fn, "nframes 0", nframes=0, frame_types=None, split=None, mv=None, qtc=None, offs=None)
        add(fn, "order: bs before nb", bs=12, nb=0)
        add(fn, "order: NULL before frame type", frame_types=I([2, 1]), qtc=_with(dict(_BASE[fn])["qtc"], 0, None))
    for fn in ("so_pack_chroma_frames", "so_pack_chroma_frames_bits", "so_pack_chroma_frames_after",
               "so_pack_chroma_frames_bits_after", "so_unpack_chroma_frames", "so_unpack_chroma_frames_bits"):
        add(fn, "nb 0", nb=0)
        add(fn, "nframes 0", nframes=0, qtc_u=None, qtc_v=None, offs=None)

    fn = "so_decode_p_frames"
    b = dict(_BASE[fn])
    add(fn, "coding 0", coding=0)
    add(fn, "coding 3", coding=3)
    add(fn, "nref_max 0", nref_max=0)
    add(fn, "nref_max 5", nref_max=5)
    add(fn, "nref0 0", nref0=0)
    add(fn, "nref0 above nref_max", nref0=3, refs0=A([P(2), P(20), P(21)]))
    add(fn, "nframes 0", nframes=0, packed=None, offs=None, refs0=None, out_split=None, out_mv=None, out_recon=None,
        err=None)
    add(fn, "out_recon[0] unaligned", out_recon=_with(b["out_recon"], 0, P(5) + 8))
    add(fn, "out_mv[1] unaligned", out_mv=_with(b["out_mv"], 1, b["out_mv"][1] + 2))
    add(fn, "recon[0] aliases refs0[0]", out_recon=_with(b["out_recon"], 0, P(2)))
    add(fn, "recon[1] aliases recon[0]", out_recon=A([P(5), P(5)]))
    add(fn, "order: bs before nframes", bs=12, nframes=-1)
    add(fn, "order: nframes before coding", nframes=-1, coding=0)
    add(fn, "order: frame 0 alias before frame 1 NULL", out_recon=_with(b["out_recon"], 0, P(2)),
        packed=_with(b["packed"], 1, None))

    fn = "so_decode_chroma_frames"
    b = dict(_BASE[fn])
    add(fn, "coding 0", coding=0)
    add(fn, "bs 8 is not chroma", bs=8)
    add(fn, "nref_max 0", nref_max=0)
    add(fn, "qp_offset 21", qp_offset=21)
    add(fn, "nref0 -1", nref0=-1)
    add(fn, "nref0 above nref_max", nref0=3)
    add(fn, "nframes 0", nframes=0, frame_types=None, packed=None, offs=None, out_recon_u=None, out_recon_v=None,
        err=None)
    add(fn, "no refs0 needs no arrays, P-frame first", nref0=0, refs0_u=None, refs0_v=None)
    add(fn, "I-frame needs no split", frame_types=I([0, 1]), split=_with(b["split"], 0, None),
        mv=_with(b["mv"], 0, None), out_recon_u=_with(b["out_recon_u"], 1, None))
    add(fn, "I-frame first without arrays, then P without split", frame_types=I([0, 1]), nref0=0, refs0_u=None,
        refs0_v=None, split=None)
    add(fn, "frame_types[0] 2", frame_types=I([2, 1]))
    add(fn, "frame_types[1] 2", frame_types=I([1, 2]))
    add(fn, "refs0_v[0] unaligned", refs0_v=A([P(5) + 4]))
    add(fn, "out_recon_u[1] unaligned", out_recon_u=_with(b["out_recon_u"], 1, b["out_recon_u"][1] + 4))
    add(fn, "recon_u[0] is recon_v[0]", out_recon_v=_with(b["out_recon_v"], 0, P(6)))
    add(fn, "recon_u[1] aliases refs0_v[0]", out_recon_u=_with(b["out_recon_u"], 1, P(5)))
    add(fn, "recon_v[1] aliases recon_u[0]", out_recon_v=_with(b["out_recon_v"], 1, P(6)))
    add(fn, "order: frame type before NULL", frame_types=I([2, 1]), packed=_with(b["packed"], 0, None))
    return t


def cases():
    """[(id, function name, [ctypes arguments])], ids unique."""
    out, seen = [], {}
    for fn, label, over in _table():
        names = [k for k, _ in _BASE[fn]]
        unknown = set(over) - set(names)
        assert not unknown, (fn, label, unknown)
        cid = f"{fn}: {label}"
        if cid in seen:   # a generic case written out again by hand
            assert seen[cid] == over, cid
            continue
        seen[cid] = over
        out.append((cid, fn, [_c(over.get(k, v)) for k, v in _BASE[fn]]))
    return out


def run(lib, fn, args):
    """(return code, so_last_error text) of one case.  A refusal of so_set_option comes first, so a
    call that returns SO_OK shows that text: it left the thread's message alone."""
    lib.so_set_option(-1, 0)
    rc = getattr(lib, fn)(*args)
    return int(rc), lib.so_last_error().decode(errors="replace")
