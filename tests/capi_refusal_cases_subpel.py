"""The refusal matrix of so_chroma_encode_frame_ex, so_chroma_recon_frame_ex and
so_decode_chroma_frames_ex, in the style of capi_refusal_cases.py (whose helpers and base calls it
takes): the mv_frac_bits rule and its place in the order of checks, and every rule the three
inherit from their base functions, reported under the new names.  Made-up addresses: no case may
reach a launch."""
from capi_refusal_cases import A, BIG, I, P, _BASE as _OLD, _c, _with, run   # noqa: F401  (run: for the test)


def _ex(fn, bits=2):
    """fn's base call with mv_frac_bits in front of the stream."""
    base = list(_OLD[fn])
    assert base[-1] == ("stream", None)
    return base[:-1] + [("mv_frac_bits", bits), ("stream", None)]


_BASE = {
    "so_chroma_encode_frame_ex": _ex("so_chroma_encode_frame"),
    "so_chroma_recon_frame_ex": _ex("so_chroma_recon_frame"),
    "so_decode_chroma_frames_ex": _ex("so_decode_chroma_frames"),
}
_FRAME = ("so_chroma_encode_frame_ex", "so_chroma_recon_frame_ex")


def _table():
    t = []

    def add(fn, label, **over):
        t.append((fn, label, over))

    # the new rule, at both values of the base call, and where it stands: behind the block size,
    # ahead of the geometry and of everything after it
    for fn in _BASE:
        for bits in (0, 3, -1):
            add(fn, f"mv_frac_bits {bits}", mv_frac_bits=bits)
        add(fn, "order: bs before mv_frac_bits", bs=8, mv_frac_bits=0)
        add(fn, "order: mv_frac_bits before geometry", mv_frac_bits=3, H=60)
        add(fn, "order: mv_frac_bits before qp", mv_frac_bits=0, qp=21)
        add(fn, "order: mv_frac_bits before qp_offset", mv_frac_bits=3, qp_offset=21)
        # the inherited scalar rules hold at 1 and at 2
        for bits in (1, 2):
            add(fn, f"bits {bits}: bs 12", mv_frac_bits=bits, bs=12)
            add(fn, f"bits {bits}: bs 0", mv_frac_bits=bits, bs=0)
            add(fn, f"bits {bits}: H 60", mv_frac_bits=bits, H=60)
            add(fn, f"bits {bits}: W 0", mv_frac_bits=bits, W=0)
            add(fn, f"bits {bits}: too large", mv_frac_bits=bits, H=BIG[0], W=BIG[1])
            add(fn, f"bits {bits}: qp 21", mv_frac_bits=bits, qp=21)
            add(fn, f"bits {bits}: qp -1", mv_frac_bits=bits, qp=-1)
            add(fn, f"bits {bits}: qp_offset 21", mv_frac_bits=bits, qp_offset=21)
            add(fn, f"bits {bits}: qp_offset -21", mv_frac_bits=bits, qp_offset=-21)
        # every pointer NULL in turn, and for an array its first and its last entry
        base = dict(_BASE[fn])
        optional = {"qp_map", "qp_row"} | ({"out_sse"} if fn != "so_chroma_encode_frame_ex" else set())
        for k, v in base.items():
            if k in optional or k == "stream":
                continue
            if isinstance(v, I) or (isinstance(v, int) and not isinstance(v, bool) and v >= 0x1000000):
                add(fn, f"null {k}", **{k: None})
            elif isinstance(v, A):
                add(fn, f"null {k}", **{k: None})
                add(fn, f"null {k}[0]", **{k: _with(v, 0, None)})
                if len(v) > 1:
                    add(fn, f"null {k}[last]", **{k: _with(v, len(v) - 1, None)})

    for fn in _FRAME:
        add(fn, "bs 8", bs=8)
        add(fn, "nref 0", nref=0)
        add(fn, "nref 5", nref=5)
        add(fn, "frame_type 2", frame_type=2)
        add(fn, "intra ignores refs", frame_type=0, refs_u=None, refs_v=None, nref=0, split=None, mv=None,
            out_recon_u=None)
        add(fn, "recon_u is recon_v", out_recon_v=P(9))
        add(fn, "recon_u aliases refs_v[0]", out_recon_u=P(3))
        add(fn, "recon_v aliases refs_u[0]", out_recon_v=P(2))
        add(fn, "recon_u unaligned", out_recon_u=P(9) + 4)
        add(fn, "refs_v[0] unaligned", refs_v=A([P(3) + 4]))
        add(fn, "order: alias before alignment", out_recon_u=P(3), out_recon_v=P(10) + 4)
        add(fn, "order: frame_type before qp", frame_type=2, qp=21)
        add(fn, "order: geometry before frame_type", H=60, frame_type=2)
    add("so_chroma_encode_frame_ex", "qtc_u unaligned", out_qtc_u=P(6) + 8)
    add("so_chroma_encode_frame_ex", "cur_v unaligned", cur_v=P(1) + 4)
    add("so_chroma_recon_frame_ex", "qtc_v unaligned", qtc_v=P(7) + 8)

    fn = "so_decode_chroma_frames_ex"
    b = dict(_BASE[fn])
    add(fn, "nframes -1", nframes=-1)
    add(fn, "coding 0", coding=0)
    add(fn, "coding 3", coding=3)
    add(fn, "bs 8 is not chroma", bs=8)
    add(fn, "nref_max 0", nref_max=0)
    add(fn, "nref_max 5", nref_max=5)
    add(fn, "nref0 -1", nref0=-1)
    add(fn, "nref0 above nref_max", nref0=3)
    add(fn, "nframes 0", nframes=0, frame_types=None, packed=None, offs=None, out_recon_u=None, out_recon_v=None,
        err=None)
    add(fn, "order: mv_frac_bits before nframes 0", nframes=0, mv_frac_bits=0, frame_types=None, packed=None,
        offs=None, out_recon_u=None, out_recon_v=None, err=None)
    add(fn, "order: mv_frac_bits before nframes -1", nframes=-1, mv_frac_bits=3)
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
    out, seen = [], set()
    for fn, label, over in _table():
        names = [k for k, _ in _BASE[fn]]
        assert set(over) <= set(names), (fn, label)
        cid = f"{fn}: {label}"
        assert cid not in seen, cid
        seen.add(cid)
        out.append((cid, fn, [_c(over.get(k, v)) for k, v in _BASE[fn]]))
    return out
