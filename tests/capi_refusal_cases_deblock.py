"""The refusal matrix of so_deblock_yuv420, in the style of capi_refusal_cases.py (whose helpers it
takes): one case per rule of include/streamoptima.h "Deblocking", and the order a call with several
faults must keep.  Made-up addresses: no case may reach a launch, so the base call itself (which is
valid) is never made; every case breaks it, or has nframes 0."""
from capi_refusal_cases import A, H, I, N, P, W, _c, _pp, _with, run   # noqa: F401  (run: for the test)

FN = "so_deblock_yuv420"
CH = (H // 2) * (W // 2)

_BASE = {
    FN: [("sy", _pp(0)), ("su", _pp(1)), ("sv", _pp(2)), ("nframes", N), ("H", H), ("W", W), ("bs", 16),
         ("split", _pp(6)), ("qp", 5), ("qp_row", None), ("qp_map", _pp(7)), ("chroma_qp_offset", 0), ("strength", 0),
         ("dy", _pp(3)), ("du", _pp(4)), ("dv", _pp(5)), ("stream", None)],
}
_LUMA = dict(su=None, sv=None, du=None, dv=None)


def _table():
    t = []
    b = dict(_BASE[FN])

    def add(label, **over):
        t.append((FN, label, over))

    # the scalar rules, in their order
    add("nframes -1", nframes=-1)
    for bs in (0, 4, 12, 32, -16):
        add(f"bs {bs}", bs=bs)
    add("H 0", H=0)
    add("H -16", H=-16)
    add("H 72", H=72)
    add("W 0", W=0)
    add("W 120", W=120)
    add("W 120 is a multiple of 8", W=120, bs=8, split=None, **_LUMA, nframes=0)
    add("too large", H=65536, W=32896)
    for qp in (-1, 21):
        add(f"qp {qp}", qp=qp)
    for off in (-21, 21):
        add(f"chroma_qp_offset {off}", chroma_qp_offset=off)
    for s in (-4, 4):
        add(f"strength {s}", strength=s)
    add("order: nframes before bs", nframes=-1, bs=12)
    add("order: bs before geometry", bs=12, H=60)
    add("order: geometry before qp", W=100, qp=21)
    add("order: qp before chroma_qp_offset", qp=21, chroma_qp_offset=21)
    add("order: chroma_qp_offset before strength", chroma_qp_offset=-21, strength=4)
    add("order: strength before NULL", strength=4, sy=None)
    # nothing to do
    add("nframes 0", nframes=0)
    add("nframes 0 without arrays", nframes=0, sy=None, dy=None, split=None, qp_map=None, **_LUMA)
    add("nframes 0, strength 4", nframes=0, strength=4)
    # pointers
    for k in ("sy", "dy"):
        add(f"null {k}", **{k: None})
        add(f"null {k}[0]", **{k: _with(b[k], 0, None)})
        add(f"null {k}[last]", **{k: _with(b[k], N - 1, None)})
    add("order: sy before dy", sy=None, dy=None)
    add("order: luma pointers before the chroma set", dy=_with(b["dy"], 1, None), su=None)
    for k in ("su", "sv", "du", "dv"):
        add(f"partial chroma: no {k}", **{k: None})
        add(f"partial chroma: only {k}", **{**_LUMA, k: b[k]})
        add(f"null {k}[0]", **{k: _with(b[k], 0, None)})
        add(f"null {k}[last]", **{k: _with(b[k], N - 1, None)})
    # aliasing: a destination against a source or another destination, whole or in part
    add("dy[0] is sy[0]", dy=_with(b["dy"], 0, b["sy"][0]))
    add("dy[1] is sy[0]", dy=_with(b["dy"], 1, b["sy"][0]))
    add("dy[0] inside sy[1]", dy=_with(b["dy"], 0, b["sy"][1] + H * W - 1))
    add("dy[0] ends inside sy[1]", dy=_with(b["dy"], 0, b["sy"][1] - 1))
    add("dy[0] is dy[1]", dy=A([P(3), P(3)]))
    add("du[0] is sv[0]", du=_with(b["du"], 0, b["sv"][0]))
    add("du[0] is dv[0]", du=_with(b["du"], 0, b["dv"][0]))
    add("dv[1] overlaps du[1]", dv=_with(b["dv"], 1, b["du"][1] + CH - 1))
    add("dv[1] inside dy[0]", dv=_with(b["dv"], 1, b["dy"][0] + 64))
    add("du[0] inside sy[0]", du=_with(b["du"], 0, b["sy"][0] + 64))
    add("luma only: dy[0] is sy[0]", **_LUMA, dy=_with(b["dy"], 0, b["sy"][0]))
    add("order: partial chroma before aliasing", su=None, dy=_with(b["dy"], 0, b["sy"][0]))
    add("order: aliasing before bs 8 chroma", bs=8, dy=_with(b["dy"], 0, b["sy"][0]))
    # what is not built
    add("chroma with bs 8", bs=8, split=None)
    add("split[0] with bs 8", bs=8, **_LUMA)
    add("split[last] with bs 8", bs=8, **_LUMA, split=A([None, P(6)]))
    add("order: chroma before split with bs 8", bs=8)
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
