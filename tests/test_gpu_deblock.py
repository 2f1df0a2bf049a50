"""so_deblock_yuv420 on the GPU against the numpy model (deblockref.py): every output byte-identical.
The planes are the designed corpus (deblockref.corpus_plane: thresholds pass and fail within one
plane; test_deblock.py shows that it reaches every branch).  The kernel's tile is 32 x 128 samples:
48 x 144 is one tile plus one block in each direction, 144 x 272 several tiles both ways."""
import numpy as np
import pytest
import torch

import deblockref as R

pytestmark = pytest.mark.gpu

SIZES16 = [(16, 16), (32, 48), (48, 80), (80, 112), (48, 144), (144, 272)]
SIZES8 = [(8, 8), (8, 24), (40, 136)]
QPS = [2, 4, 6, 8]

_engines = {}


def _engine(gpu, h, w, bs):
    from streamoptima_amd.engine import Engine
    key = (h, w, bs)
    if key not in _engines:
        _engines[key] = Engine(h, w, bs, device=gpu)
    return _engines[key]


def _frame(h, w, bs, seed, split="random", chroma=True, extremes=False, qp_src="map"):
    """One frame of the corpus as numpy: planes, split flags and a QP source."""
    rng = np.random.default_rng(seed)
    nb = (h // bs) * (w // bs)
    f = {"y": R.corpus_plane(h, w, rng, QPS, extremes), "u": None, "v": None, "split": None, "qp": 5,
         "qp_row": None, "qp_map": None}
    if chroma and bs == 16:
        f["u"] = R.corpus_plane(h // 2, w // 2, rng, QPS, extremes)
        f["v"] = R.corpus_plane(h // 2, w // 2, rng, QPS, extremes)
    if bs == 16 and split != "null":
        f["split"] = {"random": rng.integers(0, 2, nb), "all": np.ones(nb), "none": np.zeros(nb)}[split].astype(np.uint8)
    if qp_src == "map":
        f["qp_map"] = rng.choice(QPS, nb).astype(np.int32)
    elif qp_src == "rows":
        f["qp_row"] = rng.choice(QPS, h // bs).astype(np.int32)
    return f


def _model(f, bs, off=0, strength=0):
    return R.deblock_yuv420(f["y"], f["u"], f["v"], bs=bs, split=f["split"], qp=f["qp"], qp_row=f["qp_row"],
                            qp_map=f["qp_map"], chroma_qp_offset=off, strength=strength)


def _dev(a, gpu):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _run(gpu, frames, bs, off=0, strength=0, qp=5):
    """The frames through one Engine.deblock_yuv420 call -> [(y, u, v)] as numpy, after checking
    that the call left its sources alone."""
    h, w = frames[0]["y"].shape
    eng = _engine(gpu, h, w, bs)
    chroma = frames[0]["u"] is not None
    ys = [_dev(f["y"], gpu) for f in frames]
    uvs = [torch.stack([_dev(f["u"], gpu), _dev(f["v"], gpu)]) for f in frames] if chroma else None
    out_y, out_uv = eng.deblock_yuv420(ys, uvs, split=[_dev(f["split"], gpu) for f in frames], qp=qp,
                                       qp_rows=[_dev(f["qp_row"], gpu) for f in frames],
                                       qp_maps=[_dev(f["qp_map"], gpu) for f in frames], chroma_qp_offset=off,
                                       strength=strength)
    torch.cuda.synchronize()
    for i, f in enumerate(frames):
        assert np.array_equal(ys[i].cpu().numpy(), f["y"]), "the luma source changed"
        if chroma:
            assert np.array_equal(uvs[i][0].cpu().numpy(), f["u"]) and np.array_equal(uvs[i][1].cpu().numpy(), f["v"])
    oy = out_y.cpu().numpy()
    ouv = out_uv.cpu().numpy() if chroma else None
    return [(oy[i], ouv[i, 0] if chroma else None, ouv[i, 1] if chroma else None) for i in range(len(frames))]


def _same(got, exp, what):
    for name, g, e in zip("yuv", got, exp):
        if e is None:
            assert g is None
            continue
        bad = np.argwhere(g != e)
        assert bad.size == 0, f"{what}: plane {name}: {len(bad)} samples differ, first at {bad[0].tolist()}"


@pytest.mark.parametrize("split", ["random", "all", "none"])
@pytest.mark.parametrize("hw", SIZES16, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sizes_bs16(gpu, hw, split):
    f = _frame(*hw, 16, seed=hw[0] * 7 + hw[1], split=split)
    got = _run(gpu, [f], 16)[0]
    _same(got, _model(f, 16), f"{hw} {split}")
    if hw != (16, 16):
        assert not np.array_equal(got[0], f["y"])       # the filter acted


@pytest.mark.parametrize("hw", SIZES8, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sizes_bs8_luma(gpu, hw):
    f = _frame(*hw, 8, seed=hw[1], split="null")
    _same(_run(gpu, [f], 8)[0], _model(f, 8), f"{hw} bs 8")


def test_one_block_only_its_split_edges(gpu):
    f = _frame(16, 16, 16, seed=1, split="all", qp_src="scalar")
    f["qp"] = 8
    got = _run(gpu, [f], 16, qp=8)[0]
    _same(got, _model(f, 16), "16x16 split")
    changed = np.argwhere(got[0] != f["y"])
    assert len(changed) and all(6 <= r <= 9 or 6 <= c <= 9 for r, c in changed)
    assert np.array_equal(got[1], f["u"]) and np.array_equal(got[2], f["v"])     # an 8 x 8 chroma plane has no edge


@pytest.mark.parametrize("src", ["scalar", "rows", "map", "wild map", "wild rows"])
def test_qp_sources(gpu, src):
    h, w = 48, 144
    f = _frame(h, w, 16, seed=11, qp_src={"scalar": "scalar", "rows": "rows", "wild rows": "rows"}.get(src, "map"))
    wild = np.array([0, 1, 20, 21, -1, 99, -5, 2 ** 31 - 1, -2 ** 31, 7, 3, 2], dtype=np.int64)
    if src == "wild map":        # clamped, and nothing worse
        f["qp_map"] = np.resize(wild, f["qp_map"].size).astype(np.int32)
    if src == "wild rows":
        f["qp_row"] = np.array([2 ** 31 - 1, -7, 6], dtype=np.int32)
    _same(_run(gpu, [f], 16)[0], _model(f, 16), src)


def test_three_frames_one_call(gpu):
    """Different QP sources per frame, one frame without split flags, one with rows AND a map (the map wins)."""
    h, w = 48, 144
    a = _frame(h, w, 16, seed=21, qp_src="scalar")
    b = _frame(h, w, 16, seed=22, qp_src="rows", split="null")
    c = _frame(h, w, 16, seed=23, qp_src="map")
    c["qp_row"] = np.full(h // 16, 9, np.int32)
    got = _run(gpu, [a, b, c], 16)
    for i, f in enumerate((a, b, c)):
        _same(got[i], _model(f, 16), f"frame {i}")


@pytest.mark.parametrize("off", [-3, 0, 3])
def test_chroma_qp_offset(gpu, off):
    f = _frame(80, 112, 16, seed=31)
    _same(_run(gpu, [f], 16, off=off)[0], _model(f, 16, off=off), f"offset {off}")


def test_luma_only(gpu):
    f = _frame(80, 112, 16, seed=41, chroma=False)
    got = _run(gpu, [f], 16)[0]
    _same(got, _model(f, 16), "luma only")
    assert got[1] is None


@pytest.mark.parametrize("strength", [-3, 0, 3])
def test_strength(gpu, strength):
    f = _frame(80, 112, 16, seed=51)
    _same(_run(gpu, [f], 16, strength=strength)[0], _model(f, 16, strength=strength), f"strength {strength}")


@pytest.mark.parametrize("qp", [6, 9, 20])
def test_samples_at_0_and_255(gpu, qp):
    f = _frame(48, 144, 16, seed=61, extremes=True, qp_src="scalar")
    f["qp"] = qp
    assert (f["y"] == 0).any() and (f["y"] == 255).any()
    got = _run(gpu, [f], 16, qp=qp)[0]
    _same(got, _model(f, 16), f"extremes qp {qp}")


@pytest.mark.parametrize("offset", [0, 1, 4, 8])
def test_views_of_a_larger_allocation_and_guard_bytes(gpu, offset):
    """Sources and destinations at any byte offset inside larger allocations (the byte, 8-byte and
    16-byte paths of the staging and the store); nothing outside a destination plane is written."""
    h, w = 48, 144
    eng = _engine(gpu, h, w, 16)
    f = _frame(h, w, 16, seed=71 + offset)
    guard = 256

    def place(a, off):
        buf = torch.full((a.size + 2 * guard + 16,), 0xA5, dtype=torch.uint8, device=gpu)
        view = buf[guard + off:guard + off + a.size].view(a.shape)
        view.copy_(torch.from_numpy(a).to(gpu))
        return buf, view

    by, vy = place(f["y"], offset)
    bu, vu = place(f["u"], offset)
    bv, vv = place(f["v"], offset)
    dby, dy = place(np.zeros_like(f["y"]), (offset * 3) % 16)
    dbu, du = place(np.zeros_like(f["u"]), offset)
    dbv, dv = place(np.zeros_like(f["v"]), (offset + 8) % 16)
    before = [b.clone() for b in (by, bu, bv)]
    oy, ouv = eng.deblock_yuv420([vy], [(vu, vv)], split=[_dev(f["split"], gpu)], qp_maps=[_dev(f["qp_map"], gpu)],
                                 out_y=[dy], out_uv=[(du, dv)])
    torch.cuda.synchronize()
    exp = _model(f, 16)
    _same((dy.cpu().numpy(), du.cpu().numpy(), dv.cpu().numpy()), exp, f"offset {offset}")
    for b, b0 in zip((by, bu, bv), before):
        assert torch.equal(b, b0), "a source allocation changed"
    for buf, view in ((dby, dy), (dbu, du), (dbv, dv)):
        lo = view.data_ptr() - buf.data_ptr()
        flat = buf.cpu().numpy()
        assert (flat[:lo] == 0xA5).all() and (flat[lo + view.numel():] == 0xA5).all(), "guard bytes were written"


def test_refusals_reach_python(gpu):
    eng = _engine(gpu, 48, 144, 16)
    f = _frame(48, 144, 16, seed=81)
    y = _dev(f["y"], gpu)
    with pytest.raises(ValueError, match="strength"):
        eng.deblock_yuv420([y], None, strength=4)
    with pytest.raises(ValueError, match="aliases"):
        eng.deblock_yuv420([y], None, qp=5, out_y=[y])
    e8 = _engine(gpu, 8, 24, 8)
    y8 = _dev(f["y"][:8, :24], gpu)
    with pytest.raises(NotImplementedError, match="split"):
        e8.deblock_yuv420([y8], None, split=[torch.zeros(3, dtype=torch.uint8, device=gpu)], qp=5)
