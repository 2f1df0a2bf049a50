"""Chroma with quarter-sample vectors on the GPU (Engine(fme=True, chroma_subpel=True): the
mv_frac_bits = 2 instantiations of the so_chroma kernels) bit for bit against the numpy model
(tests/chromasubpelref.py) on synthetic luma symbols: qtc, tokens, SSE and reconstruction of U and
V.  32 x 48 luma (chroma 16 x 24, 2 x 3 blocks) unless a case says otherwise; every case runs in
well under a second."""
import numpy as np
import pytest
import torch

import chromaref as CR
import chromasubpelref as SR

pytestmark = pytest.mark.gpu

H, W = 32, 48
HC, WC, NBX, NBY = H // 2, W // 2, W // 16, H // 16
NB = NBX * NBY


def _textured(rng, hc, wc):
    ys, xs = np.mgrid[0:hc, 0:wc]
    base = (96 + 60 * np.sin(xs / 3.1) * np.cos(ys / 4.3)).astype(np.int64)
    return np.clip(base + rng.integers(-25, 26, (hc, wc)), 0, 255).astype(np.uint8)


def _case(seed, h=H, w=W, nref=1):
    rng = np.random.default_rng(seed)
    hc, wc, nb = h // 2, w // 2, (h // 16) * (w // 16)
    return dict(ft=1, qp=4, qp_row=None, qp_map=None, off=0, nref=nref, h=h, w=w,
                cur=[_textured(rng, hc, wc), _textured(rng, hc, wc)],
                refs=[[_textured(rng, hc, wc) for _ in range(nref)] for _ in range(2)],
                split=np.zeros(nb, np.uint8), mv=np.zeros((nb, 4, 3), np.int16))


def _planes(arrs, dev):
    """uint8 planes back to back, without slack between or behind them"""
    body = torch.from_numpy(np.stack(arrs)).to(dev)
    return [body[i] for i in range(len(arrs))]


def _sym(c, dev):
    from streamoptima_amd.engine import FrameSymbols
    extra = {}
    if c["qp_map"] is not None:
        extra["qp_map"] = torch.from_numpy(c["qp_map"]).to(dev)
    return FrameSymbols(c["ft"], torch.from_numpy(c["split"]).to(dev), torch.from_numpy(c["mv"]).to(dev), None, None,
                        None, None, qp_rd=c["qp"], qp_row=c["qp_row"], extra=extra)


def _run(eng, c, dev):
    cur, ru, rv = _planes(c["cur"], dev), _planes(c["refs"][0], dev), _planes(c["refs"][1], dev)
    got = eng.encode_chroma(_sym(c, dev), cur[0], cur[1], ru, rv, qp_offset=c["off"])
    torch.cuda.synchronize()
    return got, (ru, rv)


def _model(c, s=2):
    return SR.encode_frame(c["cur"][0], c["cur"][1], c["refs"][0], c["refs"][1], c["ft"], c["split"], c["mv"],
                           c["qp"], c["qp_row"], c["qp_map"], c["off"], s=s)


def _assert_equal(got, exp, tag):
    for k in ("qtc_u", "qtc_v", "tokens", "recon_u", "recon_v", "sse"):
        g = getattr(got, k).cpu().numpy()
        assert g.shape == exp[k].shape and (g == exp[k]).all(), (tag, k, int((g != exp[k]).sum()))


@pytest.fixture(scope="module")
def eng(gpu):
    from streamoptima_amd.engine import Engine
    return Engine(H, W, 16, 16, False, 0.0, gpu, fme=True, chroma_subpel=True)


def _check(eng, gpu, c, tag):
    got, refs = _run(eng, c, gpu)
    _assert_equal(got, _model(c), tag)
    return got, refs


def test_all_sixteen_phases(eng, gpu):
    """One vector per block, the phase (fx, fy) cycling through all 16 over three launches, the
    whole-sample part inside the plane and outside it."""
    seen = set()
    for k in range(3):
        for whole in ((4, -4), (0, 0), (-40, 36)):
            c = _case(10 + k)
            for b in range(NB):
                ph = (6 * k + b) % 16
                c["mv"][b, 0, 0:2] = (whole[0] + ph % 4, whole[1] + ph // 4)
                seen.add((ph % 4, ph // 4))
            _check(eng, gpu, c, ("phases", k, whole))
    assert len(seen) == 16


def test_all_sixteen_phases_in_one_launch(gpu):
    """64 x 128 luma: 32 blocks, two workgroups' worth of lanes in one plane pair."""
    from streamoptima_amd.engine import Engine
    e = Engine(64, 128, 16, 16, False, 0.0, gpu, fme=True, chroma_subpel=True)
    c = _case(20, 64, 128)
    for b in range(e.nb):
        c["mv"][b, 0, 0:2] = (8 + b % 4, -4 + (b // 4) % 4)
    _check(e, gpu, c, "phases 64x128")


def test_negative_vectors_floor(eng, gpu):
    for k, (dx, dy) in enumerate([(-1, -1), (-3, -5), (-5, -3), (-1, 0), (0, -3), (-5, -5), (-7, -9), (-4, -8)]):
        c = _case(30 + k)
        c["mv"][:, 0, 0], c["mv"][:, 0, 1] = dx, dy
        _check(eng, gpu, c, ("negative", dx, dy))


def test_split_blocks_four_vectors(eng, gpu):
    rng = np.random.default_rng(40)
    for k in range(3):
        c = _case(41 + k)
        c["split"][:] = 1 if k == 0 else (rng.random(NB) < 0.5)
        c["mv"][..., 0:2] = rng.integers(-23, 24, (NB, 4, 2))
        c["mv"][0, :, 0:2] = [[1, 2], [-3, 7], [6, -1], [-5, -6]]   # four phases in one block
        c["split"][0] = 1
        _check(eng, gpu, c, ("split", k))


def test_reference_index_clamp(eng, gpu):
    c = _case(50, nref=2)
    rng = np.random.default_rng(51)
    c["split"][:] = rng.random(NB) < 0.5
    c["mv"][..., 0:2] = rng.integers(-15, 16, (NB, 4, 2))
    c["mv"][..., 2] = rng.choice(np.array([0, 1, 3], np.int16), (NB, 4))
    c["mv"][0, 0, 2], c["mv"][1, 0, 2], c["mv"][2, 0, 2] = 0, 1, 3
    got, _ = _check(eng, gpu, c, "nref 2")
    # the model's own clamp is what the case is about: r = 3 reads reference 1
    c1 = dict(c, mv=np.where(np.arange(3) == 2, np.minimum(c["mv"], 1), c["mv"]).astype(np.int16))
    _assert_equal(got, _model(c1), "nref 2, r clamped by hand")


def test_every_byte_alignment(eng, gpu):
    """Wc = 24 is a multiple of 4, so the fetch of a run starts at byte (dx >> 2) & 3 of its dword."""
    for ix in range(4):
        for fx, fy in ((0, 0), (1, 0), (0, 2), (3, 3)):
            c = _case(60 + ix)
            c["mv"][:, 0, 0], c["mv"][:, 0, 1] = 4 * ix + fx, fy
            xs = 0 + ix
            assert xs % 4 == ix and xs + 3 + (fx != 0) < WC   # block 0's first run takes the aligned-dword path
            _check(eng, gpu, c, ("alignment", ix, fx, fy))
    for ix in (-1, -2, -3):   # the same from the last block column, leftwards
        c = _case(64 - ix)
        c["mv"][:, 0, 0], c["mv"][:, 0, 1] = 4 * ix + 2, 1
        _check(eng, gpu, c, ("alignment", ix))


def test_footprint_at_the_last_column_and_row(eng, gpu):
    """Uniform vectors -4 .. 4 both ways.  For the last run of a row (X = Wc - 4) the footprint's
    last column X + ix + 3 + (fx != 0) lands on Wc - 1 (the dword path, up to the plane's last
    byte) and on Wc (one past: the clamped path); the last row does the same in y."""
    ends_x, ends_y = set(), set()
    for dy in range(-4, 5):
        for dx in range(-4, 5):
            c = _case(70)
            c["mv"][:, 0, 0], c["mv"][:, 0, 1] = dx, dy
            ends_x.add(((WC - 4) + (dx >> 2) + 3 + ((dx & 3) != 0), (dx & 3) != 0))
            ends_y.add(((HC - 1) + (dy >> 2) + ((dy & 3) != 0), (dy & 3) != 0))
            _check(eng, gpu, c, ("edge", dx, dy))
    for frac in (False, True):
        assert {(WC - 1, frac), (WC, frac)} <= ends_x and {(HC - 1, frac), (HC, frac)} <= ends_y


def test_vectors_far_outside(eng, gpu):
    rng = np.random.default_rng(80)
    for k, pool in enumerate(([-203, -201, 199, 202], [-32768, 32767, -32765, 32766], [-97, 98, 4 * WC + 1, -4 * HC - 3])):
        c = _case(81 + k)
        c["split"][:] = rng.random(NB) < 0.5
        c["mv"][..., 0:2] = rng.choice(np.array(pool, np.int16), (NB, 4, 2))
        _check(eng, gpu, c, ("far", k))


def test_i_frame(eng, gpu):
    for qp in (0, 10):
        c = _case(90 + qp)
        c.update(ft=0, qp=qp)
        _check(eng, gpu, c, ("i_frame", qp))
        assert (_model(c, s=1)["recon_u"] == _model(c)["recon_u"]).all()   # no vector, no s


def test_qp_map_and_offset(eng, gpu):
    rng = np.random.default_rng(100)
    for k, (lo, hi, off) in enumerate(((0, 7, -3), (0, 13, 3), (15, 21, 4))):
        c = _case(101 + k)
        c["split"][:] = rng.random(NB) < 0.5
        c["mv"][..., 0:2] = rng.integers(-21, 22, (NB, 4, 2))
        c["qp_map"] = rng.integers(lo, hi, NB).astype(np.int32)
        c["off"] = off
        _check(eng, gpu, c, ("qp_map", k))
    c = _case(105)
    c["mv"][..., 0:2] = rng.integers(-21, 22, (NB, 4, 2))
    c["qp_row"], c["off"] = [2, 9], 1
    _check(eng, gpu, c, "qp_row")


def test_recon_kernel_equals_encoder(eng, gpu):
    rng = np.random.default_rng(110)
    for k in range(3):
        c = _case(111 + k, nref=2)
        c["split"][:] = rng.random(NB) < 0.5
        c["mv"][..., 0:2] = rng.integers(-60, 61, (NB, 4, 2)) if k else rng.integers(-9, 10, (NB, 4, 2))
        c["mv"][..., 2] = rng.integers(0, 3, (NB, 4))
        if k == 2:
            c.update(ft=0)
        enc, (ru, rv) = _run(eng, c, gpu)
        dec = eng.recon_chroma(_sym(c, gpu), enc.qtc_u, enc.qtc_v, ru, rv, qp_offset=c["off"])
        torch.cuda.synchronize()
        assert dec.tokens is None and dec.sse is None
        assert torch.equal(dec.recon_u, enc.recon_u) and torch.equal(dec.recon_v, enc.recon_v)
        exp = SR.recon_frame(enc.qtc_u.cpu().numpy(), enc.qtc_v.cpu().numpy(), c["refs"][0], c["refs"][1], c["ft"],
                             c["split"], c["mv"], HC, WC, c["qp"], c["qp_row"], c["qp_map"], c["off"], s=2)
        assert (dec.recon_u.cpu().numpy() == exp[0]).all() and (dec.recon_v.cpu().numpy() == exp[1]).all()


def test_quarter_sample_differs_from_half_sample(eng, gpu):
    """The case is not vacuous: read as half-sample vectors the same symbols predict otherwise."""
    c = _case(120)
    c["mv"][:, 0, 0:2] = (5, 6)
    got, _ = _check(eng, gpu, c, "s2")
    assert (got.recon_u.cpu().numpy() != _model(c, s=1)["recon_u"]).any()


def test_fme_without_the_flag_still_refuses(eng, gpu):
    from streamoptima_amd.engine import Engine
    c = _case(130)
    cur, ru = _planes(c["cur"], gpu), _planes(c["refs"][0], gpu)
    plain = Engine(H, W, 16, 16, False, 0.0, gpu, fme=True)
    assert not plain.chroma_subpel
    with pytest.raises(NotImplementedError):
        plain.encode_chroma(_sym(c, gpu), cur[0], cur[1], ru, ru)
    with pytest.raises(NotImplementedError):
        plain.recon_chroma(_sym(c, gpu), torch.zeros((NB, 64), dtype=torch.int16, device=gpu),
                           torch.zeros((NB, 64), dtype=torch.int16, device=gpu), ru, ru)
    with pytest.raises(NotImplementedError):
        plain.decode_chroma_frames([0], [cur[0]], [torch.zeros(NB + 1, dtype=torch.int32, device=gpu)], [None], [None],
                                   [], [], 1, 4)


def test_flag_without_fme_is_todays_chroma(gpu):
    """Engine(fme=False, chroma_subpel=True) passes 1: the existing model, and the same bytes as
    an engine without the keyword, on the vectors of test_gpu_chroma's p_rand and p_far."""
    from streamoptima_amd.engine import Engine
    with_flag = Engine(H, W, 16, 16, False, 0.0, gpu, chroma_subpel=True)
    without = Engine(H, W, 16, 16, False, 0.0, gpu)
    rng = np.random.default_rng(140)
    for k in range(2):
        c = _case(141 + k, nref=3)
        c["split"][:] = rng.random(NB) < 0.45
        c["mv"][..., 0:2] = (rng.integers(-16, 17, (NB, 4, 2)) if k == 0
                             else rng.choice(np.array([-40, -39, 39, 40], np.int16), (NB, 4, 2)))
        c["mv"][..., 2] = rng.integers(0, 3, (NB, 4))
        a, _ = _run(with_flag, c, gpu)
        b, _ = _run(without, c, gpu)
        exp = CR.encode_frame(c["cur"][0], c["cur"][1], c["refs"][0], c["refs"][1], 1, c["split"], c["mv"], c["qp"])
        _assert_equal(a, exp, ("s1", k))
        for key in ("qtc_u", "qtc_v", "tokens", "recon_u", "recon_v", "sse"):
            assert torch.equal(getattr(a, key), getattr(b, key)), key
