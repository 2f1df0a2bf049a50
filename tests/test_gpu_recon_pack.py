"""The packed tail of the tall plain run's transforms (tq16_exact's FAST: the reconstruction
bytes written in place by SDWA byte adds, the SSE from the packed rows, the token and SSE sums
over the block's lanes by DPP) against the C oracle, bit for bit: recon, per-block sse, tokens,
qtc, mv (and split, mae_num).

256 x 96 frames (two 128 x 48 tiles across and two down: window edges and interior blocks), the
tall kernel forced (SO_OPT_RUN_TALL_TILES=1), 3-frame P-runs, each case on the default kernel and
on its zero-skip twin (SO_OPT_RUN_ZERO_SKIP):

* textured: seeded bench content at QP 4;
* flats: flat 0 / 255 / 0 against a reference of the opposite extreme, at QP 0 and QP 12 -- levels
  of +-4080 at QP 0 (the largest the QTC store carries), a reconstruction whose byte add wraps mod
  256 (QP 0: prediction 255 plus a top byte of 1 = -255 mod 256; QP 12: the level -1 dequantises
  to -4096 / 16 = -256 under a prediction of 255, the stored pixel is 255 over a current 0, so
  |c - r| = 255 on every pixel of the SSE);
* checker: seeded 0 / 255 pixel noise against its complement, QP 0 and QP 12 -- residuals of
  +-255 and large levels of both signs in every row;
* ties: the adversarial tie blocks of tests/adversarial.py (the fast-transform tests' frames, cut
  to 96 rows) over a flat reference at QP 3.  Those blocks alone send waves through the forward
  fallback only (DESIGN.md section 4 records none through the inverse one), so the second run of
  the launch starts with a frame of exact inverse ties: residual c + (x + y & 1) has DC 8 (2 c + 1)
  at a step of 8 and every other coefficient below half its step, hence one odd level that
  dequantises to c + 1/2 on every pixel (pocketfft's own value lies beside the half, and its side
  decides the oracle's pixel).  The inverse certificate must flag them, which sends the wave
  through the pocketfft inverse and its packing of the row for the same tail:
  take_tq_fallback_counts()[1] > 0.
"""
import numpy as np
import pytest
import torch

import adversarial as A
from streamoptima_amd import _lib

pytestmark = pytest.mark.gpu

W, H = 256, 96
NB = (W // 16) * (H // 16)
KEYS = ("split", "mv", "qtc", "tokens", "mae_num", "recon")


def _textured():
    from streamoptima_amd.synth import synth_sequence
    seq = synth_sequence(4, H, W, seed=47, content="bench")
    return [([seq[1], seq[2], seq[3]], seq[0])]


def _flats():
    lo, hi = np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8)
    return [([lo, hi, lo], hi)]


def _checker():
    rng = np.random.default_rng(909)
    a = (rng.integers(0, 2, size=(H, W)) * 255).astype(np.uint8)
    b = (rng.integers(0, 2, size=(H, W)) * 255).astype(np.uint8)
    return [([a, 255 - a, b], 255 - a)]


def _inverse_tie_frame():
    """Block b: residual c_b + checkerboard(0 / 1) over the flat reference, c_b cycling -5..5."""
    y, x = np.mgrid[0:H, 0:W]
    c = (((y // 16) * (W // 16) + x // 16) % 11) - 5
    return (128 + c + ((x + y) & 1)).astype(np.uint8)


def _ties():
    blocks = A.run_blocks(128)
    fr = [A.frame_from_blocks(blocks[i][:NB], H, W)[0] for i in range(5)]
    flat = np.full((H, W), 128, np.uint8)
    return [([fr[0], fr[1], fr[2]], flat), ([_inverse_tie_frame(), fr[3], fr[4]], flat)]


CASES = {
    "textured_qp4": (_textured, 4),
    "flats_qp0": (_flats, 0),
    "flats_qp12": (_flats, 12),
    "checker_qp0": (_checker, 0),
    "checker_qp12": (_checker, 12),
    "ties_qp3": (_ties, 3),
}
_EXPECTED = {}


def _expected(name):
    """The case's runs and the oracle's frames, computed once: [(curs, ref0)], [[frame dict]]."""
    if name not in _EXPECTED:
        from oracle import oracle as O
        make, qp = CASES[name]
        runs = make()
        exp = []
        for curs, ref0 in runs:
            ref, frames = ref0, []
            for cur in curs:
                e = O.inter_frame(cur, [ref], 16, 16, qp, None, False, 0.015)
                d = (cur.astype(np.int64) - e["recon"].astype(np.int64)) ** 2
                e["sse"] = d.reshape(H // 16, 16, W // 16, 16).sum(axis=(1, 3)).reshape(-1)
                frames.append(e)
                ref = np.ascontiguousarray(e["recon"], dtype=np.uint8)
            exp.append(frames)
        _EXPECTED[name] = (runs, exp)
    return _EXPECTED[name]


def _plane(a, dev):
    from streamoptima_amd.engine import alloc_planes
    p = alloc_planes(1, H, W, dev)[0]
    p.copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)))
    return p


@pytest.mark.parametrize("zero_skip", [False, True])
@pytest.mark.parametrize("name", list(CASES))
def test_packed_tail_matches_oracle(gpu, name, zero_skip):
    from streamoptima_amd.engine import Engine
    runs, exp = _expected(name)
    qp = CASES[name][1]
    eng = Engine(H, W, 16, 16, False, 0.015, gpu)
    dev_runs = [([_plane(c, gpu) for c in curs], _plane(ref0, gpu), [eng.new_symbols(1) for _ in curs])
                for curs, ref0 in runs]
    eng.zero_skip = zero_skip
    with _lib.option(_lib.OPT_RUN_TALL_TILES, 1):
        eng.take_tq_fallback_counts()
        eng.encode_p_runs(dev_runs, qp, None)
        torch.cuda.synchronize()
        eng.check_run()
    fwd, inv = eng.take_tq_fallback_counts()
    print(f"{name} zero_skip {zero_skip}: fallback waves forward {fwd}, inverse {inv}")
    for r, (_, _, outs) in enumerate(dev_runs):
        for i, o in enumerate(outs):
            e = exp[r][i]
            for k in KEYS + ("sse",):
                got = getattr(o, k).cpu().numpy()
                got = got[:NB] if k == "sse" else got
                want = np.asarray(e[k])
                assert got.shape == want.shape, (r, i, k, got.shape, want.shape)
                neq = got.astype(np.int64) != want.astype(np.int64)
                assert not neq.any(), (f"run {r} frame {i} {k}: {int(neq.sum())} values differ from the oracle, "
                                       f"first at {np.flatnonzero(neq.reshape(-1))[:3].tolist()}")
    if name == "flats_qp0":      # the largest levels: +-4080 at the DC
        dc = [int(e["qtc"].reshape(NB, 256)[0, 0]) for e in exp[0]]
        assert dc == [-4080, 4080, -4080], dc
    if name == "flats_qp12":     # 0 over a prediction of 255: the pixel wraps to 255, |c - r| = 255
        assert int(exp[0][0]["sse"][0]) == 256 * 255 * 255
    if name == "ties_qp3":
        assert fwd > 0
        assert inv > 0
