"""The plain one-GPU run's fast transforms (SO_TQ_FAST: xform2d_fast with tq16_exact's
certificates and the pocketfft fallback, in the 128 x 48-tile kernels) against the C oracle, bit
for bit, on both tile geometries and both zero-skip twins at QP 0, 4 and 12.  The 32-row twins
run the pocketfft sequence alone (they were measured slower with the fast passes): the same
comparisons, and fallback counters that stay at zero.

Frames: 256 x 96 (2 x 2 tall tiles) and 256 x 112 (a ragged last tile row); an I-frame and two
P-frames of the bench and low-texture content, and the adversarial tie frames of
tests/adversarial.py (a flat reference delivers their blocks to the P-frame kernel unchanged),
which must take the forward fallback.  The fallback counters (Engine.take_tq_fallback_counts)
show that both the fast path and the fallback ran.
"""
import numpy as np
import pytest
import torch

import adversarial as A
from streamoptima_amd import _lib

pytestmark = pytest.mark.gpu

FRAMES = 3
KEYS = ("split", "mv", "qtc", "tokens", "recon")
QPS = (0, 4, 12)
TWINS = [(tall, zs) for tall in (1, 0) for zs in (False, True)]
_ORACLE = {}


def _oracle(w, h, content, qp):
    key = (w, h, content, qp)
    if key not in _ORACLE:
        from oracle.gop import encode_gop
        from streamoptima_amd.synth import synth_sequence
        seq = synth_sequence(FRAMES, h, w, seed=31, content=content)
        exp = encode_gop(seq, qp, FRAMES)
        for i, r in enumerate(exp):
            d = seq[i].astype(np.int64) - r["recon"].astype(np.int64)
            r["sse_total"] = int((d * d).sum())
        _ORACLE[key] = (seq, exp)
    return _ORACLE[key]


def _encode(gpu, seq, w, h, qp, tall, zero_skip):
    from streamoptima_amd.Encoder import Y_Video_codec
    from streamoptima_amd.engine import alloc_planes
    codec = Y_Video_codec(h, w, FRAMES, 16, 16, qp, FRAMES, 0, 0.015, False, device=gpu)
    eng = codec.engine()
    fr = alloc_planes(FRAMES, h, w, gpu)
    fr.copy_(torch.from_numpy(seq))
    with _lib.option(_lib.OPT_RUN_TALL_TILES, tall):
        eng.zero_skip = zero_skip
        eng.take_tq_fallback_counts()
        res = codec.encode_device(fr, FRAMES, check=False)
        torch.cuda.synchronize()
        eng.check_run()
    counts = eng.take_tq_fallback_counts()
    host = []
    for s in res["symbols"]:
        d = {k: getattr(s, k).cpu().numpy() for k in KEYS + ("mae_num",)}
        d["frame_type"] = s.frame_type
        host.append(d)
    return host, [int(v) for v in res["sse"].cpu().numpy()], counts


@pytest.mark.parametrize("qp", QPS)
@pytest.mark.parametrize("content", ["bench", "lowtex"])
@pytest.mark.parametrize("w,h", [(256, 96), (256, 112)])
def test_gop_matches_oracle(gpu, w, h, content, qp):
    seq, exp = _oracle(w, h, content, qp)
    for tall, zero_skip in TWINS:
        got, sse, _ = _encode(gpu, seq, w, h, qp, tall, zero_skip)
        what = f"tall {tall} zero_skip {zero_skip}"
        for i in range(FRAMES):
            assert got[i]["frame_type"] == exp[i]["frame_type"]
            for k in KEYS:
                a, b = got[i][k], np.asarray(exp[i][k])
                assert a.shape == b.shape, (what, i, k, a.shape, b.shape)
                bad = np.flatnonzero(a.reshape(-1) != b.reshape(-1))
                assert bad.size == 0, f"{what} frame {i} {k}: {bad.size} differ from the oracle, first at {bad[:3].tolist()}"
            if "mae_num" in exp[i]:
                assert (got[i]["mae_num"] == np.asarray(exp[i]["mae_num"])).all(), (what, i, "mae_num")
            assert sse[i] == exp[i]["sse_total"], (what, i, sse[i], exp[i]["sse_total"])


def test_fast_path_in_use(gpu):
    """Bench content at QP 4: fewer fallbacks than transform waves in both directions."""
    w, h = 256, 96
    seq, _ = _oracle(w, h, "bench", 4)
    _, _, (fwd, inv) = _encode(gpu, seq, w, h, 4, 1, False)
    waves = (FRAMES - 1) * ((w // 16) * (h // 16) // 4)
    print(f"fallback waves: forward {fwd}, inverse {inv} of {waves}")
    assert fwd < waves and inv < waves


# ---------------------------------------------------------------------- adversarial tie frames
def _plane(a, dev):
    from streamoptima_amd.engine import alloc_planes
    a = np.ascontiguousarray(a, dtype=np.uint8)
    p = alloc_planes(1, *a.shape, dev)[0]
    p.copy_(torch.from_numpy(a))
    return p


_TIE_EXP = {}


def _tie_expected(fi, cur, ref, qp):
    if (fi, qp) not in _TIE_EXP:
        from oracle import oracle as O
        e = O.inter_frame(cur, [ref], 16, 16, qp, None, False, 0.015)
        d = (cur.astype(np.int64) - e["recon"].astype(np.int64)) ** 2
        e["sse"] = d.reshape(A.RUN_H // 16, 16, A.RUN_W // 16, 16).sum(axis=(1, 3)).reshape(-1)
        _TIE_EXP[(fi, qp)] = e
    return _TIE_EXP[(fi, qp)]


@pytest.mark.parametrize("qp", QPS)
@pytest.mark.parametrize("tall,zero_skip", TWINS)
def test_tie_blocks_match_oracle_and_take_the_fallback(gpu, tall, zero_skip, qp):
    from streamoptima_amd.engine import Engine
    host = A.run_frames(128)[:2]
    curs = [_plane(c, gpu) for c, _ in host]
    ref = _plane(host[0][1], gpu)
    eng = Engine(A.RUN_H, A.RUN_W, 16, 16, False, 0.015, gpu)
    outs = [eng.new_symbols(1) for _ in curs]
    eng.zero_skip = zero_skip
    with _lib.option(_lib.OPT_RUN_TALL_TILES, tall):
        eng.encode_p_runs([([c], ref, [o]) for c, o in zip(curs, outs)], qp, None)
        torch.cuda.synchronize()
        eng.check_run()
    fwd, inv = eng.take_tq_fallback_counts()
    for fi, o in enumerate(outs):
        exp = _tie_expected(fi, host[fi][0], host[fi][1], qp)
        n = exp["sse"].size
        for k in KEYS + ("mae_num", "sse"):
            got = getattr(o, k).cpu().numpy()
            got = got[:n] if k == "sse" else got
            want = np.asarray(exp[k])
            assert got.shape == want.shape, (fi, k, got.shape, want.shape)
            neq = got.astype(np.int64) != want.astype(np.int64)
            assert not neq.any(), f"frame {fi} {k}: {int(neq.sum())} values differ from the oracle"
    print(f"fallback waves: forward {fwd}, inverse {inv}")
    # the DC coefficient is sum / 16 exactly: a block whose DC is n + 1/2 with n and n + 1 on
    # different levels must have sent its wave through the pocketfft sequence (QP 0 and 4 have
    # such blocks; at QP 12 no |DC| <= 2048 reaches a step of 2^12)
    sums = np.concatenate([A.frame_residuals(c, 128).sum(axis=(1, 2)) for c, _ in host])
    n = sums[sums % 16 == 8] // 16
    lev = lambda t: np.round(t / 2.0 ** qp)          # noqa: E731  (half to even, as quantize_TC)
    must = bool((lev(n) != lev(n + 1)).any())
    assert must == (qp in (0, 4))
    if not tall:
        assert (fwd, inv) == (0, 0)     # the 32-row kernels keep the pocketfft sequence throughout
    elif must:
        assert fwd > 0
