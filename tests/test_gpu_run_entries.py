"""The persistent-run instantiations no other GPU test launches (so_run_select.h's table), each
against the C oracle bit for bit on a 256 x 112 frame (adversarial.RUN_W x RUN_H: 2 x 4 tiles,
a ragged last tile row), an I-frame and a run of two P-frames:

  * the VBS one-GPU run with the test hooks compiled in (SO_OPT_COUNT_SAD_OPS), under uniform QP
    and under a row-QP schedule -- the count shows the hook kernel ran;
  * the VBS frame pipeline under a row-QP schedule (two ranks sharing the GPU).
"""
import numpy as np
import pytest
import torch

import adversarial as A
from streamoptima_amd import _lib

pytestmark = pytest.mark.gpu

QP, FRAMES, LAM = 4, 3, 0.015
QP_ROWS = [2, 3, 4, 5, 6, 4, 3]     # A.RUN_H // 16 block rows
KEYS = ("split", "mv", "qtc", "tokens", "recon")
_ORACLE = {}


def _oracle(qr):
    """(frames, the oracle's VBS symbols of the I-frame and the two P-frames), once per schedule."""
    key = None if qr is None else tuple(qr)
    if key not in _ORACLE:
        from oracle import oracle as O
        from streamoptima_amd.synth import synth_sequence
        seq = synth_sequence(FRAMES, A.RUN_H, A.RUN_W, seed=31)
        exp = [O.intra_frame(seq[0], 16, 16, QP, qr, True, LAM)]
        for i in range(1, FRAMES):
            exp.append(O.inter_frame(seq[i], [exp[-1]["recon"]], 16, 16, QP, qr, True, LAM))
        _ORACLE[key] = (seq, exp)
    return _ORACLE[key]


def _assert_frames(syms, exp, what):
    for i, (s, e) in enumerate(zip(syms, exp)):
        for k in KEYS:
            a, b = getattr(s, k).cpu().numpy(), np.asarray(e[k])
            assert a.shape == b.shape, (what, i, k, a.shape, b.shape)
            bad = np.flatnonzero(a.reshape(-1) != b.reshape(-1))
            assert bad.size == 0, f"{what} frame {i} {k}: {bad.size} differ from the oracle, first at {bad[:3].tolist()}"


@pytest.mark.parametrize("qr", [None, QP_ROWS], ids=["uniform_qp", "row_qp"])
def test_vbs_hook_run_matches_oracle(gpu, qr):
    from streamoptima_amd.engine import Engine, alloc_planes
    seq, exp = _oracle(qr)
    eng = Engine(A.RUN_H, A.RUN_W, 16, 16, True, LAM, gpu)
    fr = alloc_planes(FRAMES, A.RUN_H, A.RUN_W, gpu)
    fr.copy_(torch.from_numpy(seq))
    i0 = eng.encode_i(fr[0], QP, qr)
    outs = [eng.new_symbols(1) for _ in range(FRAMES - 1)]
    with _lib.option(_lib.OPT_COUNT_SAD_OPS, 1):
        eng.encode_p_run([fr[i] for i in range(1, FRAMES)], i0.recon, QP, outs, qp_row=qr)
        torch.cuda.synchronize()
    eng.check_run()
    assert eng.take_sad_ops() > 0
    _assert_frames([i0] + outs, exp, "hook run")


def test_vbs_frame_pipeline_row_qp_matches_oracle(gpu):
    from streamoptima_amd.engine import Engine, alloc_planes
    from streamoptima_amd.pipeline import FramePipeRank
    from test_gpu_pipeline import _streams
    seq, exp = _oracle(QP_ROWS)
    fr = alloc_planes(FRAMES, A.RUN_H, A.RUN_W, gpu)
    fr.copy_(torch.from_numpy(seq))
    world = 2
    engines = [Engine(A.RUN_H, A.RUN_W, 16, 16, True, LAM, gpu) for _ in range(world)]
    streams = _streams(gpu)[:world]
    ranks = [FramePipeRank(engines[r], world, r, FRAMES, stream=streams[r], max_wg=16) for r in range(world)]
    torch.cuda.synchronize()
    for r in range(world):
        ranks[r].connect(ranks[(r + 1) % world].info(), ranks[(r - 1) % world].info())
    for r in range(world):   # every rank's buffers before any rank's persistent grid runs
        ranks[r].prepare(FRAMES, QP_ROWS)
    torch.cuda.synchronize()
    syms = {}
    for r in range(world):
        with torch.cuda.stream(streams[r]):
            syms.update(ranks[r].encode(fr, FRAMES, QP, qp_row=QP_ROWS))
    torch.cuda.synchronize()
    for r in ranks:
        r.check()
    _assert_frames([syms[k] for k in range(FRAMES)], exp, "frame pipeline")
    for r in ranks:
        r.close()
