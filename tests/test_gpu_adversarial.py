"""Adversarial residual blocks (tests/adversarial.py) through every transform path, QP 0..12,
bit for bit against the C oracle (which tests/test_adversarial_blocks.py ties to scipy.fftpack
block by block on the same frames).

A flat reference plane makes every block's residual exactly cur - flat, so the blocks built to
sit on rounding edges (DC ties, coefficients on and next to quantisation steps, full-range
patterns, impulses) reach the transforms of: the plain persistent run on 128 x 48 and 128 x 32
tiles, with and without the zero-skip instantiation; the VBS run; the two-pass run (fused and as
the per-frame sequence); the per-frame kernels at bs 16 and 8, VBS off and on; the intra
kernels.  Each path runs uniform QP 0..12 and two per-row schedules whose qp_rd (3) is in neither
schedule, so a kernel that ignored qp_row, or indexed it with the wrong tile height, fails.
"""
import numpy as np
import pytest
import torch

import adversarial as A
from streamoptima_amd import _lib

pytestmark = pytest.mark.gpu

LAM = 0.015
KEYS = ("split", "mv", "qtc", "tokens", "mae_num", "recon")
UNIFORM = [(qp, None) for qp in range(13)]


def _settings(nby, uniform=UNIFORM):
    return uniform + [(3, A.row_schedule(nby)), (3, A.row_schedule(nby, True))]


_EXP, _DEV = {}, {}


def _expected(tag, cur, ref, bs, sr, qp, qr, vbs=False, intra=False, qp_map=None):
    """The oracle's frame (and its SSE: per block for a P-frame, per pixel row for an I-frame),
    computed once per input and QP setting and shared between the tests."""
    key = (tag, bs, qp, None if qr is None else tuple(qr), vbs, intra, None if qp_map is None else qp_map.tobytes())
    if key not in _EXP:
        from oracle import oracle as O
        if intra:
            e = O.intra_frame(cur, bs, sr, qp, qr, vbs, LAM, qp_map=qp_map)
        else:
            e = O.inter_frame(cur, [ref], bs, sr, qp, qr, vbs, LAM, qp_map=qp_map)
        d = (cur.astype(np.int64) - e["recon"].astype(np.int64)) ** 2
        h, w = cur.shape
        e["sse"] = d.sum(axis=1) if intra else d.reshape(h // bs, bs, w // bs, bs).sum(axis=(1, 3)).reshape(-1)
        _EXP[key] = e
    return _EXP[key]


def _plane(a, dev):
    from streamoptima_amd.engine import alloc_planes
    a = np.ascontiguousarray(a, dtype=np.uint8)
    p = alloc_planes(1, *a.shape, dev)[0]
    p.copy_(torch.from_numpy(a))
    return p


def _dev_frames(flat, dev):
    """The run frames of a flat level on the device: ([cur planes], the flat reference plane)."""
    if flat not in _DEV:
        fr = A.run_frames(flat)
        _DEV[flat] = ([_plane(c, dev) for c, _ in fr], _plane(fr[0][1], dev))
    return _DEV[flat]


def _mismatch(sym, exp, what):
    """'' or a message naming the first differing output of a frame, with its block indices."""
    n = exp["sse"].size
    for k in KEYS + ("sse",):
        got = getattr(sym, k).cpu().numpy()
        want = np.asarray(exp[k])
        if k == "sse":
            if got[n:].any():
                return f"{what}: sse is not zero past its {n} entries"
            got = got[:n]
        if got.shape != want.shape:
            return f"{what}: {k} shape {got.shape} != {want.shape}"
        neq = got.astype(np.int64) != want.astype(np.int64)
        if neq.any():
            where = np.flatnonzero(neq.reshape(neq.shape[0], -1).any(axis=1))
            unit = "rows" if k == "recon" or (k == "sse" and n != exp["tokens"].size) else "blocks"
            return f"{what}: {k} differs from the oracle in {where.size} {unit}, first {where[:6].tolist()}"
    return ""


def _report(bad):
    assert not bad, f"{len(bad)} mismatching frames:\n" + "\n".join(bad[:12])


# ------------------------------------------------------------------------ the persistent runs
def _run_path(gpu, flat, tall, zero_skip, vbs, settings):
    """One so_encode_p_runs launch per QP setting: every run frame an independent one-frame run
    from the shared flat plane."""
    from streamoptima_amd.engine import Engine
    host = A.run_frames(flat)
    curs, ref = _dev_frames(flat, gpu)
    eng = Engine(A.RUN_H, A.RUN_W, 16, 16, vbs, LAM, gpu)
    bad = []
    for qp, qr in settings:
        outs = [eng.new_symbols(1) for _ in curs]
        eng.zero_skip = zero_skip          # check_run re-chooses it from the content: pin it per launch
        with _lib.option(_lib.OPT_RUN_TALL_TILES, tall):
            eng.encode_p_runs([([c], ref, [o]) for c, o in zip(curs, outs)], qp, qr)
            torch.cuda.synchronize()
            eng.check_run()
        for fi, o in enumerate(outs):
            exp = _expected(("run", flat, fi), host[fi][0], host[fi][1], 16, 16, qp, qr, vbs)
            msg = _mismatch(o, exp, f"qp_rd {qp} qp_row {qr} frame {fi}")
            if msg:
                bad.append(msg)
    return bad


@pytest.mark.parametrize("zero_skip", [False, True], ids=["plain", "zero_skip"])
@pytest.mark.parametrize("tall", [1, 0], ids=["tall", "short"])
def test_plain_run(gpu, tall, zero_skip):
    with _lib.option(_lib.OPT_RUN_TALL_TILES, tall):
        assert _lib.load().so_p_run_tile_rows(A.RUN_H, A.RUN_W, 1) == (3 if tall else 2)
    _report(_run_path(gpu, 128, tall, zero_skip, False, _settings(7)))


def test_vbs_run(gpu):
    """Both VBS instantiations (uniform QP with no qp_row; per-row), the quadrant DC ties in the
    8 x 8 sub-block transforms.  qp_rd drives the RD decision under a row schedule too."""
    settings = _settings(7)
    _report(_run_path(gpu, 128, -1, False, True, settings))
    host = A.run_frames(128)
    splits = np.concatenate([_expected(("run", 128, fi), c, r, 16, 16, qp, qr, True)["split"]
                             for fi, (c, r) in enumerate(host) for qp, qr in settings])
    assert splits.any() and not splits.all()      # the reference side takes both branches


@pytest.mark.parametrize("flat", [0, 255])
def test_plain_run_full_range_residuals(gpu, flat):
    """|R| up to 255: flat planes of 0 (R in [0, 255]) and 255 (R in [-255, 0])."""
    _report(_run_path(gpu, flat, 1, False, False, [(0, None), (4, None), (11, None)]))


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "sequence"])
def test_two_pass_run(gpu, fused):
    """so_encode_p_run_2pass, one frame per call, ROI offsets -4..+4 clamped to [0, 12]: the QP
    map and the pass-2 symbols against pass-1 tokens -> oracle.qp_map -> inter_frame(qp_map)."""
    from oracle import oracle as O
    from streamoptima_amd.engine import Engine
    host = A.run_frames(128)
    curs, ref = _dev_frames(128, gpu)
    eng = Engine(A.RUN_H, A.RUN_W, 16, 16, False, LAM, gpu)
    roi = A.roi_offsets(eng.nb)
    bad = []
    with _lib.option(_lib.OPT_RUN_2PASS_FUSED, fused):
        if fused:
            assert _lib.load().so_p_run_2pass_fused(A.RUN_H, A.RUN_W) == 1
        for qp, qr in _settings(7):
            roi_dev = eng.device_const_i32(roi)
            for fi, cur in enumerate(curs):
                out = eng.new_symbols(1)
                qmap = torch.full((eng.nb,), -1, dtype=torch.int32, device=gpu)
                eng.encode_p_run_2pass([cur], ref, qp, [out], [qmap], qp_row=qr, roi_dev=roi_dev, qp_lo=0, qp_hi=12)
                torch.cuda.synchronize()
                eng.check_run()
                p1 = _expected(("run", 128, fi), host[fi][0], host[fi][1], 16, 16, qp, qr)
                qm = O.qp_map(p1["tokens"], eng.nbx, eng.nby, qp, qr, roi, 0, 12)
                what = f"qp_rd {qp} qp_row {qr} frame {fi}"
                got = qmap.cpu().numpy()
                if not np.array_equal(got, qm):
                    bad.append(f"{what}: qp_map differs in blocks {np.flatnonzero(got != qm)[:6].tolist()}")
                    continue
                exp = _expected(("run", 128, fi), host[fi][0], host[fi][1], 16, 16, qp, qr, qp_map=qm)
                msg = _mismatch(out, exp, what)
                if msg:
                    bad.append(msg)
    _report(bad)


# --------------------------------------------------------------------- the per-frame kernels
def _per_frame(gpu, tag, cur, ref, bs, sr, vbs, settings, intra=False):
    from streamoptima_amd.engine import Engine
    h, w = cur.shape
    eng = Engine(h, w, bs, sr, vbs, LAM, gpu)
    c, r = _plane(cur, gpu), _plane(ref, gpu)
    bad = []
    for qp, qr in settings:
        sym = eng.encode_i(c, qp, qr) if intra else eng.encode_p(c, [r], qp, qr)
        torch.cuda.synchronize()
        msg = _mismatch(sym, _expected(tag, cur, ref, bs, sr, qp, qr, vbs, intra), f"{tag} qp_rd {qp} qp_row {qr}")
        if msg:
            bad.append(msg)
    return bad


@pytest.mark.parametrize("vbs", [False, True], ids=["vbs0", "vbs1"])
def test_per_frame_kernels_bs16(gpu, vbs):
    """so_encode_p_rows: the run frames (256 x 112) and 144 x 64, which never takes the run."""
    bad = []
    for fi, (cur, ref) in enumerate(A.run_frames(128)):
        bad += _per_frame(gpu, ("run", 128, fi), cur, ref, 16, 16, vbs, _settings(7))
    cur, ref, _ = A.small_frames()["p144x64"]
    bad += _per_frame(gpu, "p144x64", cur, ref, 16, 16, vbs, _settings(4))
    _report(bad)


@pytest.mark.parametrize("flat", [0, 255])
def test_per_frame_kernels_full_range_residuals(gpu, flat):
    bad = []
    for fi, (cur, ref) in enumerate(A.run_frames(flat)):
        bad += _per_frame(gpu, ("run", flat, fi), cur, ref, 16, 16, False, [(0, None), (4, None), (11, None)])
    _report(bad)


def test_per_frame_kernels_bs8(gpu):
    cur, ref, _ = A.small_frames()["p64x64_bs8"]
    settings = [(qp, None) for qp in range(11)] + [(3, A.BS8_ROWS), (3, A.BS8_ROWS[::-1])]
    _report(_per_frame(gpu, "p64x64_bs8", cur, ref, 8, 8, False, settings))


@pytest.mark.parametrize("name,bs,vbs", [("i16x384", 16, False), ("i16x384", 16, True), ("i8x256", 8, False)])
def test_intra_kernels(gpu, name, bs, vbs):
    """One block wide: every block is predicted from 128, so its residual is cur - 128."""
    cur, ref, _ = A.small_frames()[name]
    _report(_per_frame(gpu, name, cur, ref, bs, bs, vbs, _settings(cur.shape[0] // bs), intra=True))
