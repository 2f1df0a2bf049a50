"""The chroma checker with sub-sample vectors: tests/chromaref.py with its prediction replaced by
the s-parametrised one (include/streamoptima.h so_chroma_encode_frame_ex, DESIGN.md "Chroma
4:2:0").  s = the fractional bits of the luma vector seen from the chroma plane: 1 for full-sample
luma vectors (chromaref's own case), 2 for half-sample ones (FMEEnable).  Transform, QP, tokens,
reconstruction and the GOP's reference-list rule are chromaref's, imported, not restated."""
import contextlib

import numpy as np

import chromaref as CR

N = CR.N


def predict(refs, split, mv, hc, wc, s=2):
    """P-frame prediction of one plane at s fractional bits:
        ix = dx >> s, fx = dx & (D - 1), x0 = clamp(X + ix), x1 = clamp(X + ix + (fx != 0)), y alike,
        P = ((D-fx)(D-fy) R[y0][x0] + fx(D-fy) R[y0][x1] + (D-fx)fy R[y1][x0] + fx fy R[y1][x1]
             + (1 << (2s - 1))) >> 2s,   D = 1 << s."""
    D = 1 << s
    nbx = wc // N
    refs = np.stack([np.asarray(r, np.int64) for r in refs])
    nref = refs.shape[0]
    ys, xs = np.mgrid[0:hc, 0:wc]
    b = (ys // N) * nbx + xs // N
    quad = 2 * ((ys % N) // 4) + (xs % N) // 4
    j = np.where(np.asarray(split)[b] != 0, quad, 0)
    m = np.asarray(mv, np.int64)[b, j]
    dx, dy, r = m[..., 0], m[..., 1], np.clip(m[..., 2], 0, nref - 1)
    ix, fx, iy, fy = dx >> s, dx & (D - 1), dy >> s, dy & (D - 1)
    x0, x1 = np.clip(xs + ix, 0, wc - 1), np.clip(xs + ix + (fx != 0), 0, wc - 1)
    y0, y1 = np.clip(ys + iy, 0, hc - 1), np.clip(ys + iy + (fy != 0), 0, hc - 1)
    acc = ((D - fx) * (D - fy) * refs[r, y0, x0] + fx * (D - fy) * refs[r, y0, x1]
           + (D - fx) * fy * refs[r, y1, x0] + fx * fy * refs[r, y1, x1])
    return (acc + (1 << (2 * s - 1))) >> (2 * s)


@contextlib.contextmanager
def _predicting(s):
    """chromaref's frame functions look `predict` up in their module: stand this one in."""
    old = CR.predict
    CR.predict = lambda refs, split, mv, hc, wc: predict(refs, split, mv, hc, wc, s)
    try:
        yield
    finally:
        CR.predict = old


def encode_frame(*args, s=2, **kw):
    with _predicting(s):
        return CR.encode_frame(*args, **kw)


def recon_frame(*args, s=2, **kw):
    with _predicting(s):
        return CR.recon_frame(*args, **kw)


def encode_gop(uv, luma, nref_frames=1, qp_offset=0, s=2):
    with _predicting(s):
        return CR.encode_gop(uv, luma, nref_frames=nref_frames, qp_offset=qp_offset)
