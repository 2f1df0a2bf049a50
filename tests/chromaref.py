"""The chroma checker of the tests: the normative 4:2:0 chroma arithmetic (DESIGN.md "Chroma
4:2:0", include/streamoptima.h so_chroma_encode_frame) in numpy + scipy.fftpack.  The reference
codes luma only, so this model -- built from the reference's per-block functions at N = 8 -- is
what the GPU kernels are held against, bit for bit.

Luma is H x W (padded, 16x16 blocks); each chroma plane is Hc x Wc = H/2 x W/2 and luma block
b = (bx, by) owns the 8x8 chroma block at (8 bx, 8 by).  Luma symbols: split uint8 [nb],
mv int16 [nb, 4, 3] = (dx, dy, ref) per quadrant (entry 0 for an unsplit block)."""
import numpy as np
from scipy.fftpack import dct, idct

N = 8


def scan_order(n=N):
    order = []
    for k in range(2 * n - 1):
        i, j = (0, k) if k < n else (k - n + 1, n - 1)
        while i < n and j >= 0:
            order.append(i * n + j)
            i += 1
            j -= 1
    return np.array(order)


_SCAN = scan_order()


def q_matrix(qp):
    """generate_Q_matrix(8, qp) (Encoder.py:938-945)."""
    s = np.arange(N)[:, None] + np.arange(N)[None, :]
    return np.where(s < N - 1, 2 ** qp, np.where(s == N - 1, 2 ** (qp + 1), 2 ** (qp + 2))).astype(np.int64)


def block_qp(nbx, nby, qp, qp_row=None, qp_map=None, qp_offset=0):
    """qpc per block: clamp(base + offset, 0, 20), base = map entry, else row entry, else qp."""
    if qp_map is not None:
        base = np.asarray(qp_map, np.int64).reshape(nby, nbx)
    elif qp_row is not None:
        base = np.repeat(np.asarray(qp_row, np.int64).reshape(nby, 1), nbx, axis=1)
    else:
        base = np.full((nby, nbx), int(qp), np.int64)
    return np.clip(base + int(qp_offset), 0, 20).reshape(-1)


def predict(refs, split, mv, hc, wc):
    """P-frame prediction of one plane: refs = the plane's reconstructions in reference-list
    order.  Every sample takes its block's (quadrant's, when split) luma MV halved."""
    nbx = wc // N
    refs = np.stack([np.asarray(r, np.int64) for r in refs])
    nref = refs.shape[0]
    ys, xs = np.mgrid[0:hc, 0:wc]
    b = (ys // N) * nbx + xs // N
    quad = 2 * ((ys % N) // 4) + (xs % N) // 4
    j = np.where(np.asarray(split)[b] != 0, quad, 0)
    m = np.asarray(mv, np.int64)[b, j]          # [hc, wc, 3]
    dx, dy, r = m[..., 0], m[..., 1], np.clip(m[..., 2], 0, nref - 1)
    ix, fx, iy, fy = dx >> 1, dx & 1, dy >> 1, dy & 1
    x0, x1 = np.clip(xs + ix, 0, wc - 1), np.clip(xs + ix + fx, 0, wc - 1)
    y0, y1 = np.clip(ys + iy, 0, hc - 1), np.clip(ys + iy + fy, 0, hc - 1)
    return (refs[r, y0, x0] + refs[r, y0, x1] + refs[r, y1, x0] + refs[r, y1, x1] + 2) >> 2


def _blocks(plane):
    hc, wc = plane.shape
    return plane.reshape(hc // N, N, wc // N, N).transpose(0, 2, 1, 3).reshape(-1, N, N)


def _plane(blocks, hc, wc):
    return blocks.reshape(hc // N, wc // N, N, N).transpose(0, 2, 1, 3).reshape(hc, wc)


def tokens_of(q):
    """len(entropy_encoder_block(q, 8)) per block (Encoder.py:1086-1131): one token per
    non-zero value plus one per maximal run in anti-diagonal scan order."""
    nz = q.reshape(-1, N * N)[:, _SCAN] != 0
    return (nz.sum(1) + 1 + (nz[:, 1:] != nz[:, :-1]).sum(1)).astype(np.int32)


def _recon(pred, qtc, qpc):
    Q = np.stack([q_matrix(q) for q in qpc])
    deq = (qtc.astype(np.int64).reshape(-1, N, N) * Q).astype(np.float64)       # rescale_QTC
    res = np.round(idct(idct(deq, axis=-2, norm="ortho"), axis=-1, norm="ortho")).astype(np.int64)
    return (_blocks(pred) + res).astype(np.uint8)                              # wraps like reconstruct_block


def _pred_plane(refs, frame_type, split, mv, hc, wc):
    if frame_type == 0:
        return np.full((hc, wc), 128, np.int64)
    return predict(refs, split, mv, hc, wc)


def encode_plane(cur, refs, frame_type, split, mv, qpc):
    hc, wc = cur.shape
    pred = _pred_plane(refs, frame_type, split, mv, hc, wc)
    res = _blocks(np.asarray(cur, np.int64) - pred).astype(np.float64)
    tc = np.round(dct(dct(res, axis=-2, norm="ortho"), axis=-1, norm="ortho")).astype(np.int64)   # apply_2d_dct
    Q = np.stack([q_matrix(q) for q in qpc])
    qtc = np.round(tc / Q).astype(np.int64)                                                        # quantize_TC
    rec = _recon(pred, qtc, qpc)
    sse = ((_blocks(np.asarray(cur, np.int64)) - rec.astype(np.int64)) ** 2).sum(axis=(1, 2)).astype(np.int32)
    return {"qtc": qtc.reshape(-1, N * N).astype(np.int16), "tokens": tokens_of(qtc),
            "recon": _plane(rec, hc, wc), "sse": sse}


def encode_frame(cur_u, cur_v, refs_u, refs_v, frame_type, split, mv, qp, qp_row=None, qp_map=None, qp_offset=0):
    """One frame's U and V.  Returns qtc_u/v int16 [nb, 64], tokens and sse int32 [2, nb],
    recon_u/v uint8 [Hc, Wc]."""
    hc, wc = cur_u.shape
    qpc = block_qp(wc // N, hc // N, qp, qp_row, qp_map, qp_offset)
    u = encode_plane(np.asarray(cur_u), refs_u, frame_type, split, mv, qpc)
    v = encode_plane(np.asarray(cur_v), refs_v, frame_type, split, mv, qpc)
    return {"qtc_u": u["qtc"], "qtc_v": v["qtc"], "tokens": np.stack([u["tokens"], v["tokens"]]),
            "recon_u": u["recon"], "recon_v": v["recon"], "sse": np.stack([u["sse"], v["sse"]])}


def recon_frame(qtc_u, qtc_v, refs_u, refs_v, frame_type, split, mv, hc, wc, qp, qp_row=None, qp_map=None,
                qp_offset=0):
    """The decoder: (recon_u, recon_v) from the quantised coefficients."""
    qpc = block_qp(wc // N, hc // N, qp, qp_row, qp_map, qp_offset)
    out = []
    for qtc, refs in ((qtc_u, refs_u), (qtc_v, refs_v)):
        pred = _pred_plane(refs, frame_type, split, mv, hc, wc)
        out.append(_plane(_recon(pred, np.asarray(qtc), qpc), hc, wc))
    return tuple(out)


def encode_gop(uv, luma, nref_frames=1, qp_offset=0):
    """GOP driver.  uv: uint8 [F, 2, Hc, Wc]; luma: per frame a dict with frame_type, split, mv,
    qp and optionally qp_row / qp_map (the luma frame's own).  The chroma reference list is the
    luma one's: starts as one all-128 plane, an I-frame clears it, every frame's reconstruction is
    appended (the oldest dropped at nref_frames)."""
    f, _, hc, wc = uv.shape
    refs_u = [np.full((hc, wc), 128, np.uint8)]
    refs_v = [np.full((hc, wc), 128, np.uint8)]
    out = []
    for i, s in enumerate(luma):
        if s["frame_type"] == 0:
            refs_u, refs_v = [], []
        fr = encode_frame(uv[i, 0], uv[i, 1], refs_u, refs_v, s["frame_type"], s.get("split"), s.get("mv"),
                          s["qp"], s.get("qp_row"), s.get("qp_map"), qp_offset)
        out.append(fr)
        if i < f - 1:
            if len(refs_u) >= nref_frames:
                refs_u.pop(0)
                refs_v.pop(0)
            refs_u.append(fr["recon_u"])
            refs_v.append(fr["recon_v"])
    return out
