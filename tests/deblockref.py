"""The deblocking post-filter in numpy: include/streamoptima.h "Deblocking", written from that text
(not from so_deblock.hip).  Exact integers; >> on numpy ints is the arithmetic shift.

    thresholds(q)                       alpha, beta, tc, tc1 of an edge with parameter q
    filter_lines(p2, .., q2, q, ...)    the six samples of many lines at once -> p1', p0', q0', q1'
    cell_grid(...)                      cellqp of every 8 x 8 cell, and which cell borders are edges
    deblock_plane(plane, grid, s)       pass 1 (vertical edges), pass 2 (horizontal edges)
    deblock_yuv420(y, u, v, ...)        Y, U and V of one frame
    Stats                               counts of the filter's branches, for the tests of the corpus
"""
import numpy as np


class Stats(dict):
    """Counts per branch; filter_lines adds to them when given one."""

    KEYS = ("lines", "off_alpha", "off_beta", "on", "ap_only", "aq_only", "ap_aq", "dl_clip_hi", "dl_clip_lo",
            "p0_clip_0", "p0_clip_255", "q0_clip_0", "q0_clip_255", "mixed_qp", "split_next_to_unsplit")

    def __init__(self):
        super().__init__({k: 0 for k in self.KEYS})


def thresholds(q):
    q = np.asarray(q, dtype=np.int64)
    s = np.int64(1) << q
    alpha = np.minimum(s, 255)
    beta = np.minimum((3 * s) >> 3, 255)
    tc = np.minimum(s >> 2, 255)
    return alpha, beta, tc, tc >> 1


def filter_lines(p2, p1, p0, q0, q1, q2, q, exists=True, stats=None):
    """All arguments broadcast to one shape.  Returns (p1', p0', q0', q1') as int64."""
    p2, p1, p0, q0, q1, q2 = (np.asarray(a, dtype=np.int64) for a in (p2, p1, p0, q0, q1, q2))
    alpha, beta, tc, tc1 = thresholds(q)
    exists = np.broadcast_to(np.asarray(exists, dtype=bool), np.broadcast(p0, tc).shape)
    d = q0 - p0
    in_alpha = np.abs(d) < alpha
    in_beta = (np.abs(p1 - p0) < beta) & (np.abs(q1 - q0) < beta)
    on = exists & in_alpha & in_beta
    ap = np.abs(p2 - p0) < beta
    aq = np.abs(q2 - q0) < beta
    raw = (4 * d + (p1 - q1) + 4) >> 3
    dl = np.clip(raw, -tc, tc)
    avg = (p0 + q0 + 1) >> 1
    n_p0 = np.clip(p0 + dl, 0, 255)
    n_q0 = np.clip(q0 - dl, 0, 255)
    n_p1 = p1 + np.clip((p2 + avg - 2 * p1) >> 1, -tc1, tc1)
    n_q1 = q1 + np.clip((q2 + avg - 2 * q1) >> 1, -tc1, tc1)
    assert n_p1[on & ap].min(initial=0) >= 0 and n_p1[on & ap].max(initial=0) <= 255
    assert n_q1[on & aq].min(initial=0) >= 0 and n_q1[on & aq].max(initial=0) <= 255
    if stats is not None:
        live = exists & (tc > 0)       # where the filter can act at all
        stats["lines"] += int(live.sum())
        stats["off_alpha"] += int((live & ~in_alpha).sum())
        stats["off_beta"] += int((live & in_alpha & ~in_beta).sum())
        act = on & (tc > 0)
        stats["on"] += int(act.sum())
        stats["ap_only"] += int((act & ap & ~aq).sum())
        stats["aq_only"] += int((act & ~ap & aq).sum())
        stats["ap_aq"] += int((act & ap & aq).sum())
        stats["dl_clip_hi"] += int((act & (raw > tc)).sum())
        stats["dl_clip_lo"] += int((act & (raw < -tc)).sum())
        stats["p0_clip_0"] += int((act & (p0 + dl < 0)).sum())
        stats["p0_clip_255"] += int((act & (p0 + dl > 255)).sum())
        stats["q0_clip_0"] += int((act & (q0 - dl < 0)).sum())
        stats["q0_clip_255"] += int((act & (q0 - dl > 255)).sum())
    return (np.where(on & ap, n_p1, p1), np.where(on, n_p0, p0), np.where(on, n_q0, q0), np.where(on & aq, n_q1, q1))


def filter_line(p2, p1, p0, q0, q1, q2, q):
    """One line, as python ints: (p1', p0', q0', q1')."""
    return tuple(int(v) for v in filter_lines(p2, p1, p0, q0, q1, q2, q))


class Grid:
    """cellqp [h/8, w/8]; vedge[cy, cx]: the border between cells (cy, cx-1) and (cy, cx) is an edge;
    hedge[cy, cx]: the border between (cy-1, cx) and (cy, cx) is."""

    def __init__(self, cellqp, vedge, hedge):
        self.cellqp, self.vedge, self.hedge = cellqp, vedge, hedge


def block_qp(nby, nbx, qp, qp_row=None, qp_map=None):
    if qp_map is not None:
        bq = np.asarray(qp_map, dtype=np.int64).reshape(nby, nbx)
    elif qp_row is not None:
        bq = np.repeat(np.asarray(qp_row, dtype=np.int64).reshape(nby, 1), nbx, axis=1)
    else:
        bq = np.full((nby, nbx), int(qp), dtype=np.int64)
    return np.clip(bq, 0, 20)


def cell_grid(H, W, bs, split=None, qp=0, qp_row=None, qp_map=None, chroma=False, chroma_qp_offset=0):
    """The grid of a luma plane (H x W), or with chroma=True of a chroma plane (H/2 x W/2) of the same
    frame.  H, W: the LUMA plane's size."""
    assert bs in (8, 16) and H % bs == 0 and W % bs == 0
    nby, nbx = H // bs, W // bs
    bq = block_qp(nby, nbx, qp, qp_row, qp_map)
    if chroma:
        assert bs == 16
        cq = np.clip(bq + int(chroma_qp_offset), 0, 20)
        vedge = np.ones((nby, nbx), dtype=bool)
        hedge = np.ones((nby, nbx), dtype=bool)
    else:
        assert not (bs == 8 and split is not None), "bs 8 with split flags is refused, not filtered"
        sp = np.zeros((nby, nbx), dtype=bool) if split is None else np.asarray(split).reshape(nby, nbx) != 0
        cpb = bs // 8
        cq = np.where(sp, np.where(bq > 0, bq - 1, 0), bq)
        cq = np.repeat(np.repeat(cq, cpb, axis=0), cpb, axis=1)
        spc = np.repeat(np.repeat(sp, cpb, axis=0), cpb, axis=1)
        cy, cx = np.indices(cq.shape)
        vedge = (cx % cpb == 0) | spc     # different blocks, or one split block
        hedge = (cy % cpb == 0) | spc
    vedge = vedge.copy()
    hedge = hedge.copy()
    vedge[:, 0] = False                   # no edge on the plane's border
    hedge[0, :] = False
    return Grid(cq, vedge, hedge)


def _pass_vertical_edges(x, cq, vedge, strength, stats):
    """Lines along the rows of x (int64 [h, w]) across every vertical edge; returns a new array."""
    h, w = x.shape
    ncx = w // 8
    out = x.copy()
    if ncx < 2:
        return out
    e = 8 * np.arange(1, ncx)                                # edge positions
    rows_cell = np.arange(h) // 8
    cqp = cq[rows_cell][:, :-1]                              # [h, ncx-1]: the cell on the p side
    cqq = cq[rows_cell][:, 1:]
    q = np.clip(np.maximum(cqp, cqq) + int(strength), 0, 20)
    ex = vedge[rows_cell][:, 1:]
    if stats is not None:
        stats["mixed_qp"] += int((ex & (cqp != cqq)).sum())
    s = [x[:, e + k] for k in (-3, -2, -1, 0, 1, 2)]
    n_p1, n_p0, n_q0, n_q1 = filter_lines(*s, q, ex, stats)
    out[:, e - 2], out[:, e - 1], out[:, e], out[:, e + 1] = n_p1, n_p0, n_q0, n_q1
    return out


def deblock_plane(plane, grid, strength=0, stats=None):
    x = np.asarray(plane).astype(np.int64)
    assert x.ndim == 2 and x.shape[0] % 8 == 0 and x.shape[1] % 8 == 0
    assert grid.cellqp.shape == (x.shape[0] // 8, x.shape[1] // 8)
    x = _pass_vertical_edges(x, grid.cellqp, grid.vedge, strength, stats)
    x = _pass_vertical_edges(x.T, grid.cellqp.T, grid.hedge.T, strength, stats).T
    assert x.min() >= 0 and x.max() <= 255
    return np.ascontiguousarray(x).astype(np.uint8)


def deblock_yuv420(y, u=None, v=None, bs=16, split=None, qp=0, qp_row=None, qp_map=None, chroma_qp_offset=0,
                   strength=0, stats=None):
    """One frame: (y', u', v'), u' and v' None for luma only."""
    H, W = y.shape
    if stats is not None and split is not None and bs == 16:
        sp = np.asarray(split).reshape(H // 16, W // 16) != 0
        stats["split_next_to_unsplit"] += int((sp[:, 1:] != sp[:, :-1]).sum() + (sp[1:] != sp[:-1]).sum())
    oy = deblock_plane(y, cell_grid(H, W, bs, split, qp, qp_row, qp_map), strength, stats)
    if u is None:
        return oy, None, None
    gc = cell_grid(H, W, bs, None, qp, qp_row, qp_map, chroma=True, chroma_qp_offset=chroma_qp_offset)
    return oy, deblock_plane(u, gc, strength, stats), deblock_plane(v, gc, strength, stats)


def smooth_sequence(n=4, h=288, w=352):
    """The smooth test sequence of the quality claim (DESIGN.md "Deblocking"): uint8 [n, h, w]."""
    rng = np.random.default_rng(1)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for t in range(n):
        f = (128 + 60 * np.sin((x + 3 * t) / 37) * np.cos((y + t) / 53) + 40 * np.sin((x + y - 2 * t) / 91)
             + 30 * ((x - 100 - 4 * t) ** 2 + (y - 120 - t) ** 2 < 40 ** 2))
        f = f + rng.normal(0, 1.5, size=(h, w))
        out.append(np.clip(np.round(f), 0, 255).astype(np.uint8))
    return np.stack(out)


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)


def corpus_plane(h, w, rng, qps=(2, 4, 6, 8), extremes=False):
    """The designed corpus: a gradient plus steps at the cell borders whose amplitudes straddle the
    thresholds of the QPs in use (alpha = s, beta = 3s/8, tc = s/4), a little noise, so that lines
    pass and fail every test within one plane.  extremes: regions at 0 and at 255."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = 40 + (xx * 3 + yy * 2) % 170
    amps = np.array([0] + [a for q in qps for a in ((1 << q) // 4, (3 << q) // 8 - 1, (3 << q) // 8 + 1,
                                                    (1 << q) - 1, (1 << q) + 1)])
    cy, cx = yy // 8, xx // 8
    step = amps[rng.integers(0, len(amps), size=(h // 8 + 1, w // 8 + 1))][cy, cx]
    sign = rng.choice([-1, 1], size=(h // 8 + 1, w // 8 + 1))[cy, cx]
    smooth = rng.integers(0, 2, size=(h // 8 + 1, w // 8 + 1))[cy, cx]      # flat cells: ap / aq hold
    f = np.where(smooth, 128, base) + sign * step // 2 + rng.integers(-2, 3, size=(h, w))
    # ramps inside a cell towards its border make |p1 - p0| and |p2 - p0| differ
    ramp = rng.integers(0, 4, size=(h // 8 + 1, w // 8 + 1))[cy, cx]
    f = f + ramp * ((xx % 8) - 4) + (ramp // 2) * ((yy % 8) - 4)
    if extremes:
        f = np.where(cx % 5 == 0, f - 200, f)
        f = np.where(cx % 5 == 2, f + 200, f)
        # spikes off the floor and the ceiling: with a large tc, p0 + dl and q0 - dl leave 0..255
        spike = (rng.random((h, w)) < 0.3) * rng.integers(0, 120, size=(h, w))
        f = np.clip(f, 0, 255)
        f = np.where(cx % 5 == 0, f + spike, f)
        f = np.where(cx % 5 == 2, f - spike, f)
    return np.clip(f, 0, 255).astype(np.uint8)
