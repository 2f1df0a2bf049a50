"""Frames for the SEA survivor-threshold tests (test_gpu_sea_slack.py): 256 x 96, 16 x 6 blocks.

Threshold frames, one per remainder class r of the current block's 4x4 cell sums and per layout
of designed blocks.  A designed block owns the 3 x 3 blocks around it in the reference and puts,
at block-aligned displacements (dx, dy in {-16, 0, 16}, the valid ones sorted by the search's
tie order |dx| + |dy|, then dx-major scan):
  * M (first) and T (second, where three are valid): the block with every cell sum moved to the
    near end of the next quantisation interval -- q' = q + 1 at s' = 16 q' for r = 8 and 15,
    q' = q - 1 at s' = 16 q' + 15 for r = 0 -- by single-sided +-1 steps, so LBq = 16 and
    SAD = 16 * 16 - K_b exactly (K_b = 128 for r = 8, 240 for r = 0 and 15): on the threshold of a
    bound with slack K_b, lost by a slack one smaller;
  * C0 (last): the block with +-1 steps that keep every cell sum's quotient: LBq = 0, the
    smallest bound of the window, and the same SAD.  So U is that SAD whichever of the three
    supplies it, M and T pass the bound with nothing to spare, and M wins the tie on |dx| + |dy|.
    A search that loses M and T returns C0 (or T for M): another vector at the same SAD.
The rest of the reference is seeded noise; every other block of the current frame is the
reference's co-located block."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

W, H = 256, 96
NBX, NBY = W // 16, H // 16
LAYOUTS = {
    "inner": ((1, 4, 7, 10, 13), (1, 4)),                  # by 4: dy = +16 is past the frame (umin_edge)
    "first": ((0, 3, 6, 9, 12, 15), (0, 3)),               # first block row, first and last column
    "last": ((0, 3, 6, 9, 12, 15), (2, 5)),                # last block row
}
SAD_TARGET = {8: 128, 0: 16, 15: 16}
K_B = {8: 128, 0: 240, 15: 240}


def valid(x, y, dx, dy):
    return 0 <= x + dx < W - 16 and 0 <= y + dy < H - 16


def roles(bx, by):
    """The valid block-aligned displacements of block (bx, by) in the search's tie order."""
    p = [(dx, dy) for dx in (-16, 0, 16) for dy in (-16, 0, 16) if valid(bx * 16, by * 16, dx, dy)]
    return sorted(p, key=lambda d: (abs(d[0]) + abs(d[1]), (d[0] + 16) * 33 + d[1] + 16))


def designed_blocks(layout):
    bxs, bys = LAYOUTS[layout]
    return [(bx, by) for by in bys for bx in bxs if len(roles(bx, by)) >= 2]


def _cells(rng, fn):
    """A 16 x 16 int array built cell by cell: fn(rng) -> 16 values of one 4x4 cell."""
    out = np.zeros((16, 16), np.int64)
    for cy in range(4):
        for cx in range(4):
            out[4 * cy:4 * cy + 4, 4 * cx:4 * cx + 4] = np.asarray(fn(rng)).reshape(4, 4)
    return out


def _steps(rng, up, down):
    v = np.array([1] * up + [-1] * down + [0] * (16 - up - down))
    return rng.permutation(v)


def threshold_pair(r, layout, seed):
    """(cur, ref) uint8 [H, W] of remainder class r in {8, 0, 15}."""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 256, size=(H, W)).astype(np.int64)
    blocks = {}
    for bx, by in designed_blocks(layout):
        base = np.repeat(np.repeat(rng.integers(16, 231, size=(4, 4)), 4, axis=0), 4, axis=1)
        ones = {8: 8, 0: 0, 15: 15}[r]
        blk = base + _cells(rng, lambda g: g.permutation([1] * ones + [0] * (16 - ones)))
        # on the threshold, (+1 steps, -1 steps) per cell: r = 8: eight +1 and r = 15: one +1
        # (s' = 16 v + 16); r = 0: one -1 (s' = 16 v - 1)
        edge = {8: (8, 0), 0: (0, 1), 15: (1, 0)}[r]
        # same quotients: r = 8: four +1 and four -1; r = 0: one +1; r = 15: one -1
        same = {8: (4, 4), 0: (1, 0), 15: (0, 1)}[r]
        p = roles(bx, by)
        for k, (dx, dy) in enumerate(p):
            x, y = bx * 16 + dx, by * 16 + dy
            if k == len(p) - 1:
                ref[y:y + 16, x:x + 16] = blk + _cells(rng, lambda g: _steps(g, *same))
            elif k < 2:
                ref[y:y + 16, x:x + 16] = blk + _cells(rng, lambda g: _steps(g, *edge))
        blocks[(bx, by)] = blk
    cur = ref.copy()
    for (bx, by), blk in blocks.items():
        cur[by * 16:by * 16 + 16, bx * 16:bx * 16 + 16] = blk
    assert cur.min() >= 0 and cur.max() <= 255 and ref.min() >= 0 and ref.max() <= 255
    return cur.astype(np.uint8), ref.astype(np.uint8)


def block_candidates(cur, ref, bx, by):
    """Every candidate of block (bx, by): arrays over (dxi, di) of validity, SAD and the quantised
    bound LBq = sum over the 16 cells of |q_cur - q_ref| (q = 4x4 sum >> 4)."""
    x, y = bx * 16, by * 16
    pad = np.zeros((H + 32, W + 32), np.int64)
    pad[16:16 + H, 16:16 + W] = ref
    win = pad[y:y + 48, x:x + 48]                                    # rows di, columns dxi
    blk = cur[y:y + 16, x:x + 16].astype(np.int64)
    v = sliding_window_view(win, (16, 16))                           # [di, dxi, 16, 16]
    sad = np.abs(v - blk).sum(axis=(2, 3)).T                         # [dxi, di]
    qc = blk.reshape(4, 4, 4, 4).sum(axis=(1, 3)) >> 4
    qr = v.reshape(33, 33, 4, 4, 4, 4).sum(axis=(3, 5)) >> 4
    lbq = np.abs(qr - qc).sum(axis=(2, 3)).T
    ok = np.array([[valid(x, y, dxi - 16, di - 16) for di in range(33)] for dxi in range(33)])
    return ok, sad, lbq


def block_slack(cur, bx, by):
    s = cur[by * 16:by * 16 + 16, bx * 16:bx * 16 + 16].astype(np.int64).reshape(4, 4, 4, 4).sum(axis=(1, 3))
    return int(np.maximum(s & 15, 15 - (s & 15)).sum())


def texture(seed):
    """Cells of 8 x 8 at seeded levels plus pixel noise: sharp SAD minima at the true shift."""
    rng = np.random.default_rng(seed)
    lv = np.repeat(np.repeat(rng.integers(30, 226, size=(H // 8, W // 8)), 8, axis=0), 8, axis=1)
    return np.clip(lv + rng.integers(-12, 13, size=(H, W)), 0, 255).astype(np.uint8)


CORNER_SHIFTS = ((16, 16), (-16, 16), (16, -16), (-16, -16))


def corner_frames(seed=7):
    """[ref0, f1, f2, f3, f4]: each frame is the one before rolled by (dy, dx) = CORNER_SHIFTS[k],
    so interior blocks find their match at a corner of the +-16 window."""
    out = [texture(seed)]
    for dy, dx in CORNER_SHIFTS:
        out.append(np.roll(out[-1], (dy, dx), axis=(0, 1)))
    return out


def noise_frames(seed=11, n=4):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(H, W)).astype(np.uint8) for _ in range(n)]
