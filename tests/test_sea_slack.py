"""The per-cell inequality behind a per-block slack of the quantised SEA bound (DESIGN.md
section 4), exhaustively over every pair of 4x4 cell sums.

With a cell sum s = 16 q + r (the current block's) and s' = 16 q' + r' (the reference's):
    |s - s'| >= 16 |q - q'| - max(r, 15 - r)
because the quantisation loses at most r where q' > q and 15 - r where q' < q.  Summed over a
block's 16 cells this is SAD >= 16 LBq - K_b with K_b = sum of max(r, 15 - r), 128 <= K_b <= 240,
where the kernels use 240 for every block."""
import numpy as np

S = np.arange(4081, dtype=np.int64)            # a 4x4 sum of bytes: 0 .. 16 * 255
s, sp = S[:, None], S[None, :]
q, qp, r = s >> 4, sp >> 4, s & 15
DIFF = np.abs(s - sp)
LOSS = np.maximum(r, 15 - r)                   # [4081, 1]
ABOVE, BELOW = qp > q, qp < q


def test_cell_inequality_holds_for_every_pair():
    assert (DIFF >= 16 * np.abs(q - qp) - LOSS).all()
    # side by side: r is the loss above, 15 - r the loss below
    assert (DIFF >= 16 * (qp - q) - r)[ABOVE].all()
    assert (DIFF >= 16 * (q - qp) - (15 - r))[BELOW].all()


def test_cell_inequality_is_tight_on_each_side():
    up = ABOVE & (DIFF == 16 * (qp - q) - r)
    dn = BELOW & (DIFF == 16 * (q - qp) - (15 - r))
    assert up[q[:, 0] < 255].any(axis=1).all()             # every s with a quotient above its own
    assert dn[q[:, 0] > 0].any(axis=1).all()               # every s with a quotient below its own
    # equality sits at the near end of the other quotient's interval
    assert (S[np.nonzero(up)[1]] & 15 == 0).all()
    assert (S[np.nonzero(dn)[1]] & 15 == 15).all()


def test_a_slack_one_smaller_fails():
    bad = DIFF < 16 * np.abs(q - qp) - (LOSS - 1)
    # for every s with a quotient on both sides some s' breaks it (q = 0 and q = 255 have one
    # side only, so there the smaller of r and 15 - r may be all that is ever lost)
    assert bad[(q[:, 0] > 0) & (q[:, 0] < 255)].any(axis=1).all()


def test_block_slack_range():
    assert int(LOSS.min()) == 8 and int(LOSS.max()) == 15  # K_b in [16 * 8, 16 * 15] = [128, 240]
    assert set(np.unique(r[LOSS == 15]).tolist()) == {0, 15}   # the kernels' flat 15: r = 0 and 15 only
