"""Offline analysis (test infrastructure: uses the C oracle).  Survivors of the plain run's
exact SEA bound per block of a whole 4K P-frame F of the bench GOP (reference = the oracle's
reconstruction chain, U = min(SAD of the smallest-bound candidate, SAD at the co-located block's
vector in frame F-1): sea2_tile's U), under two slacks of the quantised bound:
  240    16 LBq - 240 <= U: 15 per 4x4 cell, whatever the current block;
  K_b    16 LBq - K_b <= U, K_b = sum over the block's 16 cells of max(r, 15 - r), r = the
         cell sum's remainder mod 16 (128 <= K_b <= 240): the loss of the quantisation is at
         most r where the reference's quotient is larger and 15 - r where it is smaller.
Prints, per slack: survivors per block, the share of blocks with 1, <= 4, 5..16 and > 16
survivors, the 16-candidate passes per block and the share past the cap of 384; then K_b's own
distribution.
Usage: python tests/analysis/sea_slack.py [F] [H]"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from numpy.lib.stride_tricks import sliding_window_view  # noqa: E402

from oracle import oracle as O  # noqa: E402
from streamoptima_amd.synth import synth_sequence  # noqa: E402

F = int(sys.argv[1]) if len(sys.argv) > 1 else 4
h = int(sys.argv[2]) if len(sys.argv) > 2 else 2160
w = 3840
CAP = 384
seq = synth_sequence(F + 1, h, w, seed=0)
rec = O.intra_frame(seq[0], 16, 16, 4)["recon"]
prev = None
for f in range(1, F):
    r = O.inter_frame(seq[f], [rec], 16, 16, 4)
    rec, prev = r["recon"], r
cur = seq[F].astype(np.int32)
ref = rec.astype(np.int32)
nby, nbx = h // 16, w // 16
c = np.zeros((h + 1, w + 1), np.int64)
c[1:, 1:] = ref.cumsum(0).cumsum(1)
B4 = ((c[4:, 4:] - c[:-4, 4:] - c[4:, :-4] + c[:-4, :-4]) >> 4).astype(np.int32)   # [h-3, w-3]
S = cur.reshape(nby, 4, 4, nbx, 4, 4).sum(axis=(2, 5))                             # [nby, 4, nbx, 4]
A = (S >> 4).astype(np.int32)
R = S & 15
KB = np.maximum(R, 15 - R).sum(axis=(1, 3))                                        # [nby, nbx]
ys, xs = np.arange(nby) * 16, np.arange(nbx) * 16
win = sliding_window_view(ref, (16, 16))


def sad_at(dx, dy):   # [nby, nbx] SAD at per-block offsets (clipped into the frame)
    yy = np.clip(ys[:, None] + dy, 0, h - 16)
    xx = np.clip(xs[None, :] + dx, 0, w - 16)
    blk = cur.reshape(nby, 16, nbx, 16).transpose(0, 2, 1, 3)
    return np.abs(blk - win[yy, xx]).sum(axis=(2, 3))


lb = np.full((33, 33, nby, nbx), 1 << 30, np.int64)
for dxi in range(33):
    dx = dxi - 16
    vx = (xs + dx >= 0) & (xs + dx < w - 16)
    for di in range(33):
        dy = di - 16
        vy = (ys + dy >= 0) & (ys + dy < h - 16)
        yy = np.clip(ys + dy, 0, h - 16)
        xx = np.clip(xs + dx, 0, w - 16)
        Bs = B4[yy[:, None, None, None] + 4 * np.arange(4)[None, :, None, None],
                xx[None, None, :, None] + 4 * np.arange(4)[None, None, None, :]]   # [nby, 4, nbx, 4]
        v = np.abs(A - Bs).sum(axis=(1, 3))
        lb[dxi, di] = np.where(vy[:, None] & vx[None, :], v, 1 << 30)
flat = lb.reshape(33 * 33, nby, nbx)
k = flat.argmin(axis=0)                       # dx-major scan index, the kernel's tie order
U = sad_at(k // 33 - 16, k % 33 - 16)
if prev is not None:
    mvp = prev["mv"][:, 0, :].reshape(nby, nbx, 3)
    pdx, pdy = mvp[..., 0].astype(int), mvp[..., 1].astype(int)
    pv = ((xs[None, :] + pdx >= 0) & (xs[None, :] + pdx < w - 16) &
          (ys[:, None] + pdy >= 0) & (ys[:, None] + pdy < h - 16))
    U = np.where(pv, np.minimum(U, sad_at(pdx, pdy)), U)
print(f"F={F} {h}x{w}: K_b mean {KB.mean():.1f} min {KB.min()} p10 {np.percentile(KB, 10):.0f} "
      f"median {np.median(KB):.0f} p90 {np.percentile(KB, 90):.0f} max {KB.max()}")
res = {}
for name, slack in (("240", np.full_like(KB, 240)), ("K_b", KB)):
    n = (flat <= ((U + slack) >> 4)[None]).sum(axis=0)
    res[name] = n
    passes = np.where(n > 4, -(-n // 16), 0)
    print(f"slack {name:4s} survivors/block {n.mean():7.2f} median {np.median(n):5.0f} p90 {np.percentile(n, 90):6.0f}"
          f"  n==1 {np.mean(n == 1):.4f}  n<=4 {np.mean(n <= 4):.4f}  5..16 {np.mean((n > 4) & (n <= 16)):.4f}"
          f"  >16 {np.mean(n > 16):.4f}  le4 runs/block {np.mean((n > 1) & (n <= 4)):.4f}"
          f"  passes/block {np.where(n <= CAP, passes, 0).mean():.4f}  >cap {np.mean(n > CAP):.5f}")
print(f"survivors/block ratio K_b / 240: {res['K_b'].mean() / res['240'].mean():.4f}")
