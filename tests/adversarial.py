"""Test helper: residual blocks built to sit on the rounding edges of the transform and the
quantiser, frames that deliver them to a frame kernel unchanged, and a plain high-precision
reference of the levels (scipy.fftpack in FP64, the arithmetic of Encoder.py:779-816).

With a flat reference plane every motion candidate predicts the same value, so each block's
residual is exactly cur - flat: the frame kernels transform the blocks chosen here.  No fixture
files: everything comes from a seeded np.random.default_rng.

Also here: the FP64 evaluation of fwd_mfma's certificate (so_me.hip), a careless float32
transform (what the certificate guards against) and an emulation of the k-ordered chain of
single-rounding FP32 FMAs that the certificate's error bound assumes.
"""
import numpy as np
from scipy.fftpack import dct

RANGES = {128: (-128, 127), 0: (0, 255), 255: (-255, 0)}   # flat level -> residual range
KBOUND = 2.512e-7          # the proven |z - Z| / sum|R| of the FP32 chain (so_me.hip, fwd_mfma)
KFWD = 2.6e-7              # kFwdBound, the certificate's own factor
DELTA0 = 2.0 ** -20


def dct_matrix(n=16):
    """C[u][r] of the orthonormal n-point DCT-II (scipy.fftpack.dct norm='ortho')."""
    r = np.arange(n)
    c = np.sqrt(2.0 / n) * np.cos(np.pi * (2 * r[None, :] + 1) * r[:, None] / (2 * n))
    c[0] = np.sqrt(1.0 / n)
    return c


def q_exp(n, qp):
    """log2 of the reference's Q matrix: qp above the anti-diagonal, qp + 1 on it, qp + 2 below."""
    s = np.add.outer(np.arange(n), np.arange(n))
    return qp + (s >= n - 1) + (s > n - 1)


def exact_coeffs(R):
    """FP64 2-D DCT of [..., N, N] residuals, as the reference calls scipy.fftpack."""
    R = np.asarray(R, dtype=np.float64)
    return dct(dct(R, axis=-2, norm="ortho"), axis=-1, norm="ortho")


def ref_levels(R, qp):
    """The plain high-precision reference: np.round(TC / Q) of TC = np.round(dct(dct(R)))."""
    n = np.asarray(R).shape[-1]
    tc = np.round(exact_coeffs(R))
    return np.round(tc / (2.0 ** q_exp(n, qp))).astype(np.int64)


def step_distance(R, qp):
    """Per coefficient, the distance of the exact value to the nearest place where its level
    can change: mid +- 1/2 with mid the centre of the coefficient's quantisation cell (qp >= 1)."""
    n = np.asarray(R).shape[-1]
    z = exact_coeffs(R)
    q = 2.0 ** q_exp(n, qp)
    mid = (np.floor(z / q) + 0.5) * q
    return np.abs(np.abs(z - mid) - 0.5)


def cert_delta(R):
    return KFWD * np.abs(np.asarray(R, dtype=np.float64)).sum(axis=(-2, -1)) + DELTA0


def cert_flag(R, qp):
    """fwd_mfma's certificate predicate in FP64, per block: True = the block takes the FP64
    forward (some coefficient within delta of a step; every block at QP 0)."""
    R = np.asarray(R)
    if qp < 1:
        return np.ones(R.shape[:-2], dtype=bool)
    return (step_distance(R, qp) <= cert_delta(R)[..., None, None]).any(axis=(-2, -1))


def dct_matrix_f32(n=16):
    return dct_matrix(n).astype(np.float32)


def fp32_naive_levels(R, qp):
    """Levels of a float32 matrix-product DCT with no certificate (a careless fast path)."""
    R = np.asarray(R)
    n = R.shape[-1]
    c = dct_matrix_f32(n)
    z = np.matmul(np.matmul(c, R.astype(np.float32)), c.T)
    assert z.dtype == np.float32
    q = (2.0 ** q_exp(n, qp)).astype(np.float32)
    return np.rint(np.rint(z) / q).astype(np.int64)


def _fma32(a, b, c):
    """fl32(a * b + c) with one rounding, elementwise on float32 arrays: the product is exact
    in FP64, the sum is rounded to odd in FP64 (TwoSum gives the error's sign), and rounding
    that to FP32 equals rounding the exact value (53 >= 24 + 2)."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even & np.isfinite(s)
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def fp32_chain(R):
    """Y = R C^T then Z = C Y, each output a k-ordered chain of single-rounding FP32 FMAs
    from 0, with the FP32 cosine table -- the arithmetic the certificate's bound assumes of
    v_mfma_f32_16x16x4_f32.  Returns float32 [..., N, N]."""
    R = np.asarray(R)
    n = R.shape[-1]
    c = dct_matrix_f32(n)
    r = R.astype(np.float32)
    y = np.zeros(R.shape, np.float32)
    for k in range(n):                    # Y[r][v] += R[r][k] * C[v][k]
        y = _fma32(r[..., :, k, None], c[None, :, k], y)
    z = np.zeros(R.shape, np.float32)
    for k in range(n):                    # Z[u][v] += C[u][k] * Y[k][v]
        z = _fma32(c[:, k, None], y[..., k, None, :], z)
    return z


def chain_ratio(R):
    """max |fp32_chain - FP64| / (2.512e-7 sum|R|) per block (0 for an all-zero block)."""
    R = np.asarray(R)
    err = np.abs(fp32_chain(R).astype(np.float64) - exact_coeffs(R)).max(axis=(-2, -1))
    l1 = np.abs(R.astype(np.float64)).sum(axis=(-2, -1))
    return np.where(l1 > 0, err / np.maximum(KBOUND * l1, 1e-300), 0.0)


# ------------------------------------------------------------------------------ block families
def dc_tie(n, N=16, rng=None, rg=(-128, 127), qp=None):
    """Random blocks whose sum is N/2 (mod N): the DC coefficient sum / N lands on x.5.  With
    `qp` (>= 2) the sum is N mid +- N/2 for a cell centre mid of that QP, so the x.5 is a
    quantisation step itself: rint's tie decides the level."""
    rng = rng or np.random.default_rng(1)
    lo, hi = rg
    out = rng.integers(lo, hi + 1, size=(n, N, N))
    # half of them low amplitude: a small L1 sum, so a small certificate delta
    small = rng.random(n) < 0.5 if qp is None else np.ones(n, bool)
    mid = (lo + hi) // 2
    out[small] = np.clip(mid + rng.integers(-6, 7, size=(int(small.sum()), N, N)), lo, hi)
    for b in out:
        if qp is None:
            _force_sum(b, N // 2, N, rng, lo, hi)
        else:
            cell = 2 ** (qp - 1) * (2 * int(rng.integers(0, 2)) + 1) * int(rng.choice([-1, 1]))
            _set_sum(b, N * cell + int(rng.choice([-1, 1])) * (N // 2), rng, lo, hi)
    return out


def _set_sum(b, want, rng, lo, hi):
    """Single-pixel steps (in place) until b.sum() == want."""
    d = want - int(b.sum())
    while d:
        i = tuple(rng.integers(0, s) for s in b.shape)
        if lo <= b[i] + np.sign(d) <= hi:
            b[i] += np.sign(d)
            d -= np.sign(d)


def _force_sum(b, want, mod, rng, lo, hi):
    """Change pixels of b (in place, any shape view) by single steps until b.sum() = want (mod)."""
    d = (want - int(b.sum())) % mod
    while d:
        i = tuple(rng.integers(0, s) for s in b.shape)
        if b[i] < hi:
            b[i] += 1
            d -= 1


def dc_tie_quadrants(n, rng=None, rg=(-128, 127)):
    """16 x 16 blocks whose four 8 x 8 quadrants each sum to 4 (mod 8): every VBS sub-block's
    DC lands on x.5 (and so does the whole block's, sum = 16 mod 32, only when halved again)."""
    rng = rng or np.random.default_rng(2)
    lo, hi = rg
    out = rng.integers(lo, hi + 1, size=(n, 16, 16))
    small = rng.random(n) < 0.5
    mid = (lo + hi) // 2
    out[small] = np.clip(mid + rng.integers(-6, 7, size=(int(small.sum()), 16, 16)), lo, hi)
    for b in out:
        for qy in (0, 8):
            for qx in (0, 8):
                _force_sum(b[qy:qy + 8, qx:qx + 8], 4, 8, rng, lo, hi)
    return out


def lattice(n, N=16, rng=None, rg=(-128, 127)):
    """a + b s(x) + c s(y) + d s(x) s(y) with s = sign(C[N/2]), about 5 % of the pixels perturbed:
    coefficients (0,0), (0,N/2), (N/2,0), (N/2,N/2) are N-ths of integer sums (exactly on steps)."""
    rng = rng or np.random.default_rng(3)
    lo, hi = rg
    s = np.sign(dct_matrix(N)[N // 2]).astype(np.int64)
    amp = max(1, (hi - lo) // 8)
    out = np.empty((n, N, N), np.int64)
    for i in range(n):
        a = (lo + hi) // 2 + rng.integers(-amp, amp + 1)
        b, c, d = rng.integers(-amp, amp + 1, size=3)
        blk = a + b * s[None, :] + c * s[:, None] + d * np.outer(s, s)
        pert = rng.random((N, N)) < 0.05
        blk = blk + pert * rng.integers(-3, 4, size=(N, N))
        out[i] = np.clip(blk, lo, hi)
    return out


TUNED_UV = [(0, 1), (1, 0), (1, 1), (0, 2), (2, 0), (1, 2), (2, 1), (0, 3), (3, 0)]


def tuned(n, qp, rng=None, tries=40):
    """Blocks with one low-frequency coefficient closer than 1e-3 to a quantisation step
    mid +- 1/2 of `qp` but farther than the block's certificate delta, and no coefficient within
    delta: near the edge and not flagged.  A scaled basis function plus sparse noise puts the
    coefficient near the step; one exhaustive search over all pairs of single-pixel +-1 changes
    (sums of two entries of C[u] (x) C[v]: ~1e-6 apart) then places it.  Range [-128, 127]."""
    assert qp >= 1
    rng = rng or np.random.default_rng(100 + qp)
    C = dct_matrix(16)
    out = []
    while len(out) < n:
        u, v = TUNED_UV[rng.integers(len(TUNED_UV))]
        basis = np.outer(C[u], C[v])
        step = (2.0 ** (qp - 1)) * (2 * rng.integers(0, 2) + 1) + rng.choice([-0.5, 0.5])
        step *= rng.choice([-1.0, 1.0])
        if abs(step) * np.abs(basis).max() > 100:
            continue
        blk = np.rint(step * basis).astype(np.int64)
        blk += (rng.random((16, 16)) < 0.08) * rng.integers(-1, 2, size=(16, 16))
        side = rng.choice([-1.0, 1.0])
        d1 = np.concatenate([basis.ravel(), -basis.ravel()])       # pixel p: +1, pixel p: -1
        pair = d1[:, None] + d1[None, :]
        pair[np.arange(512), np.arange(512)] = np.inf              # one pixel twice
        pair[np.arange(512), (np.arange(512) + 256) % 512] = np.inf   # +1 and -1 of one pixel
        for _ in range(tries):
            delta = KFWD * (np.abs(blk).sum() + 2) + DELTA0
            if delta > 6e-4:
                break
            want = step + side * 0.5 * (delta + 1e-3)
            gap = want - exact_coeffs(blk)[u, v]
            if abs(gap) > 0.2:                                     # greedy: one of the larger entries
                order = np.argsort(-d1 * np.sign(gap))[:24]
                t = order[rng.integers(len(order))]
                blk.ravel()[t % 256] += 1 if t < 256 else -1
                continue
            i, j = np.unravel_index(np.argmin(np.abs(pair - gap)), pair.shape)
            cand = blk.copy().ravel()
            for t in (i, j):
                cand[t % 256] += 1 if t < 256 else -1
            cand = cand.reshape(16, 16)
            dist = step_distance(cand, qp)
            dl = cert_delta(cand)
            if cand.min() >= -128 and cand.max() <= 127 and dist[u, v] < 1e-3 and (dist > dl).all():
                out.append(cand)
                break
            # another coefficient landed inside delta: perturb and retry
            p = tuple(rng.integers(0, 16, size=2))
            blk[p] += rng.choice([-1, 1])
    return np.stack(out)


def extremes(N=16, rg=(-128, 127)):
    """Full-range checkerboards, stripes and ramps; constants -5..5 (shifted into the range);
    saturated constants; single impulses (8 gives DC = 0.5 at N = 16); the sign-aligned worst
    cases +-max sign(C[u] (x) C[v])."""
    lo, hi = rg
    C = dct_matrix(N)
    x = np.arange(N)
    chk = (np.add.outer(x, x) & 1).astype(np.int64)
    col = np.broadcast_to(x & 1, (N, N)).astype(np.int64)
    out = []
    for pat in (chk, col, col.T):
        out.append(lo + (hi - lo) * pat)
        out.append(hi - (hi - lo) * pat)
    ramp = lo + (np.add.outer(x, x) * (hi - lo)) // (2 * N - 2)
    out += [ramp, ramp[::-1, ::-1].copy(), np.broadcast_to(lo + x * (hi - lo) // (N - 1), (N, N)).copy()]
    zero = min(max(0, lo), hi)                                     # the in-range value nearest 0
    sgn = 1 if lo >= 0 else (-1 if hi <= 0 else 0)
    for c in range(-5, 6):
        out.append(np.full((N, N), c if sgn == 0 else sgn * abs(c), np.int64))
    out += [np.full((N, N), lo, np.int64), np.full((N, N), hi, np.int64)]
    big = hi if hi > 0 else lo
    for k, val in enumerate([1, 7, 8, 9, 24, big, lo if lo < 0 else hi]):
        val = val if sgn >= 0 else -abs(val)
        b = np.full((N, N), zero, np.int64)
        b[(5 * k + 3) % N, (7 * k + 1) % N] = np.clip(val, lo, hi)
        out.append(b)
    for (u, v) in [(0, 0), (1, 1), (N - 1, N - 1), (1, 0), (0, N - 1), (N // 2, N // 2), (3, 5), (N - 1, 1)]:
        s = np.sign(np.outer(C[u], C[v]))
        s[s == 0] = 1
        pos = np.where(s > 0, hi, lo).astype(np.int64)
        out += [pos, np.where(s > 0, lo, hi).astype(np.int64)]
    return np.stack(out)


def zero_heavy_frame_blocks(adv, rng, nbx=16, nby=7):
    """One frame's blocks for the zero-skip kernel: in every row of eight blocks the first
    four are small constants (0, +-1, +-2: all-zero levels once Q exceeds their DC) and two of the
    other four come from `adv`, so a tile holds waves that quantise to nothing and waves that
    do not."""
    out, k = [], 0
    for b in range(nbx * nby):
        bxl = (b % nbx) % 8
        if bxl in (5, 6):
            out.append(adv[k % len(adv)])
            k += 1
        else:
            out.append(np.full((16, 16), rng.choice([0, 0, 0, 0, 1, -1, 2, -2]), np.int64))
    return np.stack(out)


# ------------------------------------------------------------------------------------- frames
def frame_from_blocks(blocks, H, W, bs=16, flat=128):
    """(cur, ref): the uint8 plane flat + R with block b at raster position b (missing blocks
    are zero residuals) and the flat reference plane."""
    lo, hi = RANGES[flat]
    blocks = np.asarray(blocks)
    nbx, nby = W // bs, H // bs
    assert len(blocks) <= nbx * nby and blocks.shape[1:] == (bs, bs)
    assert blocks.min() >= lo and blocks.max() <= hi, (blocks.min(), blocks.max(), flat)
    R = np.zeros((nby * nbx, bs, bs), np.int64)
    R[: len(blocks)] = blocks
    cur = flat + R.reshape(nby, nbx, bs, bs).transpose(0, 2, 1, 3).reshape(H, W)
    assert cur.min() >= 0 and cur.max() <= 255
    return cur.astype(np.uint8), np.full((H, W), flat, np.uint8)


def frame_residuals(cur, flat, bs=16):
    """[nb, bs, bs] residuals of a frame from frame_from_blocks, in block raster order."""
    H, W = cur.shape
    r = cur.astype(np.int64) - flat
    return r.reshape(H // bs, bs, W // bs, bs).transpose(0, 2, 1, 3).reshape(-1, bs, bs)


def expected_levels(R, nbx, qp, qp_row=None, qp_map=None):
    """ref_levels per block of a frame ([nb, bs*bs]) under a uniform, per-row or per-block QP."""
    nb, bs = R.shape[0], R.shape[-1]
    out = np.empty((nb, bs * bs), np.int64)
    for b in range(nb):
        q = qp_map[b] if qp_map is not None else (qp_row[b // nbx] if qp_row is not None else qp)
        out[b] = ref_levels(R[b], int(q)).reshape(-1)
    return out


RUN_W, RUN_H = 256, 112       # 16 x 7 blocks: tall tile rows 3 + 3 + 1, short ones 2 + 2 + 2 + 1
ROW_QPS = [0, 11, 1, 7, 4, 5, 12]
_CACHE = {}


def run_blocks(flat=128):
    """The block set of the GPU tests, [frames, 112, 16, 16]: the families shuffled together so
    that every 128 x 32 and 128 x 48 tile mixes them (flat 128: five such frames and a sixth for
    the zero-skip kernel; flat 0 / 255: two frames of the families that fit the range)."""
    if flat in _CACHE:
        return _CACHE[flat]
    rng = np.random.default_rng(20260 + flat)
    rg = RANGES[flat]
    per = (RUN_W // 16) * (RUN_H // 16)
    fams = [dc_tie(70 if flat != 128 else 200, 16, rng, rg), lattice(40 if flat != 128 else 72, 16, rng, rg),
            dc_tie_quadrants(60 if flat != 128 else 64, rng, rg), extremes(16, rg)]
    if flat == 128:
        fams += [tuned(16, qp, rng) for qp in range(1, 8)]
        fams += [dc_tie(8, 16, rng, rg, qp) for qp in range(2, 8)]
    blocks = np.concatenate(fams)
    nfr = 5 if flat == 128 else 2
    need = nfr * per
    if len(blocks) < need:
        blocks = np.concatenate([blocks, dc_tie(need - len(blocks), 16, rng, rg)])
    assert len(blocks) == need, (len(blocks), need)
    blocks = blocks[rng.permutation(need)].reshape(nfr, per, 16, 16)
    if flat == 128:
        adv = np.concatenate([fams[0][:12], fams[1][:6], fams[4][:4], fams[8][:4], fams[10][:4]])
        blocks = np.concatenate([blocks, zero_heavy_frame_blocks(adv, rng)[None]])
    _CACHE[flat] = blocks
    return blocks


def run_frames(flat=128):
    """[(cur, ref)] for run_blocks(flat)."""
    return [frame_from_blocks(b, RUN_H, RUN_W, 16, flat) for b in run_blocks(flat)]


def bs8_blocks():
    """64 blocks of 8 x 8 residuals (range of flat 128): DC ties, lattice, extremes."""
    if "bs8" not in _CACHE:
        rng = np.random.default_rng(808)
        ext = extremes(8)
        b = np.concatenate([dc_tie(64 - 8 - 20, 8, rng), lattice(8, 8, rng), ext[rng.permutation(len(ext))[:20]]])
        _CACHE["bs8"] = b[rng.permutation(64)]
    return _CACHE["bs8"]


def small_frames():
    """name -> (cur, ref, bs) of the frames besides the 256 x 112 run frames: 144 x 64 (W % 128
    != 0: per-frame kernels only), 64 x 64 at bs 8, and the one-block-wide intra frames (every
    block at x == 0, predicted from 128, so its residual is cur - 128)."""
    blocks = run_blocks(128)
    return {
        "p144x64": frame_from_blocks(blocks[2][:36], 64, 144) + (16,),
        "p64x64_bs8": frame_from_blocks(bs8_blocks(), 64, 64, 8) + (8,),
        "i16x384": frame_from_blocks(blocks[1][40:64], 384, 16) + (16,),
        "i8x256": frame_from_blocks(bs8_blocks()[:32], 256, 8, 8) + (8,),
    }


def row_schedule(nby, reverse=False):
    """ROW_QPS (or its reverse) repeated over nby block rows."""
    base = ROW_QPS[::-1] if reverse else ROW_QPS
    return [base[i % len(base)] for i in range(nby)]


BS8_ROWS = [0, 10, 1, 7, 4, 5, 9, 2]      # the row schedule of the 64 x 64 bs-8 frame


def roi_offsets(nb=112):
    """A per-block ROI offset map covering -4..+4 (two-pass run; clamped to qp_lo..qp_hi after
    the row QP and the token term are added)."""
    rng = np.random.default_rng(44)
    roi = rng.integers(-4, 5, size=nb)
    roi[:9] = np.arange(-4, 5)
    return roi.astype(np.int32)
