"""The deblocking post-filter's numpy model (deblockref.py, written from include/streamoptima.h
"Deblocking"): where it must leave a plane alone, a hand-computed line for every branch, that the
designed corpus of the GPU tests reaches every branch, and the quality claim through the CPU oracle."""
import numpy as np
import pytest

import deblockref as R


def _corpus(seed=3, h=80, w=112, extremes=True):
    rng = np.random.default_rng(seed)
    y = R.corpus_plane(h, w, rng, extremes=extremes)
    nb = (h // 16) * (w // 16)
    split = rng.integers(0, 2, nb).astype(np.uint8)
    qp_map = rng.choice([2, 4, 6, 8], nb).astype(np.int32)
    return y, split, qp_map


# ---- where nothing may change -----------------------------------------------------------------
@pytest.mark.parametrize("qp, strength", [(0, 0), (1, 0), (2, -1), (4, -3), (0, 1)])
def test_identity_below_q2(qp, strength):
    y, split, _ = _corpus()
    out, _, _ = R.deblock_yuv420(y, bs=16, split=split, qp=qp, strength=strength)
    assert np.array_equal(out, y)
    out8, _, _ = R.deblock_yuv420(y, bs=8, qp=qp, strength=strength)
    assert np.array_equal(out8, y)


def test_a_single_unsplit_block_has_no_edge():
    y = R.corpus_plane(16, 16, np.random.default_rng(0))
    out, _, _ = R.deblock_yuv420(y, bs=16, split=np.zeros(1, np.uint8), qp=8)
    assert np.array_equal(out, y)
    split, _, _ = R.deblock_yuv420(y, bs=16, split=np.ones(1, np.uint8), qp=8)
    assert not np.array_equal(split, y)
    # ... and its split edges are the lines x = 8 and y = 8 alone
    changed = np.argwhere(split != y)
    assert all(6 <= r <= 9 or 6 <= c <= 9 for r, c in changed)


def test_samples_further_than_two_from_every_edge_stay():
    y, split, qp_map = _corpus()
    out, _, _ = R.deblock_yuv420(y, bs=16, split=np.ones_like(split), qp_map=qp_map, strength=3)
    assert not np.array_equal(out, y)
    yy, xx = np.indices(y.shape)
    far = ((yy % 8 >= 2) & (yy % 8 <= 5)) & ((xx % 8 >= 2) & (xx % 8 <= 5))   # every multiple of 8 is at most an edge
    assert np.array_equal(out[far], y[far])
    # unsplit: only the multiples of 16 are edges
    out, _, _ = R.deblock_yuv420(y, bs=16, split=None, qp_map=qp_map, strength=3)
    far = ((yy % 16 >= 2) & (yy % 16 <= 13)) & ((xx % 16 >= 2) & (xx % 16 <= 13))
    assert np.array_equal(out[far], y[far])
    # the plane's border is no edge
    flat = np.full((8, 24), 100, np.uint8)
    flat[:, :8] = 90
    o8, _, _ = R.deblock_yuv420(flat, bs=8, qp=6)
    assert np.array_equal(o8[:, 10:], flat[:, 10:]) and not np.array_equal(o8[:, 6:10], flat[:, 6:10])


def test_output_is_uint8_everywhere():
    rng = np.random.default_rng(5)
    y = rng.choice(np.array([0, 1, 3, 252, 254, 255], np.uint8), size=(48, 80))
    for strength in (-3, 0, 3):
        out, _, _ = R.deblock_yuv420(y, bs=16, split=np.ones(15, np.uint8), qp=20, strength=strength)
        assert out.dtype == np.uint8       # deblock_plane asserts 0..255 before the cast


# ---- one hand-computed line per branch ----------------------------------------------------------
def test_thresholds():
    assert [int(v) for v in R.thresholds(4)] == [16, 6, 4, 2]
    assert [int(v) for v in R.thresholds(1)] == [2, 0, 0, 0]
    assert [int(v) for v in R.thresholds(2)] == [4, 1, 1, 0]
    assert [int(v) for v in R.thresholds(20)] == [255, 255, 255, 127]
    assert [int(v) for v in R.thresholds(9)] == [255, 192, 128, 64]


def test_hand_computed_lines():
    # q = 4: alpha 16, beta 6, tc 4, tc1 2
    # off by alpha: |d| = 16
    assert R.filter_line(100, 100, 100, 116, 116, 116, 4) == (100, 100, 116, 116)
    # off by beta on the p side: |p1 - p0| = 6
    assert R.filter_line(100, 94, 100, 104, 104, 104, 4) == (94, 100, 104, 104)
    # off by beta on the q side
    assert R.filter_line(100, 100, 100, 104, 110, 104, 4) == (100, 100, 104, 110)
    # on, ap and aq: d = 8, dl = (32 - 8 + 4) >> 3 = 3, avg = 104;
    # p1' = 100 + clip((100 + 104 - 200) >> 1 = 2) = 102, q1' = 108 + clip((108 + 104 - 216) >> 1 = -2) = 106
    assert R.filter_line(100, 100, 100, 108, 108, 108, 4) == (102, 103, 105, 106)
    # on, ap only: q2 = 120 is 12 from q0
    assert R.filter_line(100, 100, 100, 108, 108, 120, 4) == (102, 103, 105, 108)
    # on, aq only: p2 = 80
    assert R.filter_line(80, 100, 100, 108, 108, 108, 4) == (100, 103, 105, 106)
    # on, neither
    assert R.filter_line(80, 100, 100, 108, 108, 120, 4) == (100, 103, 105, 108)
    # dl clipped at +tc: d = 12, (48 - 12 + 4) >> 3 = 5 -> 4; avg = 106; p1' = 100 + clip(3) = 102, q1' = 112 - 2
    assert R.filter_line(100, 100, 100, 112, 112, 112, 4) == (102, 104, 108, 110)
    # dl clipped at -tc: d = -13, (-52 + 13 + 4) >> 3 = -5 -> -4; avg = 107
    assert R.filter_line(113, 113, 113, 100, 100, 100, 4) == (111, 109, 104, 102)
    # the floor of a negative quotient: d = -1, p1 - q1 = -4: (-4 - 4 + 4) >> 3 = -1; avg = 100;
    # p1' = 98 + clip((100 + 100 - 196) >> 1 = 2), q1' = 102 + clip((99 + 100 - 204) >> 1 = -3 -> -2)
    assert R.filter_line(100, 98, 100, 99, 102, 99, 4) == (100, 99, 100, 100)
    # p0' clipped at 255 and q0' at 0 need a large tc: q = 10, alpha 255, beta 255, tc 255, tc1 127
    # d = 55: dl = (220 + (254 - 2) + 4) >> 3 = 59; p0' = clip(200 + 59) = 255, q0' = 255 - 59
    assert R.filter_line(254, 254, 200, 255, 2, 2, 10)[1:3] == (255, 196)
    # p0 = 20, q0 = 10, p1 = 0, q1 = 250: dl = (-40 - 250 + 4) >> 3 = -36: p0' = clip(-16) = 0, q0' = 46
    assert R.filter_line(20, 0, 20, 10, 250, 10, 10)[1:3] == (0, 46)
    # q < 2: the identity whatever the samples
    assert R.filter_line(100, 100, 100, 101, 101, 101, 1) == (100, 100, 101, 101)


def test_strength_moves_a_line_across_the_threshold():
    line = (100, 100, 100, 108, 108, 108)
    assert R.filter_line(*line, 3) == (100, 100, 108, 108)          # alpha 8: off
    assert R.filter_line(*line, 3 + 1) != (100, 100, 108, 108)      # strength +1: on
    y, split, qp_map = _corpus()
    outs = [R.deblock_yuv420(y, bs=16, split=split, qp_map=qp_map, strength=s)[0] for s in (-3, 0, 3)]
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2])
    # lines on at 0 and off at -3, and lines off at 0 and on at +3
    s = [R.Stats() for _ in range(3)]
    for st, k in zip(s, (-3, 0, 3)):
        R.deblock_yuv420(y, bs=16, split=split, qp_map=qp_map, strength=k, stats=st)
    assert s[0]["on"] < s[1]["on"] < s[2]["on"]


# ---- the corpus of the GPU tests reaches every branch -------------------------------------------
def test_corpus_reaches_every_branch():
    y, split, qp_map = _corpus()
    st = R.Stats()
    R.deblock_yuv420(y, bs=16, split=split, qp_map=qp_map, stats=st)
    # large QPs for the clips of p0' / q0' at 0 and 255
    R.deblock_yuv420(y, bs=16, split=split, qp=9, stats=st)
    print(dict(st))
    for k in R.Stats.KEYS:
        assert st[k] > 0, (k, dict(st))


# ---- the quality claim, through the oracle --------------------------------------------------------
@pytest.fixture(scope="module")
def smooth():
    return R.smooth_sequence()


def _filtered(frames, qp, vbs):
    from oracle.gop import encode_gop
    out = []
    for i, r in enumerate(encode_gop(frames, qp, 4, vbs=vbs)):
        recon = r["recon"]
        f, _, _ = R.deblock_yuv420(recon, bs=16, split=r["split"] if vbs else None, qp=qp)
        out.append((R.psnr(frames[i], recon), R.psnr(frames[i], f), recon, f))
    return out


@pytest.mark.parametrize("vbs", [False, True])
@pytest.mark.parametrize("qp", [5, 7])
def test_quality_gain_on_the_smooth_sequence(smooth, qp, vbs):
    """At least 0.3 dB of luma PSNR on every frame (a scratch model measured 0.56 dB or more)."""
    res = _filtered(smooth, qp, vbs)
    gains = [b - a for a, b, _, _ in res]
    print(f"qp {qp} vbs {vbs}: before {[round(a, 2) for a, _, _, _ in res]} gain {[round(g, 2) for g in gains]}")
    assert min(gains) >= 0.3, gains


def test_identical_at_qp1(smooth):
    for vbs in (False, True):
        for _, _, recon, f in _filtered(smooth[:2], 1, vbs):
            assert np.array_equal(recon, f)
