"""The SSIM checker of the tests: skimage.metrics.structural_similarity(a, b, win_size=win) on two
uint8 frames, restated from its published algorithm (Wang et al. 2004 with a uniform window:
data_range 255, K1 0.01, K2 0.03, sample covariance, the border of (win - 1) // 2 cropped before
the mean).  skimage is not a dependency of this project, so no skimage-generated fixture exists;
`ssim_exact` is an independent formulation (exact integer window sums from integral images) that
tests/test_ssim.py holds `ssimref` against."""
import numpy as np
from scipy.ndimage import uniform_filter

K1, K2, L = 0.01, 0.03, 255
C1, C2 = (K1 * L) ** 2, (K2 * L) ** 2


def ssimref(a, b, win=11):
    """Float-filter formulation: means by uniform_filter, cov_norm = NP / (NP - 1), crop, mean."""
    x, y = np.asarray(a).astype(np.float64), np.asarray(b).astype(np.float64)
    if x.shape != y.shape or x.ndim != 2 or min(x.shape) < win or win % 2 == 0:
        raise ValueError(f"ssimref: frames {x.shape} / {y.shape}, win {win}")
    npix = win * win
    cov_norm = npix / (npix - 1)
    ux, uy = uniform_filter(x, size=win), uniform_filter(y, size=win)
    uxx, uyy, uxy = uniform_filter(x * x, size=win), uniform_filter(y * y, size=win), uniform_filter(x * y, size=win)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    s = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    pad = (win - 1) // 2
    return float(s[pad:s.shape[0] - pad, pad:s.shape[1] - pad].mean(dtype=np.float64))


def _box(v, win):
    """Exact int64 sums of v over every win x win window that lies inside it."""
    c = np.zeros((v.shape[0] + 1, v.shape[1] + 1), np.int64)
    c[1:, 1:] = v.cumsum(0).cumsum(1)
    return c[win:, win:] - c[:-win, win:] - c[win:, :-win] + c[:-win, :-win]


def ssim_exact(a, b, win=11):
    """Exact-integer formulation: S from the int64 window sums, numerators formed in integers."""
    x, y = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    npix = win * win
    sx, sy, sxx, syy, sxy = _box(x, win), _box(y, win), _box(x * x, win), _box(y * y, win), _box(x * y, win)
    ux, uy = sx / npix, sy / npix
    d = npix * (npix - 1)
    vx, vy, vxy = (npix * sxx - sx * sx) / d, (npix * syy - sy * sy) / d, (npix * sxy - sx * sy) / d
    s = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return float(s.mean(dtype=np.float64))


def contents(kind, h, w, seed=0):
    """A pair of uint8 frames of one of the test contents."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "noise":          # independent noise: local S goes negative
        return a, rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "near":           # a near copy (+-3), clipped
        return a, np.clip(a.astype(np.int64) + rng.integers(-3, 4, (h, w)), 0, 255).astype(np.uint8)
    if kind == "wrap":           # a mod-256 wrapped copy (the codec's astype(uint8) reconstruction)
        return a, (a.astype(np.int64) + rng.integers(-3, 4, (h, w))).astype(np.uint8)
    if kind == "same":
        return a, a.copy()
    if kind == "extreme":
        return np.full((h, w), 255, np.uint8), np.zeros((h, w), np.uint8)
    raise ValueError(kind)


KINDS = ("noise", "near", "wrap", "same", "extreme")
