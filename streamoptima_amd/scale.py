"""Resampling 4:2:0 pictures (so_scale_yuv420: include/streamoptima.h "Scaling", so_scale.hip).

`taps` builds the integer tap table of one axis on the host (numpy); `ScalePlan` holds the four
tables of a (source size, destination size, filter) on the device, built once and reused.  The
arithmetic that consumes them is exact integers; tests/scaleref.py restates it in numpy.
"""
from __future__ import annotations

import ctypes

import numpy as np

ONE = 16384          # a tap row sums to this (14 fractional bits)
MAX_TAPS = 32        # the bound of the build (so_scale.hip kScaleMaxTaps)
FILTERS = {"bilinear": 1, "bicubic": 2, "lanczos3": 3}   # name -> support of the unstretched kernel


def _kernel(name: str, x: np.ndarray) -> np.ndarray:
    ax = np.abs(x)
    if name == "bilinear":
        return np.maximum(0.0, 1.0 - ax)
    if name == "bicubic":   # Catmull-Rom, a = -0.5
        return np.where(ax <= 1.0, (1.5 * ax - 2.5) * ax * ax + 1.0,
                        np.where(ax < 2.0, ((-0.5 * ax + 2.5) * ax - 4.0) * ax + 2.0, 0.0))
    return np.where(ax < 3.0, np.sinc(x) * np.sinc(x / 3.0), 0.0)


def check_filter(name) -> str:
    if name not in FILTERS:
        raise ValueError(f"scale filter {name!r} (one of {sorted(FILTERS)})")
    return name


def taps(n_src: int, n_dst: int, filter: str = "lanczos3"):
    """The tap table that resamples n_src samples to n_dst: (coef int16 [n_dst, T], first int32
    [n_dst]).  Output sample j is sum_t coef[j, t] * src[clamp(first[j] + t, 0, n_src - 1)] / 16384.
    Its centre in source coordinates is (j + 0.5) n_src / n_dst - 0.5; when shrinking, the kernel
    is stretched by n_src / n_dst.  Every row sums to exactly 16384 (the tap of largest weight
    carries the rounding), sum |coef| <= 32768, and T <= 32 or the ratio is refused."""
    a = FILTERS[check_filter(filter)]
    n_src, n_dst = int(n_src), int(n_dst)
    if n_src <= 0 or n_dst <= 0:
        raise ValueError(f"taps: {n_src} -> {n_dst} samples (both positive)")
    s = max(1.0, n_src / n_dst)
    support = a * s
    c = (np.arange(n_dst, dtype=np.float64) + 0.5) * n_src / n_dst - 0.5
    lo = np.floor(c - support).astype(np.int64) + 1
    k = int(np.ceil(2 * support)) + 1
    pos = lo[:, None] + np.arange(k, dtype=np.int64)[None, :]
    d = pos - c[:, None]
    w = np.where(np.abs(d) < support, _kernel(filter, d / s), 0.0)   # strictly inside the support
    w = w / w.sum(axis=1, keepdims=True) * ONE
    q = np.rint(w).astype(np.int64)
    rows = np.arange(n_dst)
    q[rows, np.argmax(w, axis=1)] += ONE - q.sum(axis=1)             # argmax: the first on a tie
    nz = q != 0
    lead = np.argmax(nz, axis=1)
    last = k - 1 - np.argmax(nz[:, ::-1], axis=1)
    t = int((last - lead + 1).max())
    if t > MAX_TAPS:
        raise ValueError(f"taps: {filter} at {n_src} -> {n_dst} (ratio {n_src / n_dst:.3g}:1) needs {t} taps; "
                         f"the build holds {MAX_TAPS}")
    idx = lead[:, None] + np.arange(t)[None, :]
    coef = np.where(idx <= last[:, None], np.take_along_axis(q, np.minimum(idx, k - 1), axis=1), 0)
    first = (lo + lead).astype(np.int32)
    assert (coef.sum(axis=1) == ONE).all(), "tap rows must sum to 16384"
    assert (np.abs(coef).sum(axis=1) <= 2 * ONE).all(), "tap rows must keep sum |coef| <= 32768"
    assert 1 <= t <= MAX_TAPS
    return np.ascontiguousarray(coef.astype(np.int16)), np.ascontiguousarray(first)


def check_size(hw, what: str, chroma: bool) -> tuple:
    try:
        h, w = (int(v) for v in hw)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be (height, width), got {hw!r}") from None
    if h <= 0 or w <= 0:
        raise ValueError(f"{what} {h}x{w}: sizes are positive")
    if chroma and (h % 2 or w % 2):
        raise ValueError(f"{what} {h}x{w}: a 4:2:0 picture is even both ways")
    return h, w


class ScalePlan:
    """The tables that take src_hw = (hs, ws) pictures to dst_hw = (hd, wd): luma horizontal and
    vertical and, with chroma, the same for the half-size planes.  Built on the host and uploaded
    once; Engine.scale_yuv420 and the streams reuse it for every launch."""

    def __init__(self, src_hw, dst_hw, filter: str = "lanczos3", chroma: bool = True, device="cuda"):
        import torch
        self.chroma = bool(chroma)
        self.src_hw, self.dst_hw, host = self.check(src_hw, dst_hw, filter, self.chroma)   # refusals before any upload
        self.filter = filter
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"ScalePlan: the tables live on the GPU, not on {self.device}")
        self.tables = [(torch.from_numpy(c).to(self.device), torch.from_numpy(f).to(self.device), c.shape[1])
                       for c, f in host]

    @staticmethod
    def check(src_hw, dst_hw, filter: str = "lanczos3", chroma: bool = True):
        """What the constructor refuses, on the host alone: ValueError for an unknown filter, sizes that
        are not positive (or with chroma odd) and a ratio beyond the tap bound.  Returns the checked
        sizes and the host tables (luma h, luma v and with chroma the half-size planes' h, v)."""
        check_filter(filter)
        hs, ws = check_size(src_hw, "ScalePlan src_hw", chroma)
        hd, wd = check_size(dst_hw, "ScalePlan dst_hw", chroma)
        axes = [(ws, wd), (hs, hd)] + ([(ws // 2, wd // 2), (hs // 2, hd // 2)] if chroma else [])
        return (hs, ws), (hd, wd), [taps(ns, nd, filter) for ns, nd in axes]

    def table_args(self) -> list:
        """The (coef, first, taps) arguments of so_scale_yuv420, luma h, luma v, chroma h, chroma v."""
        out = []
        for c, f, t in self.tables:
            out += [c.data_ptr(), f.data_ptr(), t]
        if not self.chroma:
            out += [None, None, 0] * 2
        return out


def plane_views(planes, n: int | None, hw: tuple, device, what: str):
    """uint8 planes on `device`, as an [n, H, W] tensor or a sequence of [H, W] tensors or views
    whose rows are contiguous, each holding at least hw = (h, w) samples from its top-left corner
    -> (pointer array, n, row pitch).  All views share one pitch."""
    import torch
    from .colour import _on
    ps = list(planes)
    if n is not None and len(ps) != n:
        raise ValueError(f"{what}: {len(ps)} planes for {n} frames")
    h, w = hw
    pitch = None
    for p in ps:
        if (not isinstance(p, torch.Tensor) or p.dtype != torch.uint8 or p.dim() != 2 or not _on(p, device)
                or p.shape[0] < h or p.shape[1] < w or (p.stride(1) != 1 and p.shape[1] > 1)
                or (p.shape[0] > 1 and p.stride(0) < p.shape[1])):
            raise ValueError(f"{what} must be uint8 planes of at least {h}x{w} with contiguous rows on {device}")
        pp = p.stride(0) if p.shape[0] > 1 else max(p.shape[1], 1)
        if pitch is None:
            pitch = pp
        elif pp != pitch:
            raise ValueError(f"{what}: the planes of one call share a row pitch ({pitch} and {pp})")
    return (ctypes.c_void_p * max(len(ps), 1))(*[p.data_ptr() for p in ps]), len(ps), int(pitch or w)
