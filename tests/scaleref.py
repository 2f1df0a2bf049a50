"""Numpy restatement of the scaling arithmetic (include/streamoptima.h "Scaling").

Only the tap tables come from the product (streamoptima_amd.scale.taps); the two passes, the
rounding, the clamps and the 128 padding are written out here.
"""
import numpy as np

from streamoptima_amd.scale import taps


def hpass(src, coef, first):
    """mid [hs, n_dst] int64 before the int16 clamp: (hsum + 128) >> 8."""
    src = np.asarray(src, dtype=np.int64)
    ws = src.shape[1]
    idx = np.clip(first.astype(np.int64)[:, None] + np.arange(coef.shape[1])[None, :], 0, ws - 1)   # [wd, T]
    hsum = (src[:, idx] * coef.astype(np.int64)[None, :, :]).sum(axis=2)
    return (hsum + 128) >> 8


def vpass(mid, coef, first):
    """out [n_dst, w] uint8 and the value before the clip."""
    hs = mid.shape[0]
    idx = np.clip(first.astype(np.int64)[:, None] + np.arange(coef.shape[1])[None, :], 0, hs - 1)   # [hd, T]
    vsum = (mid[idx, :] * coef.astype(np.int64)[:, :, None]).sum(axis=1)
    raw = (vsum + (1 << 19)) >> 20
    return np.clip(raw, 0, 255).astype(np.uint8), raw


def scale_plane(src, dst_hw, filter, detail=False):
    """One 8-bit plane [hs, ws] -> [hd, wd]: horizontal, then vertical."""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 2
    hs, ws = src.shape
    hd, wd = dst_hw
    ch, fh = taps(ws, wd, filter)
    cv, fv = taps(hs, hd, filter)
    mid_raw = hpass(src, ch, fh)
    mid = np.clip(mid_raw, -32768, 32767)
    out, raw = vpass(mid, cv, fv)
    return (out, mid_raw, raw) if detail else out


def pad128(plane, Hp, Wp):
    out = np.full((Hp, Wp), 128, np.uint8)
    out[:plane.shape[0], :plane.shape[1]] = plane
    return out


def scale_yuv420(y, u, v, dst_hw, filter, plane_hw=None):
    """4:2:0 planes y [hs, ws], u, v [hs/2, ws/2] -> (y, u, v) at dst_hw, each set into a plane of
    plane_hw = (Hp, Wp) (chroma: half) with 128 outside the picture.  u = v = None: luma only."""
    hd, wd = dst_hw
    Hp, Wp = plane_hw or dst_hw
    oy = pad128(scale_plane(y, (hd, wd), filter), Hp, Wp)
    if u is None:
        return oy, None, None
    ou = pad128(scale_plane(u, (hd // 2, wd // 2), filter), Hp // 2, Wp // 2)
    ov = pad128(scale_plane(v, (hd // 2, wd // 2), filter), Hp // 2, Wp // 2)
    return oy, ou, ov
