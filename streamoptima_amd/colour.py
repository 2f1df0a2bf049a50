"""Colour conversion between 8-bit RGB and the codec's padded 4:2:0 planes (so_rgb_to_yuv420,
so_yuv420_to_rgb: include/streamoptima.h "Colour conversion", so_colour.hip).

`Colour` names the arithmetic (matrix and range); the helpers turn tensors -- whole pictures or
cropped views of larger ones -- into the device pointers and pitches the C entry points take.
Nothing here touches pixels on the host.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import torch

from . import _lib


@dataclass(frozen=True)
class Colour:
    """matrix: "bt601" (Kr 0.299, Kb 0.114) or "bt709" (Kr 0.2126, Kb 0.0722).
    full_range: True = Y and C in 0..255; False = Y in 16..235, C in 16..240."""
    matrix: str = "bt601"
    full_range: bool = True

    def __post_init__(self):
        if self.matrix not in _lib.COLOUR_MATRICES:
            raise ValueError(f"colour matrix {self.matrix!r} (one of {sorted(_lib.COLOUR_MATRICES)})")
        if not isinstance(self.full_range, (bool, int)) or self.full_range not in (0, 1):
            raise ValueError(f"full_range {self.full_range!r} (True or False)")
        object.__setattr__(self, "full_range", bool(self.full_range))

    @property
    def matrix_code(self) -> int:
        return _lib.COLOUR_MATRICES[self.matrix]


def _on(t: torch.Tensor, device) -> bool:
    d = torch.device(device)
    return t.device.type == d.type and (d.index is None or t.device.index is None or t.device.index == d.index)


def as_colour(colour) -> Colour:
    """None -> the default (BT.601, full range); anything but a Colour raises."""
    if colour is None:
        return Colour()
    if not isinstance(colour, Colour):
        raise ValueError(f"colour must be a streamoptima_amd.colour.Colour, got {type(colour).__name__}")
    return colour


def layout_code(layout: str) -> int:
    if layout not in _lib.COLOUR_LAYOUTS:
        raise ValueError(f"RGB layout {layout!r} (\"hwc\": [F, H, W, 3], or \"chw\": [F, 3, H, W])")
    return _lib.COLOUR_LAYOUTS[layout]


def rgb_shape(nframes: int, h: int, w: int, layout: str) -> tuple:
    return (nframes, h, w, 3) if layout_code(layout) == 0 else (nframes, 3, h, w)


def rgb_pointers(rgb: torch.Tensor, layout: str, device, what: str = "rgb"):
    """A uint8 RGB tensor or view on `device` -> (pointer array, F, h, w, row pitch, plane stride).
    hwc: [F, h, w, 3] with the three channels of a pixel adjacent and the pixels of a row adjacent;
    chw: [F, 3, h, w] with the pixels of a row adjacent.  Rows, planes and frames may be any
    distance apart (a crop of a larger picture is such a view); a 3-D tensor is one frame."""
    code = layout_code(layout)
    if not isinstance(rgb, torch.Tensor) or rgb.dtype != torch.uint8 or rgb.dim() not in (3, 4):
        raise ValueError(f"{what} must be a uint8 tensor {list(rgb_shape('F', 'h', 'w', layout))}")
    if not _on(rgb, device):
        raise ValueError(f"{what} is on {rgb.device}, the engine on {device}")
    t = rgb if rgb.dim() == 4 else rgb[None]
    if code == 0:
        n, h, w, c = t.shape
        ok = c == 3 and t.stride(3) == 1 and (t.stride(2) == 3 or w == 1) and (t.stride(1) >= 3 * w or h == 1)
        pitch, plane = (t.stride(1) if h > 1 else 3 * w), 0
    else:
        n, c, h, w = t.shape
        ok = c == 3 and (t.stride(3) == 1 or w == 1) and (t.stride(2) >= w or h == 1) and t.stride(1) > 0
        pitch, plane = (t.stride(2) if h > 1 else w), t.stride(1)
    if not ok or (n > 1 and t.stride(0) < 0):
        raise ValueError(f"{what}: a {layout} picture needs shape {list(rgb_shape('F', 'h', 'w', layout))} with "
                         f"contiguous pixels in a row (shape {list(rgb.shape)}, strides {list(rgb.stride())})")
    base, step = t.data_ptr(), t.stride(0) if n > 1 else 0
    ptrs = (ctypes.c_void_p * max(n, 1))(*[base + i * step for i in range(n)])
    return ptrs, n, h, w, int(pitch), int(plane)


def plane_pointers(planes, n: int, shape: tuple, device, what: str):
    """`planes`: a tensor [n, *shape] or a sequence of n tensors of `shape`, uint8 on `device`, each
    dense -> pointer array."""
    ps = list(planes)
    if len(ps) != n:
        raise ValueError(f"{what}: {len(ps)} planes for {n} frames")
    for p in ps:
        if (not isinstance(p, torch.Tensor) or p.dtype != torch.uint8 or tuple(p.shape) != tuple(shape)
                or not p.is_contiguous() or not _on(p, device)):
            raise ValueError(f"{what} must be dense uint8 {list(shape)} planes on {device}")
    return (ctypes.c_void_p * max(n, 1))(*[p.data_ptr() for p in ps])
