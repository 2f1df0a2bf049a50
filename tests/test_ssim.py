"""Device SSIM, the parts that need no GPU: the host-side validation of so_ssim_u8, the checker
checked against an independent formulation, and the codec's opt-in keyword."""
import ctypes

import numpy as np
import pytest

import ssimref


def test_ssim_validation_without_gpu():
    from streamoptima_amd import _lib, build
    build.build()
    lib = _lib.load()
    n = 2
    a = (ctypes.c_void_p * n)(0x10000, 0x20000)
    b = (ctypes.c_void_p * n)(0x30000, 0x40000)
    out, ws = ctypes.c_void_p(0x50000), ctypes.c_void_p(0x60000)

    def call(pa=a, pb=b, nf=n, h=64, w=96, pitch_a=96, pitch_b=96, win=11, o=out, s=ws):
        return lib.so_ssim_u8(pa, pb, nf, h, w, pitch_a, pitch_b, win, o, s, None)
    for win in (10, 1, 2, 17, 16, -11):
        assert call(win=win) == _lib.SO_E_INVALID, win
        assert b"win" in lib.so_last_error()
    assert call(h=10) == _lib.SO_E_INVALID
    assert b"window" in lib.so_last_error()
    assert call(w=10) == _lib.SO_E_INVALID
    assert call(pitch_a=95) == _lib.SO_E_INVALID
    assert b"pitch" in lib.so_last_error()
    assert call(pitch_b=95) == _lib.SO_E_INVALID
    assert call(pa=None) == _lib.SO_E_INVALID
    assert call(pb=None) == _lib.SO_E_INVALID
    assert call(o=None) == _lib.SO_E_INVALID
    assert b"NULL" in lib.so_last_error()
    assert call(s=None) == _lib.SO_E_INVALID
    assert call(pa=(ctypes.c_void_p * n)(0x10000, None)) == _lib.SO_E_INVALID
    assert call(nf=0, pa=None, pb=None, o=None, s=None) == _lib.SO_OK
    with pytest.raises(ValueError):
        _lib.check(call(win=4), "so_ssim_u8")
    assert lib.so_ssim_workspace_elems(1, 11, 11, 11) == 1
    assert lib.so_ssim_workspace_elems(3, 64, 96, 11) > 0
    assert lib.so_ssim_workspace_elems(30, 2160, 3840, 11) % 30 == 0
    assert lib.so_ssim_workspace_elems(1, 10, 96, 11) == 0
    assert lib.so_ssim_workspace_elems(1, 64, 96, 8) == 0


@pytest.mark.parametrize("h,w,win", [(11, 11, 11), (23, 37, 11), (40, 19, 7), (9, 64, 3), (70, 130, 11), (33, 31, 15)])
def test_ssimref_agrees_with_the_exact_integer_formulation(h, w, win):
    for k, kind in enumerate(ssimref.KINDS):
        a, b = ssimref.contents(kind, h, w, seed=100 * h + w + k)
        assert abs(ssimref.ssimref(a, b, win) - ssimref.ssim_exact(a, b, win)) <= 1e-12, kind


def test_ssimref_known_values():
    a, b = ssimref.contents("same", 20, 30, seed=1)
    assert ssimref.ssim_exact(a, b) == 1.0
    assert ssimref.ssimref(a, b) == pytest.approx(1.0, abs=1e-12)
    a, b = ssimref.contents("extreme", 20, 30)
    assert ssimref.ssimref(a, b) == pytest.approx(ssimref.C1 / (65025 + ssimref.C1), abs=1e-12)
    a, b = ssimref.contents("noise", 64, 64, seed=3)
    assert abs(ssimref.ssimref(a, b)) < 0.05          # independent noise: no structure in common
    with pytest.raises(ValueError):
        ssimref.ssimref(np.zeros((10, 40), np.uint8), np.zeros((10, 40), np.uint8))


def test_codec_ssim_keyword():
    from streamoptima_amd.Encoder import Y_Video_codec
    frames = np.zeros((2, 64, 128), np.uint8)
    c = Y_Video_codec(64, 128, 2, 16, 16, 4, 2, 0, 0.015, False, y_only_frame_arr=frames, device="cuda:0")
    assert c.ssim is False and c.ssim_per_frame is None
    c = Y_Video_codec(64, 128, 2, 16, 16, 4, 2, 0, 0.015, False, y_only_frame_arr=frames, device="cuda:0", ssim=True)
    assert c.ssim is True and c.ssim_per_frame is None
