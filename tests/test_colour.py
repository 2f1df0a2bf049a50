"""Colour conversion without a GPU: the integer model (colourref.py) against the float64 formulas,
its range, the exhaustive round trip, the tables the headers state, and what the C entry points and
the Python facade refuse."""
import ctypes
import os
import re

import numpy as np
import pytest

import colourref
from conftest import ROOT

TABLES = [(m, fr) for m in ("bt601", "bt709") for fr in (True, False)]
IDS = [f"{m}_{'full' if fr else 'limited'}" for m, fr in TABLES]


def _real_forward(rgb, matrix, full_range):
    """rint of the float64 formulas: Y per pixel, C from the mean of each 2 x 2 cell."""
    m = colourref.float_forward(matrix, full_range)
    p = rgb.astype(np.float64)
    y = p @ m[0] + colourref.yoff(full_range)
    mean = (p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2]) / 4.0
    return y, mean @ m[1] + 128.0, mean @ m[2] + 128.0


@pytest.mark.parametrize("matrix,full_range", TABLES, ids=IDS)
def test_model_is_within_one_of_the_real_formulas(matrix, full_range):
    """The coefficient error is below 0.01 and there is one rounding: |integer - rint(real)| <= 1."""
    rgb = colourref.sample_frames(2, 64, 96, seed=11)
    y, uv = colourref.rgb_to_yuv420(rgb, matrix, full_range, 64, 96)
    ry, ru, rv = _real_forward(rgb, matrix, full_range)
    worst = 0.0
    for got, real in ((y, ry), (uv[:, 0], ru), (uv[:, 1], rv)):
        worst = max(worst, float(np.abs(got.astype(np.float64) - real).max()))
        assert np.abs(got.astype(np.int64) - np.rint(real).astype(np.int64)).max() <= 1
    print(matrix, full_range, "worst |integer - real|", worst)
    # the inverse tables are the closed form of the matrix inverse
    assert np.allclose(np.linalg.inv(colourref.float_forward(matrix, full_range)),
                       colourref.float_inverse(matrix, full_range), rtol=0, atol=1e-12)


@pytest.mark.parametrize("matrix,full_range", TABLES, ids=IDS)
def test_primaries_and_random_input_stay_in_range(matrix, full_range):
    """Before the clip the values leave 0..255 by at most one step (pure red and blue reach 256 at
    full range); after it they lie in 0..255, and inside the nominal limited range where it is set."""
    f = colourref.forward_table(matrix, full_range).astype(np.int64)
    rng = np.random.default_rng(5)
    cols = np.concatenate([colourref.PRIMARIES, rng.integers(0, 256, (4096, 3), dtype=np.uint8)]).astype(np.int64)
    y_raw = (cols @ f[0] + (colourref.yoff(full_range) << 16) + 32768) >> 16
    c_raw = [((4 * cols) @ f[k] + (128 << 18) + (1 << 17)) >> 18 for k in (1, 2)]
    assert y_raw.min() >= 0 and y_raw.max() <= 255
    assert min(c.min() for c in c_raw) >= 0 and max(c.max() for c in c_raw) <= 256
    if full_range:
        assert max(c[:8].max() for c in c_raw) == 256          # the clip is needed
    pic = np.repeat(np.repeat(cols.astype(np.uint8).reshape(1, 8, -1, 3), 2, axis=1), 2, axis=2)
    y, uv = colourref.rgb_to_yuv420(pic, matrix, full_range, pic.shape[1], pic.shape[2])
    assert y.dtype == np.uint8 and uv.dtype == np.uint8
    assert np.array_equal(y[0, ::2, ::2].ravel(), np.clip(y_raw, 0, 255))
    assert np.array_equal(uv[0, 0].ravel(), np.clip(c_raw[0], 0, 255))
    assert np.array_equal(uv[0, 1].ravel(), np.clip(c_raw[1], 0, 255))
    if not full_range:
        assert y.min() >= 16 and y.max() <= 235 and uv.min() >= 16 and uv.max() <= 240
    back = colourref.yuv420_to_rgb(y, uv, pic.shape[1], pic.shape[2], matrix, full_range)
    assert back.dtype == np.uint8 and back.shape == pic.shape


@pytest.mark.parametrize("matrix,full_range", TABLES, ids=IDS)
def test_round_trip_over_all_colours(matrix, full_range):
    """Every one of the 2^24 colours as a 2 x 2 cell, forward and back: each channel within 1 at full
    range and within 2 at limited range."""
    bound = 1 if full_range else 2
    g, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    worst = 0
    for r0 in range(0, 256, 16):
        cells = np.empty((16, 256, 256, 3), np.uint8)
        cells[..., 0] = np.arange(r0, r0 + 16, dtype=np.uint8)[:, None, None]
        cells[..., 1], cells[..., 2] = g, b
        pic = np.repeat(np.repeat(cells, 2, axis=1), 2, axis=2)
        y, uv = colourref.rgb_to_yuv420(pic, matrix, full_range, 512, 512)
        back = colourref.yuv420_to_rgb(y, uv, 512, 512, matrix, full_range)
        worst = max(worst, int(np.abs(back.astype(np.int16) - pic.astype(np.int16)).max()))
    print(matrix, full_range, "worst round-trip error", worst)
    assert worst <= bound


def _ints(text):
    return [int(v) for v in re.findall(r"-?\d+", text)]


def test_header_tables_equal_the_rule():
    """The integers in include/streamoptima.h's comment and in so_colour.h are what the rule gives."""
    hdr = open(os.path.join(ROOT, "include", "streamoptima.h")).read()
    rows = re.findall(r"\* +(601|709) (full|limited) +((?:\[[-\d, ]+\] ?){3})", hdr)
    assert len(rows) == 8, rows
    seen = {}
    for std, rng, body in rows:
        seen.setdefault((f"bt{std}", rng == "full"), []).append(np.array(_ints(body)).reshape(3, 3))
    src = open(os.path.join(ROOT, "streamoptima_amd", "csrc", "so_colour.h")).read()
    arrays = {name: np.array(_ints(re.sub(r"//.*", "", body))).reshape(4, 3, 3)
              for name, body in re.findall(r"(kColourFwd|kColourInv)\[4\]\[9\] = \{(.*?)\};", src, re.S)}
    for i, (matrix, full_range) in enumerate(TABLES):
        fwd, inv = colourref.forward_table(matrix, full_range), colourref.inverse_table(matrix, full_range)
        assert int(fwd[0].sum()) == int(np.rint((1.0 if full_range else 219.0 / 255.0) * 65536.0))
        assert fwd[1].sum() == 0 and fwd[2].sum() == 0
        assert np.array_equal(seen[(matrix, full_range)][0], fwd) and np.array_equal(seen[(matrix, full_range)][1], inv)
        assert np.array_equal(arrays["kColourFwd"][i], fwd) and np.array_equal(arrays["kColourInv"][i], inv)
    assert colourref.forward_table("bt601", True).tolist() == [[19595, 38470, 7471], [-11058, -21710, 32768],
                                                                 [32768, -27439, -5329]]
    assert colourref.forward_table("bt709", False).tolist() == [[11966, 40254, 4064], [-6596, -22188, 28784],
                                                                  [28784, -26145, -2639]]


# ---- the C entry points, no GPU: every refusal comes before a launch -------------------------------
H, W, HP, WP = 18, 22, 32, 32


def _arr(*ps):
    return (ctypes.c_void_p * len(ps))(*ps)


def _fwd(lib, **kw):
    a = dict(rgb=_arr(0x100000), n=1, h=H, w=W, layout=0, pitch=3 * W, plane=0, matrix=0, full=1, hp=HP, wp=WP,
             y=_arr(0x200000), u=_arr(0x300000), v=_arr(0x400000))
    a.update(kw)
    return lib.so_rgb_to_yuv420(a["rgb"], a["n"], a["h"], a["w"], a["layout"], a["pitch"], a["plane"], a["matrix"],
                                a["full"], a["hp"], a["wp"], a["y"], a["u"], a["v"], None)


def _inv(lib, **kw):
    a = dict(rgb=_arr(0x100000), n=1, h=H, w=W, layout=0, pitch=3 * W, plane=0, matrix=0, full=1, hp=HP, wp=WP,
             y=_arr(0x200000), u=_arr(0x300000), v=_arr(0x400000))
    a.update(kw)
    return lib.so_yuv420_to_rgb(a["y"], a["u"], a["v"], a["n"], a["hp"], a["wp"], a["h"], a["w"], a["matrix"],
                                a["full"], a["layout"], a["rgb"], a["pitch"], a["plane"], None)


BAD = [
    (dict(h=17), b"h 17"), (dict(w=21), b"w 21"), (dict(h=0), b"h 0"), (dict(w=-2), b"w -2"),
    (dict(hp=16), b"Hp 16"), (dict(wp=20), b"Wp 20"), (dict(hp=33), b"Hp 33"), (dict(wp=33), b"Wp 33"),
    (dict(pitch=3 * W - 1), b"pitch"), (dict(layout=1, pitch=W - 1, plane=H * W), b"pitch"),
    (dict(layout=1, pitch=W, plane=0), b"plane_stride"),
    (dict(matrix=2), b"matrix 2"), (dict(matrix=-1), b"matrix -1"), (dict(full=2), b"full_range 2"),
    (dict(layout=2), b"layout 2"), (dict(n=-1), b"nframes -1"),
    (dict(rgb=None), b"rgb is NULL"), (dict(y=None), b"y is NULL"), (dict(u=None), b"u is NULL"),
    (dict(v=None), b"v is NULL"), (dict(rgb=_arr(None)), b"rgb[0] is NULL"), (dict(y=_arr(None)), b"y[0] is NULL"),
    (dict(u=_arr(None)), b"u[0] is NULL"), (dict(v=_arr(None)), b"v[0] is NULL"),
    # aliasing: a destination against a destination, and against the source
    (dict(u=_arr(0x200000 + HP * WP - 1)), b"aliases"), (dict(v=_arr(0x300000)), b"aliases"),
    (dict(rgb=_arr(0x200000 + 5)), b"aliases"), (dict(rgb=_arr(0x400000 - 3 * W)), b"aliases"),
]


@pytest.mark.parametrize("call", [_fwd, _inv], ids=["so_rgb_to_yuv420", "so_yuv420_to_rgb"])
def test_entry_points_refuse_bad_arguments_without_gpu(call):
    from streamoptima_amd import _lib, build
    build.build()
    lib = _lib.load()
    for kw, text in BAD:
        if call is _inv and kw.keys() & {"u", "v"} and text == b"aliases":
            continue          # two SOURCE planes may share bytes
        assert call(lib, **kw) == _lib.SO_E_INVALID, kw
        msg = lib.so_last_error()
        assert text in msg and (b"so_rgb_to_yuv420" if call is _fwd else b"so_yuv420_to_rgb") in msg, (kw, msg)
    # nothing to do is not an error, with valid scalars only
    assert call(lib, n=0, rgb=None, y=None, u=None, v=None) == _lib.SO_OK
    assert call(lib, n=0, h=17) == _lib.SO_E_INVALID
    with pytest.raises(ValueError):
        _lib.check(call(lib, matrix=7), "colour")


def test_batches_are_checked_across_frames_without_gpu():
    from streamoptima_amd import _lib, build
    build.build()
    lib = _lib.load()
    ny = HP * WP
    two = dict(n=2, rgb=_arr(0x100000, 0x110000), u=_arr(0x300000, 0x310000), v=_arr(0x400000, 0x410000))
    # forward: frame 1's Y plane starts inside frame 0's
    assert _fwd(lib, y=_arr(0x200000, 0x200000 + ny - 2), **two) == _lib.SO_E_INVALID
    assert b"y[1] aliases y[0]" in lib.so_last_error()
    assert _fwd(lib, n=2, rgb=_arr(0x100000, 0x100000), y=_arr(0x200000, None), u=two["u"], v=two["v"]) == _lib.SO_E_INVALID
    assert b"y[1] is NULL" in lib.so_last_error()
    # inverse: two destination pictures one byte short of lying side by side in one canvas (side by
    # side they interleave row by row and share nothing: test_gpu_colour.py converts into such a pair)
    canvas = 3 * 2 * W
    side = dict(n=2, pitch=canvas, y=_arr(0x200000, 0x210000), u=two["u"], v=two["v"])
    assert _inv(lib, rgb=_arr(0x100000, 0x100000 + 3 * W - 1), **side) == _lib.SO_E_INVALID
    assert b"rgb[0] aliases rgb[1]" in lib.so_last_error()
    # ... and a destination picture laid over a source plane of another frame
    assert _inv(lib, rgb=_arr(0x100000, 0x210000 + 7), **side) == _lib.SO_E_INVALID
    assert b"aliases" in lib.so_last_error()


# ---- the Python facade ------------------------------------------------------------------------------
def _codec(**kw):
    from streamoptima_amd.Encoder import Y_Video_codec
    args = dict(h_pixels=32, w_pixels=48, frames=2, block_size=16, search_range=16, Qp=4, intra_dur=8, intra_mode=0,
                device="cpu")
    args.update(kw)
    return Y_Video_codec(**args)


def test_colour_value():
    from streamoptima_amd.colour import Colour, as_colour, layout_code
    assert Colour() == Colour("bt601", True) and as_colour(None) == Colour()
    assert Colour("bt709", False).matrix_code == 1 and Colour("bt709", 0).full_range is False
    for bad in (dict(matrix="bt2020"), dict(matrix=None), dict(full_range=2), dict(full_range="yes")):
        with pytest.raises(ValueError):
            Colour(**bad)
    with pytest.raises(ValueError):
        as_colour("bt601")
    assert layout_code("hwc") == 0 and layout_code("chw") == 1
    with pytest.raises(ValueError):
        layout_code("nhwc")


def test_facade_refuses_what_is_not_built():
    from streamoptima_amd.colour import Colour
    from streamoptima_amd.hostdecode import HostStreamDecoder
    from streamoptima_amd.hoststream import HostStreamEncoder
    rgb = np.zeros((2, 32, 48, 3), np.uint8)
    c = _codec(chroma=True, rgb_frame_arr=rgb, colour=Colour("bt709", False))
    assert c.rgb_f_arr is rgb and c.colour == Colour("bt709", False)
    off = _codec(y_only_frame_arr=np.zeros((2, 32, 48), np.uint8))
    assert off.rgb_f_arr is None and off.colour == Colour()
    with pytest.raises(ValueError):
        _codec(rgb_frame_arr=rgb)                                              # luma-only codec
    with pytest.raises(ValueError):
        _codec(chroma=True, rgb_frame_arr=rgb[:, :, :, :2])
    with pytest.raises(ValueError):
        _codec(chroma=True, rgb_frame_arr=rgb.astype(np.float32))
    with pytest.raises(ValueError):
        _codec(chroma=True, rgb_frame_arr=np.zeros((2, 3, 32, 48), np.uint8))  # chw is not this argument's layout
    with pytest.raises(ValueError):
        _codec(chroma=True, rgb_frame_arr=rgb, y_only_frame_arr=np.zeros((2, 32, 48), np.uint8))
    with pytest.raises(ValueError):
        _codec(chroma=True, rgb_frame_arr=rgb, colour="bt709")
    with pytest.raises(ValueError):
        off.encode_device_rgb(None, 8)
    with pytest.raises(ValueError):
        off.save_rgb("unused.rgb")
    with pytest.raises(ValueError):
        c.save_rgb("unused.rgb")                                               # nothing encoded yet
    # the refusals that stand: chroma with FME, block_size 8, intra_mode 1 -- with RGB too
    with pytest.raises(NotImplementedError):
        _codec(chroma=True, rgb_frame_arr=rgb, FMEEnable=True)
    with pytest.raises(NotImplementedError):
        _codec(chroma=True, rgb_frame_arr=rgb, block_size=8)
    with pytest.raises(NotImplementedError):
        _codec(chroma=True, rgb_frame_arr=rgb, intra_mode=1)
    # the streams: refused before a buffer is allocated
    with pytest.raises(ValueError):
        HostStreamEncoder(off, 2, input="rgb")
    with pytest.raises(ValueError):
        HostStreamEncoder(c, 2, input="bgr")
    with pytest.raises(ValueError):
        HostStreamDecoder(c.decoder, output="bgr")
    with pytest.raises(ValueError):
        HostStreamDecoder(c.decoder, output="rgb", colour="bt601")
