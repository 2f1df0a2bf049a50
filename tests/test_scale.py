"""Scaling without a GPU: the tap tables (streamoptima_amd.scale.taps), the numpy model of the
arithmetic (scaleref.py), so_scale_yuv420's host-side refusals and the facades' refusals."""
import ctypes
import inspect

import numpy as np
import pytest

import scaleref

FILTERS = ["bilinear", "bicubic", "lanczos3"]
PAIRS = [(50, 36), (36, 100), (96, 48), (64, 64), (2, 8), (8, 2), (160, 32), (3840, 1920), (1920, 3840)]
SUPPORT = {"bilinear": 1, "bicubic": 2, "lanczos3": 3}


def _dense(coef, first, n_src):
    """The table as an [n_dst, n_src + 2 m] matrix over source positions -m .. n_src + m (no clamping)."""
    n_dst, t = coef.shape
    m = 4 * t + 8
    d = np.zeros((n_dst, n_src + 2 * m), np.int64)
    for j in range(n_dst):
        d[j, m + first[j]:m + first[j] + t] = coef[j]
    return d


@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("pair", PAIRS, ids=[f"{a}-{b}" for a, b in PAIRS])
def test_tap_tables(pair, filt):
    from streamoptima_amd.scale import taps
    ns, nd = pair
    coef, first = taps(ns, nd, filt)
    assert coef.dtype == np.int16 and first.dtype == np.int32
    assert coef.shape[0] == nd and first.shape == (nd,)
    c = coef.astype(np.int64)
    assert (c.sum(axis=1) == 16384).all()
    assert (np.abs(c).sum(axis=1) <= 32768).all()
    t = coef.shape[1]
    assert 1 <= t <= 32
    # the tap count: the integer positions strictly inside a support of a * max(1, ns / nd) each way
    # (2 a s of them when the centres fall between samples), less what rounds to zero at the ends
    a, s = SUPPORT[filt], max(1.0, ns / nd)
    assert t <= int(np.ceil(2 * a * s)) + 1
    if ns == nd:
        assert t == 1 and (coef[:, 0] == 16384).all() and (first == np.arange(nd)).all()
    if ns == 2 * nd:
        assert t == {"bilinear": 4, "bicubic": 8, "lanczos3": 12}[filt]
    if (ns, nd) == (160, 32):
        assert t == {"bilinear": 9, "bicubic": 19, "lanczos3": 29}[filt]
    # no row is all padding at either end somewhere: T is the longest trimmed row
    assert (c[:, 0] != 0).all() and (c[:, -1] != 0).any()
    # every row holds its centre's nearest sample (what sizes the kernel's staging window)
    centre = (np.arange(nd) + 0.5) * ns / nd - 0.5
    near = np.floor(centre + 0.5).astype(np.int64)
    assert ((first <= near) & (near < first + t)).all()
    if ns % nd == 0 or nd % ns == 0:
        d = _dense(coef, first, ns)
        assert np.array_equal(d, d[::-1, ::-1])                  # output j mirrors output n - 1 - j


def test_tap_refusals():
    from streamoptima_amd.scale import ScalePlan, taps
    with pytest.raises(ValueError, match="8"):
        taps(160, 20, "lanczos3")                                # 8:1 needs 48 taps
    with pytest.raises(ValueError):
        taps(64, 64, "nearest")
    with pytest.raises(ValueError):
        taps(0, 64, "bilinear")
    assert taps(160, 20, "bicubic")[0].shape[1] == 32            # 8:1 bicubic is the bound itself
    assert taps(160, 32, "lanczos3")[0].shape[1] == 29
    for bad in (dict(src_hw=(51, 70), dst_hw=(36, 46)), dict(src_hw=(50, 70), dst_hw=(36, 45)),
                dict(src_hw=(50, 70), dst_hw=(0, 46)), dict(src_hw=(-2, 70), dst_hw=(36, 46)),
                dict(src_hw=(50, 70), dst_hw=(36, 46), filter="area"), dict(src_hw=(640, 70), dst_hw=(36, 46)),
                dict(src_hw=(50, 70), dst_hw=(36, 46), device="cpu")):
        with pytest.raises(ValueError):
            ScalePlan(**{"device": "cuda", **bad})
    ScalePlan.check((51, 71), (37, 47), "bicubic", chroma=False)  # luma alone may be odd
    with pytest.raises(ValueError):
        ScalePlan.check((51, 71), (37, 0), "bicubic", chroma=False)


# ---- the model -----------------------------------------------------------------------------------------
def _checker(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((((yy // 3) + (xx // 3)) & 1) * 255).astype(np.uint8)


@pytest.mark.parametrize("filt", FILTERS)
def test_model_properties(filt):
    rng = np.random.default_rng(3)
    noise = rng.integers(0, 256, (50, 70), dtype=np.uint8)
    for dst in ((36, 46), (100, 152), (50, 70), (10, 14)):
        for value in (0, 1, 128, 254, 255):
            out = scaleref.scale_plane(np.full((50, 70), value, np.uint8), dst, filt)
            assert out.shape == dst and (out == value).all()      # a constant stays that constant
    assert np.array_equal(scaleref.scale_plane(noise, (50, 70), filt), noise)   # identity is a copy
    for src, dst in ((noise, (36, 46)), (noise, (100, 152)), (_checker(96, 128), (48, 64)), (_checker(36, 46), (100, 152)),
                     (_checker(160, 160), (32, 32))):
        out, mid, raw = scaleref.scale_plane(src, dst, filt, detail=True)
        assert np.abs(mid).max() <= 32640                          # the int16 clamp never acts
        assert np.abs(raw).max() < 2 ** 11


def test_model_clips_at_both_ends_on_a_checker():
    out, mid, raw = scaleref.scale_plane(_checker(36, 46), (100, 152), "lanczos3", detail=True)
    assert (raw < 0).any() and (raw > 255).any()
    assert out.min() == 0 and out.max() == 255
    out, mid, raw = scaleref.scale_plane(_checker(96, 128), (48, 64), "lanczos3", detail=True)
    assert (raw < 0).any() and (raw > 255).any()


def test_model_yuv420_pads_with_128():
    rng = np.random.default_rng(4)
    y = rng.integers(0, 256, (20, 28), dtype=np.uint8)
    u, v = (rng.integers(0, 256, (10, 14), dtype=np.uint8) for _ in range(2))
    oy, ou, ov = scaleref.scale_yuv420(y, u, v, (36, 46), "bicubic", (48, 48))
    assert oy.shape == (48, 48) and ou.shape == ov.shape == (24, 24)
    assert (oy[36:] == 128).all() and (oy[:, 46:] == 128).all() and (ou[18:] == 128).all() and (ov[:, 23:] == 128).all()
    assert np.array_equal(oy[:36, :46], scaleref.scale_plane(y, (36, 46), "bicubic"))
    assert np.array_equal(ov[:18, :23], scaleref.scale_plane(v, (18, 23), "bicubic"))
    assert scaleref.scale_yuv420(y, None, None, (36, 46), "bicubic")[1:] == (None, None)


# ---- the C entry's validation, no GPU ------------------------------------------------------------------
HS, WS, HD, WD, HP, WP = 20, 28, 36, 46, 48, 48


def _arr(*ps):
    return (ctypes.c_void_p * len(ps))(*ps)


def _call(lib, **kw):
    a = dict(sy=_arr(0x100000), su=_arr(0x200000), sv=_arr(0x300000), n=1, hs=HS, ws=WS, py=WS, pc=WS // 2,
             dy=_arr(0x400000), du=_arr(0x500000), dv=_arr(0x600000), hd=HD, wd=WD, hp=HP, wp=WP)
    for i, t in enumerate(("yh", "yv", "ch", "cv")):
        a.update({f"coef_{t}": 0x700000 + 0x10000 * i, f"first_{t}": 0x708000 + 0x10000 * i, f"taps_{t}": 6})
    a.update(kw)
    tables = [a[f"{k}_{t}"] for t in ("yh", "yv", "ch", "cv") for k in ("coef", "first", "taps")]
    return lib.so_scale_yuv420(a["sy"], a["su"], a["sv"], a["n"], a["hs"], a["ws"], a["py"], a["pc"], a["dy"], a["du"],
                               a["dv"], a["hd"], a["wd"], a["hp"], a["wp"], *tables, None)


LUMA = dict(su=None, sv=None, du=None, dv=None)
BAD = [
    (dict(hs=0), b"hs 0"), (dict(ws=-4), b"ws -4"), (dict(hs=21), b"hs 21"), (dict(ws=27), b"ws 27"),
    (dict(hd=0), b"hd 0"), (dict(wd=-2), b"wd -2"), (dict(hd=35), b"hd 35"), (dict(wd=45), b"wd 45"),
    (dict(hp=34), b"Hp 34"), (dict(wp=44), b"Wp 44"), (dict(hp=49), b"Hp 49"), (dict(wp=47), b"Wp 47"),
    (dict(py=WS - 1), b"pitch_y"), (dict(pc=WS // 2 - 1), b"pitch_c"),
    (dict(taps_yh=0), b"taps_yh 0"), (dict(taps_yv=33), b"taps_yv 33"), (dict(taps_ch=-1), b"taps_ch -1"),
    (dict(taps_cv=40), b"taps_cv 40"),
    (dict(n=-1), b"nframes -1"),
    (dict(sy=None), b"sy is NULL"), (dict(dy=None), b"dy is NULL"),
    (dict(su=None), b"su is NULL"), (dict(sv=None), b"sv is NULL"), (dict(du=None), b"du is NULL"),
    (dict(dv=None), b"dv is NULL"), (dict(su=None, sv=None), b"su is NULL"),
    (dict(sy=_arr(None)), b"sy[0] is NULL"), (dict(su=_arr(None)), b"su[0] is NULL"), (dict(sv=_arr(None)), b"sv[0] is NULL"),
    (dict(dy=_arr(None)), b"dy[0] is NULL"), (dict(du=_arr(None)), b"du[0] is NULL"), (dict(dv=_arr(None)), b"dv[0] is NULL"),
    (dict(coef_yh=None), b"coef_yh is NULL"), (dict(first_yv=None), b"first_yv is NULL"),
    (dict(coef_ch=None), b"coef_ch is NULL"), (dict(first_cv=None), b"first_cv is NULL"),
    # aliasing: a destination against a destination, and against a source
    (dict(du=_arr(0x400000 + HP * WP - 1)), b"aliases"), (dict(dv=_arr(0x500000)), b"aliases"),
    (dict(dy=_arr(0x100000 + 5)), b"aliases"), (dict(sy=_arr(0x400000 + HP * WP - 1)), b"aliases"),
    (dict(dv=_arr(0x300000 - (HP // 2) * (WP // 2) + 1)), b"aliases"),
    # luma only: odd sizes are allowed, the rest still holds
    (dict(LUMA, hs=0), b"hs 0"), (dict(LUMA, hp=35), b"Hp 35"), (dict(LUMA, py=WS - 1), b"pitch_y"),
    (dict(LUMA, taps_yh=33), b"taps_yh 33"), (dict(LUMA, dy=_arr(0x100000 + 5)), b"aliases"),
]


def test_entry_point_refuses_bad_arguments_without_gpu():
    from streamoptima_amd import _lib, build
    build.build()
    lib = _lib.load()
    for kw, text in BAD:
        assert _call(lib, **kw) == _lib.SO_E_INVALID, kw
        msg = lib.so_last_error()
        assert text in msg and b"so_scale_yuv420" in msg, (kw, msg)
    # two SOURCE planes may share bytes; a source may repeat
    # nothing to do is not an error, with valid scalars only
    assert _call(lib, n=0, sy=None, su=None, sv=None, dy=None, du=None, dv=None) == _lib.SO_OK
    assert _call(lib, n=0) == _lib.SO_OK
    assert _call(lib, n=0, hs=21) == _lib.SO_E_INVALID
    assert _call(lib, n=0, **LUMA, hs=21, ws=27, hd=35, wd=45, hp=35, wp=45, coef_ch=None, first_ch=None, taps_ch=0,
                 coef_cv=None, first_cv=None, taps_cv=0) == _lib.SO_OK
    with pytest.raises(ValueError):
        _lib.check(_call(lib, taps_yh=99), "scale")
    # a ratio no tile can hold (far past anything 32 taps resample) is refused as unsupported, not launched
    assert _call(lib, n=0, **LUMA, hs=4, ws=1 << 28, py=1 << 28, hd=4, wd=64, hp=4, wp=64) == _lib.SO_E_UNSUPPORTED


def test_batches_are_checked_across_frames_without_gpu():
    from streamoptima_amd import _lib, build
    build.build()
    lib = _lib.load()
    two = dict(n=2, sy=_arr(0x100000, 0x100000), su=_arr(0x200000, 0x200000), sv=_arr(0x300000, 0x300000),
               du=_arr(0x500000, 0x510000), dv=_arr(0x600000, 0x610000))
    assert _call(lib, dy=_arr(0x400000, 0x400000 + HP * WP - 2), **two) == _lib.SO_E_INVALID
    assert b"dy[1] aliases dy[0]" in lib.so_last_error()
    assert _call(lib, dy=_arr(0x400000, None), **two) == _lib.SO_E_INVALID
    assert b"dy[1] is NULL" in lib.so_last_error()
    # frame 1's destination over frame 0's source view (rows pitch apart: the span is what counts)
    assert _call(lib, dy=_arr(0x400000, 0x100000 + 64 * (HS - 1)), py=64, **two) == _lib.SO_E_INVALID
    assert b"aliases" in lib.so_last_error()


# ---- the Python facades --------------------------------------------------------------------------------
def _codec(**kw):
    from streamoptima_amd.Encoder import Y_Video_codec
    args = dict(h_pixels=32, w_pixels=48, frames=2, block_size=16, search_range=16, Qp=4, intra_dur=8, intra_mode=0,
                device="cpu")
    args.update(kw)
    return Y_Video_codec(**args)


def test_facades_refuse_before_anything_is_allocated():
    from streamoptima_amd.decoder import decoder
    from streamoptima_amd.hostdecode import HostStreamDecoder
    from streamoptima_amd.hoststream import HostStreamEncoder
    c = _codec(chroma=True)
    luma = _codec()
    for bad in (dict(source_size=(33, 48)), dict(source_size=(32, 0)), dict(source_size=(64,)), dict(source_size=64),
                dict(source_size=(64, 96), scale="nearest"), dict(source_size=(32 * 8, 48 * 8)),
                dict(source_size=(32 * 6, 48), scale="lanczos3"), dict(source_size=(64, 96), input="bgr")):
        with pytest.raises(ValueError):
            HostStreamEncoder(c, 2, **bad)
    with pytest.raises(ValueError):
        HostStreamEncoder(luma, 2, source_size=(0, 3))
    with pytest.raises(ValueError):
        HostStreamEncoder(luma, 2, source_size=(64, 96), input="rgb")
    for bad in (dict(output_size=(33, 48)), dict(output_size=(0, 48)), dict(output_size=(64, 96), scale="nearest"),
                dict(output_size=(4, 6)), dict(output_size=96), dict(output_size=(64, 96), output="bgr")):
        with pytest.raises(ValueError):
            HostStreamDecoder(c.decoder, **bad)
    # the new arguments default to "off", on every layer that passes them on
    for fn, name in ((HostStreamEncoder.__init__, "source_size"), (HostStreamDecoder.__init__, "output_size"),
                     (decoder.decode_packed_stream, "output_size"), (decoder.decode_to_rgb, "output_size")):
        sig = inspect.signature(fn).parameters
        assert sig[name].default is None and sig["scale"].default == "lanczos3", fn
