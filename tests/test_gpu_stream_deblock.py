"""decoder(deblock=True) through every decode path against the numpy model (deblockref.py), bit for
bit: what decode_packed_file and the stream decoder deliver with deblock=True is the model applied to
the reconstructions (the padded planes the encoder holds; the same calls with deblock=False deliver
exactly those, cropped).  That the P-frames after a filtered frame still come out as the model of
THEIR raw reconstruction shows that the references were not filtered.  A 64 x 96 picture and a
40 x 56 one (coded in 48 x 64 planes: the filter reads the padding), 5 frames with 2 I-frames,
chroma, VBS on."""
import os

import numpy as np
import pytest
import torch

import colourref
import deblockref as R
import scaleref

pytestmark = pytest.mark.gpu

F, INTRA, QP, LAM, OFF = 5, 3, 6, 0.015, 1
MATRIX, FULL = "bt709", False
CASES = {
    "64x96": dict(h=64, w=96),
    "40x56": dict(h=40, w=56),
    "fme": dict(h=64, w=96, fme=True, strength=1),
    "rc2pass": dict(h=64, w=96, rc=3),
    # rate control without maps: the row QPs of every frame reach the filter (in the stream decoder as
    # views of the unit's staging buffer)
    "rc1": dict(h=64, w=96, rc=1),
}
_MADE = {}


def _tables():
    import json

    from conftest import GOLDEN
    return json.load(open(os.path.join(GOLDEN, "rc_schedule.json")))["tables"]


def _colour():
    from streamoptima_amd.colour import Colour
    return Colour(MATRIX, FULL)


def _decoder(gpu, name, deblock, strength=None):
    from streamoptima_amd.decoder import decoder
    cfg = CASES[name]
    kw = dict(RCFlag=cfg["rc"], targetBR="200 kbps", qp_rate_tables=_tables()) if cfg.get("rc") else {}
    if deblock:
        kw.update(deblock=True, deblock_strength=cfg.get("strength", 0) if strength is None else strength)
    return decoder(0, INTRA, 16, F, cfg["h"], cfg["w"], QP, 1, bool(cfg.get("fme")), LAM, True, device=gpu,
                   chroma_subpel=bool(cfg.get("fme")), **kw)


@pytest.fixture(scope="module")
def made(gpu, tmp_path_factory):
    """name -> the encoded codec, its packed files by coding, the raw frames (cropped) and the
    model's frames (cropped), each (y, u, v) per frame; made on first use."""
    root = tmp_path_factory.mktemp("deblock_stream")

    def get(name):
        if name in _MADE:
            return _MADE[name]
        from streamoptima_amd.Encoder import Y_Video_codec
        from streamoptima_amd.synth import synth_sequence
        cfg = CASES[name]
        h, w = cfg["h"], cfg["w"]
        y = synth_sequence(F, h, w, seed=9)
        uv = np.stack([synth_sequence(F, h // 2, w // 2, seed=109), synth_sequence(F, h // 2, w // 2, seed=209)], axis=1)
        kw = dict(RCFlag=cfg["rc"], targetBR="200 kbps", qp_rate_tables=_tables()) if cfg.get("rc") else {}
        cwd = os.getcwd()
        os.chdir(root)
        try:
            enc = Y_Video_codec(h, w, F, 16, 16, QP, INTRA, 0, LAM, True, FMEEnable=bool(cfg.get("fme")),
                                y_only_frame_arr=y, device=gpu, chroma=True, chroma_qp_offset=OFF, uv_frame_arr=uv,
                                chroma_subpel=bool(cfg.get("fme")), **kw)
            enc.encode()
            paths = {}
            for coding in ("varint", "bits", "huff"):
                paths[coding] = str(root / f"{name}_{coding}.sopk")
                enc.transmit_packed420(paths[coding], coding=coding)
        finally:
            os.chdir(cwd)
        assert [s.frame_type for s in enc._symbols] == [0, 1, 1, 0, 1]
        rc = bool(cfg.get("rc"))
        raw, model = [], []
        for s, cs in zip(enc._symbols, enc.chroma_symbols):
            planes = [t.cpu().numpy() for t in (s.recon, cs.recon_u, cs.recon_v)]
            qm = s.extra.get("qp_map")
            out = R.deblock_yuv420(*planes, bs=16, split=s.split.cpu().numpy(), qp=QP,
                                   qp_row=s.qp_row if rc and s.qp_row else None,
                                   qp_map=None if qm is None else qm.cpu().numpy(), chroma_qp_offset=OFF,
                                   strength=cfg.get("strength", 0))

            def crop(p3):
                return (p3[0][:h, :w].copy(), p3[1][:h // 2, :w // 2].copy(), p3[2][:h // 2, :w // 2].copy())
            raw.append(crop(planes))
            model.append(crop(out))
        assert any(s.split.any() for s in enc._symbols), "no split block: VBS is not exercised"
        if cfg.get("rc") == 3:
            assert all("qp_map" in s.extra for s in enc._symbols), "two-pass RC left no QP map"
        if cfg.get("rc") == 1:
            rows = [list(s.qp_row) for s in enc._symbols]
            assert all(len(r) == -(-h // 16) for r in rows) and not any("qp_map" in s.extra for s in enc._symbols)
            assert any(q != QP for r in rows for q in r), "the row QPs are the decoder's Qp: the route is not exercised"
        assert all((m[0] != r[0]).any() for m, r in zip(model, raw)), "the filter left a frame alone"
        assert any((m[1] != r[1]).any() for m, r in zip(model, raw)), "the filter left all chroma alone"
        _MADE[name] = dict(enc=enc, paths=paths, raw=raw, model=model, root=root)
        return _MADE[name]
    return get


def _same(got, want, what):
    assert len(got) == len(want) == F, what
    for i, (g, w) in enumerate(zip(got, want)):
        for k, name in enumerate("yuv"):
            assert g[k].shape == w[k].shape and np.array_equal(g[k], w[k]), (what, i, name)


def _file_frames(dec, path):
    ys = [a.copy() for a in dec.decode_packed_file(path)]
    return [(y, u.copy(), v.copy()) for y, (u, v) in zip(ys, dec.decoded_chroma)]


def _stream_frames(dec, path, **kw):
    from streamoptima_amd.hostdecode import HostStreamDecoder
    got = []
    hs = HostStreamDecoder(dec, **kw)
    info = hs.decode_file(path, lambda i, y, u, v: got.append((y.copy(), u.copy(), v.copy())))
    assert info["frames"] == F
    return got


FILE_CASES = [("64x96", "varint"), ("64x96", "bits"), ("64x96", "huff"), ("40x56", "varint"), ("40x56", "huff"),
              ("fme", "varint"), ("rc2pass", "varint"), ("rc1", "varint"), ("rc1", "huff")]


@pytest.mark.parametrize("name,coding", FILE_CASES)
def test_decode_packed_file(gpu, made, tmp_path, name, coding):
    m = made(name)
    path = m["paths"][coding]
    _same(_file_frames(_decoder(gpu, name, False), path), m["raw"], "deblock off: the bytes of before")
    dec = _decoder(gpu, name, True)
    _same(_file_frames(dec, path), m["model"], "deblock on")
    out = str(tmp_path / "dec.yuv")
    dec.save_yuv420(out)
    assert open(out, "rb").read() == b"".join(p.tobytes() for f in m["model"] for p in f)
    dec.save_decoded_frames(str(tmp_path / "dec.y"))
    assert open(str(tmp_path / "dec.y"), "rb").read() == b"".join(f[0].tobytes() for f in m["model"])


STREAM_CASES = [(n, c, fused) for n, c in FILE_CASES for fused in (True, False)
                if not (c == "huff" and not fused)]      # a "huff" file takes the unfused path either way


@pytest.mark.parametrize("name,coding,fused", STREAM_CASES)
def test_stream_decoder(gpu, made, name, coding, fused):
    m = made(name)
    path = m["paths"][coding]
    _same(_stream_frames(_decoder(gpu, name, False), path, chunk=2, nbuf=2, fused=fused), m["raw"], "deblock off")
    _same(_stream_frames(_decoder(gpu, name, True), path, chunk=2, nbuf=2, fused=fused), m["model"], "deblock on")


@pytest.mark.parametrize("chunk,nbuf", [(1, 1), (3, 2)])
def test_stream_decoder_units(gpu, made, chunk, nbuf):
    m = made("40x56")
    dec = _decoder(gpu, "40x56", True)
    for _ in range(2):                               # the display planes are reused
        _same(_stream_frames(dec, m["paths"]["bits"], chunk=chunk, nbuf=nbuf), m["model"], (chunk, nbuf))


def test_facade_keyword_cache_key_and_files(gpu, made, tmp_path):
    m = made("64x96")
    path = m["paths"]["varint"]
    dec = _decoder(gpu, "64x96", False)
    got = []
    dec.decode_packed_stream(path, consume=lambda i, y, u, v: got.append((y.copy(), u.copy(), v.copy())), deblock=True)
    _same(got, m["model"], "decode_packed_stream(deblock=True)")
    again = []
    dec.decode_packed_stream(path, consume=lambda i, y, u, v: again.append((y.copy(), u.copy(), v.copy())))
    _same(again, m["raw"], "the same decoder at its defaults")
    on = _decoder(gpu, "64x96", True)
    out = str(tmp_path / "s.yuv")
    assert on.decode_packed_stream(path, out_path=out)["frames"] == F
    assert open(out, "rb").read() == b"".join(p.tobytes() for f in m["model"] for p in f)
    # another strength is another stream decoder, and other frames
    other = []
    on.decode_packed_stream(path, consume=lambda i, y, u, v: other.append(y.copy()), deblock_strength=3)
    assert any((a != f[0]).any() for a, f in zip(other, m["model"]))
    with pytest.raises(ValueError):
        _decoder(gpu, "64x96", True, strength=4)


@pytest.mark.parametrize("name", ["64x96", "40x56"])
def test_rgb_and_output_size_read_the_filtered_frames(gpu, made, tmp_path, name):
    from streamoptima_amd.hostdecode import HostStreamDecoder
    m = made(name)
    h, w = CASES[name]["h"], CASES[name]["w"]
    path = m["paths"]["varint"]
    dec = _decoder(gpu, name, True)
    rgb = [colourref.yuv420_to_rgb(y[None], np.stack([u, v])[None], h, w, MATRIX, FULL)[0] for y, u, v in m["model"]]
    got = []
    HostStreamDecoder(dec, chunk=2, output="rgb", colour=_colour()).decode_file(path, lambda i, p: got.append(p.copy()))
    assert len(got) == F and all(np.array_equal(a, b) for a, b in zip(got, rgb))
    out = (96, 144)
    planes = [scaleref.scale_yuv420(y, u, v, out, "bicubic") for y, u, v in m["model"]]
    got = []
    HostStreamDecoder(dec, chunk=2, output_size=out, scale="bicubic").decode_file(
        path, lambda i, y, u, v: got.append((y.copy(), u.copy(), v.copy())))
    _same(got, planes, "output_size")
    rgb2 = [colourref.yuv420_to_rgb(y[None], np.stack([u, v])[None], out[0], out[1], MATRIX, FULL)[0] for y, u, v in planes]
    b = str(tmp_path / "o.rgb")
    assert dec.decode_to_rgb(path, b, colour=_colour(), output_size=out, scale="bicubic")["frames"] == F
    assert open(b, "rb").read() == b"".join(p.tobytes() for p in rgb2)


def test_luma_only_file_filters_luma_alone(gpu, made, tmp_path):
    m = made("64x96")
    enc = m["enc"]
    path = str(tmp_path / "luma.sopk")
    from streamoptima_amd import packedfile
    # the luma symbols of the 4:2:0 encode on their own (chroma does not touch them)
    packedfile.write(path, enc.engine(), enc._symbols, enc.encoded_package["Qp_per_row_per_frame"], coding="varint")
    dec = _decoder(gpu, "64x96", True)
    want = [f[0] for f in m["model"]]
    assert all(np.array_equal(a, b) for a, b in zip(dec.decode_packed_file(path), want))
    from streamoptima_amd.hostdecode import HostStreamDecoder
    got = []
    HostStreamDecoder(dec, chunk=2).decode_file(path, lambda i, y, u, v: got.append((y.copy(), u, v)))
    assert len(got) == F and all(u is None and v is None and np.array_equal(y, b) for (y, u, v), b in zip(got, want))


def test_off_allocates_and_launches_nothing(gpu, made):
    from streamoptima_amd.hostdecode import HostStreamDecoder
    dec = _decoder(gpu, "64x96", False)
    assert dec.deblock is False and dec.deblock_strength == 0
    hs = HostStreamDecoder(dec)
    assert hs.deblock is False and all(s.db_y is None and s.db_uv is None for s in hs.sets)
    on = HostStreamDecoder(_decoder(gpu, "64x96", True), chunk=3)
    assert all(tuple(s.db_y.shape) == (3, 64, 96) and tuple(s.db_uv.shape) == (3, 2, 32, 48) for s in on.sets)
    # the closed loop of the encoder keeps its own decoder at the defaults
    assert made("64x96")["enc"].decoder.deblock is False


@pytest.mark.parametrize("name", ["40x56", "rc2pass", "rc1"])
def test_text_bitstream(gpu, made, tmp_path, name):
    """decode_bitstream: decode() filters luma, decode_chroma() U and V (without their luma)."""
    m = made(name)
    files = [str(tmp_path / n) for n in ("mv.txt", "res.txt", "qp.txt", "chroma.txt")]
    m["enc"].transmit_bitstream(mv_file=files[0], residual_file=files[1], qp_map_file=files[2],
                                chroma_residual_file=files[3])
    for on, want in ((False, m["raw"]), (True, m["model"])):
        dec = _decoder(gpu, name, on)
        ys = dec.decode_bitstream(files[0], files[1], qp_map_file=files[2], chroma_residual_file=files[3],
                                  chroma_qp_offset=OFF)
        _same([(y, u, v) for y, (u, v) in zip(ys, dec.decoded_chroma)], want, ("text", on))
        assert all(np.array_equal(a, b) for a, b in zip(dec.decoded_vid, ys))
        # luma alone: decode_bitstream without the chroma file filters in decode()
        _same([(y, u, v) for y, (_, u, v) in zip(dec.decode_bitstream(files[0], files[1], qp_map_file=files[2]), want)],
              want, ("text, luma only", on))
    with pytest.raises(ValueError, match="decode\\(\\)"):
        fresh = _decoder(gpu, name, True)
        fresh.decode_chroma([0], [[]], [[]], [[]])


def test_decode_symbols(gpu, made):
    """decode_symbols (device symbols, the encoder's closed loop) with and without the filter."""
    m = made("64x96")
    enc = m["enc"]
    dec = _decoder(gpu, "64x96", True)
    ys = dec.decode_symbols(enc._symbols, chroma_symbols=enc.chroma_symbols)
    got = [(y.cpu().numpy()[:64, :96], u.cpu().numpy()[:32, :48], v.cpu().numpy()[:32, :48])
           for y, (u, v) in zip(ys, dec.decoded_chroma_device)]
    _same(got, m["model"], "decode_symbols")
    assert torch.equal(enc._symbols[1].recon, enc.decoder.decode_symbols(enc._symbols)[1])    # the raw frame, still
