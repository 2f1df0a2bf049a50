"""Chroma under FMEEnable through the codec, the packed file and the streams
(chroma_subpel=True), on 4 frames (I P P P) of 32 x 48 luma, VBS off and on: luma untouched, chroma
against the numpy model (tests/chromasubpelref.py) fed the GPU's half-sample luma vectors, the file
in both codings through decode_packed_file, the fused chroma decode against unpack + reconstruct,
and HostStreamEncoder -> HostStreamDecoder with planar and RGB ends."""
import os

import numpy as np
import pytest
import torch

import chromasubpelref as SR
import colourref

pytestmark = pytest.mark.gpu

H, W, F, INTRA, QP, LAM, OFF = 32, 48, 4, 8, 4, 0.015, 1
MATRIX, FULL = "bt709", False
_MADE = {}


def _colour():
    from streamoptima_amd.colour import Colour
    return Colour(MATRIX, FULL)


def _content():
    if "content" not in _MADE:
        from streamoptima_amd.synth import synth_sequence
        rgb = np.ascontiguousarray(np.stack([synth_sequence(F, H, W, seed=51 + 10 * c) for c in range(3)], axis=-1))
        y, uv = colourref.rgb_to_yuv420(rgb, MATRIX, FULL, H, W)   # H, W are multiples of 16: no padding
        _MADE["content"] = (rgb, y, uv)
    return _MADE["content"]


def _codec(gpu, vbs, chroma=True, **kw):
    from streamoptima_amd.Encoder import Y_Video_codec
    if chroma:
        kw = dict(dict(chroma=True, chroma_qp_offset=OFF, chroma_subpel=True, colour=_colour()), **kw)
    return Y_Video_codec(H, W, F, 16, 16, QP, INTRA, 0, LAM, vbs, FMEEnable=True, device=gpu, **kw)


def _decoder(gpu, vbs, subpel=True):
    from streamoptima_amd.decoder import decoder
    return decoder(0, INTRA, 16, F, H, W, QP, 1, True, LAM, vbs, device=gpu, chroma_subpel=subpel)


@pytest.fixture(scope="module")
def made(gpu, tmp_path_factory):
    """vbs -> the encoded codec pair (chroma off / on), the packed files of both codings, and what
    decode_packed_file gives for the varint one; made on first use."""
    root = tmp_path_factory.mktemp("subpel_chain")

    def get(vbs):
        if vbs in _MADE:
            return _MADE[vbs]
        _, y, uv = _content()
        cwd = os.getcwd()
        os.chdir(root)
        try:
            plain = _codec(gpu, vbs, chroma=False, y_only_frame_arr=y)
            psnr_plain = plain.encode()
            enc = _codec(gpu, vbs, y_only_frame_arr=y, uv_frame_arr=uv)
            psnr = enc.encode()
            paths = {}
            for coding in ("varint", "bits"):
                paths[coding] = str(root / f"vbs{int(vbs)}_{coding}.sopk")
                enc.transmit_packed420(paths[coding], coding=coding)
            dec = _decoder(gpu, vbs)
            ys = [a.copy() for a in dec.decode_packed_file(paths["varint"])]
            cs = [(u.copy(), v.copy()) for u, v in dec.decoded_chroma]
        finally:
            os.chdir(cwd)
        _MADE[vbs] = dict(plain=plain, enc=enc, psnr=(psnr_plain, psnr), paths=paths, dec=dec, y=ys, c=cs, root=root)
        return _MADE[vbs]
    return get


@pytest.mark.parametrize("vbs", [False, True])
def test_codec_luma_untouched_chroma_is_the_model(made, vbs):
    m = made(vbs)
    plain, enc = m["plain"], m["enc"]
    assert m["psnr"][0] == m["psnr"][1]
    assert [s.frame_type for s in enc._symbols] == [0, 1, 1, 1]
    for a, b in zip(enc._symbols, plain._symbols):
        assert a.frame_type == b.frame_type
        for k in ("split", "mv", "qtc", "tokens", "mae_num", "recon"):
            assert torch.equal(getattr(a, k), getattr(b, k)), k
    _, _, uv = _content()
    luma = []
    for s in enc._symbols:
        d = dict(frame_type=s.frame_type, qp=s.qp_rd)
        if s.frame_type == 1:
            d.update(split=s.split.cpu().numpy(), mv=s.mv.cpu().numpy())
        luma.append(d)
    used = np.concatenate([d["mv"][:, 0, 0:2].reshape(-1) for d in luma[1:]])
    assert (used & 1).any(), "no half-sample luma vector: the content does not exercise FME"
    if vbs:
        assert any(d["split"].any() for d in luma[1:])
    exp = SR.encode_gop(uv, luma, nref_frames=1, qp_offset=OFF, s=2)
    for i in range(F):
        for k in ("qtc_u", "qtc_v", "tokens", "recon_u", "recon_v", "sse"):
            g = getattr(enc.chroma_symbols[i], k).cpu().numpy()
            assert g.shape == exp[i][k].shape and (g == exp[i][k]).all(), (i, k)
    # read as half-sample chroma vectors the same symbols give other planes: s matters here
    half = SR.encode_gop(uv, luma, nref_frames=1, qp_offset=OFF, s=1)
    assert any((half[i]["recon_u"] != exp[i]["recon_u"]).any() for i in range(1, F))
    # the closed loop of encode()
    for i in range(F):
        du, dv = enc.decoded_chroma_device[i]
        assert torch.equal(du, enc.chroma_symbols[i].recon_u) and torch.equal(dv, enc.chroma_symbols[i].recon_v)


@pytest.mark.parametrize("coding", ["varint", "bits"])
@pytest.mark.parametrize("vbs", [False, True])
def test_packed_file_round_trip(made, gpu, tmp_path, vbs, coding):
    from streamoptima_amd import packedfile
    m = made(vbs)
    enc, path = m["enc"], m["paths"][coding]
    meta = packedfile.read(path, gpu)
    assert meta["layout"] == 1 and meta["coding"] == coding and meta["chroma_packed"] is not None
    dec = _decoder(gpu, vbs)
    out = dec.decode_packed_file(path)
    for i in range(F):
        assert (out[i] == enc._symbols[i].recon.cpu().numpy()).all(), i
        du, dv = dec.decoded_chroma[i]
        cs = enc.chroma_symbols[i]
        assert (du == cs.recon_u.cpu().numpy()).all() and (dv == cs.recon_v.cpu().numpy()).all(), i
    a, b = str(tmp_path / "enc.yuv"), str(tmp_path / "dec.yuv")
    enc.save_yuv420(a)
    dec.save_yuv420(b)
    data = open(a, "rb").read()
    assert len(data) == F * H * W * 3 // 2 and data == open(b, "rb").read()
    # the vector precision is the decoder's argument: without it the file is refused as before
    with pytest.raises(NotImplementedError):
        _decoder(gpu, vbs, subpel=False).decode_packed_file(path)


@pytest.mark.parametrize("coding", ["varint", "bits"])
@pytest.mark.parametrize("vbs", [False, True])
def test_fused_chroma_decode_equals_unpack_and_recon(made, gpu, vbs, coding):
    from streamoptima_amd.engine import FrameSymbols
    enc = made(vbs)["enc"]
    eng = enc.engine()
    assert eng.fme and eng.chroma_subpel
    syms = enc._symbols
    coffs, cout = eng.pack_chroma_symbols(enc.chroma_symbols, coding=coding)
    cpacked, co = [cout[i] for i in range(F)], [coffs[i] for i in range(F)]
    qtcs = eng.unpack_chroma_symbols(cpacked, co, coding=coding)
    want, ru, rv = [], [], []
    for s, (qu, qv) in zip(syms, qtcs):
        if s.frame_type == 0:
            ru, rv = [], []
        lum = FrameSymbols(s.frame_type, s.split, s.mv, None, None, None, None, qp_rd=QP)
        r = eng.recon_chroma(lum, qu, qv, ru, rv, OFF)
        want.append((r.recon_u, r.recon_v))
        ru, rv = [r.recon_u], [r.recon_v]
    types = [s.frame_type for s in syms]
    split = [None if s.frame_type == 0 else s.split for s in syms]
    mv = [None if s.frame_type == 0 else s.mv for s in syms]
    gu, gv, err = eng.decode_chroma_frames(types, cpacked, co, split, mv, [], [], 1, QP, OFF, coding=coding)
    torch.cuda.synchronize()
    assert err.tolist() == [0] * F
    for i in range(F):
        assert torch.equal(gu[i], want[i][0]) and torch.equal(gv[i], want[i][1]), i
        assert torch.equal(gu[i], enc.chroma_symbols[i].recon_u), i
    # frame 2 with the last byte of its longest record cut off: err names frame and block, the
    # call succeeds and every other block of the frame is the expected one
    oh = co[2].cpu().numpy().astype(np.int64)
    lens = np.diff(oh)
    b = int(np.argmax(lens))
    assert lens[b] > 2
    data = cout[2, :oh[-1]].cpu().numpy()
    end = int(oh[b + 1])
    oh2 = oh.copy()
    oh2[b + 1:] -= 1
    cpacked[2] = torch.from_numpy(np.concatenate([data[:end - 1], data[end:]])).to(gpu)
    co[2] = torch.from_numpy(oh2.astype(np.int32)).to(gpu)
    hu, hv, err = eng.decode_chroma_frames(types, cpacked, co, split, mv, [], [], 1, QP, OFF, coding=coding)
    torch.cuda.synchronize()
    assert err.tolist() == [0, 0, 1 + b, 0]
    assert torch.equal(hu[1], want[1][0]) and torch.equal(hv[1], want[1][1])
    keep = torch.ones((H // 2, W // 2), dtype=torch.bool, device=gpu)
    nbx = W // 16
    keep[(b // nbx) * 8:(b // nbx) * 8 + 8, (b % nbx) * 8:(b % nbx) * 8 + 8] = False
    assert torch.equal(hu[2][keep], want[2][0][keep]) and torch.equal(hv[2][keep], want[2][1][keep])


def _pinned(a):
    return torch.from_numpy(np.array(a)).pin_memory()


def _collect(hs, path):
    got = []
    hs.decode_file(path, lambda i, y, u, v: got.append((y.copy(), u.copy(), v.copy())))
    return got


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("vbs", [False, True])
def test_streams_deliver_the_same_planes(made, gpu, tmp_path, vbs, fused):
    from streamoptima_amd.hostdecode import HostStreamDecoder
    from streamoptima_amd.hoststream import HostStreamEncoder
    m = made(vbs)
    _, y, uv = _content()
    hs = HostStreamEncoder(_codec(gpu, vbs), F, chunk=2, lengths=True)
    res = hs.encode(_pinned(y), INTRA, uv_host=_pinned(uv))
    path = str(tmp_path / "streamed.sopk")
    hs.write_packed(path, res)
    assert open(path, "rb").read() == open(m["paths"]["varint"], "rb").read()
    for chunk, nbuf in ((1, 1), (2, 2)) if fused else ((2, 2),):
        hd = HostStreamDecoder(m["dec"], chunk=chunk, nbuf=nbuf, fused=fused)
        assert hd.chroma_ok
        got = _collect(hd, path)
        assert len(got) == F
        for i, (gy, gu, gv) in enumerate(got):
            assert (gy == m["y"][i]).all() and (gu == m["c"][i][0]).all() and (gv == m["c"][i][1]).all(), (chunk, i)
    out = str(tmp_path / "out.yuv")
    HostStreamDecoder(m["dec"]).decode_to_yuv(path, out)
    ref = str(tmp_path / "ref.yuv")
    m["dec"].decode_packed_file(path)
    m["dec"].save_yuv420(ref)
    assert open(out, "rb").read() == open(ref, "rb").read()


@pytest.mark.parametrize("vbs", [False, True])
def test_rgb_ends(made, gpu, tmp_path, vbs):
    """output="rgb": colourref applied to the delivered planes; input="rgb": the file of the
    planar stream fed colourref's planes of the same pictures; and an output_size."""
    from streamoptima_amd.hostdecode import HostStreamDecoder
    from streamoptima_amd.hoststream import HostStreamEncoder
    m = made(vbs)
    rgb, _, _ = _content()
    path = m["paths"]["varint"]
    want = [colourref.yuv420_to_rgb(y[None], np.stack([u, v])[None], H, W, MATRIX, FULL)[0]
            for y, (u, v) in zip(m["y"], m["c"])]
    got = []
    hd = HostStreamDecoder(m["dec"], chunk=2, nbuf=2, output="rgb", colour=_colour())
    hd.decode_file(path, lambda i, p: got.append(p.copy()))
    assert len(got) == F
    for i in range(F):
        assert got[i].shape == (H, W, 3) and (got[i] == want[i]).all(), i
    if not vbs:
        hs = HostStreamEncoder(_codec(gpu, vbs), F, chunk=2, lengths=True, input="rgb")
        a = str(tmp_path / "rgb.sopk")
        hs.write_packed(a, hs.encode(_pinned(rgb), INTRA))
        assert open(a, "rb").read() == open(path, "rb").read()
        # source_size at the picture's own size: the resampler's identity tables, the same file
        _, y, uv = _content()
        hs = HostStreamEncoder(_codec(gpu, vbs), F, chunk=2, lengths=True, source_size=(H, W))
        hs.write_packed(a, hs.encode(_pinned(y), INTRA, uv_host=_pinned(uv)))
        assert open(a, "rb").read() == open(path, "rb").read()
        small = []
        HostStreamDecoder(m["dec"], output="rgb", colour=_colour(), output_size=(16, 24)).decode_file(
            path, lambda i, p: small.append(p.shape))
        assert small == [(16, 24, 3)] * F
    # without the keyword the decoder's streams refuse as before
    with pytest.raises(NotImplementedError):
        HostStreamDecoder(_decoder(gpu, vbs, subpel=False), output="rgb")
    with pytest.raises(NotImplementedError):
        HostStreamDecoder(_decoder(gpu, vbs, subpel=False)).decode_file(path, lambda *a: None)
