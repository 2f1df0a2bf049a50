"""Chroma 4:2:0 through the streaming path, layer by layer, always against the resident encode
(encode_device without hooks), bit for bit: encode_device with the streaming hooks;
hoststream.HostStreamEncoder with pinned Y and UV planes in and one payload per frame out;
HostStreamEncoder.write_packed -> decoder.decode_packed_file, the file equal to the resident
transmit_packed420 (transmit_packed without chroma); and what is refused."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

QP, LAM = 4, 0.015


def _tables():
    from conftest import GOLDEN
    return json.load(open(os.path.join(GOLDEN, "rc_schedule.json")))["tables"]


def _planes(f, h, w, seed):
    """y [F, h, w], uv [F, 2, h/2, w/2] uint8 (numpy)."""
    from streamoptima_amd.synth import synth_sequence
    y = synth_sequence(f, h, w, seed=seed)
    uv = np.stack([synth_sequence(f, h // 2, w // 2, seed=seed + 100), synth_sequence(f, h // 2, w // 2, seed=seed + 200)],
                  axis=1)
    return y, uv


def _codec(gpu, h, w, f, intra_dur, vbs=False, chroma=True, y=None, uv=None, **kw):
    from streamoptima_amd.Encoder import Y_Video_codec
    if "RCFlag" in kw:
        kw.update(targetBR="200 kbps", qp_rate_tables=_tables())
    if chroma:
        kw.update(chroma=True, chroma_qp_offset=1, uv_frame_arr=uv)
    return Y_Video_codec(h, w, f, 16, 16, QP, intra_dur, 0, LAM, vbs, y_only_frame_arr=y, device=gpu, **kw)


def _same_luma(a, b, what):
    assert a.frame_type == b.frame_type, what
    for name in ("split", "qtc", "tokens", "mae_num", "recon", "sse"):
        assert torch.equal(getattr(a, name), getattr(b, name)), (what, name)
    # the motion vectors a decoder reads: all four of a split block, the first of an unsplit one
    used = (a.split != 0).view(-1, *[1] * (a.mv.dim() - 1)).expand_as(a.mv).clone()
    used[:, 0] = True
    assert torch.equal(a.mv[used], b.mv[used]), (what, "mv")
    assert ("qp_map" in a.extra) == ("qp_map" in b.extra), what
    if "qp_map" in a.extra:
        assert torch.equal(a.extra["qp_map"], b.extra["qp_map"]), what


def _same_chroma(a, b, what):
    assert a.frame_type == b.frame_type and a.qp_offset == b.qp_offset, what
    for name in ("qtc_u", "qtc_v", "tokens", "sse", "recon_u", "recon_v"):
        assert torch.equal(getattr(a, name), getattr(b, name)), (what, name)


# ---- encode_device with hooks == encode_device without -----------------------------------------------
F, INTRA = 7, 3                                   # I P P I P P I: two I-frames inside the GOP

ROI_64x128 = np.zeros((4, 8), np.int32)
ROI_64x128[1:3, 2:6] = -2
ROI_64x128[0] = 2
ROI_64x96 = np.ascontiguousarray(ROI_64x128[:, :6])

HOOK_CASES = {
    # the persistent run: the smallest shape Engine.pipelined_ok accepts, and 288 x 384
    "run_16x128_c1": dict(h=16, w=128, chunk=1), "run_16x128_c2": dict(h=16, w=128, chunk=2),
    "run_16x128_c3": dict(h=16, w=128, chunk=3),
    "run_288x384_c1": dict(h=288, w=384, chunk=1), "run_288x384_c2": dict(h=288, w=384, chunk=2, pre=True),
    "run_288x384_c3": dict(h=288, w=384, chunk=3),
    # two-pass RC with ROI in one persistent launch per unit: QP maps reach chroma
    "run2pass_roi_64x128": dict(h=64, w=128, chunk=2, run="2pass", kw=dict(RCFlag=3, roi=ROI_64x128)),
    # the per-frame path (W % 128 != 0)
    "frame_vbs": dict(h=64, w=96, chunk=1, run=None, vbs=True),
    # nRefFrames 3 goes with VBSEnable here: without it the multi-reference search of this content is
    # not repeatable from one luma-only encode_device call to the next (it differs from the oracle
    # too), chroma or not, so two encodes of it cannot be compared
    "frame_vbs_nref3": dict(h=64, w=96, chunk=1, run=None, vbs=True, kw=dict(nRefFrames=3)),
    "frame_rc1": dict(h=64, w=96, chunk=1, run=None, kw=dict(RCFlag=1)),
    "frame_vbs_nref3_rc1": dict(h=64, w=96, chunk=1, run=None, vbs=True, pre=True, kw=dict(nRefFrames=3, RCFlag=1)),
    "frame_roi": dict(h=64, w=96, chunk=1, run=None, kw=dict(roi=ROI_64x96)),
    "frame_rc2_switch": dict(h=64, w=96, chunk=1, run=None, switch=True, kw=dict(RCFlag=2, intra_thresh=10 ** 9)),
}


@pytest.mark.parametrize("case", list(HOOK_CASES))
def test_encode_device_hooks_match_resident(gpu, case):
    from streamoptima_amd.engine import ChromaSymbols, FrameSymbols
    from streamoptima_amd.hoststream import HostStreamEncoder
    cfg = HOOK_CASES[case]
    h, w, chunk = cfg["h"], cfg["w"], cfg["chunk"]
    y, uv = _planes(F, h, w, seed=23)
    if cfg.get("switch"):
        y[4:] = _planes(F, h, w, seed=77)[0][4:]          # a cut before frame 4: its residual is the largest
    c = _codec(gpu, h, w, F, INTRA, vbs=cfg.get("vbs", False), **dict(cfg.get("kw", {})))
    eng = c.engine()
    run = cfg.get("run", "plain")
    assert eng.pipelined_ok(c.nRefFrames) == (run is not None)
    fr, uvd = c._upload_padded(y), c._upload_uv_padded(uv)
    if cfg.get("switch"):
        # a threshold between the P-frames' residual sizes: the largest one is re-encoded as I
        sizes = [int(s.tokens.sum()) for s in c.encode_device(fr, INTRA, uv_dev=uvd)["symbols"] if s.frame_type == 1]
        assert min(sizes) < max(sizes)
        c.intra_thresh = (min(sizes) + max(sizes)) // 2
    ref = c.encode_device(fr, INTRA, uv_dev=uvd)
    if cfg.get("switch"):
        print(case, "frame types", ref["frame_type"])
        assert any(t == 0 for i, t in enumerate(ref["frame_type"]) if i % INTRA), ref["frame_type"]
    if cfg.get("kw", {}).get("roi") is not None:
        assert all("qp_map" in s.extra for s in ref["symbols"])
    assert any(bool(cs.qtc_u.any()) or bool(cs.qtc_v.any()) for cs in ref["chroma_symbols"])

    calls, waits = [], []
    pre = [eng.new_chroma_symbols() for _ in range(F)] if cfg.get("pre") else None
    got = c.encode_device(fr, INTRA, uv_dev=uvd, chunk=chunk, wait_input=lambda k0, k1: waits.append((k0, k1)),
                          on_output=lambda *a: calls.append(a), chroma_symbols=pre)
    assert got["frame_type"] == ref["frame_type"] and got["qp_rows"] == ref["qp_rows"]
    assert torch.equal(got["sse"], ref["sse"])
    for i in range(F):
        _same_luma(got["symbols"][i], ref["symbols"][i], (case, i))
        _same_chroma(got["chroma_symbols"][i], ref["chroma_symbols"][i], (case, i))
    assert torch.equal(got["chroma_sums"], ref["chroma_sums"])
    if pre is not None:
        assert all(a is b for a, b in zip(got["chroma_symbols"], pre))

    # the call pattern: four arguments, the units HostStreamEncoder uploads by
    assert all(len(a) == 4 for a in calls)
    units = HostStreamEncoder._units(SimpleNamespace(nframes=F, chunk=chunk), INTRA)
    assert [(a[0], a[1]) for a in calls] == units == waits
    for k0, k1, syms, csyms in calls:
        assert len(syms) == len(csyms) == k1 - k0
        assert all(isinstance(s, FrameSymbols) for s in syms) and all(isinstance(s, ChromaSymbols) for s in csyms)
        assert all(cs is got["chroma_symbols"][k] for cs, k in zip(csyms, range(k0, k1)))


def test_luma_only_callback_keeps_three_arguments(gpu):
    y, _ = _planes(4, 64, 128, seed=3)
    c = _codec(gpu, 64, 128, 4, 4, chroma=False)
    calls = []
    c.encode_device(c._upload_padded(y), 4, chunk=2, on_output=lambda *a: calls.append(a))
    assert [len(a) for a in calls] == [3, 3, 3] and [(a[0], a[1]) for a in calls] == [(0, 1), (1, 3), (3, 4)]


# ---- HostStreamEncoder ----------------------------------------------------------------------------------
H, W, CHUNK = 288, 384, 2
_RESIDENT = {}


def _stream_codec(gpu, chroma=True):
    return _codec(gpu, H, W, F, INTRA, chroma=chroma)


def _resident(gpu, seed):
    """The resident encode of content `seed`, packed on its own: pinned inputs and expected host
    results, computed once."""
    if seed not in _RESIDENT:
        y, uv = _planes(F, H, W, seed=seed)
        c = _stream_codec(gpu)
        eng = c.engine()
        fr, uvd = c._upload_padded(y), c._upload_uv_padded(uv)
        res = c.encode_device(fr, INTRA, uv_dev=uvd)
        loffs, lout = eng.pack_symbols(res["symbols"])
        coffs, cout = eng.pack_chroma_symbols(res["chroma_symbols"])
        loffs, coffs = loffs.cpu().numpy().astype(np.int64), coffs.cpu().numpy().astype(np.int64)
        sums = res["chroma_sums"].cpu()
        _RESIDENT[seed] = dict(
            y_host=fr.cpu().pin_memory(), uv_host=uvd.cpu().pin_memory(),
            luma=[lout[i, :loffs[i, -1]].cpu() for i in range(F)],
            chroma=[cout[i, :coffs[i, -1]].cpu() for i in range(F)],
            luma_lens=np.diff(loffs, axis=1), chroma_lens=np.diff(coffs, axis=1),
            sse=res["sse"].cpu(), csse=sums[:, :2].contiguous(), ctok=sums[:, 2:].contiguous(),
            frame_type=res["frame_type"])
    return _RESIDENT[seed]


def _check_result(got, want, lengths):
    assert set(got) == {"packed", "bytes", "luma_bytes", "sse", "frame_type", "chroma_sse", "chroma_tokens"} | (
        {"block_bytes", "chroma_block_bytes"} if lengths else set())
    assert got["frame_type"] == want["frame_type"]
    assert torch.equal(got["sse"], want["sse"])
    assert got["chroma_sse"].dtype == torch.int64 and tuple(got["chroma_sse"].shape) == (F, 2)
    assert torch.equal(got["chroma_sse"], want["csse"]) and torch.equal(got["chroma_tokens"], want["ctok"])
    assert got["luma_bytes"] == [t.numel() for t in want["luma"]]
    assert got["bytes"] == [a.numel() + b.numel() for a, b in zip(want["luma"], want["chroma"])]
    for i in range(F):
        assert torch.equal(got["packed"][i], torch.cat([want["luma"][i], want["chroma"][i]])), i
    if lengths:
        assert got["block_bytes"].dtype == np.uint16 and got["chroma_block_bytes"].dtype == np.uint16
        assert np.array_equal(got["block_bytes"], want["luma_lens"])
        assert np.array_equal(got["chroma_block_bytes"], want["chroma_lens"])


@pytest.mark.parametrize("nbuf", [1, 2])
def test_host_stream_chroma_matches_resident(gpu, nbuf):
    """One GOP twice (the buffers are reused), then three GOPs of different content back to back."""
    from streamoptima_amd.hoststream import HostStreamEncoder
    lengths = nbuf == 2
    hs = HostStreamEncoder(_stream_codec(gpu), F, chunk=CHUNK, nbuf=nbuf, lengths=lengths)
    want = _resident(gpu, 5)
    for _ in range(2):
        _check_result(hs.encode(want["y_host"], INTRA, uv_host=want["uv_host"]), want, lengths)
    seeds, seen = (6, 5, 7), []
    wants = [_resident(gpu, s) for s in seeds]

    def consume(k, r):
        _check_result(r, wants[k], lengths)
        seen.append(k)
    hs.encode_stream([x["y_host"] for x in wants], INTRA, consume, uv_gops=[x["uv_host"] for x in wants])
    assert seen == [0, 1, 2]


def test_luma_only_stream_beside_it_is_unchanged(gpu):
    """A chroma=False encoder: exactly the keys it always returned, and the resident luma bytes;
    with lengths=True it gains "block_bytes" alone."""
    from streamoptima_amd.hoststream import HostStreamEncoder
    y, _ = _planes(F, H, W, seed=5)
    c = _stream_codec(gpu, chroma=False)
    fr = c._upload_padded(y)
    res = c.encode_device(fr, INTRA)
    offs, out = c.engine().pack_symbols(res["symbols"])
    host = fr.cpu().pin_memory()
    got = HostStreamEncoder(c, F, chunk=CHUNK).encode(host, INTRA)
    assert set(got) == {"packed", "bytes", "sse", "frame_type"}
    assert got["frame_type"] == res["frame_type"] and torch.equal(got["sse"], res["sse"].cpu())
    assert got["bytes"] == offs[:, -1].tolist()
    for i in range(F):
        assert torch.equal(got["packed"][i], out[i, :int(offs[i, -1])].cpu()), i
    got = HostStreamEncoder(c, F, chunk=CHUNK, lengths=True).encode(host, INTRA)
    assert set(got) == {"packed", "bytes", "sse", "frame_type", "block_bytes"}
    assert np.array_equal(got["block_bytes"], np.diff(offs.cpu().numpy().astype(np.int64), axis=1))
    for i in range(F):
        assert torch.equal(got["packed"][i], out[i, :int(offs[i, -1])].cpu()), i


# ---- end to end: a streamed GOP as a file the decoder reads ----------------------------------------
@pytest.mark.parametrize("chroma", [True, False])
def test_streamed_file_decodes_and_equals_the_resident_file(gpu, tmp_path, monkeypatch, chroma):
    from streamoptima_amd import packedfile
    from streamoptima_amd.decoder import decoder
    from streamoptima_amd.hoststream import HostStreamEncoder
    monkeypatch.chdir(tmp_path)
    y, uv = _planes(F, H, W, seed=9)
    enc = _codec(gpu, H, W, F, INTRA, chroma=chroma, y=y, uv=uv)
    enc.encode()
    resident = str(tmp_path / "resident.sopk")
    (enc.transmit_packed420 if chroma else enc.transmit_packed)(resident)
    hs = HostStreamEncoder(enc, F, chunk=CHUNK, lengths=True)
    y_host = enc._upload_padded(y).cpu().pin_memory()
    uv_host = enc._upload_uv_padded(uv).cpu().pin_memory() if chroma else None
    res = hs.encode(y_host, INTRA, uv_host=uv_host)
    streamed = str(tmp_path / "streamed.sopk")
    size = hs.write_packed(streamed, res)
    assert size == os.path.getsize(streamed)
    assert open(streamed, "rb").read() == open(resident, "rb").read()
    assert packedfile.read(streamed, gpu)["layout"] == (1 if chroma else 0)
    dec = decoder(0, INTRA, 16, F, H, W, QP, 1, False, LAM, False, device=gpu)
    out = dec.decode_packed_file(streamed)
    for i in range(F):
        assert (out[i] == enc._symbols[i].recon.cpu().numpy()[:H, :W]).all(), i
    if chroma:
        for i, cs in enumerate(enc.chroma_symbols):
            du, dv = dec.decoded_chroma[i]
            assert (du == cs.recon_u.cpu().numpy()).all() and (dv == cs.recon_v.cpu().numpy()).all(), i
    else:
        assert dec.decoded_chroma is None
    with pytest.raises(ValueError, match="lengths"):
        hs_plain = HostStreamEncoder(enc, F, chunk=CHUNK)
        hs_plain.write_packed(str(tmp_path / "no.sopk"), hs_plain.encode(y_host, INTRA, uv_host=uv_host))


# ---- refusals --------------------------------------------------------------------------------------------
def test_refusals(gpu):
    from streamoptima_amd.Encoder import Y_Video_codec
    from streamoptima_amd.hoststream import HostStreamEncoder
    want = _resident(gpu, 5)
    y_host, uv_host = want["y_host"], want["uv_host"]
    hs = HostStreamEncoder(_stream_codec(gpu), F, chunk=CHUNK)
    with pytest.raises(ValueError):
        hs.encode(y_host, INTRA)                                          # missing
    with pytest.raises(ValueError):
        hs.encode(y_host, INTRA, uv_host=uv_host.clone())                 # not page-locked
    with pytest.raises(ValueError):
        hs.encode(y_host, INTRA, uv_host=uv_host[:, :1].contiguous().pin_memory())   # one plane per frame
    with pytest.raises(ValueError):
        hs.encode(y_host, INTRA, uv_host=uv_host[:F - 1].contiguous().pin_memory())  # a frame short
    with pytest.raises(ValueError):
        hs.encode_stream([y_host, y_host], INTRA, lambda k, r: None, uv_gops=[uv_host])
    with pytest.raises(ValueError):
        HostStreamEncoder(_stream_codec(gpu, chroma=False), F, chunk=CHUNK).encode(y_host, INTRA, uv_host=uv_host)
    _check_result(hs.encode(y_host, INTRA, uv_host=uv_host), want, False)   # still usable after a refusal
    with pytest.raises(NotImplementedError):
        Y_Video_codec(H, W, F, 16, 16, QP, INTRA, 0, LAM, False, FMEEnable=True, chroma=True, device=gpu)
    c = _stream_codec(gpu)
    with pytest.raises(ValueError):                                       # chroma symbols for another frame count
        c.encode_device(c._upload_padded(_planes(F, H, W, 5)[0]), INTRA, uv_dev=c._upload_uv_padded(_planes(F, H, W, 5)[1]),
                        chunk=2, chroma_symbols=[c.engine().new_chroma_symbols()])
