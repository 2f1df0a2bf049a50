"""so_pack_chroma_frames (_bits) / so_unpack_chroma_frames (_bits) on the GPU against the
plain-Python model (tests/packchromaref.py) on its corpus and mutants, called through ctypes on
tensors made from the corpus; then the public path (transmit_packed420 / transmit_packed with QP
maps -> decode_packed_file).  Every output buffer starts as a sentinel and ends in a guard region;
every comparison is exact equality of bytes or integers."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import packchromaref as R

pytestmark = pytest.mark.gpu

GUARD = 2048                                     # bytes past `cap` in out; > one record's bound
TAIL = 16                                        # guard elements past every other output row
OUT_FILL, OFFS_FILL, I16_FILL = 0xAB, 0x5A5A5A5A, 0x7B7B
PACK = {"varint": "so_pack_chroma_frames", "bits": "so_pack_chroma_frames_bits"}
UNPACK = {"varint": "so_unpack_chroma_frames", "bits": "so_unpack_chroma_frames_bits"}


def _lib():
    from streamoptima_amd import _lib as m
    return m.load(), m


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t if isinstance(t, int) else t.data_ptr() for t in ts])


def _dev(a, gpu):
    return torch.from_numpy(np.array(a, order="C")).to(gpu)      # a copy: corpus arrays are read-only


def _frame(coding, idx):
    """Records idx of the corpus as one frame -> ((qtc_u, qtc_v), the model's bytes per record)."""
    qu, qv = R.corpus()
    blocks = R.record_bytes(coding)
    return (qu[idx], qv[idx]), [blocks[i] for i in idx]


def _pack(gpu, coding, frames, cap, totals=True):
    """The packer on [(qtc_u, qtc_v)] -> offs [n, nb + 1 + TAIL], out [n, cap + GUARD], totals
    [n + 2], as numpy."""
    lib, m = _lib()
    n, nb = len(frames), frames[0][0].shape[0]
    dev = [[_dev(a, gpu) for a in f] for f in frames]
    offs = torch.full((n, nb + 1 + TAIL), OFFS_FILL, dtype=torch.int32, device=gpu)
    out = torch.full((n, cap + GUARD), OUT_FILL, dtype=torch.uint8, device=gpu)
    tot = torch.full((n + 2,), OFFS_FILL, dtype=torch.int32, device=gpu)
    rc = getattr(lib, PACK[coding])(n, _ptrs([d[0] for d in dev]), _ptrs([d[1] for d in dev]), nb, _ptrs(list(offs)),
                                    _ptrs(list(out)), cap, tot.data_ptr() + 4 if totals else None,
                                    m.stream_handle(gpu))
    m.check(rc, PACK[coding])
    torch.cuda.synchronize()
    return offs.cpu().numpy(), out.cpu().numpy(), tot.cpu().numpy()


def _offsets(blk):
    return np.concatenate(([0], np.cumsum([len(x) for x in blk])))


def _check_pack(offs, out, tot, blocks, cap, totals=True):
    """offs complete whatever the cap; exactly the records with offs[b + 1] <= cap written,
    byte-exact; the sentinel everywhere else, guards included (no byte at or past cap)."""
    for i, blk in enumerate(blocks):
        nb = len(blk)
        want_offs = _offsets(blk)
        assert np.array_equal(offs[i, :nb + 1], want_offs), (i, np.flatnonzero(offs[i, :nb + 1] != want_offs)[:8])
        assert (offs[i, nb + 1:] == OFFS_FILL).all(), i
        fit = int(want_offs[want_offs <= cap].max())          # offsets ascend: a prefix fits
        want = np.full(out.shape[1], OUT_FILL, np.uint8)
        want[:fit] = np.frombuffer(b"".join(blk), np.uint8)[:fit]
        assert np.array_equal(out[i], want), (i, np.flatnonzero(out[i] != want)[:8])
        if totals:
            assert tot[i + 1] == want_offs[-1], i
    assert tot[0] == OFFS_FILL and tot[-1] == OFFS_FILL
    if not totals:
        assert (tot == OFFS_FILL).all()


def _cap_for(blocks):
    return max(sum(len(x) for x in blk) for blk in blocks) + 64


class _Unpack:
    """The unpacker on streams that share one device buffer; outputs poisoned, each row with TAIL
    guard elements.  launch() is asynchronous; fetch() synchronises."""

    def __init__(self, gpu, coding, streams, offs, nb, ncalls=1):
        self.gpu, self.coding, self.nb, n = gpu, coding, nb, len(streams)
        starts = np.concatenate(([0], np.cumsum([len(s) for s in streams])))
        self.packed = _dev(np.frombuffer(b"".join(streams) + b"\xff" * 64, np.uint8), gpu)
        self.in_ptr = [self.packed.data_ptr() + int(s) for s in starts[:-1]]
        self.offs = _dev(np.asarray(offs, np.int32).reshape(n, nb + 1), gpu)
        self.q = torch.full((2, n, nb * 64 + TAIL), I16_FILL, dtype=torch.int16, device=gpu)
        self.err = torch.zeros(ncalls, dtype=torch.int32, device=gpu)

    def launch(self, frames, call=0):
        lib, m = _lib()
        row = lambda t: _ptrs([t[f].data_ptr() for f in frames])   # noqa: E731
        rc = getattr(lib, UNPACK[self.coding])(len(frames), _ptrs([self.in_ptr[f] for f in frames]), row(self.offs),
                                               self.nb, row(self.q[0]), row(self.q[1]),
                                               self.err.data_ptr() + 4 * call, m.stream_handle(self.gpu))
        m.check(rc, UNPACK[self.coding])

    def fetch(self):
        torch.cuda.synchronize()
        q = self.q.cpu().numpy()
        assert (q[:, :, self.nb * 64:] == I16_FILL).all()            # nothing past a row's records
        return q[0, :, :self.nb * 64], q[1, :, :self.nb * 64], self.err.cpu().numpy()


def _check_unpack(got, frames):
    qu, qv, err = got
    assert err.tolist() == [0] * err.size
    for i, (u, v) in enumerate(frames):
        assert np.array_equal(qu[i], u.reshape(-1)), (i, np.flatnonzero(qu[i] != u.reshape(-1))[:8])
        assert np.array_equal(qv[i], v.reshape(-1)), (i, np.flatnonzero(qv[i] != v.reshape(-1))[:8])


# ---- the packers against the model ----------------------------------------------------------------
@pytest.mark.parametrize("coding", R.CODINGS)
def test_pack_chroma_corpus_bytes_exact(gpu, coding):
    """The corpus as one frame: bytes, offsets and the total equal the model's (null totals: the
    same bytes); then the unpacker inverts the kernel's own stream and the model's."""
    n = R.corpus()[0].shape[0]
    frame, blk = _frame(coding, np.arange(n))
    cap = _cap_for([blk])
    offs, out, tot = _pack(gpu, coding, [frame], cap)
    _check_pack(offs, out, tot, [blk], cap)
    offs2, out2, tot2 = _pack(gpu, coding, [frame], cap, totals=False)
    _check_pack(offs2, out2, tot2, [blk], cap, totals=False)
    own = out[0, :int(offs[0, n])].tobytes()
    u = _Unpack(gpu, coding, [own, b"".join(blk)], [offs[0, :n + 1], _offsets(blk)], n)
    u.launch([0, 1])
    _check_unpack(u.fetch(), [frame, frame])


@pytest.mark.parametrize("nframes,nb", [(1, 1), (2, 31), (2, 33), (3, 257), (33, 5)])
@pytest.mark.parametrize("coding", R.CODINGS)
def test_pack_chroma_launch_geometry(gpu, coding, nframes, nb):
    """Grid tails and the one-ahead loads (a workgroup is 4 waves x 8 records, two per iteration:
    nb 1, 31, 33, 257), and more frames than one launch takes by value (33 > 32)."""
    n = R.corpus()[0].shape[0]
    frames, blocks = zip(*[_frame(coding, (i * 37 + 11 * nb + np.arange(nb) * 3) % n) for i in range(nframes)])
    cap = _cap_for(blocks)
    offs, out, tot = _pack(gpu, coding, list(frames), cap)
    _check_pack(offs, out, tot, blocks, cap)
    u = _Unpack(gpu, coding, [b"".join(blk) for blk in blocks], [_offsets(blk) for blk in blocks], nb)
    u.launch(list(range(nframes)))
    _check_unpack(u.fetch(), frames)


@pytest.mark.parametrize("coding", R.CODINGS)
def test_pack_chroma_capacity_guard(gpu, coding):
    """cap below the total: offs[nb] still holds the full length and no byte at or past cap is
    written (the sentinel stays), at caps on and around a record boundary."""
    nb, k = 64, 32
    n = R.corpus()[0].shape[0]
    frame, blk = _frame(coding, np.linspace(0, n - 1, nb).astype(int))
    o = _offsets(blk)
    total = int(o[nb])
    for cap in (0, int(o[k]) - 1, int(o[k]), int(o[k]) + 1, total - 1, total):
        offs, out, tot = _pack(gpu, coding, [frame], cap)
        assert int(offs[0, nb]) == total
        _check_pack(offs, out, tot, [blk], cap)


# ---- damaged and non-canonical input: the unpackers against the strict model --------------------------
@pytest.mark.parametrize("coding", R.CODINGS)
def test_unpack_chroma_agrees_with_the_model_on_every_mutant(gpu, coding):
    """Every mutant is a frame of one record.  One err word per call: the mutants the model accepts
    go 32 to a call, each of which must leave err 0 and give the model's blocks; a mutant the model
    rejects has a call to itself, which must set err to 1."""
    ms = R.mutants(coding)
    good = [i for i, m in enumerate(ms) if isinstance(m[2], dict)]
    bad = [i for i, m in enumerate(ms) if isinstance(m[2], str)]
    assert len(good) > 100 and len(bad) > 100
    calls = [good[j:j + 32] for j in range(0, len(good), 32)] + [[i] for i in bad]
    u = _Unpack(gpu, coding, [m[1] for m in ms], [[0, len(m[1])] for m in ms], 1, ncalls=len(calls))
    for c, members in enumerate(calls):
        u.launch(members, call=c)
    qu, qv, err = u.fetch()
    nclean = -(-len(good) // 32)
    wrong = [(c, int(err[c]), [ms[i][0] for i in calls[c]][:4]) for c in range(len(calls))
             if int(err[c]) != (0 if c < nclean else 1)]
    assert not wrong, wrong[:8]
    for i in good:
        assert np.array_equal(qu[i], ms[i][2]["qtc_u"]) and np.array_equal(qv[i], ms[i][2]["qtc_v"]), ms[i][0]


@pytest.mark.parametrize("coding", R.CODINGS)
def test_unpack_chroma_reversed_offsets(gpu, coding):
    """offs[b + 1] < offs[b] is malformed for record b, whatever its bytes."""
    frame, blk = _frame(coding, np.arange(40, 46))
    o = _offsets(blk)
    rev = o.copy()
    rev[3] = rev[2] - 1
    verdicts = R.unpack_frame_strict(b"".join(blk), rev.tolist(), coding)
    assert verdicts[2] == "offs" and isinstance(verdicts[0], dict)
    culprits = {b for b, v in enumerate(verdicts) if isinstance(v, str)}
    u = _Unpack(gpu, coding, [b"".join(blk)] * 2, [o, rev], 6, ncalls=2)
    u.launch([0], call=0)
    u.launch([1], call=1)
    qu, qv, err = u.fetch()
    assert int(err[0]) == 0 and int(err[1]) - 1 in culprits
    assert np.array_equal(qu[0], frame[0].reshape(-1)) and np.array_equal(qv[0], frame[1].reshape(-1))


# ---- the public path ---------------------------------------------------------------------------------
H, W, F = 48, 80, 4


def _tables():
    from conftest import GOLDEN
    return json.load(open(os.path.join(GOLDEN, "rc_schedule.json")))["tables"]


def _roi_map():
    m = np.zeros((H // 16, W // 16), np.int32)
    m[1:3, 1:4] = -2
    m[0] = 2
    return m


CASES = {
    "chroma": dict(vbs=False, chroma=True, kw={}),
    "chroma_rc1_vbs": dict(vbs=True, chroma=True, kw=dict(RCFlag=1, targetBR="200 kbps")),
    "roi_2pass": dict(vbs=False, chroma=False, kw=dict(RCFlag=3, targetBR="200 kbps", intra_thresh=10 ** 9), roi=True),
    "roi_2pass_chroma": dict(vbs=False, chroma=True, kw=dict(RCFlag=3, targetBR="200 kbps", intra_thresh=10 ** 9),
                             roi=True),
}


@pytest.mark.parametrize("case", list(CASES))
def test_transmit_packed_then_decode(gpu, tmp_path, monkeypatch, case):
    """encode() -> transmit_packed420 (transmit_packed without chroma) in both codings ->
    decode_packed_file: luma equal to the encoder's reconstructions, decoded_chroma equal to the
    encoder's chroma reconstructions, save_yuv420 the encoder's bytes; the QP maps travel."""
    from streamoptima_amd import packedfile
    from streamoptima_amd.Encoder import Y_Video_codec
    from streamoptima_amd.decoder import decoder
    from streamoptima_amd.synth import synth_sequence
    monkeypatch.chdir(tmp_path)
    cfg = CASES[case]
    y = synth_sequence(F, H, W, seed=17)
    y[:, :, :32] = 60                             # flat next to texture: two-pass moves QPs
    uv = np.stack([synth_sequence(F, H // 2, W // 2, seed=18), synth_sequence(F, H // 2, W // 2, seed=19)], axis=1)
    kw = dict(cfg["kw"])
    if "RCFlag" in kw:
        kw["qp_rate_tables"] = _tables()
    dec_kw = {k: v for k, v in kw.items() if k != "intra_thresh"}
    if cfg.get("roi"):
        kw["roi"] = _roi_map()
    if cfg["chroma"]:
        kw.update(chroma=True, chroma_qp_offset=1, uv_frame_arr=uv)
    enc = Y_Video_codec(H, W, F, 16, 16, 4, 2, 0, 0.015, cfg["vbs"], y_only_frame_arr=y, device=gpu, **kw)
    enc.encode()
    assert [s.frame_type for s in enc._symbols] == [0, 1, 0, 1]
    has_maps = any("qp_map" in s.extra for s in enc._symbols)
    assert has_maps == bool(cfg.get("roi"))
    if case == "chroma_rc1_vbs":
        assert all(q for q in enc.encoded_package["Qp_per_row_per_frame"])
    if cfg["chroma"]:
        assert any(c.qtc_u.any() or c.qtc_v.any() for c in enc.chroma_symbols)
        with pytest.raises(NotImplementedError, match="transmit_packed420"):
            enc.transmit_packed(str(tmp_path / "no.sopk"))
        enc.save_yuv420(str(tmp_path / "enc.yuv"))
    else:
        with pytest.raises(ValueError):
            enc.transmit_packed420(str(tmp_path / "no.sopk"))
    sizes = {}
    for coding in R.CODINGS:
        path = str(tmp_path / f"gop_{coding}.sopk")
        size = (enc.transmit_packed420 if cfg["chroma"] else enc.transmit_packed)(path, coding=coding)
        assert size == os.path.getsize(path) > 0
        sizes[coding] = size
        meta = packedfile.read(path, gpu)
        assert meta["layout"] == 1 and meta["coding"] == coding
        assert (meta["chroma_packed"] is not None) == cfg["chroma"] and (meta["qp_maps"] is not None) == has_maps
        if has_maps:
            for s, m in zip(enc._symbols, meta["qp_maps"]):
                assert ("qp_map" in s.extra) == (m is not None)
                assert m is None or torch.equal(m, s.extra["qp_map"].reshape(-1))
        if cfg["chroma"]:
            assert meta["chroma_qp_offset"] == 1
            for c, p, o in zip(enc.chroma_symbols, meta["chroma_packed"], meta["chroma_offs"]):
                want = R.pack_frame(c.qtc_u.cpu().numpy(), c.qtc_v.cpu().numpy(), coding)
                assert p.cpu().numpy().tobytes() == b"".join(want) and o.tolist() == _offsets(want).tolist()
        dec = decoder(0, 2, 16, F, H, W, 4, 1, False, 0.015, cfg["vbs"], device=gpu, **dec_kw)
        out = dec.decode_packed_file(path)
        for i in range(F):
            assert (out[i] == enc._symbols[i].recon.cpu().numpy()[:H, :W]).all(), (coding, i)
        if cfg["chroma"]:
            for i, c in enumerate(enc.chroma_symbols):
                du, dv = dec.decoded_chroma[i]
                assert (du == c.recon_u.cpu().numpy()[:H // 2, :W // 2]).all(), (coding, i)
                assert (dv == c.recon_v.cpu().numpy()[:H // 2, :W // 2]).all(), (coding, i)
            dec.save_yuv420(str(tmp_path / "dec.yuv"))
            assert (tmp_path / "dec.yuv").read_bytes() == (tmp_path / "enc.yuv").read_bytes()
            for other in (decoder(0, 2, 16, F, H, W, 4, 1, True, 0.015, cfg["vbs"], device=gpu, **dec_kw),):
                with pytest.raises(NotImplementedError):
                    other.decode_packed_file(path)
        else:
            assert dec.decoded_chroma is None
    print(case, sizes)
    assert sizes["bits"] < sizes["varint"]


def test_engine_chroma_pack_round_trip_and_errors(gpu):
    """Engine.pack_chroma_symbols -> unpack_chroma_symbols on corpus records; a damaged stream raises."""
    from streamoptima_amd.engine import ChromaSymbols, Engine
    eng = Engine(H, W, 16, 16, False, 0.0, gpu)
    nb = eng.nb
    frames = [_frame("varint", np.arange(nb) * 7 + 100 * i)[0] for i in range(2)]
    csyms = [ChromaSymbols(0, _dev(u, gpu), _dev(v, gpu), None, None) for u, v in frames]
    for coding in R.CODINGS:
        assert eng.pack_chroma_bound(coding) == nb * R.BOUND[coding]
        totals = torch.zeros(2, dtype=torch.int32, device=gpu)
        offs, out = eng.pack_chroma_symbols(csyms, totals=totals, coding=coding)
        assert out.shape == (2, nb * R.BOUND[coding]) and torch.equal(totals, offs[:, nb])
        packed = [out[i, :int(offs[i, nb])] for i in range(2)]
        got = eng.unpack_chroma_symbols(packed, list(offs), coding=coding)
        for (u, v), (gu, gv) in zip(frames, got):
            assert np.array_equal(gu.cpu().numpy(), u) and np.array_equal(gv.cpu().numpy(), v)
        cut = offs[0].clone()
        cut[nb] -= 1
        with pytest.raises(ValueError, match="malformed"):
            eng.unpack_chroma_symbols([packed[0]], [cut], coding=coding)
    with pytest.raises(ValueError):
        eng.pack_chroma_symbols(csyms, coding="nope")
    with pytest.raises(ValueError):
        eng.pack_chroma_symbols([], coding="bits")
