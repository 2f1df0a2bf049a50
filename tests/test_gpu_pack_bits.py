"""so_pack_frames_bits / so_unpack_frames_bits on the GPU against the plain-Python model of the
"bits" coding (tests/packbitsref.py) on the edge corpus (tests/packbitcases.py), called
through ctypes on tensors made from the corpus; then the public path (transmit_packed with
coding="bits" -> decode_packed_file).  Every output buffer starts as a sentinel and ends in a
guard region; every comparison is exact equality of bytes or integers."""
import ctypes
import os

import numpy as np
import pytest
import torch

import packbitcases
from packbitsref import unpack_block_bits_strict

pytestmark = pytest.mark.gpu

GUARD = 4096                                     # bytes past `cap` in out; > one block's bound
TAIL = 16                                        # guard elements past every other output row
OUT_FILL, OFFS_FILL, SPLIT_FILL, I16_FILL = 0xAB, 0x5A5A5A5A, 0xEE, 0x7B7B
NBS = (1, 31, 32, 33, 257)                       # one workgroup: 4 waves x 8 blocks, two per iteration
NFRAMES = (1, 32, 33)                            # a launch takes 32 frames by value


def _lib():
    from streamoptima_amd import _lib as m
    return m.load(), m


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t if isinstance(t, int) else t.data_ptr() for t in ts])


def _dev(a, gpu):
    return torch.from_numpy(np.array(a, order="C")).to(gpu)      # a copy: corpus arrays are read-only


def _frame(kind, ftype, idx):
    """Blocks idx of a corpus as one frame -> ((ftype, split, mv, qtc), the model's bytes per block)."""
    split, mv, qtc = packbitcases.corpus(kind, ftype)
    blocks = packbitcases.block_bytes(kind, ftype)
    return (ftype, split[idx], mv[idx], qtc[idx]), [blocks[i] for i in idx]


def _varied_frames(kind, nframes, nb):
    """nframes frames of nb blocks: different content, frame types mixed in one call."""
    n = packbitcases.corpus(kind, 0)[0].size
    return [_frame(kind, (i + nb) % 2, (i * 37 + 11 * nb + np.arange(nb)) % n) for i in range(nframes)]


def _pack(gpu, frames, bs, cap, totals=True):
    """so_pack_frames_bits on [(ftype, split, mv, qtc)] -> offs [n, nb + 1 + TAIL], out
    [n, cap + GUARD], totals [n + 2] (or None), as numpy."""
    lib, m = _lib()
    n, nb = len(frames), frames[0][1].size
    dev = [[_dev(a, gpu) for a in f[1:]] for f in frames]
    offs = torch.full((n, nb + 1 + TAIL), OFFS_FILL, dtype=torch.int32, device=gpu)
    out = torch.full((n, cap + GUARD), OUT_FILL, dtype=torch.uint8, device=gpu)
    tot = torch.full((n + 2,), OFFS_FILL, dtype=torch.int32, device=gpu)
    rc = lib.so_pack_frames_bits(n, (ctypes.c_int32 * n)(*[f[0] for f in frames]), _ptrs([d[0] for d in dev]),
                                 _ptrs([d[1] for d in dev]), _ptrs([d[2] for d in dev]), nb, bs, _ptrs(list(offs)),
                                 _ptrs(list(out)), cap, tot.data_ptr() + 4 if totals else None, m.stream_handle(gpu))
    m.check(rc, "so_pack_frames_bits")
    torch.cuda.synchronize()
    return offs.cpu().numpy(), out.cpu().numpy(), tot.cpu().numpy()


def _offsets(blk):
    return np.concatenate(([0], np.cumsum([len(x) for x in blk])))


def _check_pack(offs, out, tot, blocks, cap, totals=True):
    """offs complete whatever the cap; exactly the blocks with offs[b + 1] <= cap written,
    byte-exact; the sentinel everywhere else, guards included."""
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
    """so_unpack_frames_bits on streams that share one device buffer; outputs poisoned, each
    row with TAIL guard elements.  launch() is asynchronous; fetch() synchronises."""

    def __init__(self, gpu, streams, offs, nb, bs, ncalls=1):
        self.gpu, self.nb, self.bs, n = gpu, nb, bs, len(streams)
        starts = np.concatenate(([0], np.cumsum([len(s) for s in streams])))
        self.packed = _dev(np.frombuffer(b"".join(streams) + b"\xff" * 64, np.uint8), gpu)
        self.in_ptr = [self.packed.data_ptr() + int(s) for s in starts[:-1]]
        self.offs = _dev(np.asarray(offs, np.int32).reshape(n, nb + 1), gpu)
        self.split = torch.full((n, nb + TAIL), SPLIT_FILL, dtype=torch.uint8, device=gpu)
        self.mv = torch.full((n, nb * 12 + TAIL), I16_FILL, dtype=torch.int16, device=gpu)
        self.qtc = torch.full((n, nb * bs * bs + TAIL), I16_FILL, dtype=torch.int16, device=gpu)
        self.err = torch.zeros(ncalls, dtype=torch.int32, device=gpu)
        self.rows = [self.offs.data_ptr(), self.split.data_ptr(), self.mv.data_ptr(), self.qtc.data_ptr()]
        self.stride = [t.stride(0) * t.element_size() for t in (self.offs, self.split, self.mv, self.qtc)]

    def launch(self, frames, ftypes, call=0):
        lib, m = _lib()
        n = len(frames)
        row = lambda k: _ptrs([self.rows[k] + f * self.stride[k] for f in frames])   # noqa: E731
        rc = lib.so_unpack_frames_bits(n, (ctypes.c_int32 * n)(*ftypes), _ptrs([self.in_ptr[f] for f in frames]),
                                       row(0), self.nb, self.bs, row(1), row(2), row(3),
                                       self.err.data_ptr() + 4 * call, m.stream_handle(self.gpu))
        m.check(rc, "so_unpack_frames_bits")

    def fetch(self):
        torch.cuda.synchronize()
        return self.split.cpu().numpy(), self.mv.cpu().numpy(), self.qtc.cpu().numpy(), self.err.cpu().numpy()


def _expected_rows(ftype, split, mv, qtc):
    """One frame's output rows as _Unpack lays them out: untouched elements keep the poison."""
    nb = split.size
    assert I16_FILL not in mv and I16_FILL not in qtc      # an unwritten element cannot pass
    w = 12 if ftype == 1 else 4
    s = np.full(nb + TAIL, SPLIT_FILL, np.uint8)
    s[:nb] = split
    m = np.full(nb * 12 + TAIL, I16_FILL, np.int16)
    m[:nb * w] = packbitcases.used_mv(split, mv).reshape(-1)
    q = np.full(qtc.size + TAIL, I16_FILL, np.int16)
    q[:qtc.size] = qtc.reshape(-1)
    return s, m, q


def _check_unpack(got, frames):
    split, mv, qtc, err = got
    assert err.tolist() == [0] * err.size
    for i, (ftype, sp, m, q) in enumerate(frames):
        ws, wm, wq = _expected_rows(ftype, sp, m, q)
        assert np.array_equal(split[i], ws), i
        assert np.array_equal(mv[i], wm), (i, np.flatnonzero(mv[i] != wm)[:8])
        assert np.array_equal(qtc[i], wq), (i, np.flatnonzero(qtc[i] != wq)[:8])


# ---- the packer against the model's writer --------------------------------------------------------
@pytest.mark.parametrize("ftype", [0, 1])
@pytest.mark.parametrize("kind", packbitcases.KINDS)
def test_pack_bits_corpus_bytes_exact(gpu, kind, ftype):
    """Every corpus as one frame: bytes, offsets and the total equal the model's (null totals:
    the same bytes); then so_unpack_frames_bits inverts the kernel's own stream and the
    model's, outputs poisoned first."""
    bs = packbitcases.block_size(kind)
    n = packbitcases.corpus(kind, ftype)[0].size
    frame, blk = _frame(kind, ftype, np.arange(n))
    cap = _cap_for([blk])
    offs, out, tot = _pack(gpu, [frame], bs, cap)
    _check_pack(offs, out, tot, [blk], cap)
    offs2, out2, tot2 = _pack(gpu, [frame], bs, cap, totals=False)
    _check_pack(offs2, out2, tot2, [blk], cap, totals=False)
    own = out[0, :int(offs[0, n])].tobytes()
    u = _Unpack(gpu, [own, b"".join(blk)], [offs[0, :n + 1], _offsets(blk)], n, bs)
    u.launch([0, 1], [ftype, ftype])
    _check_unpack(u.fetch(), [frame, frame])


@pytest.mark.parametrize("nframes", NFRAMES)
@pytest.mark.parametrize("kind", packbitcases.KINDS)
def test_pack_bits_launch_geometry(gpu, kind, nframes):
    bs = packbitcases.block_size(kind)
    for nb in NBS:
        frames, blocks = zip(*_varied_frames(kind, nframes, nb))
        cap = _cap_for(blocks)
        offs, out, tot = _pack(gpu, list(frames), bs, cap)
        _check_pack(offs, out, tot, blocks, cap)
        u = _Unpack(gpu, [b"".join(blk) for blk in blocks], [_offsets(blk) for blk in blocks], nb, bs)
        u.launch(list(range(nframes)), [f[0] for f in frames])
        _check_unpack(u.fetch(), frames)


def test_pack_bits_scan_carry_with_one_byte_blocks(gpu):
    """nb = 8193, one past the scan's 8192-count tile, every block the all-zero intra block (one
    byte, 0x18) but three: the offsets are the block indices until the first of them."""
    nb = 8193
    split = np.zeros(nb, np.uint8)
    mv = np.zeros((nb, 4), np.int16)
    qtc = np.zeros((nb, 64), np.int16)
    qtc[[5, 8191, 8192], 0] = [1, -2, 300]
    from packbitsref import pack_blocks_bits
    few = pack_blocks_bits(split[[0, 5, 8191, 8192]], mv[:4], qtc[[0, 5, 8191, 8192]], 8, 0)
    assert few[0] == b"\x18"
    blk = [few[0]] * nb
    blk[5], blk[8191], blk[8192] = few[1:]
    cap = _cap_for([blk])
    offs, out, tot = _pack(gpu, [(0, split, mv, qtc)], 8, cap)
    _check_pack(offs, out, tot, [blk], cap)
    assert offs[0, 4] == 4 and offs[0, nb] > nb


def test_pack_bits_capacity_guard_edges(gpu):
    nb, k = 64, 32
    n = packbitcases.corpus("m16", 1)[0].size
    frame, blk = _frame("m16", 1, np.linspace(0, n - 1, nb).astype(int))
    o = _offsets(blk)
    total = int(o[nb])
    for cap in (0, int(o[k]) - 1, int(o[k]), int(o[k]) + 1, total - 1, total):
        offs, out, tot = _pack(gpu, [frame], 16, cap)
        _check_pack(offs, out, tot, [blk], cap)


def test_pack_bits_on_a_second_device(gpu):
    """As test_gpu_pack_edges.py test_pack_unpack_on_a_second_device, in the bits coding: 33 blocks
    of m16, two inter frames, packed and unpacked on cuda:0 and then with cuda:1 current and every
    buffer on it, each time the model's bytes and the corpus back."""
    if torch.cuda.device_count() < 2:
        pytest.skip("fewer than two devices are visible")
    nb, n = 33, packbitcases.corpus("m16", 1)[0].size
    frames, blocks = zip(*[_frame("m16", 1, (i * 37 + np.arange(nb)) % n) for i in range(2)])
    cap = _cap_for(blocks)
    for dev in (gpu, torch.device("cuda:1")):
        with torch.cuda.device(dev):
            offs, out, tot = _pack(dev, list(frames), 16, cap)
            _check_pack(offs, out, tot, blocks, cap)
            u = _Unpack(dev, [b"".join(blk) for blk in blocks], [_offsets(blk) for blk in blocks], nb, 16)
            u.launch([0, 1], [1, 1])
            _check_unpack(u.fetch(), frames)


# ---- damaged and non-canonical input: the unpacker against the strict model -------------------------
def _mutated_frames(kind, ftype):
    """[(stream, offs, {block: the model's verdict on its bytes})]: a valid frame of short corpus
    blocks (packbitcases.mutant_base) with one block damaged or rewritten; and reversed offsets."""
    bs = packbitcases.block_size(kind)
    base = packbitcases.mutant_base(kind, ftype, 12)
    o = _offsets(base)
    whole = b"".join(base)
    model = lambda data: unpack_block_bits_strict(data, bs, ftype)   # noqa: E731
    out = []
    for b, block in enumerate(base):
        for _, data in packbitcases.mutants(block, bs, ftype):
            blk = base[:b] + [data] + base[b + 1:]
            out.append((b"".join(blk), _offsets(blk), {b: model(data)}))
        if 1 <= b < len(base) - 1:
            rev = o.copy()                      # offs[b + 1] < offs[b], both inside the stream
            rev[b + 1] = rev[b] - 1
            out.append((whole, rev, {b: None, b + 1: model(whole[rev[b + 1]:rev[b + 2]])}))
    return base, out


@pytest.mark.parametrize("ftype", [0, 1])
@pytest.mark.parametrize("kind", packbitcases.KINDS)
def test_unpack_bits_agrees_with_strict_model(gpu, kind, ftype):
    """For every mutated frame: err == 1 + the block the model calls malformed (one of them
    where a call holds several), else err == 0 and the block's outputs are the model's; every
    untouched block decodes as in the valid frame.  One err word per call: the frames the
    model accepts go 32 to a call, each of which must leave err 0; a frame with a malformed
    block has a call to itself, and one last call holds several of them."""
    bs = packbitcases.block_size(kind)
    nn = bs * bs
    w = 12 if ftype == 1 else 4
    base, frames = _mutated_frames(kind, ftype)
    nb = len(base)
    assert all(len(x) <= packbitcases.SHORT for x in base)
    bad = [i for i, f in enumerate(frames) if any(v is None for v in f[2].values())]
    good = [i for i, f in enumerate(frames) if i not in set(bad)]
    assert len(bad) > 100 and len(good) > 100, (len(bad), len(good))
    clean = [good[j:j + 32] for j in range(0, len(good), 32)]
    calls = clean + [[i] for i in bad] + [bad[::len(bad) // 7]]
    u = _Unpack(gpu, [f[0] for f in frames], [f[1] for f in frames], nb, bs, ncalls=len(calls))
    for c, members in enumerate(calls):
        u.launch(members, [ftype] * len(members), call=c)
    split, mv, qtc, err = u.fetch()
    for c, members in enumerate(calls):
        culprits = {b for i in members for b, v in frames[i][2].items() if v is None}
        if c < len(clean):
            assert not culprits and int(err[c]) == 0, (c, int(err[c]), [sorted(frames[i][2]) for i in members])
        else:
            assert int(err[c]) - 1 in culprits, (c, int(err[c]), sorted(culprits))
    # outputs: the valid frame's, with the touched blocks as the model has them
    valid = [unpack_block_bits_strict(x, bs, ftype) for x in base]
    ws, wm, wq = _expected_rows(ftype, np.array([v["split"] for v in valid], np.uint8),
                                np.stack([v["mv"] for v in valid]), np.stack([v["qtc"] for v in valid]))
    es, em, eq = (np.tile(x, (len(frames), 1)) for x in (ws, wm, wq))
    for i, (_, _, touched) in enumerate(frames):
        for b, v in touched.items():
            if v is None:                        # a malformed block's outputs are unspecified
                split[i, b], es[i, b] = 0, 0
                mv[i, b * w:(b + 1) * w], em[i, b * w:(b + 1) * w] = 0, 0
                qtc[i, b * nn:(b + 1) * nn], eq[i, b * nn:(b + 1) * nn] = 0, 0
            else:
                es[i, b], em[i, b * w:(b + 1) * w] = v["split"], v["mv"].reshape(-1)[:w]
                eq[i, b * nn:(b + 1) * nn] = v["qtc"]
    for name, got, want in (("split", split, es), ("mv", mv, em), ("qtc", qtc, eq)):
        wrong = np.flatnonzero((got != want).any(axis=1))
        assert wrong.size == 0, (name, wrong[:8], [sorted(frames[i][2]) for i in wrong[:8]])


# ---- the public path ---------------------------------------------------------------------------------
def _rc_kw():
    import json
    from conftest import GOLDEN
    tables = json.load(open(os.path.join(GOLDEN, "rc_schedule.json")))["tables"]
    return dict(RCFlag=1, targetBR="2 mbps", qp_rate_tables=tables)


@pytest.mark.parametrize("case", ["vbs_64x128", "cif_p_rc1"])
def test_transmit_packed_bits_then_decode(gpu, tmp_path, monkeypatch, case):
    """transmit_packed in both codings -> decode_packed_file: identical frames, equal to the
    encoder's reconstructions; the "bits" file is the smaller; a decoder of another geometry
    refuses either; an unknown coding is refused."""
    from streamoptima_amd import packedfile
    from streamoptima_amd.Encoder import Y_Video_codec
    from streamoptima_amd.decoder import decoder
    from streamoptima_amd.synth import synth_sequence
    monkeypatch.chdir(tmp_path)
    h, w, frames, vbs, kw = (64, 128, 4, True, {}) if case == "vbs_64x128" else (288, 352, 4, False, _rc_kw())
    seq = synth_sequence(frames, h, w, seed=31)
    enc = Y_Video_codec(h, w, frames, 16, 16, 4, frames, 0, 0.015, vbs, y_only_frame_arr=seq, device=gpu, **kw)
    enc.encode()
    assert [s.frame_type for s in enc._symbols] == [0] + [1] * (frames - 1)
    p1, p2 = str(tmp_path / "gop_v1.sopk"), str(tmp_path / "gop_v2.sopk")
    size1 = enc.transmit_packed(p1)
    size2 = enc.transmit_packed(p2, coding="bits")
    assert size1 == os.path.getsize(p1) and size2 == os.path.getsize(p2)
    print(case, "varint", size1, "bits", size2, round(size2 / size1, 3))
    assert 0 < size2 < size1
    with pytest.raises(ValueError):
        enc.transmit_packed(str(tmp_path / "nope.sopk"), coding="nope")
    with pytest.raises(ValueError):
        enc.engine().pack_symbols(enc._symbols, coding="nope")
    assert packedfile.read(p1, gpu)["coding"] == "varint" and packedfile.read(p2, gpu)["coding"] == "bits"
    dec = decoder(0, frames, 16, frames, h, w, 4, 1, False, 0.015, vbs, device=gpu, **kw)
    out1 = dec.decode_packed_file(p1)
    out2 = dec.decode_packed_file(p2)
    for i in range(frames):
        want = enc._symbols[i].recon.cpu().numpy()[:h, :w]
        assert (out1[i] == want).all() and (out2[i] == want).all(), i
    other = decoder(0, frames, 16, frames, h + 16, w, 4, 1, False, 0.015, vbs, device=gpu, **kw)
    for p in (p1, p2):
        with pytest.raises(ValueError):
            other.decode_packed_file(p)
