"""so_pack_chroma_frames_after / _bits_after on the GPU: the chroma records of a frame placed
behind a base that earlier work on the stream wrote to device memory (in use: the luma stream's
length), against the plain packers (so_pack_chroma_frames / _bits), which in turn are checked
against the plain-Python model (tests/packchromaref.py).  Called through ctypes.  Every output
starts as 0xAA and ends in guard bytes that must survive; every comparison is exact."""
import ctypes
from functools import lru_cache

import numpy as np
import pytest
import torch

import packbitcases
import packchromaref as R
from streamoptima_amd.bitstream import scan_order

pytestmark = pytest.mark.gpu

FILL = 0xAA
GUARD = 2048                                     # bytes past `cap` in out; > one record's bound
TAIL = 16                                        # guard elements past every offs row
OFFS_FILL = 0x5A5A5A5A
BASES = (0, 1, 2, 3, 4093)                       # every byte alignment of a record's start, and a large one
SIZES = (1, 51, 130)                             # 16 x 16; 48 x 272: a partial last workgroup (32 records a
#                                                  workgroup); more records than the grid has waves: a wave loops
CONTENTS = ("random", "zero", "corners")
PLAIN = {"varint": "so_pack_chroma_frames", "bits": "so_pack_chroma_frames_bits"}
AFTER = {"varint": "so_pack_chroma_frames_after", "bits": "so_pack_chroma_frames_bits_after"}


def _lib():
    from streamoptima_amd import _lib as m
    return m.load(), m


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t if isinstance(t, int) else t.data_ptr()
                                         for t in ts])


@lru_cache(maxsize=None)
def _corner_records():
    """Records that hold 32767 or -32768: from the chroma corpus (packcases.scan_vectors(128)) and
    from packbitcases.extra_vectors(128), positions 0..63 U's block, 64..127 V's."""
    qu, qv = R.corpus()
    recs = [(qu[i], qv[i]) for i in range(qu.shape[0])]
    order = scan_order(8)
    for v, _ in packbitcases.extra_vectors(128):
        u, w = np.zeros(64, np.int16), np.zeros(64, np.int16)
        u[order], w[order] = np.asarray(v[:64], np.int16), np.asarray(v[64:], np.int16)
        recs.append((u, w))
    hot = [r for r in recs if max(int(np.max(r[0])), int(np.max(r[1]))) == 32767
           or min(int(np.min(r[0])), int(np.min(r[1]))) == -32768]
    assert len(hot) >= 8
    return hot


@lru_cache(maxsize=None)
def _frames(content: str, nb: int):
    """len(BASES) frames of nb records: ((qtc_u, qtc_v) int16 [nb, 64] each, ...)."""
    n = len(BASES)
    if content == "zero":
        return tuple((np.zeros((nb, 64), np.int16), np.zeros((nb, 64), np.int16)) for _ in range(n))
    if content == "corners":
        hot = _corner_records()
        pick = lambda i, j: hot[(i * 131 + j * 7) % len(hot)]   # noqa: E731
        return tuple((np.stack([pick(i, j)[0] for j in range(nb)]), np.stack([pick(i, j)[1] for j in range(nb)]))
                     for i in range(n))
    rng = np.random.default_rng(1000 + nb)
    out = []
    for i in range(n):
        q = rng.integers(-300, 301, size=(2, nb, 64)).astype(np.int16)
        q[rng.random((2, nb, 64)) < (0.2 + 0.15 * i)] = 0        # sparser frame by frame: runs of every length
        out.append((q[0], q[1]))
    return tuple(out)


@lru_cache(maxsize=None)
def _model(content: str, nb: int, coding: str):
    """The model's bytes per record, per frame."""
    return tuple(tuple(R.pack_frame(u, v, coding)) for u, v in _frames(content, nb))


@lru_cache(maxsize=None)
def _pinned_totals():
    """One page-locked int32 array for every test (an allocation stays registered for the process)."""
    from streamoptima_amd.hostmem import device_ptr, pinned_empty
    t = pinned_empty((len(BASES) + 2,), torch.int32)
    return t, device_ptr(t)


def _run(gpu, name, frames, cap, bases=None, rows=None, base_ptrs="tensor"):
    """One call of entry point `name` on the current stream -> (rc, offs, out, totals) as numpy.
    bases: one per frame, written to a device tensor by fill_ kernels enqueued right before the
    call, with no synchronisation in between (the tensor held other values until then)."""
    lib, m = _lib()
    n, nb = len(frames), frames[0][0].shape[0]
    dev = [[torch.from_numpy(np.array(a, order="C")).to(gpu) for a in f] for f in frames]
    offs = torch.full((n, nb + 1 + TAIL), OFFS_FILL, dtype=torch.int32, device=gpu)
    out = torch.full((n, (rows or cap) + GUARD), FILL, dtype=torch.uint8, device=gpu)
    tot_h, tot_d = _pinned_totals()
    tot_h.fill_(OFFS_FILL)
    args = [n, _ptrs([d[0] for d in dev]), _ptrs([d[1] for d in dev]), nb, _ptrs(list(offs)), _ptrs(list(out))]
    if bases is not None or base_ptrs != "tensor":
        base = torch.full((n,), 0x7FFFFFF0, dtype=torch.int32, device=gpu)   # a base no buffer could take
        torch.cuda.synchronize()
        for i, b in enumerate(bases or []):
            base[i:i + 1].fill_(int(b))                                      # stream-ordered before the pack
        if base_ptrs == "tensor":
            args.append(_ptrs([base[i:i + 1] for i in range(n)]))
        elif base_ptrs == "null":
            args.append(None)
        else:                                                                # one NULL entry
            args.append(_ptrs([None if i == base_ptrs else base[i:i + 1] for i in range(n)]))
    rc = getattr(lib, name)(*args, cap, tot_d + 4, m.stream_handle(gpu))
    torch.cuda.synchronize()
    return rc, offs.cpu().numpy(), out.cpu().numpy(), tot_h.numpy().copy()


def _offsets(blk):
    return np.concatenate(([0], np.cumsum([len(x) for x in blk])))


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("nb", SIZES)
@pytest.mark.parametrize("coding", R.CODINGS)
def test_records_land_behind_each_frames_base(gpu, coding, nb, content):
    """Five frames in one call, one base each.  offs equals the plain packer's; out[base : base +
    total] equals the plain packer's bytes, which equal the model's; everything before the base and
    past the end is still 0xAA; totals (page-locked host memory) hold base + total."""
    frames, model = list(_frames(content, nb)), _model(content, nb, coding)
    n = len(frames)
    totals = [sum(len(x) for x in blk) for blk in model]
    pcap = max(totals) + 64
    rc, poffs, pout, ptot = _run(gpu, PLAIN[coding], frames, pcap)
    assert rc == 0
    for i, blk in enumerate(model):                       # the plain entry points: unchanged bytes
        assert np.array_equal(poffs[i, :nb + 1], _offsets(blk)), i
        assert pout[i, :totals[i]].tobytes() == b"".join(blk), i
        assert (pout[i, totals[i]:] == FILL).all() and ptot[i + 1] == totals[i], i
    assert ptot[0] == OFFS_FILL and ptot[n + 1] == OFFS_FILL

    cap = max(BASES) + max(totals) + 64
    rc, offs, out, tot = _run(gpu, AFTER[coding], frames, cap, bases=BASES)
    assert rc == 0
    assert np.array_equal(offs, poffs)                    # relative offsets, the tail guard included
    for i, base in enumerate(BASES):
        want = np.full(out.shape[1], FILL, np.uint8)
        want[base:base + totals[i]] = pout[i, :totals[i]]
        assert np.array_equal(out[i], want), (i, base, np.flatnonzero(out[i] != want)[:8])
        assert tot[i + 1] == base + totals[i], (i, base)
    assert tot[0] == OFFS_FILL and tot[n + 1] == OFFS_FILL


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("coding", R.CODINGS)
def test_capacity_counts_from_the_base(gpu, coding, base):
    """cap == base + total: everything is written.  cap == base + total - 1: the last record alone
    is missing and its bytes stay 0xAA; offs and totals are complete either way."""
    nb = 51
    frame, blk = _frames("random", nb)[1], _model("random", nb, coding)[1]
    o = _offsets(blk)
    total, last = int(o[nb]), int(o[nb - 1])
    assert total > last
    data = np.frombuffer(b"".join(blk), np.uint8)
    for cap, fit in ((base + total, total), (base + total - 1, last)):
        rc, offs, out, tot = _run(gpu, AFTER[coding], [frame], cap, bases=[base], rows=base + total + 64)
        assert rc == 0
        assert np.array_equal(offs[0, :nb + 1], o) and (offs[0, nb + 1:] == OFFS_FILL).all()
        want = np.full(out.shape[1], FILL, np.uint8)
        want[base:base + fit] = data[:fit]
        assert np.array_equal(out[0], want), (cap, np.flatnonzero(out[0] != want)[:8])
        assert tot[1] == base + total and tot[0] == OFFS_FILL and tot[2] == OFFS_FILL


@pytest.mark.parametrize("coding", R.CODINGS)
def test_null_base_is_invalid_and_launches_nothing(gpu, coding):
    lib, m = _lib()
    frames = list(_frames("random", 51))[:2]
    for base_ptrs in ("null", 1):
        rc, offs, out, tot = _run(gpu, AFTER[coding], frames, 51 * R.BOUND[coding], bases=[0, 0],
                                  base_ptrs=base_ptrs)
        assert rc == m.SO_E_INVALID
        assert b"base" in lib.so_last_error()
        assert (offs == OFFS_FILL).all() and (out == FILL).all() and (tot == OFFS_FILL).all()


def test_engine_packs_chroma_behind_luma(gpu):
    """Engine.pack_chroma_symbols(after=) in both codings: one row per frame holds pack_symbols'
    bytes, then the bytes pack_chroma_symbols gives on its own; the totals hold the combined
    length; bad arguments are refused on the host."""
    from streamoptima_amd.engine import ChromaSymbols, Engine
    eng = Engine(48, 272, 16, 16, False, 0.0, gpu)
    nb, n = eng.nb, 3
    assert nb == 51
    rng = np.random.default_rng(5)
    syms = []
    for i in range(n):
        s = eng.new_symbols(i % 2)
        s.split.zero_()
        s.mv.copy_(torch.from_numpy(rng.integers(-16, 17, size=tuple(s.mv.shape)).astype(np.int16)))
        q = rng.integers(-40, 41, size=(nb, 256)).astype(np.int16)
        q[rng.random((nb, 256)) < 0.8] = 0
        s.qtc.copy_(torch.from_numpy(q))
        syms.append(s)
    csyms = [ChromaSymbols(0, torch.from_numpy(u.copy()).to(gpu), torch.from_numpy(v.copy()).to(gpu), None, None)
             for u, v in _frames("random", nb)[:n]]
    for coding in R.CODINGS:
        loffs, lout = eng.pack_symbols(syms, coding=coding)
        coffs, cout = eng.pack_chroma_symbols(csyms, coding=coding)
        cap = eng.pack_bound(coding=coding) + eng.pack_chroma_bound(coding)
        row = torch.full((n, cap + GUARD), FILL, dtype=torch.uint8, device=gpu)
        offs, _ = eng.pack_symbols(syms, out=row[:, :cap], coding=coding)
        tot = torch.zeros(n, dtype=torch.int32, device=gpu)
        coffs2, out2 = eng.pack_chroma_symbols(csyms, out=row[:, :cap], totals=tot, coding=coding, after=offs)
        assert out2.data_ptr() == row.data_ptr() and torch.equal(coffs2, coffs) and torch.equal(offs, loffs)
        for i in range(n):
            nl, nc = int(loffs[i, nb]), int(coffs[i, nb])
            assert int(tot[i]) == nl + nc
            assert torch.equal(row[i, :nl], lout[i, :nl]) and torch.equal(row[i, nl:nl + nc], cout[i, :nc])
            assert (row[i, nl + nc:] == FILL).all()
        with pytest.raises(ValueError):                   # out is required, with room for both streams
            eng.pack_chroma_symbols(csyms, coding=coding, after=offs)
        with pytest.raises(ValueError):
            eng.pack_chroma_symbols(csyms, out=row[:, :eng.pack_bound(coding=coding)], coding=coding, after=offs)
        with pytest.raises(ValueError):
            eng.pack_chroma_symbols(csyms, out=row[:, :cap], coding=coding, after=offs.to(torch.int64))
        with pytest.raises(ValueError):
            eng.pack_chroma_symbols(csyms, out=row[:, :cap], coding=coding, after=offs[:, :nb])
        with pytest.raises(ValueError):
            eng.pack_chroma_symbols(csyms, out=row[:, :cap], coding=coding, after=offs.cpu())
