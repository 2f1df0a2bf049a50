"""so_pack_chroma_frames_huff / _huff_after / so_unpack_chroma_frames_huff on the GPU against the
plain-Python model of the "huff" coding (tests/packhuffref.py), on the chroma corpus
(tests/packchromaref.py): bytes and offsets exact, the _after variant's placement and combined
totals, the capacity guard, per-frame tables, and the strict decoder's verdicts
(tests/packhuffcases.py).  Called through ctypes; every output starts as a sentinel and ends in
guard bytes that must survive; every comparison is exact."""
import ctypes
from functools import lru_cache

import numpy as np
import pytest
import torch

import packchromaref as R
import packhuffcases as C
import packhuffref as H

pytestmark = pytest.mark.gpu

FILL, OFFS_FILL, I16_FILL = 0xAA, 0x5A5A5A5A, 0x7B7B
GUARD, TAIL = 2048, 16
NBS = (1, 2, 63, 64, 65, 257)


def _lib():
    from streamoptima_amd import _lib as m
    return m.load(), m


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t if isinstance(t, int) else t.data_ptr() for t in ts])


@lru_cache(maxsize=None)
def _frame(first: int, nb: int):
    """nb records of the corpus from `first` on (wrapping) -> ((qtc_u, qtc_v), the model's bytes)."""
    qu, qv = R.corpus()
    i = (first + np.arange(nb)) % qu.shape[0]
    return (qu[i], qv[i]), tuple(H.pack_chroma_records_huff(qu[i], qv[i]))


def _offsets(blk):
    return np.concatenate(([0], np.cumsum([len(x) for x in blk])))


def _pack(gpu, frames, cap, bases=None, width=None):
    """so_pack_chroma_frames_huff (bases: _huff_after, the bases written by kernels enqueued right
    before the call) -> offs, out, totals as numpy."""
    lib, m = _lib()
    n, nb = len(frames), frames[0][0].shape[0]
    dev = [[torch.from_numpy(np.array(a, order="C")).to(gpu) for a in f] for f in frames]
    offs = torch.full((n, nb + 1 + TAIL), OFFS_FILL, dtype=torch.int32, device=gpu)
    out = torch.full((n, (width or cap) + GUARD), FILL, dtype=torch.uint8, device=gpu)
    tot = torch.full((n + 2,), OFFS_FILL, dtype=torch.int32, device=gpu)
    args = [n, _ptrs([d[0] for d in dev]), _ptrs([d[1] for d in dev]), nb, _ptrs(list(offs)), _ptrs(list(out))]
    name = "so_pack_chroma_frames_huff"
    if bases is not None:
        base = torch.full((n,), 0x7FFFFFF0, dtype=torch.int32, device=gpu)
        torch.cuda.synchronize()
        for i, b in enumerate(bases):
            base[i:i + 1].fill_(int(b))
        args.append(_ptrs([base[i:i + 1] for i in range(n)]))
        name += "_after"
    rc = getattr(lib, name)(*args, cap, tot.data_ptr() + 4, m.stream_handle(gpu))
    m.check(rc, name)
    torch.cuda.synchronize()
    return offs.cpu().numpy(), out.cpu().numpy(), tot.cpu().numpy()


def _check_pack(offs, out, tot, blocks, cap, bases=None):
    for i, blk in enumerate(blocks):
        nb, base = len(blk), 0 if bases is None else bases[i]
        want_offs = _offsets(blk)
        assert np.array_equal(offs[i, :nb + 1], want_offs), (i, np.flatnonzero(offs[i, :nb + 1] != want_offs)[:8])
        assert (offs[i, nb + 1:] == OFFS_FILL).all(), i
        room = want_offs[base + want_offs <= cap]
        fit = int(room.max()) if room.size else 0
        want = np.full(out.shape[1], FILL, np.uint8)
        if base + want_offs[1] <= cap:
            want[base:base + fit] = np.frombuffer(b"".join(blk), np.uint8)[:fit]
        assert np.array_equal(out[i], want), (i, np.flatnonzero(out[i] != want)[:8])
        assert tot[i + 1] == base + want_offs[-1], i
    assert tot[0] == OFFS_FILL and tot[-1] == OFFS_FILL


def _unpack(gpu, streams, offs, nb, ncalls=None):
    """so_unpack_chroma_frames_huff, one call for all frames (ncalls: one call and err word per
    frame) -> q int16 [n, 2, nb * 64 + TAIL], err."""
    lib, m = _lib()
    n = len(streams)
    starts = np.concatenate(([0], np.cumsum([len(s) for s in streams])))
    packed = torch.from_numpy(np.frombuffer(b"".join(streams) + b"\xff" * 64, np.uint8).copy()).to(gpu)
    o = torch.from_numpy(np.asarray(offs, np.int32).reshape(n, nb + 1)).to(gpu)
    q = torch.full((n, 2, nb * 64 + TAIL), I16_FILL, dtype=torch.int16, device=gpu)
    err = torch.zeros(ncalls or 1, dtype=torch.int32, device=gpu)
    groups = [[i] for i in range(n)] if ncalls else [list(range(n))]
    for c, g in enumerate(groups):
        rc = lib.so_unpack_chroma_frames_huff(len(g), _ptrs([packed.data_ptr() + int(starts[i]) for i in g]),
                                              _ptrs([o[i] for i in g]), nb, _ptrs([q[i, 0] for i in g]),
                                              _ptrs([q[i, 1] for i in g]), err.data_ptr() + 4 * c, m.stream_handle(gpu))
        m.check(rc, "so_unpack_chroma_frames_huff")
    torch.cuda.synchronize()
    return q.cpu().numpy(), err.cpu().numpy()


def _check_unpack(q, frames):
    for i, (qu, qv) in enumerate(frames):
        for j, want in enumerate((qu, qv)):
            assert np.array_equal(q[i, j, :want.size], want.reshape(-1)), (i, j)
            assert (q[i, j, want.size:] == I16_FILL).all(), (i, j)


@pytest.mark.parametrize("nframes,nbs", [(1, NBS), (3, (2, 65))])
def test_pack_chroma_huff_bytes_exact_and_round_trip(gpu, nframes, nbs):
    """The corpus in frames of every launch geometry, 1 and 3 frames a call: the model's tables,
    bytes, offsets and totals; the unpacker inverts the kernel's stream."""
    for nb in nbs:
        frames, blocks = zip(*[_frame(5 + 97 * i + nb, nb) for i in range(nframes)])
        cap = max(sum(len(x) for x in blk) for blk in blocks) + 64
        offs, out, tot = _pack(gpu, list(frames), cap)
        _check_pack(offs, out, tot, blocks, cap)
        own = [out[i, :int(offs[i, nb])].tobytes() for i in range(nframes)]
        q, err = _unpack(gpu, own, [offs[i, :nb + 1] for i in range(nframes)], nb)
        assert err.tolist() == [0]
        _check_unpack(q, frames)


def test_pack_chroma_huff_whole_corpus(gpu):
    nb = R.corpus()[0].shape[0]
    frame, blk = _frame(0, nb)
    cap = sum(len(x) for x in blk) + 64
    offs, out, tot = _pack(gpu, [frame], cap)
    _check_pack(offs, out, tot, [blk], cap)
    q, err = _unpack(gpu, [b"".join(blk)], [_offsets(blk)], nb)
    assert err.tolist() == [0]
    _check_unpack(q, [frame])


def test_pack_chroma_huff_after_combined_offsets(gpu):
    """Three frames, a base each (every alignment of the first byte): offs stays relative, the
    records land at base + offs[b], the totals are base + offs[nb], bytes before the base untouched."""
    nb, bases = 65, (0, 3, 4093)
    frames, blocks = zip(*[_frame(11 + 41 * i, nb) for i in range(3)])
    width = max(b + sum(len(x) for x in blk) for b, blk in zip(bases, blocks)) + 64
    offs, out, tot = _pack(gpu, list(frames), width, bases=bases)
    _check_pack(offs, out, tot, blocks, width, bases=bases)
    # the capacity counts from the buffer's start: the base alone can pass it
    o = _offsets(blocks[1])
    for cap in (2, 3 + int(o[1]) - 1, 3 + int(o[1]), 3 + int(o[40]), 3 + int(o[nb]) - 1):
        offs, out, tot = _pack(gpu, [frames[1]], cap, bases=[3], width=width)
        _check_pack(offs, out, tot, [blocks[1]], cap, bases=[3])


def test_pack_chroma_huff_capacity_guard_edges(gpu):
    nb, k = 64, 32
    frame, blk = _frame(40, nb)
    o = _offsets(blk)
    for cap in (0, int(o[1]) - 1, int(o[1]), int(o[k]) - 1, int(o[k]), int(o[k]) + 1, int(o[nb]) - 1, int(o[nb])):
        offs, out, tot = _pack(gpu, [frame], cap)
        _check_pack(offs, out, tot, [blk], cap)


def test_pack_chroma_huff_tables_are_per_frame(gpu):
    nb = 65
    z = np.zeros((nb, 64), np.int16)
    rng = np.random.default_rng(11)
    noise = tuple((rng.integers(-300, 301, (nb, 64)) * (rng.random((nb, 64)) < 0.4)).astype(np.int16) for _ in range(2))
    frames = [(z, z), noise, (z, z)]
    blocks = [H.pack_chroma_records_huff(u, v) for u, v in frames]
    T = H.CHROMA_TABLE_BYTES
    assert [len(b) for b in blocks[0]] == [T + 1] + [1] * (nb - 1) and blocks[0][0][:T] != blocks[1][0][:T]
    cap = max(sum(len(x) for x in blk) for blk in blocks) + 64
    offs, out, tot = _pack(gpu, frames, cap)
    _check_pack(offs, out, tot, blocks, cap)
    q, err = _unpack(gpu, [b"".join(b) for b in blocks], [_offsets(b) for b in blocks], nb)
    assert err.tolist() == [0]
    _check_unpack(q, frames)


def test_unpack_chroma_huff_agrees_with_strict_model(gpu):
    qu, qv, cases = C.chroma_cases()
    nb = 6
    q, err = _unpack(gpu, [b"".join(r) for _, r, _ in cases], [_offsets(r) for _, r, _ in cases], nb, ncalls=len(cases))
    for c, (name, recs, bad) in enumerate(cases):
        kind, res = H.verdict(H.unpack_chroma_records_huff_strict, recs)
        assert (kind == "bad") == (bad is not None), name
        assert int(err[c]) == (0 if bad is None else bad + 1), (name, int(err[c]))
        if bad is None:
            _check_unpack(q[c:c + 1], [(qu, qv)])
        elif bad:                                   # records before and after the bad one decode as usual
            keep = np.arange(nb) != bad
            assert np.array_equal(q[c, 0, :nb * 64].reshape(nb, 64)[keep], qu[keep]), name
    # every single-bit flip of record 3's bytes: the model's verdict
    good = cases[0][1]
    muts = []
    for bit in range(8 * len(good[3])):
        raw = bytearray(good[3])
        raw[bit >> 3] ^= 0x80 >> (bit & 7)
        muts.append(list(good[:3]) + [bytes(raw)] + list(good[4:]))
    q, err = _unpack(gpu, [b"".join(r) for r in muts], [_offsets(r) for r in muts], nb, ncalls=len(muts))
    verdicts = [H.verdict(H.unpack_chroma_records_huff_strict, r) for r in muts]
    assert {k for k, _ in verdicts} == {"ok", "bad"}
    for c, (kind, res) in enumerate(verdicts):
        assert int(err[c]) == (4 if kind == "bad" else 0), (c, int(err[c]), kind)
        if kind == "ok":
            assert np.array_equal(q[c, 0, :nb * 64].reshape(nb, 64), res["qtc_u"])
            assert np.array_equal(q[c, 1, :nb * 64].reshape(nb, 64), res["qtc_v"])


def test_unpack_chroma_huff_mutant_frames_agree_with_strict_model(gpu):
    """The table mutants (frames of 7 records) and a seeded sample of record mutants (frames of one
    record) of packhuffcases.gpu_frames, one call and one err word per frame: err is 0 exactly when
    the model accepts every record, else it names a record the model rejects -- record 0 for
    malformed tables, and then nothing of the frame is written; every record the model accepts
    decodes to the model's values; guard elements stay untouched."""
    frames = C.gpu_frames(2)
    assert sum(all(v[0] == "ok" for v in f[4]) for f in frames) > 50 and sum(not f[3] for f in frames) > 50
    for nb in sorted({len(f[2]) for f in frames}):
        group = [f for f in frames if len(f[2]) == nb]
        q, err = _unpack(gpu, [b"".join(f[2]) for f in group], [_offsets(f[2]) for f in group], nb, ncalls=len(group))
        for c, (name, _, recs, tables_ok, verdicts) in enumerate(group):
            bad = {b for b, v in enumerate(verdicts) if v[0] == "bad"}
            e = int(err[c])
            assert (e == 0) == (not bad), (name, e, sorted(bad))
            assert e == 0 or e - 1 in bad, (name, e, sorted(bad))
            assert (q[c, :, nb * 64:] == I16_FILL).all(), name
            if not tables_ok:
                assert e == 1 and (q[c] == I16_FILL).all(), name
                continue
            for b, (verdict, res) in enumerate(verdicts):
                if verdict == "ok":
                    assert np.array_equal(q[c, 0, b * 64:(b + 1) * 64], res[2][:64]), (name, b)
                    assert np.array_equal(q[c, 1, b * 64:(b + 1) * 64], res[2][64:]), (name, b)
