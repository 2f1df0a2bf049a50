"""so_pack_frames / so_pack_frames_ex / so_unpack_frames on edge-case symbols (tests/packcases.py),
called through ctypes on tensors made from the corpus: the packer against the plain-Python
writer (tests/packref.py pack_frame), the unpacker against the writer's bytes (not the
kernel's own) and, on damaged and non-canonical input, against the strict model of the format
(packref.unpack_block_strict).  Every output buffer starts as a sentinel and ends in a guard
region; every comparison is exact equality of bytes or integers."""
import ctypes

import numpy as np
import pytest
import torch

import packcases
from packref import unpack_block_strict

pytestmark = pytest.mark.gpu

GUARD = 4096                                     # bytes past `cap` in out; > one block's bound
TAIL = 16                                        # guard elements past every other output row
OUT_FILL, OFFS_FILL, SPLIT_FILL, I16_FILL = 0xAB, 0x5A5A5A5A, 0xEE, 0x7B7B
# one workgroup: 4 waves x 8 blocks; a wave takes two blocks per iteration, the next one prefetched
NBS = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 63, 64, 65)
NFRAMES = (1, 2, 33)                             # 33: one past a launch's 32 frames


def _lib():
    from streamoptima_amd import _lib as m
    return m.load(), m


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t if isinstance(t, int) else t.data_ptr() for t in ts])


def _dev(a, gpu):
    return torch.from_numpy(np.array(a, order="C")).to(gpu)      # a copy: corpus arrays are read-only


def _frame(kind, ftype, idx):
    """Blocks idx of a corpus as one frame -> ((ftype, split, mv, qtc), the writer's bytes per block)."""
    split, mv, qtc = packcases.corpus(kind, ftype)
    blocks = packcases.block_bytes(kind, ftype)
    return (ftype, split[idx], mv[idx], qtc[idx]), [blocks[i] for i in idx]


def _varied_frames(kind, nframes, nb):
    """nframes frames of nb blocks: different content, frame types mixed in one call."""
    n = packcases.corpus(kind, 0)[0].size
    return [_frame(kind, (i + nb) % 2, (i * 37 + 11 * nb + np.arange(nb)) % n) for i in range(nframes)]


def _pack(gpu, frames, bs, cap, ex=True):
    """so_pack_frames(_ex) on [(ftype, split, mv, qtc)] -> offs [n, nb + 1 + TAIL], out
    [n, cap + GUARD], totals [n + 2] (or None), as numpy."""
    lib, m = _lib()
    n, nb = len(frames), frames[0][1].size
    dev = [[_dev(a, gpu) for a in f[1:]] for f in frames]
    offs = torch.full((n, nb + 1 + TAIL), OFFS_FILL, dtype=torch.int32, device=gpu)
    out = torch.full((n, cap + GUARD), OUT_FILL, dtype=torch.uint8, device=gpu)
    tot = torch.full((n + 2,), OFFS_FILL, dtype=torch.int32, device=gpu)
    args = [n, (ctypes.c_int32 * n)(*[f[0] for f in frames]), _ptrs([d[0] for d in dev]), _ptrs([d[1] for d in dev]),
            _ptrs([d[2] for d in dev]), nb, bs, _ptrs(list(offs)), _ptrs(list(out)), cap]
    if ex:
        rc = lib.so_pack_frames_ex(*args, tot.data_ptr() + 4, m.stream_handle(gpu))
    else:
        rc = lib.so_pack_frames(*args, m.stream_handle(gpu))
    m.check(rc, "so_pack_frames")
    torch.cuda.synchronize()
    return offs.cpu().numpy(), out.cpu().numpy(), tot.cpu().numpy() if ex else None


def _check_pack(offs, out, tot, blocks, cap):
    """offs complete whatever the cap; exactly the blocks with offs[b + 1] <= cap written,
    byte-exact; the sentinel everywhere else, guards included."""
    for i, blk in enumerate(blocks):
        nb = len(blk)
        want_offs = np.concatenate(([0], np.cumsum([len(x) for x in blk])))
        assert np.array_equal(offs[i, :nb + 1], want_offs), i
        assert (offs[i, nb + 1:] == OFFS_FILL).all(), i
        fit = int(want_offs[want_offs <= cap].max())          # offsets ascend: a prefix fits
        want = np.full(out.shape[1], OUT_FILL, np.uint8)
        want[:fit] = np.frombuffer(b"".join(blk), np.uint8)[:fit]
        assert np.array_equal(out[i], want), (i, np.flatnonzero(out[i] != want)[:8])
        if tot is not None:
            assert tot[i + 1] == want_offs[-1], i
    if tot is not None:
        assert tot[0] == OFFS_FILL and tot[-1] == OFFS_FILL


def _cap_for(blocks):
    return max(sum(len(x) for x in blk) for blk in blocks) + 64


class _Unpack:
    """so_unpack_frames on streams that share one device buffer; outputs poisoned, each row
    with TAIL guard elements.  launch() is asynchronous; fetch() synchronises."""

    def __init__(self, gpu, streams, offs, nb, bs, ncalls=1):
        self.gpu, self.nb, self.bs, n = gpu, nb, bs, len(streams)
        starts = np.concatenate(([0], np.cumsum([len(s) for s in streams])))
        self.packed = _dev(np.frombuffer(b"".join(streams) + b"\x80" * 64, np.uint8), gpu)
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
        rc = lib.so_unpack_frames(n, (ctypes.c_int32 * n)(*ftypes), _ptrs([self.in_ptr[f] for f in frames]), row(0),
                                  self.nb, self.bs, row(1), row(2), row(3), self.err.data_ptr() + 4 * call,
                                  m.stream_handle(self.gpu))
        m.check(rc, "so_unpack_frames")

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
    m[:nb * w] = packcases.used_mv(split, mv).reshape(-1)
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


def _offsets(blk):
    return np.concatenate(([0], np.cumsum([len(x) for x in blk])))


# ---- the packer against the Python writer ---------------------------------------------------------
@pytest.mark.parametrize("ftype", [0, 1])
@pytest.mark.parametrize("kind", packcases.KINDS)
def test_pack_corpus_bytes_exact(gpu, kind, ftype):
    """Every corpus as one frame: bytes, offsets and the total of so_pack_frames_ex equal the
    writer's; then so_unpack_frames on the kernel's own stream returns the corpus."""
    bs = packcases.block_size(kind)
    n = packcases.corpus(kind, ftype)[0].size
    frame, blk = _frame(kind, ftype, np.arange(n))
    cap = _cap_for([blk])
    offs, out, tot = _pack(gpu, [frame], bs, cap)
    _check_pack(offs, out, tot, [blk], cap)
    offs2, out2, _ = _pack(gpu, [frame], bs, cap, ex=False)
    assert np.array_equal(offs2, offs) and np.array_equal(out2, out)
    u = _Unpack(gpu, [out[0, :int(offs[0, n])].tobytes()], offs[0, :n + 1], n, bs)
    u.launch([0], [ftype])
    _check_unpack(u.fetch(), [frame])


@pytest.mark.parametrize("nframes", NFRAMES)
@pytest.mark.parametrize("kind", packcases.KINDS)
def test_pack_block_counts_around_launch_geometry(gpu, kind, nframes):
    bs = packcases.block_size(kind)
    for nb in NBS:
        frames, blocks = zip(*_varied_frames(kind, nframes, nb))
        cap = _cap_for(blocks)
        offs, out, tot = _pack(gpu, list(frames), bs, cap)
        _check_pack(offs, out, tot, blocks, cap)


@pytest.mark.parametrize("nb", [8191, 8192, 8193, 16385])
def test_pack_scan_tile_carry(gpu, nb):
    """Block counts around the scan's 8192-count tile and past two tiles, block size 8, lengths
    that vary from block to block (331 corpus blocks, cycled), two frames in one call."""
    sel = np.linspace(0, packcases.corpus("u8", 0)[0].size - 1, 331).astype(int)
    frames, blocks = zip(*[_frame("u8", ft, sel[(np.arange(nb) + 5 * ft) % sel.size]) for ft in (1, 0)])
    assert len({len(x) for x in blocks[0][:331]}) > 20
    cap = _cap_for(blocks)
    offs, out, tot = _pack(gpu, list(frames), 8, cap)
    _check_pack(offs, out, tot, blocks, cap)


def test_pack_capacity_guard_edges(gpu):
    nb, k = 64, 32
    n = packcases.corpus("m16", 1)[0].size
    frame, blk = _frame("m16", 1, np.linspace(0, n - 1, nb).astype(int))
    o = _offsets(blk)
    total = int(o[nb])
    for cap in (0, int(o[k]) - 1, int(o[k]), int(o[k]) + 1, total - 1, total):
        offs, out, tot = _pack(gpu, [frame], 16, cap)
        _check_pack(offs, out, tot, [blk], cap)


def test_pack_unpack_on_a_second_device(gpu):
    """The scan tables belong to the code object, so they are there on every device of a process:
    33 blocks of m16, two inter frames, packed and unpacked first on cuda:0 and then, in the same
    process, with cuda:1 current and every buffer on it -- each time the writer's bytes and the
    corpus back.  (Tables filled once per process would be zero on the second device: wrong
    bytes, every index still in bounds.)"""
    if torch.cuda.device_count() < 2:
        pytest.skip("fewer than two devices are visible")
    nb, n = 33, packcases.corpus("m16", 1)[0].size
    frames, blocks = zip(*[_frame("m16", 1, (i * 37 + np.arange(nb)) % n) for i in range(2)])
    cap = _cap_for(blocks)
    for dev in (gpu, torch.device("cuda:1")):
        with torch.cuda.device(dev):
            offs, out, tot = _pack(dev, list(frames), 16, cap)
            _check_pack(offs, out, tot, blocks, cap)
            u = _Unpack(dev, [b"".join(blk) for blk in blocks], [_offsets(blk) for blk in blocks], nb, 16)
            u.launch([0, 1], [1, 1])
            _check_unpack(u.fetch(), frames)


# ---- the unpacker against the Python writer's bytes ------------------------------------------------
@pytest.mark.parametrize("nframes", NFRAMES)
@pytest.mark.parametrize("kind", packcases.KINDS)
def test_unpack_writer_bytes(gpu, kind, nframes):
    """split and qtc equal the corpus, used mv entries equal and unused ones 0, no element of
    the poisoned outputs left unwritten, none past the rows touched, err 0."""
    bs = packcases.block_size(kind)
    for nb in NBS:
        frames, blocks = zip(*_varied_frames(kind, nframes, nb))
        u = _Unpack(gpu, [b"".join(blk) for blk in blocks], [_offsets(blk) for blk in blocks], nb, bs)
        u.launch(list(range(nframes)), [f[0] for f in frames])
        _check_unpack(u.fetch(), frames)


@pytest.mark.parametrize("ftype", [0, 1])
@pytest.mark.parametrize("kind", packcases.KINDS)
def test_unpack_writer_bytes_whole_corpus(gpu, kind, ftype):
    bs = packcases.block_size(kind)
    n = packcases.corpus(kind, ftype)[0].size
    frame, blk = _frame(kind, ftype, np.arange(n))
    u = _Unpack(gpu, [b"".join(blk)], [_offsets(blk)], n, bs)
    u.launch([0], [ftype])
    _check_unpack(u.fetch(), [frame])


# ---- damaged and non-canonical input: the unpacker against the strict model -------------------------
def _mutated_frames(kind, ftype):
    """[(stream, offs, {block: the model's verdict on its bytes})]: a valid frame of corpus
    blocks (packcases.mutation_base) with one block (for a moved offset, two neighbours) damaged or rewritten.  Offsets
    always stay inside the frame's own stream."""
    bs = packcases.block_size(kind)
    base = packcases.mutation_base(kind, ftype)
    nb = len(base)
    o = _offsets(base)
    whole = b"".join(base)
    model = lambda data: unpack_block_strict(data, bs, ftype)   # noqa: E731
    out = []
    for b, block in enumerate(base):
        for _, data in packcases.mutations(block, bs, ftype, prev_byte=base[b - 1][-1]):
            blk = base[:b] + [data] + base[b + 1:]
            out.append((b"".join(blk), _offsets(blk), {b: model(data)}))
        if 1 <= b < nb - 1:
            cut = o.copy()                      # the block's last byte goes to the next block
            cut[b + 1] -= 1
            out.append((whole, cut, {b: model(block[:-1]), b + 1: model(block[-1:] + base[b + 1])}))
            rev = o.copy()                      # offs[b + 1] < offs[b], both inside the stream
            rev[b + 1] = rev[b] - 1
            out.append((whole, rev, {b: None, b + 1: model(whole[rev[b + 1]:rev[b + 2]])}))
    return base, out


@pytest.mark.parametrize("kind,ftype", [("m16", 1), ("m16", 0), ("u8", 1), ("u8", 0)])
def test_unpack_agrees_with_strict_model(gpu, kind, ftype):
    """For every mutated frame: err == 1 + the block the model calls malformed (one of them
    where a call holds several), else err == 0 and the block's outputs are the model's; every
    untouched block decodes as in the valid frame.  One err word per call: the frames the
    model accepts go 32 to a call, each of which must leave err 0; a frame with a malformed
    block has a call to itself, and one last call holds several of them."""
    bs = packcases.block_size(kind)
    nn = bs * bs
    w = 12 if ftype == 1 else 4
    base, frames = _mutated_frames(kind, ftype)
    nb = len(base)
    bad = [i for i, f in enumerate(frames) if any(v is None for v in f[2].values())]
    good = [i for i, f in enumerate(frames) if i not in set(bad)]
    assert len(bad) > 100 and len(good) > 100
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
    valid = [unpack_block_strict(x, bs, ftype) for x in base]
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
