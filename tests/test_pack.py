"""Packed symbol stream, host side: the decoder (bitstream.varints / unpack_frame) against the
plain-Python writer in tests/packref.py, so_pack_bound, the edge-case corpus of
tests/packcases.py and the strict model of the format (packref.unpack_block_strict) against
the writer and against bitstream.unpack_frame (no GPU needed)."""
import numpy as np
import pytest

import packcases
import packref
from packref import pack_frame, random_symbols, rle_reference_loop, unpack_block_strict, varint, varint_padded
from streamoptima_amd import bitstream


def test_varint_known_vectors():
    assert varint(0) == b"\x00" and varint(-1) == b"\x01" and varint(1) == b"\x02"
    assert varint(63) == b"\x7e" and varint(-64) == b"\x7f" and varint(64) == b"\x80\x01"
    assert varint(-32768) == b"\xff\xff\x03"
    vals = [0, -1, 1, 63, -64, 64, 255, -256, 32767, -32768]
    buf = np.frombuffer(b"".join(varint(v) for v in vals), np.uint8)
    assert bitstream.varints(buf).tolist() == vals
    with pytest.raises(ValueError):
        bitstream.varints(np.frombuffer(b"\x80", np.uint8))


def test_rle_restatement_matches_package_tokens():
    rng = np.random.default_rng(3)
    for n in (16, 8):
        for _ in range(50):
            blk = np.where(rng.random((n, n)) < rng.random(), rng.integers(-9, 10, (n, n)), 0)
            assert rle_reference_loop(blk, n) == [int(x) for x in bitstream.entropy_encoder_block(blk, n)]


@pytest.mark.parametrize("bs,ftype,vbs", [(16, 1, False), (16, 1, True), (16, 0, True), (8, 1, False), (8, 0, False)])
def test_pack_unpack_round_trip(bs, ftype, vbs):
    rng = np.random.default_rng(bs * 10 + ftype + vbs)
    nb = 60
    split, mv, qtc = random_symbols(rng, nb, bs, ftype, vbs)
    buf = np.frombuffer(pack_frame(split, mv, qtc, bs, ftype), np.uint8)
    got = bitstream.unpack_frame(buf, nb, bs, ftype)
    assert np.array_equal(got["split"], split)
    assert np.array_equal(got["qtc"], qtc)
    for b in range(nb):
        k = 4 if split[b] else 1
        assert np.array_equal(got["mv"][b, :k], mv[b, :k])
    with pytest.raises(ValueError):
        bitstream.unpack_frame(buf[:-1], nb, bs, ftype)
    with pytest.raises(ValueError):
        bitstream.unpack_frame(np.concatenate([buf, [0]]).astype(np.uint8), nb, bs, ftype)


def test_pack_bound_covers_worst_case():
    from streamoptima_amd import _lib
    lib = _lib.load()
    for bs in (16, 8):
        nn = bs * bs
        assert lib.so_pack_bound(7, bs) == 7 * (1 + 36 + 3 * (nn + nn // 2 + 4))
        # the longest token list: alternating non-zero / zero, every value an int16 extreme
        blk = np.zeros(nn, np.int16)
        blk[::2] = -32768
        order = bitstream.scan_order(bs)
        dense = np.zeros(nn, np.int16)
        dense[order] = blk
        split = np.zeros(1, np.uint8)
        mv = np.full((1, 4, 3), -32768, np.int16)
        worst = len(pack_frame(split, mv, dense[None], bs, 1))
        assert worst <= lib.so_pack_bound(1, bs)
    assert lib.so_pack_bound(0, 16) == 0 and lib.so_pack_bound(10, 12) == 0


def test_packed_container_read(tmp_path):
    """packedfile.read on a container written by hand from the plain-Python packer: block
    offsets from the u16 lengths, per-row QPs, and the checks on malformed files."""
    import struct

    import torch
    from streamoptima_amd import packedfile
    rng = np.random.default_rng(9)
    nb, bs = 12, 16
    frames = []
    for ft in (0, 1):
        split, mv, qtc = random_symbols(rng, nb, bs, ft, vbs=True)
        blocks = [pack_frame(split[b:b + 1], mv[b:b + 1], qtc[b:b + 1], bs, ft) for b in range(nb)]
        frames.append((ft, blocks, split, qtc))
    path = tmp_path / "x.sopk"

    def write(extra=b"", fudge=0):
        with open(path, "wb") as f:
            f.write(b"SOPK" + struct.pack("<6I", 1, 64, 48, bs, len(frames), nb))
            for ft, blocks, _, _ in frames:
                q = [3, 4, 5, 6] if ft == 1 else []
                body = b"".join(blocks)
                lens = np.array([len(x) for x in blocks], np.uint16)
                f.write(struct.pack("<BH", ft, len(q)) + np.array(q, np.int8).tobytes()
                        + struct.pack("<I", len(body) + fudge) + lens.tobytes() + body)
            f.write(extra)
    write()
    m = packedfile.read(str(path), torch.device("cpu"))
    assert (m["h"], m["w"], m["bs"], m["nb"], m["frame_types"]) == (64, 48, bs, nb, [0, 1])
    assert m["qp_rows"] == [[], [3, 4, 5, 6]]
    for (ft, blocks, split, qtc), pk, off in zip(frames, m["packed"], m["offs"]):
        assert off.tolist() == np.concatenate(([0], np.cumsum([len(x) for x in blocks]))).tolist()
        got = bitstream.unpack_frame(pk.numpy(), nb, bs, ft)
        assert np.array_equal(got["split"], split) and np.array_equal(got["qtc"], qtc)
    write(extra=b"\x00")
    with pytest.raises(ValueError):
        packedfile.read(str(path), torch.device("cpu"))
    write(fudge=1)
    with pytest.raises(ValueError):
        packedfile.read(str(path), torch.device("cpu"))


# ---- the strict model, the edge-case corpus and the host decoder against both -------------------
def test_strict_model_known_vectors():
    z = lambda *nums: b"".join(varint(x) for x in nums)   # noqa: E731
    ok = unpack_block_strict(z(0, 5, -2, 7, 3, 0), 8, 0)
    assert ok["split"] == 0 and ok["mv"].tolist() == [5, 0, 0, 0]
    assert ok["qtc"][:3].tolist() == [7, 3, 0] and np.count_nonzero(ok["qtc"]) == 2
    # accepted, not canonical: an over-long varint, a 0 inside a list, the last run as Z
    assert unpack_block_strict(z(0, 5) + varint_padded(0, 5), 8, 0) is not None
    assert unpack_block_strict(z(0, 5, -2, 0, 4, 0), 8, 0)["qtc"][1] == 4
    assert not unpack_block_strict(z(0, 5, 64), 8, 0)["qtc"].any()
    assert unpack_block_strict(z(0, 5, 63, -1, 9), 8, 0)["qtc"][63] == 9
    # malformed
    for bad in (z(0, 5) + varint_padded(0, 6), z(0, 5, 65), z(0, 0, 100), z(0, 5, 63, -2, 1, 1), z(0, 5, -65),
                z(2, 5, 0), z(1, 5, 5, 5, 5, 0, 0, 0, 0), z(-1, 5, 0), z(0, 32768, 0), z(0, -32769, 0),
                z(0, 5, -1, 40000, 0), z(0, 5, -1, 2 ** 31, 0), z(0, 5, 2 ** 32 + 3, 0), z(0, 5, 0, 0), z(0, 5),
                z(0, 5, -1), z(0, 5, 0)[:-1] + b"\x80", b""):
        assert unpack_block_strict(bad, 8, 0) is None, bad
    sp = unpack_block_strict(z(1, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 0, -1, 5, 0, 0, 64), 16, 1)
    assert sp["split"] == 1 and sp["mv"].tolist() == [[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]]
    assert sp["qtc"][64] == 5 and np.count_nonzero(sp["qtc"]) == 1


def _runs(vec, seg):
    """(first, last) scan positions of every maximal run inside each segment of vec."""
    for s0 in range(0, vec.size, seg):
        nz = vec[s0:s0 + seg] != 0
        cut = np.flatnonzero(nz[1:] != nz[:-1]) + 1
        for a, e in zip(np.concatenate(([0], cut)), np.concatenate((cut, [seg]))):
            yield s0 + int(a), s0 + int(e) - 1


@pytest.mark.parametrize("ftype", [0, 1])
@pytest.mark.parametrize("kind", packcases.KINDS)
def test_corpus_teeth(kind, ftype):
    """What makes the corpus worth packing: every varint length in every role that can have
    it, every scan position first and last of a run, the largest block, and the writer's
    bytes decoding back to the corpus under the strict model."""
    from streamoptima_amd import _lib
    split, mv, qtc = packcases.corpus(kind, ftype)
    bs = packcases.block_size(kind)
    nn = bs * bs
    blocks = packcases.block_bytes(kind, ftype)
    want_mv = packcases.used_mv(split, mv)
    assert kind == "s16" or (mv[split == 0, 1:] != 0).any()   # unused entries the packer must ignore
    lens = {"split": set(), "mv": set(), "token": set(), "coef": set()}
    first, last, tokens = set(), set(), set()
    for b, data in enumerate(blocks):
        got = unpack_block_strict(data, bs, ftype)
        assert got is not None, b
        assert got["split"] == split[b] and np.array_equal(got["mv"], want_mv[b]), b
        assert np.array_equal(got["qtc"], qtc[b]), b
        for role, s, e, val, k, n in packref.block_layout(data, bs, ftype):
            lens[role].add(e - s)
            if role == "token":
                tokens.add(val)
        vec = qtc[b][packcases.placement(bs, bool(split[b]))]
        for a, e in _runs(vec, 64 if split[b] else nn):
            first.add(a)
            last.add(e)
    assert lens["mv"] == {1, 2, 3} and lens["coef"] == {1, 2, 3} and lens["split"] == {1}
    assert lens["token"] == ({1, 2} if kind in ("u16", "m16") else {1})   # |token| <= 64 fits a byte
    assert first == set(range(nn)) and last == set(range(nn))
    assert {-64, 63} <= tokens and (kind in ("s16", "u8") or {64, -65} <= tokens)
    bound = _lib.load().so_pack_bound(1, bs)
    assert max(map(len, blocks)) <= bound
    if kind in ("s16", "m16") and ftype == 1:
        assert max(map(len, blocks)) > 800
    if kind == "m16":
        assert 0 < int(split.sum()) < split.size
    assert {int(x) for x in np.unique(qtc)} >= set(packcases.VALUES)
    for c in range(mv[0].size):                    # dx, dy and the ref slot of every sub-block
        assert {int(x) for x in np.unique(mv.reshape(split.size, -1)[:, c])} >= set(packcases.VALUES)
    whole = pack_frame(split, mv, qtc, bs, ftype)
    assert whole == b"".join(blocks)
    got = bitstream.unpack_frame(np.frombuffer(whole, np.uint8), split.size, bs, ftype)
    assert np.array_equal(got["split"], split) and np.array_equal(got["mv"], want_mv)
    assert np.array_equal(got["qtc"], qtc)


@pytest.mark.parametrize("kind,ftype", [("m16", 1), ("m16", 0), ("u8", 1), ("u8", 0)])
def test_host_decoder_agrees_with_strict_model(kind, ftype):
    """bitstream.unpack_frame on a one-block stream raises ValueError exactly when the strict
    model calls the block malformed, and returns the model's symbols otherwise."""
    bs = packcases.block_size(kind)
    base = packcases.mutation_base(kind, ftype)
    verdicts = [0, 0]
    for b, block in enumerate(base):
        for name, data in packcases.mutations(block, bs, ftype, prev_byte=base[b - 1][-1]):
            want = unpack_block_strict(data, bs, ftype)
            verdicts[want is not None] += 1
            buf = np.frombuffer(data, np.uint8)
            if want is None:
                with pytest.raises(ValueError):
                    bitstream.unpack_frame(buf, 1, bs, ftype)
                continue
            got = bitstream.unpack_frame(buf, 1, bs, ftype)
            assert got["split"][0] == want["split"], (b, name)
            assert np.array_equal(got["mv"][0], want["mv"]) and np.array_equal(got["qtc"][0], want["qtc"]), (b, name)
    assert min(verdicts) > 100, verdicts             # both verdicts are exercised


def test_host_decoder_issue_cases():
    """The inputs the two decoders used to disagree on."""
    z = lambda *nums: np.frombuffer(b"".join(varint(x) for x in nums), np.uint8)   # noqa: E731
    for buf, bs in ((z(0, 0, 100), 8), (z(2, 0, 0), 16), (z(1, 0, 0, 0, 0, 0, 0, 0, 0), 8), (z(-1, 0, 0), 16),
                    (z(0, 40000, 0), 16), (z(0, 0, -1, 40000), 16), (z(0, 0, -1, -32769), 16),
                    (z(0, 0, -3, 1), 16), (z(0, 0, -300, 1), 16)):
        with pytest.raises(ValueError):
            bitstream.unpack_frame(buf, 1, bs, 0)
    with pytest.raises(ValueError):
        bitstream.unpack_frame(np.frombuffer(varint(0) * 2 + varint_padded(0, 6), np.uint8), 1, 16, 0)
    ok = bitstream.unpack_frame(np.frombuffer(varint(0) * 2 + varint_padded(0, 5), np.uint8), 1, 16, 0)
    assert not ok["qtc"].any()
