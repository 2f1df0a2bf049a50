"""The "bits" coding of the packed stream, host side (no GPU needed): the model's writer against
its strict decoder on the edge corpus (tests/packbitcases.py), bitstream.unpack_frame_bits
against the model, so_pack_bits_bound, the coding argument, the container's two versions, and
the size condition on the golden GOPs."""
import struct

import numpy as np
import pytest

import packbitcases
import packbitsref
import packcases
import packref
from conftest import golden
from packbitsref import block_bits_layout, pack_blocks_bits, pack_frame_bits, se, se_k, ue, unpack_block_bits_strict
from streamoptima_amd import bitstream


def _bits(s):
    return packbitsref.bits_to_bytes(s + "0" * (-len(s) % 8))


def test_code_known_vectors():
    assert [ue(z) for z in range(5)] == ["1", "010", "011", "00100", "00101"]
    assert se(0) == "1" and se(-1) == "010" and se(1) == "011" and se(-2) == "00100"
    assert se_k(0, 2) == "100" and se_k(-1, 1) == "11" and se_k(3, 1) == "001000"
    assert se(-32768) == "0" * 16 + "1" + "0" * 16 and len(se(32767)) == 31
    assert len(se_k(-32768, 3)) == 30
    for v in (0, 1, -1, 5, -300, 32767, -32768):
        for k in range(4):
            assert len(se_k(v, k)) == 2 * ((packbitsref.zz(v) >> k) + 1).bit_length() - 1 + k


def test_strict_model_known_vectors():
    # intra 8x8: split 0, k 0, mv 5, "-2" 7 3, "0"
    ok = unpack_block_bits_strict(_bits("0" + "00" + se(5) + se(-2) + se(7) + se(3) + se(0)), 8, 0)
    assert ok["split"] == 0 and ok["k"] == 0 and ok["mv"].tolist() == [5, 0, 0, 0]
    assert ok["qtc"][:3].tolist() == [7, 3, 0] and np.count_nonzero(ok["qtc"]) == 2
    assert _bits("0" + "00" + se(0) + se(0)) == b"\x18"          # the all-zero block: one byte
    # accepted, not canonical: another k, k != 0 with no coefficient, a 0 in a list, the last run as Z
    assert unpack_block_bits_strict(_bits("0" + "10" + se(5) + se(-2) + se_k(7, 2) + se_k(3, 2) + se(0)), 8, 0)["qtc"][0] == 7
    assert unpack_block_bits_strict(_bits("0" + "11" + se(5) + se(0)), 8, 0)["k"] == 3
    assert unpack_block_bits_strict(_bits("0" + "00" + se(5) + se(-2) + se(0) + se(4) + se(0)), 8, 0)["qtc"][1] == 4
    assert not unpack_block_bits_strict(_bits("0" + "00" + se(5) + se(64)), 8, 0)["qtc"].any()
    # malformed
    for bad in (b"", _bits("1" + "00" + se(5) * 4 + se(0) * 4),                   # split at 8x8
                _bits("0" + "00" + se(5) + se(65)), _bits("0" + "00" + se(5) + se(-65)),
                _bits("0" + "00" + se(5) + se(63) + se(-2) + se(1) + se(1)),
                _bits("0" + "00" + se(5) + "0" * 17 + "1" + "0" * 17),           # 17 prefix zeros
                _bits("0" + "00" + se(5) + "0" * 16 + "1" + "0" * 15 + "1" + se(0)),   # z = 65536
                _bits("0" + "01" + se(5) + se(-1) + "0" * 15 + "1" + "1" * 15 + "1" + se(0)),   # z = 131069 at k = 1
                _bits("0" + "00" + se(5) + se(0)) + b"\x00",                       # 8 or more bits left
                _bits("0" + "00" + se(5) + se(0) + "1"),                           # a set pad bit
                _bits("0" + "00" + se(5)), _bits("0" + "00" + se(5) + se(-1))):    # the bytes end
        assert unpack_block_bits_strict(bad, 8, 0) is None, bad
    sp = unpack_block_bits_strict(_bits("1" + "01" + "".join(se(v) for v in range(1, 13)) + se(0) + se(-1) + se_k(5, 1)
                                        + se(0) + se(0) + se(64)), 16, 1)
    assert sp["split"] == 1 and sp["mv"].tolist() == [[1, 2, 3], [4, 5, 6], [7, 8, 9], [10, 11, 12]]
    assert sp["qtc"][64] == 5 and np.count_nonzero(sp["qtc"]) == 1


@pytest.mark.parametrize("ftype", [0, 1])
@pytest.mark.parametrize("kind", packbitcases.KINDS)
def test_corpus_round_trip_and_teeth(kind, ftype):
    """The model's writer -> strict decoder returns every corpus block; and what makes the
    corpus worth packing: every code length in every role that can have it, every order k and
    exact ties, every pad length, the longest and the shortest block, every block in its bound."""
    from streamoptima_amd import _lib
    split, mv, qtc = packbitcases.corpus(kind, ftype)
    bs = packbitcases.block_size(kind)
    blocks = packbitcases.block_bytes(kind, ftype)
    want_mv = packbitcases.used_mv(split, mv)
    s0, m0, q0 = packcases.corpus(kind, ftype)
    n0 = s0.size
    assert np.array_equal(split[:n0], s0) and np.array_equal(mv[:n0], m0) and np.array_equal(qtc[:n0], q0)
    lens = {"mv": set(), "token": set(), "coef": set()}       # coef: the value's length at order 0
    longest_coef = 0
    ks, pads, ties = set(), set(), set()
    for b, data in enumerate(blocks):
        got = unpack_block_bits_strict(data, bs, ftype)
        assert got is not None, b
        assert got["split"] == split[b] and np.array_equal(got["mv"], want_mv[b]), b
        assert np.array_equal(got["qtc"], qtc[b]), b
        coefs = [int(x) for x in qtc[b] if x]
        cost = [sum(len(se_k(v, k)) for v in coefs) for k in range(4)]
        assert got["k"] == (cost.index(min(cost)) if coefs else 0), b       # minimal, ties to the smallest
        ks.add(got["k"])
        if coefs and got["k"] < 3 and cost[got["k"]] == cost[got["k"] + 1]:
            ties.add(got["k"])
        for role, s, e, val, k, n in block_bits_layout(data, bs, ftype):
            if role in lens:
                lens[role].add(len(se(val)))
                assert e - s == len(se_k(val, got["k"]) if role == "coef" else se(val))
            if role == "coef":
                longest_coef = max(longest_coef, e - s)
            if role == "pad":
                pads.add(e - s)
    odd = set(range(1, 34, 2))
    assert lens["mv"] == odd and lens["coef"] == odd - {1}                  # 1 bit: the value 0, no coefficient
    # no order-0 code beats its order-2 code, so next to a -32768 the canonical k is never 0: its
    # longest canonical code has 32 bits (k = 1); 33-bit codes are mv values, or another k (mutants)
    assert longest_coef == 32
    assert lens["token"] >= ({1, 3, 5, 7, 9, 11, 13, 15, 17, 19} if kind in ("u16", "m16") else set(range(1, 15, 2)))
    assert ks == {0, 1, 2, 3} and ties == {0, 1, 2}
    assert pads == set(range(8))
    bound = _lib.load().so_pack_bits_bound(1, bs)
    assert max(map(len, blocks)) <= bound
    if ftype == 0:
        assert min(map(len, blocks)) == (2 if kind == "s16" else 1)         # split: 3 + 4 + 4 bits
    # the longest: every coefficient (30 bits at k = 3) and every used mv value (33 bits) -32768
    nmv = {("u16", 0): 1, ("u16", 1): 3, ("u8", 0): 1, ("u8", 1): 3}.get((kind, ftype), 4 * (3 if ftype else 1))
    nlists = 1 if kind in ("u16", "u8") else 4
    tok = len(se(-(bs * bs // nlists)))
    assert max(map(len, blocks)) == -(-(3 + 33 * nmv + nlists * tok + 30 * bs * bs) // 8)
    whole = pack_frame_bits(split, mv, qtc, bs, ftype)
    assert whole == b"".join(blocks)
    got = bitstream.unpack_frame_bits(np.frombuffer(whole, np.uint8), split.size, bs, ftype)
    assert np.array_equal(got["split"], split) and np.array_equal(got["mv"], want_mv)
    assert np.array_equal(got["qtc"], qtc)
    for cut in (whole[:-1], whole + b"\x00", whole[1:]):
        with pytest.raises(ValueError):
            bitstream.unpack_frame_bits(np.frombuffer(cut, np.uint8), split.size, bs, ftype)


@pytest.mark.parametrize("kind,ftype", [("m16", 1), ("m16", 0), ("s16", 1), ("u16", 0), ("u8", 1), ("u8", 0)])
def test_host_decoder_agrees_with_strict_model(kind, ftype):
    """bitstream.unpack_frame_bits on a one-block stream raises ValueError exactly when the
    strict model calls the block malformed, and returns the model's symbols otherwise."""
    bs = packbitcases.block_size(kind)
    verdicts = [0, 0]
    for b, block in enumerate(packbitcases.mutant_base(kind, ftype)):
        for name, data in packbitcases.mutants(block, bs, ftype):
            want = unpack_block_bits_strict(data, bs, ftype)
            verdicts[want is not None] += 1
            buf = np.frombuffer(data, np.uint8)
            if want is None:
                with pytest.raises(ValueError):
                    bitstream.unpack_frame_bits(buf, 1, bs, ftype)
                continue
            got = bitstream.unpack_frame_bits(buf, 1, bs, ftype)
            assert got["split"][0] == want["split"], (b, name)
            assert np.array_equal(got["mv"][0], want["mv"]) and np.array_equal(got["qtc"][0], want["qtc"]), (b, name)
    assert min(verdicts) > 100, verdicts             # both verdicts are exercised


def test_non_canonical_k_decodes_to_the_same_symbols():
    split, mv, qtc = packbitcases.corpus("m16", 1)
    idx = np.linspace(0, split.size - 1, 40).astype(int)
    want_mv = packbitcases.used_mv(split, mv)
    for k in range(4):
        blocks = pack_blocks_bits(split[idx], mv[idx], qtc[idx], 16, 1, k=k)
        for i, data in zip(idx, blocks):
            got = unpack_block_bits_strict(data, 16, 1)
            assert got["k"] == k and np.array_equal(got["qtc"], qtc[i]) and np.array_equal(got["mv"], want_mv[i])
        got = bitstream.unpack_frame_bits(np.frombuffer(b"".join(blocks), np.uint8), idx.size, 16, 1)
        assert np.array_equal(got["qtc"], qtc[idx])


def test_pack_bits_bound_is_the_formula():
    from streamoptima_amd import _lib
    lib = _lib.load()
    for bs in (16, 8):
        nn = bs * bs
        per_block = -(-(3 + 12 * 33 + 33 * nn + 19 * (nn // 2 + 4)) // 8)
        for nb in (1, 7, 32400):
            assert lib.so_pack_bits_bound(nb, bs) == nb * per_block
    assert lib.so_pack_bits_bound(1, 16) < 65536              # a block's length fits the container's u16
    assert lib.so_pack_bits_bound(0, 16) == 0 and lib.so_pack_bits_bound(-3, 8) == 0
    assert lib.so_pack_bits_bound(10, 12) == 0 and lib.so_pack_bits_bound(10, 32) == 0


def test_bits_entry_points_validate_on_the_host_like_the_varint_ones():
    """Without a GPU: the same error codes for a bad block size, block count, frame count, null
    arrays and frame types, from both codings' entry points."""
    import ctypes
    from streamoptima_amd import _lib
    lib = _lib.load()
    one = (ctypes.c_void_p * 1)(0x1000)
    null1 = (ctypes.c_void_p * 1)(None)
    ft = (ctypes.c_int32 * 1)(1)
    bad_ft = (ctypes.c_int32 * 1)(2)

    def pack(fn, n=1, types=ft, split=one, nb=4, bs=16, offs=one):
        return fn(n, types, split, one, one, nb, bs, offs, one, 0, None, None)

    def unpack(fn, n=1, types=ft, packed=one, nb=4, bs=16, err=0x1000):
        return fn(n, types, packed, one, nb, bs, one, one, one, err, None)
    for call, a, b in ((pack, lib.so_pack_frames_ex, lib.so_pack_frames_bits),
                       (unpack, lib.so_unpack_frames, lib.so_unpack_frames_bits)):
        cases = [dict(bs=12), dict(nb=0), dict(n=-1), dict(n=0), dict(types=None), dict(types=bad_ft)]
        cases += [dict(split=None), dict(split=null1), dict(offs=null1)] if call is pack else \
                 [dict(packed=None), dict(packed=null1), dict(err=None)]
        for kw in cases:
            ra, rb = call(a, **kw), call(b, **kw)
            assert ra == rb, (kw, ra, rb)
            assert ra == (_lib.SO_OK if kw == dict(n=0) else _lib.SO_E_UNSUPPORTED if "bs" in kw else _lib.SO_E_INVALID), kw
    assert pack(lib.so_pack_frames_bits, bs=12) == _lib.SO_E_UNSUPPORTED
    assert b"so_pack_frames_bits" in lib.so_last_error()


class _NoDevice:
    """An engine stand-in that records what the container writer asks for (no GPU)."""
    h, w, bs, nb = 32, 32, 16, 4

    def __init__(self):
        self.codings = []

    def pack_symbols(self, symbols, coding="varint"):
        self.codings.append(coding)
        raise RuntimeError("no device")


def test_coding_argument_is_checked():
    from streamoptima_amd import packedfile
    from streamoptima_amd.engine import pack_coding_is_bits
    assert pack_coding_is_bits("varint") is False and pack_coding_is_bits("bits") is True
    with pytest.raises(ValueError):
        pack_coding_is_bits("nope")
    eng = _NoDevice()
    with pytest.raises(ValueError):
        packedfile.write("/nonexistent/x.sopk", eng, [], coding="nope")
    assert eng.codings == []
    for coding in ("varint", "bits"):
        with pytest.raises(RuntimeError):
            packedfile.write("/nonexistent/x.sopk", eng, [], coding=coding)
    assert eng.codings == ["varint", "bits"]


def test_container_versions(tmp_path):
    """A version-1 container written by a stub still reads, as "varint"; the same layout with
    version 2 reads as "bits" with the model's bytes intact; any other version is rejected."""
    import torch
    from streamoptima_amd import packedfile
    rng = np.random.default_rng(4)
    nb, bs = 12, 16
    split, mv, qtc = packref.random_symbols(rng, nb, bs, 1, vbs=True)
    per_coding = {1: [packref.pack_frame(split[b:b + 1], mv[b:b + 1], qtc[b:b + 1], bs, 1) for b in range(nb)],
                  2: pack_blocks_bits(split, mv, qtc, bs, 1)}
    path = tmp_path / "x.sopk"

    def write(version, blocks):
        body = b"".join(blocks)
        with open(path, "wb") as f:
            f.write(b"SOPK" + struct.pack("<6I", version, 64, 48, bs, 1, nb))
            f.write(struct.pack("<BH", 1, 2) + np.array([3, 4], np.int8).tobytes() + struct.pack("<I", len(body))
                    + np.array([len(x) for x in blocks], np.uint16).tobytes() + body)
    for version, coding, dec in ((1, "varint", bitstream.unpack_frame), (2, "bits", bitstream.unpack_frame_bits)):
        write(version, per_coding[version])
        m = packedfile.read(str(path), torch.device("cpu"))
        assert m["coding"] == coding and (m["h"], m["w"], m["bs"], m["nb"]) == (64, 48, bs, nb)
        assert m["frame_types"] == [1] and m["qp_rows"] == [[3, 4]]
        assert m["packed"][0].numpy().tobytes() == b"".join(per_coding[version])
        assert m["offs"][0].tolist() == np.concatenate(([0], np.cumsum([len(x) for x in per_coding[version]]))).tolist()
        got = dec(m["packed"][0].numpy(), nb, bs, 1)
        assert np.array_equal(got["split"], split) and np.array_equal(got["qtc"], qtc)
    for version in (0, 3, 258):
        write(version, per_coding[2])
        with pytest.raises(ValueError):
            packedfile.read(str(path), torch.device("cpu"))


@pytest.mark.parametrize("name", ["gop_cif_vbs0", "gop_fast_vbs1", "gop_small_rc2"])
def test_bits_stream_is_smaller_on_the_golden_gops(name):
    """The size condition on the format: every frame's "bits" stream from the model is strictly
    smaller than the varint writer's (measured: 0.49-0.56 of it on the two QP-4 GOPs, 0.60-0.73
    on the all-intra low-QP one)."""
    g = golden(name + ".npz")
    for i, ft in enumerate(g["frame_type"].tolist()):
        split, mv, qtc = g[f"split{i}"], g[f"mv{i}"], g[f"qtc{i}"]
        varint = packref.pack_frame(split, mv, qtc, 16, ft)
        bits = pack_frame_bits(split, mv, qtc, 16, ft)
        print(name, i, len(varint), len(bits), round(len(bits) / len(varint), 3))
        assert len(bits) < len(varint), (i, len(bits), len(varint))
        got = bitstream.unpack_frame_bits(np.frombuffer(bits, np.uint8), split.size, 16, ft)
        assert np.array_equal(got["qtc"], qtc) and np.array_equal(got["split"], split)
