"""The "huff" coding of the packed stream without a GPU: the plain-Python model (packhuffref.py)
round-trips the edge corpus and the goldens, is smaller than the "bits" coding on the CIF goldens,
keeps code lengths within 15 bits, rejects every malformed rule, and bitstream.unpack_frame_huff /
unpack_chroma_frame_huff agree with its strict decoder."""
import struct

import numpy as np
import pytest

import packbitcases
import packchromaref as R
import packhuffcases as C
import packhuffref as H
from conftest import golden
from packbitsref import pack_frame_bits
from streamoptima_amd import bitstream

GOLDENS = (("cif_p_vbs0", 1), ("cif_i_qp6_vbs0", 0), ("cif_p_vbs1", 1), ("i_64x128_vbs1", 0))


def _u8(data) -> np.ndarray:
    return np.frombuffer(bytes(data), np.uint8)


def _same_luma(got, split, mv, qtc):
    return (np.array_equal(got["split"], split) and np.array_equal(got["qtc"], qtc)
            and np.array_equal(got["mv"], packbitcases.used_mv(split, mv)))


def _round_trip(split, mv, qtc, bs, ft):
    blocks = H.pack_blocks_huff(split, mv, qtc, bs, ft)
    assert _same_luma(H.unpack_blocks_huff_strict(blocks, bs, ft), split, mv, qtc)
    assert _same_luma(bitstream.unpack_frame_huff(_u8(b"".join(blocks)), split.size, bs, ft), split, mv, qtc)
    return blocks


def test_value_mapping_known_vectors():
    assert [H.symbol(v) for v in (0, -1, 15, -16)] == [(0, ""), (1, ""), (30, ""), (31, "")]
    assert H.symbol(16) == (32, "00000") and H.symbol(-32) == (32, "11111")       # z = 32, 63: n = 6
    assert H.symbol(32) == (33, "000000")                                         # z = 64: n = 7
    assert H.symbol(-32768) == (42, "1" * 15) and H.symbol(32767) == (42, "1" * 14 + "0")
    assert [H.cls(p) for p in (0, 1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 255)] == [0, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6]
    # canonical codes: by (length, symbol)
    lens = [0] * 43
    lens[0], lens[5], lens[7], lens[42] = 2, 1, 3, 3
    assert H.canonical_codes(lens) == {5: "0", 0: "10", 7: "110", 42: "111"}


def test_huffman_lengths_rule():
    c = [0] * 43
    assert H.huffman_lengths(c) == [0] * 43
    c[9] = 5
    assert H.huffman_lengths(c) == [0] * 9 + [1] + [0] * 33                       # one used symbol: length 1
    c[3] = 5
    assert H.huffman_lengths(c)[3] == 1 and H.huffman_lengths(c)[9] == 1
    # ties by (weight, node number): 1, 1, 2 -> leaves 0 and 1 merge first (node 43, weight 2); then
    # the two smallest of {2: (2, 2), 43: (2, 43)} are merged
    assert H.huffman_lengths([1, 1, 2] + [0] * 40)[:3] == [2, 2, 1]
    # all four equal: (0, 1) -> 43, (2, 3) -> 44
    assert H.huffman_lengths([7, 7, 7, 7] + [0] * 39)[:4] == [2, 2, 2, 2]


def test_length_limit_on_fibonacci_counts(monkeypatch):
    """Fibonacci-like counts force a Huffman depth above 15; the rule halves the counts until the
    lengths fit, the result is a prefix code, and a frame with such statistics round-trips."""
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    counts = fib + [0] * 13
    lens = H.huffman_lengths(counts)
    assert max(lens) <= 15
    assert all((n > 0) == (c > 0) for n, c in zip(lens, counts))
    assert H.kraft(lens) <= 1 << 15
    assert len(set(H.canonical_codes(lens).values())) == 30
    # a frame whose coefficients at scan positions 32..255 (table coef6) are symbol s + 1 fib[s]
    # times, s < 22, shuffled, the most frequent one filling the last block; positions 0..31 hold 1
    import packcases
    vals = [H.unzz(s + 1) for s in range(22) for _ in range(fib[s])]
    vals += [H.unzz(22)] * (-len(vals) % 224)
    np.random.default_rng(1).shuffle(vals)
    nb = len(vals) // 224
    scan = np.ones((nb, 256), np.int16)
    scan[:, 32:] = np.array(vals, np.int16).reshape(nb, 224)
    qtc = np.zeros((nb, 256), np.int16)
    qtc[:, packcases.placement(16, False)] = scan
    split, mv = np.zeros(nb, np.uint8), np.zeros((nb, 4, 3), np.int16)
    blocks = _round_trip(split, mv, qtc, 16, 1)
    tables = H.parse_tables(blocks[0], 15)
    assert 0 < max(tables[14]) <= 15
    monkeypatch.setattr(H, "MAXLEN", 99)
    assert max(H.huffman_lengths([0] + fib[:21] + [fib[21] + nb * 224 - sum(fib[:22])] + [0] * 20)) == 21   # the limit did bind


def test_huffman_rounds_counts_the_halvings():
    fib = list(C.FIB)
    for scale, rounds in ((1, 1), (2, 2), (4, 3)):
        counts = [scale * c for c in fib] + [0] * 26
        lens, got = H.huffman_rounds(counts)
        assert got == rounds and lens == H.huffman_lengths(counts) == H.huffman_lengths(H.halved(counts, rounds))
        assert H.huffman_rounds(H.halved(counts, rounds - 1))[1] == 1      # no round fewer would do
    assert H.huffman_rounds(fib[:16] + [0] * 27) == (H.huffman_lengths(fib[:16] + [0] * 27), 0)
    assert max(H.huffman_lengths(fib[:16] + [0] * 27)) == 15
    assert H.huffman_rounds([0] * 43) == ([0] * 43, 0) and H.huffman_rounds([3] + [0] * 42) == ([1] + [0] * 42, 0)


@pytest.mark.parametrize("name", C.LIMIT_NAMES)
def test_limit_frames_design_and_round_trip(name):
    """The frames designed to bind the 15-bit limit (packhuffcases.limit_frames): what each is for holds
    by the model, and each round-trips through the model's strict decoder and the host decoder."""
    C.check_limit_design(name)
    for f, blocks in zip(C.limit_frames()[name], C.limit_model(name)):
        whole = _u8(b"".join(blocks))
        if f["kind"] == "chroma":
            got = H.unpack_chroma_records_huff_strict(blocks)
            assert np.array_equal(got["qtc_u"], f["qu"]) and np.array_equal(got["qtc_v"], f["qv"])
            got = bitstream.unpack_chroma_frame_huff(whole, len(blocks))
            assert np.array_equal(got["qtc_u"], f["qu"]) and np.array_equal(got["qtc_v"], f["qv"])
        else:
            assert _same_luma(H.unpack_blocks_huff_strict(blocks, f["bs"], f["ftype"]), f["split"], f["mv"], f["qtc"])
            got = bitstream.unpack_frame_huff(whole, len(blocks), f["bs"], f["ftype"])
            assert _same_luma(got, f["split"], f["mv"], f["qtc"])


@pytest.mark.parametrize("name,ft", GOLDENS)
def test_goldens_round_trip(name, ft):
    g = golden(name + ".npz")
    _round_trip(g["split"], g["mv"], g["qtc"], 16, ft)


@pytest.mark.parametrize("name,ft", GOLDENS[:3])
def test_huff_stream_is_smaller_than_bits_on_the_cif_goldens(name, ft):
    """The size condition: the model's total bytes, tables included, are below the "bits" model's."""
    g = golden(name + ".npz")
    huff = H.pack_frame_huff(g["split"], g["mv"], g["qtc"], 16, ft)
    bits = pack_frame_bits(g["split"], g["mv"], g["qtc"], 16, ft)
    print(name, len(bits), len(huff), round(len(huff) / len(bits), 3))
    assert len(huff) < len(bits)


@pytest.mark.parametrize("kind", packbitcases.KINDS)
@pytest.mark.parametrize("ft", [0, 1])
def test_corpus_round_trip(kind, ft):
    """Every kind of the edge corpus: the int16 extremes reach every escape symbol."""
    split, mv, qtc = packbitcases.corpus(kind, ft)
    bs = packbitcases.block_size(kind)
    blocks = _round_trip(split, mv, qtc, bs, ft)
    heads, records = H.luma_records(split, mv, qtc, bs, ft)
    assert {H.symbol(v)[0] for rec in records for _, v in rec} >= set(range(32, 43))
    assert len(blocks[0]) >= H.LUMA_TABLE_BYTES
    whole = b"".join(blocks)
    for cut in (whole[:-1], whole + b"\x00", whole[1:]):
        with pytest.raises(ValueError):
            bitstream.unpack_frame_huff(_u8(cut), split.size, bs, ft)


def test_all_zero_frame_has_single_symbol_tables():
    nb = 5
    split, mv, qtc = np.zeros(nb, np.uint8), np.zeros((nb, 4, 3), np.int16), np.zeros((nb, 256), np.int16)
    blocks = _round_trip(split, mv, qtc, 16, 1)
    tables = H.parse_tables(blocks[0], 15)
    assert tables[0] == [1] + [0] * 42 and tables[1] == [1] + [0] * 42            # mv 0 and token 0: length 1
    assert all(not any(t) for t in tables[2:])
    # split bit, 3 mv codes and one token of one bit each: 5 bits, one byte
    assert [len(b) for b in blocks] == [H.LUMA_TABLE_BYTES + 1] + [1] * (nb - 1)
    # the other bit pattern matches no code
    bad = list(blocks)
    bad[2] = b"\x40"
    assert H.verdict(H.unpack_blocks_huff_strict, bad, 16, 1) == ("bad", 2)


def test_chroma_round_trip():
    qu, qv = R.corpus()
    for lo, hi in ((0, qu.shape[0]), (5, 6), (40, 105)):
        recs = H.pack_chroma_records_huff(qu[lo:hi], qv[lo:hi])
        got = H.unpack_chroma_records_huff_strict(recs)
        assert np.array_equal(got["qtc_u"], qu[lo:hi]) and np.array_equal(got["qtc_v"], qv[lo:hi])
        got = bitstream.unpack_chroma_frame_huff(_u8(b"".join(recs)), hi - lo)
        assert np.array_equal(got["qtc_u"], qu[lo:hi]) and np.array_equal(got["qtc_v"], qv[lo:hi])
        assert len(recs[0]) >= H.CHROMA_TABLE_BYTES
    z = np.zeros((3, 64), np.int16)
    recs = H.pack_chroma_records_huff(z, z)
    assert [len(r) for r in recs] == [H.CHROMA_TABLE_BYTES + 1, 1, 1]
    got = bitstream.unpack_chroma_frame_huff(_u8(b"".join(recs)), 3)
    assert not got["qtc_u"].any() and not got["qtc_v"].any()


# ---- strict decode -----------------------------------------------------------------------------------
def test_strict_decode_rules():
    cases = C.all_cases()
    split, mv, qtc = C.small_frame()
    seen = set()
    for name, blocks, bad in cases:
        kind, res = H.verdict(H.unpack_blocks_huff_strict, blocks, 16, 1)
        if bad is None:
            assert kind == "ok" and _same_luma(res, split, mv, qtc), name
            got = bitstream.unpack_frame_huff(_u8(b"".join(blocks)), 6, 16, 1)
            assert _same_luma(got, split, mv, qtc), name
        else:
            assert (kind, res) == ("bad", bad), (name, kind, res)
            seen.add(name)
            if name in ("a byte appended", "code past the end", "empty block", "empty block 0"):
                continue        # the host decoder knows no block boundaries: checked one block at a time below
            with pytest.raises(ValueError):
                bitstream.unpack_frame_huff(_u8(b"".join(blocks)), 6, 16, 1)
    assert len(seen) == 10
    # split at block size 8: the same bytes read at bs 8
    bad, _ = C.split_at_bs8()
    assert H.verdict(H.unpack_blocks_huff_strict, bad, 8, 1) == ("bad", 0)
    with pytest.raises(ValueError):
        bitstream.unpack_frame_huff(_u8(bad[0]), 1, 8, 1)


def test_host_decoder_agrees_with_strict_model_on_one_block_frames():
    """Every single-bit flip of short one-block frames' code bytes, the last byte cut and a byte
    appended: bitstream.unpack_frame_huff raises exactly when the strict model calls it malformed."""
    split, mv, qtc = C.small_frame()
    verdicts = [0, 0]
    for b in (0, 1, 2, 5):
        for ft in (0, 1):
            m = mv[b:b + 1] if ft else mv[b:b + 1, :, 0]
            blocks = H.pack_blocks_huff(split[b:b + 1], m, qtc[b:b + 1], 16, ft)
            base, T = blocks[0], H.LUMA_TABLE_BYTES
            muts = [base[:-1], base + b"\x00", base + b"\x80"]
            for bit in list(range(8 * T, 8 * len(base))) + list(range(0, 8 * T, 37)):
                raw = bytearray(base)
                raw[bit >> 3] ^= 0x80 >> (bit & 7)
                muts.append(bytes(raw))
            for data in muts:
                kind, want = H.verdict(H.unpack_blocks_huff_strict, [data], 16, ft)
                verdicts[kind == "ok"] += 1
                if kind == "bad":
                    with pytest.raises(ValueError):
                        bitstream.unpack_frame_huff(_u8(data), 1, 16, ft)
                else:
                    got = bitstream.unpack_frame_huff(_u8(data), 1, 16, ft)
                    assert all(np.array_equal(got[k], want[k]) for k in ("split", "mv", "qtc"))
    assert min(verdicts) > 20, verdicts


def test_chroma_strict_decode_rules():
    qu, qv, cases = C.chroma_cases()
    for name, recs, bad in cases:
        kind, res = H.verdict(H.unpack_chroma_records_huff_strict, recs)
        if bad is None:
            assert kind == "ok" and np.array_equal(res["qtc_u"], qu) and np.array_equal(res["qtc_v"], qv), name
            got = bitstream.unpack_chroma_frame_huff(_u8(b"".join(recs)), 6)
            assert np.array_equal(got["qtc_u"], qu) and np.array_equal(got["qtc_v"], qv), name
        else:
            assert (kind, res) == ("bad", bad), (name, kind, res)
            if name in ("kraft above 1", "short tables", "no code matches"):
                with pytest.raises(ValueError):
                    bitstream.unpack_chroma_frame_huff(_u8(b"".join(recs)), 6)
    good = cases[0][1]
    for data in (good[0][:-1], good[0] + b"\x00"):
        assert H.verdict(H.unpack_chroma_records_huff_strict, [data] + good[1:])[0] == "bad"
        with pytest.raises(ValueError):
            bitstream.unpack_chroma_frame_huff(_u8(data), 1)


# ---- the library's host side and the container ------------------------------------------------------
def test_huff_bounds_are_the_formulas():
    from streamoptima_amd import _lib
    lib = _lib.load()
    for bs in (16, 8):
        nn = bs * bs
        per_block = -(-(1 + 12 * 30 + 30 * nn + 24 * (nn // 2 + 4)) // 8)
        for nb in (1, 7, 32400):
            assert lib.so_pack_huff_bound(nb, bs) == nb * per_block + 323
    assert lib.so_pack_huff_bound(1, 16) < 65536              # block 0's length fits the container's u16
    assert lib.so_pack_huff_bound(0, 16) == 0 and lib.so_pack_huff_bound(10, 12) == 0
    assert lib.so_pack_chroma_huff_bound(7) == 7 * 678 + 301 and lib.so_pack_chroma_huff_bound(0) == 0
    # the longest block the model can write stays inside the bound
    split, mv, qtc = packbitcases.corpus("m16", 1)
    longest = max(len(b) for b in H.pack_blocks_huff(split, mv, qtc, 16, 1)[1:])
    assert longest <= -(-(1 + 12 * 30 + 30 * 256 + 24 * 132) // 8)


def test_huff_entry_points_validate_on_the_host_like_their_bits_twins():
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

    def cpack(fn, n=1, qu=one, nb=4, offs=one):
        return fn(n, qu, one, nb, offs, one, 0, None, None)

    def cafter(fn, n=1, qu=one, nb=4, offs=one, base=one):
        return fn(n, qu, one, nb, offs, one, base, 0, None, None)

    def cunpack(fn, n=1, packed=one, nb=4, err=0x1000):
        return fn(n, packed, one, nb, one, one, err, None)
    luma = [dict(bs=12), dict(nb=0), dict(n=-1), dict(n=0), dict(types=None), dict(types=bad_ft)]
    chroma = [dict(nb=0), dict(n=-1), dict(n=0)]
    for call, a, b, cases in (
            (pack, lib.so_pack_frames_bits, lib.so_pack_frames_huff,
             luma + [dict(split=None), dict(split=null1), dict(offs=null1)]),
            (unpack, lib.so_unpack_frames_bits, lib.so_unpack_frames_huff,
             luma + [dict(packed=None), dict(packed=null1), dict(err=None)]),
            (cpack, lib.so_pack_chroma_frames_bits, lib.so_pack_chroma_frames_huff,
             chroma + [dict(qu=None), dict(qu=null1), dict(offs=null1)]),
            (cafter, lib.so_pack_chroma_frames_bits_after, lib.so_pack_chroma_frames_huff_after,
             chroma + [dict(qu=null1), dict(base=None), dict(base=null1)]),
            (cunpack, lib.so_unpack_chroma_frames_bits, lib.so_unpack_chroma_frames_huff,
             chroma + [dict(packed=None), dict(packed=null1), dict(err=None)])):
        for kw in cases:
            ra, rb = call(a, **kw), call(b, **kw)
            assert ra == rb, (kw, ra, rb)
            assert ra == (_lib.SO_OK if kw == dict(n=0) else _lib.SO_E_UNSUPPORTED if "bs" in kw else _lib.SO_E_INVALID), kw
    assert pack(lib.so_pack_frames_huff, bs=12) == _lib.SO_E_UNSUPPORTED
    assert b"so_pack_frames_huff" in lib.so_last_error()


def test_coding_helpers_and_container_version(tmp_path):
    import torch
    from streamoptima_amd import packedfile
    from streamoptima_amd.engine import Engine, pack_coding_is_bits, pack_coding_suffix
    assert [pack_coding_suffix(c) for c in ("varint", "bits", "huff")] == ["", "_bits", "_huff"]
    with pytest.raises(ValueError):
        pack_coding_suffix("nope")
    with pytest.raises(ValueError):
        pack_coding_is_bits("huff")                           # keeps its meaning: "varint" / "bits" only
    assert [Engine._coding_number(c) for c in ("varint", "bits", "huff")] == [1, 2, 3]
    assert packedfile.VERSIONS == {"varint": 1, "bits": 2, "huff": 3}
    split, mv, qtc = C.small_frame()
    blocks = H.pack_blocks_huff(split, mv, qtc, 16, 1)
    path = str(tmp_path / "x.sopk")
    frame = {"frame_type": 1, "qp_rows": [], "block_bytes": [len(b) for b in blocks], "payload": b"".join(blocks)}
    packedfile.write_frames(path, 32, 48, 16, 6, "huff", [frame])
    with open(path, "rb") as f:
        assert struct.unpack_from("<I", f.read(), 4)[0] == 3
    m = packedfile.read(path, torch.device("cpu"))
    assert m["coding"] == "huff" and m["layout"] == 0
    assert _same_luma(bitstream.unpack_frame_huff(m["packed"][0].numpy(), 6, 16, 1), split, mv, qtc)
    hdr, frames = packedfile.open_frames(path)
    assert hdr["coding"] == "huff" and len(list(frames)) == 1
    # a frame whose first block cannot hold the tables is rejected by both readers
    short = dict(frame, block_bytes=[5] + [len(b) for b in blocks[1:]], payload=b"".join(blocks)[len(blocks[0]) - 5:])
    packedfile.write_frames(path, 32, 48, 16, 6, "huff", [short])
    with pytest.raises(ValueError):
        packedfile.read(path, torch.device("cpu"))
    with pytest.raises(ValueError):
        list(packedfile.open_frames(path)[1])
