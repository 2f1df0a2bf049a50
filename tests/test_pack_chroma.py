"""The packed chroma stream and container layout 1, host side (no GPU needed): the model
(tests/packchromaref.py) against itself on the corpus, bitstream.unpack_chroma_frame (_bits)
against the model on the corpus and on every mutant, the two bound functions, argument validation
of the four entry points, and packedfile's layout 1 written by hand from the model's bytes."""
import ctypes
import struct

import numpy as np
import pytest

import packchromaref as R
from streamoptima_amd import bitstream

DECODERS = {"varint": bitstream.unpack_chroma_frame, "bits": bitstream.unpack_chroma_frame_bits}


def test_known_records():
    z = np.zeros(64, np.int16)
    assert R.pack_record(z, z, "varint") == b"\x00\x00"              # the shortest varint record: two "0" tokens
    assert R.pack_record(z, z, "bits") == b"\x30"                    # k 00, se(0) se(0), four pad bits
    u = z.copy()
    u[0], u[1] = 7, -3                                               # scan positions 0 and 1
    assert R.pack_record(u, z, "varint") == bytes([3, 14, 5, 0, 0])  # -2, 7, -3, 0 | 0
    got = R.unpack_record_strict(bytes([3, 14, 5, 0, 0]), "varint")
    assert got["qtc_u"][:2].tolist() == [7, -3] and not got["qtc_v"].any() and got["notes"] == set()
    # V's list starts anew: a non-zero run over the seam is two lists
    full = np.full(64, 5, np.int16)
    assert R.pack_record(full, full, "varint") == (bytes([127]) + bytes([10]) * 64) * 2
    assert R.unpack_record_strict(b"", "varint") == "varint_end"
    assert R.unpack_record_strict(b"", "bits") == "code_end"
    assert R.unpack_record_strict(b"\x00", "varint") == "varint_end"  # U's list only
    assert R.unpack_record_strict(b"\x00\x00\x00", "varint") == "bytes_left"
    assert R.unpack_record_strict(b"\x30\x00", "bits") == "bits_left"
    assert R.unpack_record_strict(b"\x31", "bits") == "pad_set"
    assert R.unpack_record_strict(b"\x70", "bits")["notes"] == {"k_without_coef"}
    assert R.unpack_frame_strict(b"\x00\x00\x00\x00", [0, 2, 1, 4], "varint")[1] == "offs"


@pytest.mark.parametrize("coding", R.CODINGS)
def test_model_round_trip_on_the_corpus(coding):
    """pack -> strict unpack is the identity, canonical (no notes), within the bound; the host decoder
    returns the same from the records one by one and from the whole frame."""
    from streamoptima_amd import _lib
    qu, qv = R.corpus()
    n = qu.shape[0]
    assert n > 900
    assert any(not qu[i].any() and not qv[i].any() for i in range(n))            # the all-zero record
    alt = [i for i in range(n) if (qu[i] == -32768).sum() + (qv[i] == -32768).sum() == 64
           and np.count_nonzero(qu[i]) + np.count_nonzero(qv[i]) == 64]
    assert len(alt) >= 2                                                         # alternating -32768, both phases
    blocks = R.record_bytes(coding)
    ks = set()
    for i, data in enumerate(blocks):
        got = R.unpack_record_strict(data, coding)
        assert isinstance(got, dict), (i, got)
        assert np.array_equal(got["qtc_u"], qu[i]) and np.array_equal(got["qtc_v"], qv[i]), i
        assert got["notes"] == set(), (i, got["notes"])
        ks.add(got["k"])
        one = DECODERS[coding](np.frombuffer(data, np.uint8), 1)
        assert np.array_equal(one["qtc_u"][0], qu[i]) and np.array_equal(one["qtc_v"][0], qv[i]), i
    assert ks == ({None} if coding == "varint" else {0, 1, 2, 3})
    lens = [len(x) for x in blocks]
    lib = _lib.load()
    bound = (lib.so_pack_chroma_bound if coding == "varint" else lib.so_pack_chroma_bits_bound)(1)
    assert bound == R.BOUND[coding] and max(lens) <= bound
    assert min(lens) == (2 if coding == "varint" else 1)
    # the longest token stream: 32 "-1" lists and 32 runs per plane
    assert max(len(R.record_layout(blocks[i], coding)) for i in alt) >= 2 * (32 + 32 + 31)
    whole = b"".join(blocks)
    got = DECODERS[coding](np.frombuffer(whole, np.uint8), n)
    assert np.array_equal(got["qtc_u"], qu) and np.array_equal(got["qtc_v"], qv)
    for cut in (whole[:-1], whole + b"\x00"):
        with pytest.raises(ValueError):
            DECODERS[coding](np.frombuffer(cut, np.uint8), n)


@pytest.mark.parametrize("coding", R.CODINGS)
def test_mutants_reach_every_rule_and_form(coding):
    """No rule goes untested silently: the mutants hold a record malformed by every rule and an
    accepted one in every non-canonical form, as the model's codes say."""
    ms = R.mutants(coding)
    rules = {v for _, _, v in ms if isinstance(v, str)}
    forms = set().union(*(v["notes"] for _, _, v in ms if isinstance(v, dict)))
    assert rules == set(R.RULES[coding]), (sorted(set(R.RULES[coding]) - rules), sorted(rules - set(R.RULES[coding])))
    assert forms == set(R.FORMS[coding]), (sorted(set(R.FORMS[coding]) - forms), sorted(forms))
    kinds = {name.split(" ", 1)[1].split(" ")[0] for name, _, _ in ms}
    assert {"bit", "cut", "+"} <= kinds
    if coding == "varint":
        assert any("in 5 bytes" in name for name, _, _ in ms) and any("in 6 bytes" in name for name, _, _ in ms)
    accepted = sum(isinstance(v, dict) for _, _, v in ms)
    assert accepted > 100 and len(ms) - accepted > 100, (accepted, len(ms))


@pytest.mark.parametrize("coding", R.CODINGS)
def test_host_decoder_agrees_with_the_model_on_every_mutant(coding):
    for name, data, want in R.mutants(coding):
        buf = np.frombuffer(data, np.uint8)
        if isinstance(want, str):
            with pytest.raises(ValueError):
                DECODERS[coding](buf, 1)
            continue
        got = DECODERS[coding](buf, 1)
        assert np.array_equal(got["qtc_u"][0], want["qtc_u"]) and np.array_equal(got["qtc_v"][0], want["qtc_v"]), name


def test_bounds_are_the_formulas():
    from streamoptima_amd import _lib
    lib = _lib.load()
    per_varint = 2 * 3 * (64 + 32 + 4)
    per_bits = -(-(2 + 2 * (33 * 64 + 19 * 36)) // 8)
    assert (per_varint, per_bits) == (600, 700)
    for nb in (1, 7, 32400):
        assert lib.so_pack_chroma_bound(nb) == nb * per_varint
        assert lib.so_pack_chroma_bits_bound(nb) == nb * per_bits
    for nb in (0, -3):
        assert lib.so_pack_chroma_bound(nb) == 0 and lib.so_pack_chroma_bits_bound(nb) == 0
    assert per_varint < 65536 and per_bits < 65536                   # a record's length fits the container's u16


def test_entry_points_validate_on_the_host():
    """Without a GPU: SO_E_INVALID with an so_last_error text for a NULL required pointer (an array
    or one of its entries) and for nb <= 0 or a negative frame count; SO_OK for no frames; a NULL
    totals is not an error in itself (the call fails on the next argument checked)."""
    from streamoptima_amd import _lib
    lib = _lib.load()
    one = (ctypes.c_void_p * 1)(0x1000)
    null1 = (ctypes.c_void_p * 1)(None)

    def pack(fn, n=1, qu=one, qv=one, nb=4, offs=one, out=one):
        return fn(n, qu, qv, nb, offs, out, 0, None, None)

    def unpack(fn, n=1, packed=one, offs=one, nb=4, qu=one, qv=one, err=0x1000):
        return fn(n, packed, offs, nb, qu, qv, err, None)
    table = [(pack, "so_pack_chroma_frames", ("qu", "qv", "offs", "out")),
             (pack, "so_pack_chroma_frames_bits", ("qu", "qv", "offs", "out")),
             (unpack, "so_unpack_chroma_frames", ("packed", "offs", "qu", "qv")),
             (unpack, "so_unpack_chroma_frames_bits", ("packed", "offs", "qu", "qv"))]
    for call, name, arrays in table:
        fn = getattr(lib, name)
        cases = [dict(nb=0), dict(nb=-2), dict(n=-1)] + [{a: None} for a in arrays] + [{a: null1} for a in arrays]
        if call is unpack:
            cases.append(dict(err=None))
        for kw in cases:
            assert call(fn, **kw) == _lib.SO_E_INVALID, (name, kw)
            text = lib.so_last_error()
            assert name.encode() in text, (name, kw, text)
            if "nb" not in kw and "n" not in kw:
                assert b"is NULL" in text, (name, kw, text)
        assert call(fn, n=0) == _lib.SO_OK
        assert call(fn, n=0, **{arrays[0]: None}) == _lib.SO_OK      # nothing is read for no frames
        assert call(fn, n=0, nb=0) == _lib.SO_E_INVALID


# ---- the container ------------------------------------------------------------------------------------
NB, BS, H, W = 12, 16, 48, 64


def _luma(coding):
    import packref
    from packbitsref import pack_blocks_bits
    rng = np.random.default_rng(4)
    split, mv, qtc = packref.random_symbols(rng, NB, BS, 1, vbs=True)
    if coding == "varint":
        return [packref.pack_frame(split[b:b + 1], mv[b:b + 1], qtc[b:b + 1], BS, 1) for b in range(NB)]
    return pack_blocks_bits(split, mv, qtc, BS, 1)


def _section(blocks):
    body = b"".join(blocks)
    return struct.pack("<I", len(body)) + np.array([len(x) for x in blocks], np.uint16).tobytes() + body


def _layout1(coding, flags, frames, qp_offset=-2, version=None):
    """frames: [(luma blocks, qp map or None, chroma records)] -> the file's bytes, written by hand."""
    v = (1 << 16 | {"varint": 1, "bits": 2}[coding]) if version is None else version
    out = b"SOPK" + struct.pack("<6I", v, H, W, BS, len(frames), NB) + struct.pack("<Ii", flags, qp_offset)
    for luma, qmap, chroma in frames:
        out += struct.pack("<BH", 1, 2) + np.array([3, 4], np.int8).tobytes() + _section(luma)
        if flags & 2:
            out += b"\0" if qmap is None else b"\1" + np.asarray(qmap, np.uint8).tobytes()
        if flags & 1:
            out += _section(chroma)
    return out


def _offsets(blocks):
    return np.concatenate(([0], np.cumsum([len(x) for x in blocks]))).tolist()


@pytest.mark.parametrize("flags", [1, 2, 3])
@pytest.mark.parametrize("coding", R.CODINGS)
def test_layout_1_reads_back_every_field(tmp_path, coding, flags):
    import torch
    from streamoptima_amd import packedfile
    luma = _luma(coding)
    records = R.record_bytes(coding)
    chroma = [list(records[5:5 + NB]), list(records[300:300 + NB])]
    qmaps = [np.arange(NB) * 21 % 256, None]
    qmaps[0][3], qmaps[0][4] = 255, 0
    path = str(tmp_path / "x.sopk")
    with open(path, "wb") as f:
        f.write(_layout1(coding, flags, [(luma, qmaps[i], chroma[i]) for i in range(2)]))
    m = packedfile.read(path, torch.device("cpu"))
    assert (m["layout"], m["coding"], m["h"], m["w"], m["bs"], m["nb"]) == (1, coding, H, W, BS, NB)
    assert m["frame_types"] == [1, 1] and m["qp_rows"] == [[3, 4], [3, 4]]
    for i in range(2):
        assert m["packed"][i].numpy().tobytes() == b"".join(luma) and m["offs"][i].tolist() == _offsets(luma)
    if flags & 2:
        assert m["qp_maps"][0].dtype == torch.int32 and m["qp_maps"][0].tolist() == qmaps[0].tolist()
        assert m["qp_maps"][1] is None
    else:
        assert m["qp_maps"] is None
    if flags & 1:
        assert m["chroma_qp_offset"] == -2
        qu, qv = R.corpus()
        for i, first in enumerate((5, 300)):
            assert m["chroma_packed"][i].numpy().tobytes() == b"".join(chroma[i])
            assert m["chroma_offs"][i].dtype == torch.int32 and m["chroma_offs"][i].tolist() == _offsets(chroma[i])
            got = DECODERS[coding](m["chroma_packed"][i].numpy(), NB)
            assert np.array_equal(got["qtc_u"], qu[first:first + NB]) and np.array_equal(got["qtc_v"], qv[first:first + NB])
    else:
        assert m["chroma_packed"] is None and m["chroma_offs"] is None and m["chroma_qp_offset"] is None


def test_read_rejects_damaged_containers(tmp_path):
    import torch
    from streamoptima_amd import packedfile
    luma, records = _luma("bits"), list(R.record_bytes("bits")[40:40 + NB])
    good = _layout1("bits", 3, [(luma, np.arange(NB), records)])
    path = str(tmp_path / "x.sopk")

    def read(data):
        with open(path, "wb") as f:
            f.write(data)
        return packedfile.read(path, torch.device("cpu"))
    assert read(good)["layout"] == 1
    csec = len(good) - len(_section(records))                        # where the chroma section starts
    total = struct.unpack_from("<I", good, csec)[0]
    wrong_sum = good[:csec] + struct.pack("<I", total + 1) + good[csec + 4:] + b"\x00"
    one_len = csec + 4                                               # the first record's u16 length
    wrong_len = good[:one_len] + struct.pack("<H", len(records[0]) + 1) + good[one_len + 2:]
    for name, data in (("a chroma length sum above cbytes", wrong_len), ("cbytes above the length sum", wrong_sum),
                       ("trailing bytes", good + b"\x00"), ("a truncated file", good[:-1]),
                       ("an unknown flag bit", _layout1("bits", 4 | 3, [(luma, np.arange(NB), records)])),
                       ("flag bit 31", _layout1("bits", 1 << 31 | 1, [(luma, None, records)])),
                       ("layout 2", _layout1("bits", 3, [(luma, np.arange(NB), records)], version=2 << 16 | 2)),
                       ("layout 1 coding 3", _layout1("bits", 3, [(luma, np.arange(NB), records)], version=1 << 16 | 3)),
                       ("layout 1 coding 0", _layout1("bits", 3, [(luma, np.arange(NB), records)], version=1 << 16))):
        with pytest.raises(ValueError):
            read(data)
            pytest.fail(name)
    # layout 0: versions 0, 3 and 258 stay rejected, 1 and 2 stay readable with the new keys None
    body = struct.pack("<BH", 1, 0) + _section(luma)
    for version in (0, 3, 258):
        with pytest.raises(ValueError):
            read(b"SOPK" + struct.pack("<6I", version, H, W, BS, 1, NB) + body)
    m = read(b"SOPK" + struct.pack("<6I", 2, H, W, BS, 1, NB) + body)
    assert m["layout"] == 0 and m["coding"] == "bits"
    assert all(m[k] is None for k in ("qp_maps", "chroma_packed", "chroma_offs", "chroma_qp_offset"))


class _Sym:
    def __init__(self, frame_type, qp_map=None):
        self.frame_type = frame_type
        self.extra = {} if qp_map is None else {"qp_map": qp_map}


class _Chroma:
    qp_offset = 3


class _StubEngine:
    """An engine stand-in that hands the container writer the model's bytes (no GPU)."""
    h, w, bs, nb = H, W, BS, NB

    def __init__(self, coding, nframes):
        self.luma = _luma(coding)
        self.records = [list(R.record_bytes(coding)[100 * i:100 * i + NB]) for i in range(nframes)]

    @staticmethod
    def _pack(frames):
        import torch
        offs = np.array([_offsets(blocks) for blocks in frames], np.int32)
        out = np.full((len(frames), int(offs[:, -1].max()) + 8), 0xAB, np.uint8)
        for i, blocks in enumerate(frames):
            out[i, :offs[i, -1]] = np.frombuffer(b"".join(blocks), np.uint8)
        return torch.from_numpy(offs), torch.from_numpy(out)

    def pack_symbols(self, symbols, coding="varint"):
        return self._pack([self.luma] * len(symbols))

    def pack_chroma_symbols(self, csyms, coding="varint"):
        return self._pack(self.records[:len(csyms)])


@pytest.mark.parametrize("coding", R.CODINGS)
def test_write_picks_the_layout(tmp_path, coding):
    """Neither chroma nor a QP map: the bytes of the layout-0 writer (restated here).  Either of
    them: layout 1, equal to the file written by hand, and read back."""
    import torch
    from streamoptima_amd import packedfile
    eng = _StubEngine(coding, 2)
    path = str(tmp_path / "x.sopk")
    syms = [_Sym(0), _Sym(1)]
    rows = [[3, 4], []]
    size = packedfile.write(path, eng, syms, rows, coding=coding)
    want = b"SOPK" + struct.pack("<6I", {"varint": 1, "bits": 2}[coding], H, W, BS, 2, NB)
    for s, q in zip(syms, rows):
        want += struct.pack("<BH", s.frame_type, len(q)) + np.asarray(q, np.int8).tobytes() + _section(eng.luma)
    assert open(path, "rb").read() == want and size == len(want)
    qmap = torch.arange(NB, dtype=torch.int32) * 20
    with_map = [_Sym(0), _Sym(1, qmap)]
    for csyms, ss, flags in ((None, with_map, 2), ([_Chroma(), _Chroma()], syms, 1), ([_Chroma(), _Chroma()], with_map, 3)):
        size = packedfile.write(path, eng, ss, rows, coding=coding, chroma_symbols=csyms)
        data = open(path, "rb").read()
        assert size == len(data)
        assert struct.unpack_from("<I", data, 4)[0] == 1 << 16 | {"varint": 1, "bits": 2}[coding]
        assert struct.unpack_from("<Ii", data, 28) == (flags, 3 if flags & 1 else 0)
        m = packedfile.read(path, torch.device("cpu"))
        assert m["layout"] == 1 and m["frame_types"] == [0, 1] and m["qp_rows"] == rows
        assert (m["qp_maps"] is None) == (not flags & 2) and (m["chroma_packed"] is None) == (not flags & 1)
        if flags & 2:
            assert m["qp_maps"][0] is None and m["qp_maps"][1].tolist() == qmap.tolist()
        if flags & 1:
            assert [x.numpy().tobytes() for x in m["chroma_packed"]] == [b"".join(r) for r in eng.records]
            assert m["chroma_qp_offset"] == 3
    for bad in (256, -1):
        q = qmap.clone()
        q[5] = bad
        with pytest.raises(ValueError):
            packedfile.write(path, eng, [_Sym(0), _Sym(1, q)], rows, coding=coding)
    with pytest.raises(ValueError):
        packedfile.write(path, eng, syms, rows, coding=coding, chroma_symbols=[_Chroma()])


def test_facade_methods_without_gpu():
    """transmit_packed keeps refusing a chroma codec and names the new method; transmit_packed420
    refuses a luma-only one."""
    from streamoptima_amd.Encoder import Y_Video_codec
    args = dict(h_pixels=32, w_pixels=48, frames=2, block_size=16, search_range=16, Qp=4, intra_dur=8, intra_mode=0,
                y_only_frame_arr=np.zeros((2, 32, 48), np.uint8), device="cpu")
    c = Y_Video_codec(**args, chroma=True, uv_frame_arr=np.zeros((2, 2, 16, 24), np.uint8))
    with pytest.raises(NotImplementedError, match="transmit_packed420"):
        c.transmit_packed("unused.bin")
    with pytest.raises(ValueError, match="chroma"):
        Y_Video_codec(**args).transmit_packed420("unused.bin")
