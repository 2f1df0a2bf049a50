"""Host-side logic (no GPU): rate-control schedule, text bitstream, package building,
synthetic input, the numpy CPU-baseline port."""
import gzip
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden


def _codec(h, w, **kw):
    from streamoptima_amd.Encoder import Y_Video_codec
    return Y_Video_codec(h, w, 1, 16, 16, 4, 1, 0, 0.015, False, y_only_frame_arr=np.zeros((1, h, w), np.uint8),
                         **kw)


def test_rc_schedule_matches_reference():
    js = json.load(open(os.path.join(GOLDEN, "rc_schedule.json")))
    for case in js["cases"]:
        enc = _codec(case["h"], case["w"], RCFlag=1, targetBR=case["target"], qp_rate_tables=js["tables"])
        assert enc.bitrate_per_row == case["bitrate_per_row"]
        if None in case["qps"]:
            with pytest.raises(TypeError):
                enc.row_qp_schedule(case["h"] // 16)
        else:
            assert enc.row_qp_schedule(case["h"] // 16) == case["qps"]


def test_target_bitrate_units():
    assert _codec(32, 32, targetBR="3 kbps").target_bitrate == 3 * 1024
    assert _codec(32, 32, targetBR="2 mbps").target_bitrate == 2 * 1048576
    assert _codec(32, 32, targetBR="777 bps").target_bitrate == 777


def test_q_matrix_and_set_qp():
    enc = _codec(32, 32)
    q = enc.generate_Q_matrix(4, 2)
    assert q.tolist() == [[4, 4, 4, 8], [4, 4, 8, 16], [4, 8, 16, 16], [8, 16, 16, 16]]
    enc.set_Qp(0)
    assert enc.Qpm1 == 0 and enc.Qm1.shape == (8, 8)


@pytest.mark.parametrize("name,rc", [("gop_cif_vbs0", None), ("gop_cif_vbs1_rc1", 1), ("gop_small_rc2", 2)])
def test_bitstream_text_matches_reference(name, rc):
    from streamoptima_amd.bitstream import differential_encoder_frame, entropy_encoder_frame
    from streamoptima_amd.package import frame_mvs, frame_residuals
    js = json.load(gzip.open(os.path.join(GOLDEN, name + "_bitstream.json.gz"), "rt"))
    g = golden(name + ".npz")
    w = g["frames"].shape[2]
    for i, ft in enumerate(g["frame_type"].tolist()):
        host = {"frame_type": ft, "split": g[f"split{i}"], "mv": g[f"mv{i}"], "qtc": g[f"qtc{i}"]}
        line = f"{ft}|" + differential_encoder_frame(ft, frame_mvs(host, 16), g[f"qp_per_row{i}"].tolist(), rc, w / 16)
        assert line == js["mv_lines"][i]
        assert entropy_encoder_frame(frame_residuals(host, 16), 16) == js["residual_lines"][i]


def test_entropy_block_and_token_count():
    from streamoptima_amd.bitstream import entropy_encoder_block, token_count
    g = golden("dct_tokens.npz")
    for b, t in zip(g["tok_in16"][:500], g["tok16"][:500]):
        assert len(entropy_encoder_block(b.astype(np.int64), 16)) == t
        from streamoptima_amd.bitstream import scan_order
        assert token_count(b.reshape(-1)[scan_order(16)], 16) == t
    assert entropy_encoder_block(g["tok_in16"][5].astype(np.int64), 16) == g["tok_list16_first"].tolist()


def test_synth_numpy_torch_identical():
    import torch
    from streamoptima_amd.synth import synth_sequence, synth_sequence_torch
    a = synth_sequence(3, 48, 80, seed=77)
    b = synth_sequence_torch(3, 48, 80, seed=77, device="cpu").numpy()
    assert (a == b).all()
    assert a.dtype == np.uint8 and a.std() > 10


def test_numpy_port_matches_reference_outputs():
    """oracle/ref_numpy.py (the CPU baseline) reproduces the reference's P-frame tokens and
    reconstruction (VBS off, golden vector 3)."""
    from oracle.ref_numpy import inter_rows
    g = golden("cif_p_vbs0.npz")
    tok, rec = inter_rows(g["cur"].astype(np.float64), g["ref"], range(0, 3))
    assert (rec[:48] == g["recon"][:48]).all()
    assert tok == int(g["tokens"].reshape(18, 22)[:3].sum())


def test_unsupported_modes_raise():
    from streamoptima_amd.Encoder import Y_Video_codec
    z = np.zeros((1, 32, 32), np.uint8)
    with pytest.raises(NotImplementedError):
        Y_Video_codec(32, 32, 1, 16, 16, 4, 1, 1, 0.015, False, y_only_frame_arr=z)
    with pytest.raises(ValueError):      # NameError on `mvp` in the reference (Encoder.py:609)
        Y_Video_codec(32, 32, 1, 16, 16, 4, 1, 0, 0.015, True, y_only_frame_arr=z, fast_me=True, ParallelMode=2)
    with pytest.raises(NotImplementedError):
        Y_Video_codec(32, 32, 1, 16, 16, 4, 1, 0, 0.015, False, y_only_frame_arr=z, ParallelMode=3)


def test_me_mode_selection():
    """fast_me / FMEEnable / ParallelMode pick the C-ABI ME mode (include/streamoptima.h)."""
    from streamoptima_amd import _lib
    from streamoptima_amd.Encoder import Y_Video_codec
    z = np.zeros((1, 32, 32), np.uint8)
    mk = lambda **k: Y_Video_codec(32, 32, 1, 16, 16, 4, 1, 0, 0.015, False, y_only_frame_arr=z, **k)  # noqa: E731
    assert mk()._me_mode() == _lib.ME_FULL
    assert mk(fast_me=True)._me_mode() == _lib.ME_FAST
    assert mk(fast_me=True, ParallelMode=2)._me_mode() == _lib.ME_FAST_PAR
    assert mk(ParallelMode=2)._me_mode() == _lib.ME_FULL
    assert mk(FMEEnable=True).FMEEnable


def test_engine_refuses_cpu_device():
    from streamoptima_amd import _lib
    from streamoptima_amd.engine import Engine
    with pytest.raises(_lib.HipPathError):
        Engine(32, 32, 16, 16, False, None, "cpu")


@pytest.mark.parametrize("name,rc", [("gop_cif_vbs0", None), ("gop_cif_vbs1_rc1", 1), ("gop_small_rc2", 2),
                                     ("gop_fme_vbs1", None), ("gop_fast_vbs1", None)])
def test_bitstream_parsers_on_reference_lines(name, rc):
    """differential_decoder_frame / entropy_decoder_frame (decoder.py:589-664) read the
    reference's own text lines back into its symbols (split, MVs, QTC, per-row QPs)."""
    import gzip
    import json
    from conftest import GOLDEN, golden
    from streamoptima_amd import bitstream as B
    g = golden(name + ".npz")
    js = json.load(gzip.open(os.path.join(GOLDEN, name + "_bitstream.json.gz"), "rt"))
    w = g["frames"].shape[2]
    for i, (ml, rl) in enumerate(zip(js["mv_lines"], js["residual_lines"])):
        ft, mvs, qps = B.differential_decoder_frame(ml, rc, w / 16)
        res = B.entropy_decoder_frame(rl, 16)
        assert ft == g["frame_type"][i]
        if rc:
            assert qps == g[f"qp_per_row{i}"].tolist()
        for b, (m, r) in enumerate(zip(mvs, res)):
            assert m[0] == r[0] == g[f"split{i}"][b]
            q = (np.asarray(r[1]).reshape(-1) if m[0] == 0
                 else np.concatenate([np.asarray(x).reshape(-1) for x in r[1]]))
            assert (q == g[f"qtc{i}"][b]).all()
            mv = g[f"mv{i}"][b]
            got = [m[1]] if m[0] == 0 else m[1]
            for k, v in enumerate(got):
                assert tuple(np.atleast_1d(v)) == tuple(np.atleast_1d(mv[k])), (i, b, k)
        # and the writer reproduces the line from the parsed symbols
        assert B.entropy_encoder_frame(res, 16) == rl


def test_entropy_block_round_trip():
    from streamoptima_amd import bitstream as B
    rng = np.random.default_rng(3)
    for n in (16, 8):
        for _ in range(200):
            q = rng.integers(-3, 4, size=(n, n)) * (rng.random((n, n)) < rng.random())
            assert (np.array(B.entropy_decoder_block(B.entropy_encoder_block(q, n), n)) == q).all()


def test_oracle_qp_map_rule():
    """Two-pass / ROI QP map: delta from the block's share of its row's pass-1
    tokens, ROI offsets on top, clamped."""
    from oracle import oracle as O
    t = np.array([10, 10, 10, 10,   40, 5, 2, 1], np.int32)      # two rows of 4 blocks
    qm = O.qp_map(t, 4, 2, 4, None, None, 0, 12)
    assert qm[:4].tolist() == [4, 4, 4, 4]                      # flat row: no change
    # row 2: sum 48, mean 12: 40 -> >=2x (+1, <4x), 5 -> <1/2 (-1), 2 -> <1/4 (-2), 1 -> -2
    assert qm[4:].tolist() == [5, 3, 2, 2]
    roi = np.array([-3, 0, 0, 9, 0, 0, 0, 0], np.int32)
    qm = O.qp_map(t, 4, 2, 4, [6, 1], roi, 0, 12)
    assert qm.tolist() == [3, 6, 6, 12, 2, 0, 0, 0]
    assert O.qp_map(None, 4, 2, 4, None, roi, 0, 12).tolist() == [1, 4, 4, 12, 4, 4, 4, 4]


def test_roi_rectangles_to_blocks():
    from streamoptima_amd.Encoder import Y_Video_codec
    z = np.zeros((1, 48, 64), np.uint8)
    enc = Y_Video_codec(48, 64, 1, 16, 16, 4, 1, 0, 0.015, False, y_only_frame_arr=z,
                        roi=[(0, 0, 32, 16, -2), (16, 16, 64, 48, 1)])
    assert enc.roi_block_offsets().reshape(3, 4).tolist() == [[-2, -2, 0, 0], [0, 1, 1, 1], [0, 1, 1, 1]]
    enc2 = Y_Video_codec(48, 64, 1, 16, 16, 4, 1, 0, 0.015, False, y_only_frame_arr=z,
                         roi=np.arange(12).reshape(3, 4))
    assert enc2.roi_block_offsets().tolist() == list(range(12))


def test_device_dct_header_bitwise_vs_oracle(tmp_path):
    """streamoptima_amd/csrc/so_dct.h (the kernels' FP64 DCT-II/III, with its exact
    power-of-two folds) compiled for the host matches the oracle's pocketfft restatement
    bit for bit on random, tie-heavy and dequantised vectors (tests/host/dct_host_check.cpp)."""
    import shutil
    import subprocess
    from oracle import oracle as O
    O.build()
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "dct_check")
    libdir = os.path.dirname(O.LIB_PATH)
    subprocess.run([gxx, "-O2", "-ffp-contract=off", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                    os.path.join(root, "tests", "host", "dct_host_check.cpp"), f"-L{libdir}", "-lso_oracle",
                    f"-Wl,-rpath,{libdir}", "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe, "300000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_run_kernel_selection_truth_table(tmp_path):
    """streamoptima_amd/csrc/so_run_select.h (which persistent-run instantiation a launch uses)
    compiled alone for the host gives, for every combination of its inputs, the entry written out
    in tests/host/run_select_check.cpp; every entry is reachable and the capacity filters count
    9 plain and 7 VBS entries."""
    import shutil
    import subprocess
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "run_select_check")
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", "-Werror",
                    os.path.join(root, "tests", "host", "run_select_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def _unpack_check_cases():
    """[(coding 0/1, kind 0 luma 16 / 1 luma 8 / 2 chroma, frame type, bytes, the strict model's verdict:
    None = malformed, else (split, mv, qtc) flat)]: the corpora of tests/packcases.py, tests/packbitcases.py
    and tests/packchromaref.py and every mutant of theirs."""
    import packbitcases
    import packcases
    import packchromaref
    from packbitsref import unpack_block_bits_strict
    from packref import unpack_block_strict
    cases = []

    def luma(coding, bs, ftype, data, model):
        v = model(data, bs, ftype)
        want = None if v is None else (int(v["split"]), np.asarray(v["mv"]).reshape(-1), np.asarray(v["qtc"]))
        cases.append((coding, 0 if bs == 16 else 1, ftype, data, want))

    for kind in packcases.KINDS:
        bs = packcases.block_size(kind)
        for ftype in (0, 1):
            for data in packcases.block_bytes(kind, ftype):
                luma(0, bs, ftype, data, unpack_block_strict)
            for data in packbitcases.block_bytes(kind, ftype):
                luma(1, bs, ftype, data, unpack_block_bits_strict)
            base = packcases.mutation_base(kind, ftype)
            for b, block in enumerate(base):
                for _, data in packcases.mutations(block, bs, ftype, prev_byte=base[b - 1][-1]):
                    luma(0, bs, ftype, data, unpack_block_strict)
            for block in packbitcases.mutant_base(kind, ftype):
                for _, data in packbitcases.mutants(block, bs, ftype):
                    luma(1, bs, ftype, data, unpack_block_bits_strict)
    for c, coding in enumerate(packchromaref.CODINGS):
        todo = [(d, packchromaref.unpack_record_strict(d, coding)) for d in packchromaref.record_bytes(coding)]
        todo += [(d, v) for _, d, v in packchromaref.mutants(coding)]
        for data, v in todo:
            want = None if isinstance(v, str) else (0, np.zeros(0, np.int16), np.concatenate([v["qtc_u"], v["qtc_v"]]))
            cases.append((c, 2, 0, data, want))
    return cases


_UNPACK_CHECK = []


def _unpack_check_exe(tmp_path) -> str:
    """tests/host/unpack_check.cpp built once per session, under both sanitizers."""
    import shutil
    import subprocess
    if not _UNPACK_CHECK:
        cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
        assert cxx is not None, "no host C++ compiler"
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        exe = str(tmp_path / "unpack_check")
        subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-isystem", "/opt/rocm/include",
                        os.path.join(root, "tests", "host", "unpack_check.cpp"), "-o", exe],
                       check=True, capture_output=True)
        _UNPACK_CHECK.append(exe)
    return _UNPACK_CHECK[0]


_OUT_REC = np.dtype([("bad", np.uint8), ("split", np.uint8), ("mv", np.int16, 12), ("q", np.int16, 256)])


def test_unpack_record_bodies_under_sanitizers(tmp_path):
    """The strict decoders of streamoptima_amd/csrc/so_packfmt.h (the record bodies the unpack kernels
    run), compiled for the host with AddressSanitizer and UndefinedBehaviorSanitizer
    (tests/host/unpack_check.cpp: a child process, every record and every output in a heap allocation
    of exactly its size): on every corpus record and every mutant, in both codings, accept / reject
    and the decoded split, mv values and coefficients equal the strict models', and no access leaves
    a record's bytes or its outputs."""
    import struct
    import subprocess
    exe = _unpack_check_exe(tmp_path)
    cases = _unpack_check_cases()
    assert sum(c[4] is None for c in cases) > 1000 and sum(c[4] is not None for c in cases) > 1000
    assert {(c[0], c[1]) for c in cases} == {(a, b) for a in (0, 1) for b in (0, 1, 2)}
    src, dst = str(tmp_path / "records.bin"), str(tmp_path / "decoded.bin")
    with open(src, "wb") as f:
        for coding, kind, ftype, data, _ in cases:
            f.write(struct.pack("<BBBBI", coding, kind, ftype, 0, len(data)) + data)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = np.fromfile(dst, dtype=_OUT_REC)
    assert got.size == len(cases)
    for i, (coding, kind, ftype, data, want) in enumerate(cases):
        g = got[i]
        assert bool(g["bad"]) == (want is None), (i, coding, kind, ftype, data.hex())
        if want is not None:
            split, mv, q = want
            assert g["split"] == split, (i, coding, kind, ftype, data.hex())
            assert np.array_equal(g["mv"][:mv.size], mv) and not g["mv"][mv.size:].any(), (i, coding, kind, ftype)
            assert np.array_equal(g["q"][:q.size], q) and not g["q"][q.size:].any(), (i, coding, kind, ftype)


def test_unpack_huff_record_bodies_under_sanitizers(tmp_path):
    """The same program on coding 2 = huff: the table rule, HuffDec, HuffReader, the list parser and the
    two record bodies of so_packfmt.h, the functions the huff unpack kernels call.  Every case of
    tests/packhuffcases.py host_cases() -- the table bytes, the record's bytes, the expanded tables and
    every output each in a heap allocation of exactly their size: accept / reject, split, mv values and
    coefficients equal the strict model's (tests/packhuffref.py unpack_record_huff_strict) per record.
    The counts are caps against an empty corpus: per kind more than 1,000 accepted and 1,000 rejected
    records, and every rule the model can reject a record of that kind by."""
    import struct
    import subprocess
    import packhuffcases as C
    exe = _unpack_check_exe(tmp_path)
    cases = C.host_cases()
    want = [C.case_verdict(c) for c in cases]
    for kind in (0, 1, 2):
        mine = [w for c, w in zip(cases, want) if c[0] == kind]
        assert sum(k == "ok" for k, _ in mine) > 1000 and sum(k == "bad" for k, _ in mine) > 1000, kind
        assert {r for k, r in mine if k == "bad"} == set(C.REASONS[kind]), kind
    src, dst = str(tmp_path / "huff_records.bin"), str(tmp_path / "huff_decoded.bin")
    with open(src, "wb") as f:
        for kind, ftype, tb, body, _ in cases:
            f.write(struct.pack("<BBBBII", 2, kind, ftype, 0, len(body), len(tb)) + tb + body)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = np.fromfile(dst, dtype=_OUT_REC)
    assert got.size == len(cases)
    for g, (kind, ftype, tb, body, name), (verdict, res) in zip(got, cases, want):
        where = (name, kind, ftype, tb[:8].hex(), body.hex())
        assert bool(g["bad"]) == (verdict == "bad"), where
        if verdict == "ok":
            split, mv, q = res
            assert g["split"] == split, where
            assert np.array_equal(g["mv"][:mv.size], mv) and not g["mv"][mv.size:].any(), where
            assert np.array_equal(g["q"][:q.size], q) and not g["q"][q.size:].any(), where
        elif res in ("short tables", "spare nibble", "kraft"):
            assert not g["split"] and not g["mv"].any() and not g["q"].any(), where     # nothing decoded
