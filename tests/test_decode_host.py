"""The fused luma decoder's parse step on the host under sanitizers (tests/host/decode_check.cpp):
so_packfmt.h's decode_luma_p_record -- the strict record body plus the reference-index check -- on
every luma corpus record and mutant of tests/packcases.py and tests/packbitcases.py, read as a
P-frame record, for reference lists of 1 to 4 planes."""
import os
import shutil
import struct
import subprocess

import numpy as np


def _cases():
    """[(coding 0/1, kind 0 luma 16 / 1 luma 8, bytes, the strict model's verdict of the bytes as an inter
    record: None = malformed, else (split, mv [12], qtc))]."""
    import packbitcases
    import packcases
    from packbitsref import unpack_block_bits_strict
    from packref import unpack_block_strict
    cases, seen = [], set()

    def luma(coding, bs, data, model):
        key = (coding, bs, bytes(data))
        if key in seen:
            return
        seen.add(key)
        v = model(data, bs, 1)
        want = None if v is None else (int(v["split"]), np.asarray(v["mv"]).reshape(-1), np.asarray(v["qtc"]))
        cases.append((coding, 0 if bs == 16 else 1, bytes(data), want))

    for kind in packcases.KINDS:
        bs = packcases.block_size(kind)
        for ftype in (0, 1):
            for data in packcases.block_bytes(kind, ftype):
                luma(0, bs, data, unpack_block_strict)
            for data in packbitcases.block_bytes(kind, ftype):
                luma(1, bs, data, unpack_block_bits_strict)
            base = packcases.mutation_base(kind, ftype)
            for b, block in enumerate(base):
                for _, data in packcases.mutations(block, bs, ftype, prev_byte=base[b - 1][-1]):
                    luma(0, bs, data, unpack_block_strict)
            for block in packbitcases.mutant_base(kind, ftype):
                for _, data in packbitcases.mutants(block, bs, ftype):
                    luma(1, bs, data, unpack_block_bits_strict)
    return cases


def test_fused_parse_and_reference_check_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no host C++ compiler"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    exe = str(tmp_path / "decode_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-isystem", os.path.join(rocm, "include"),
                    os.path.join(root, "tests", "host", "decode_check.cpp"), "-o", exe],
                   check=True, capture_output=True)
    cases = _cases()
    accepted = [c for c in cases if c[3] is not None]
    assert len(accepted) > 500 and len(cases) - len(accepted) > 1000
    assert {(c[0], c[1]) for c in accepted} == {(a, b) for a in (0, 1) for b in (0, 1)}
    # the corpus must reach the new check from both sides: used indices above 0 and at most 3
    top = [int(max(w[1].reshape(4, 3)[:4 if w[0] else 1, 2])) for _, _, _, w in accepted]
    low = [int(min(w[1].reshape(4, 3)[:4 if w[0] else 1, 2])) for _, _, _, w in accepted]
    assert any(1 <= t <= 3 for t in top) and any(t >= 4 for t in top) and any(v < 0 for v in low)
    src, dst = str(tmp_path / "records.bin"), str(tmp_path / "decoded.bin")
    nrefs = (1, 2, 3, 4)
    with open(src, "wb") as f:
        for coding, kind, data, _ in cases:
            for nref in nrefs:
                f.write(struct.pack("<BBBBI", coding, kind, nref, 0, len(data)) + data)
    r = subprocess.run([exe, src, dst], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rec = np.dtype([("bad", np.uint8), ("split", np.uint8), ("clean", np.uint8), ("fetched", np.uint8),
                    ("mv", np.int16, 12), ("q", np.int16, 256)])
    got = np.fromfile(dst, dtype=rec).reshape(len(cases), len(nrefs))
    verdicts = set()
    for i, (coding, kind, data, want) in enumerate(cases):
        for k, nref in enumerate(nrefs):
            g = got[i, k]
            what = (i, coding, kind, nref, data.hex())
            assert g["clean"] == 1, what
            ok = want is not None
            if ok:
                used = want[1].reshape(4, 3)[:4 if want[0] else 1, 2]
                ok = bool(((used >= 0) & (used < nref)).all())
            verdicts.add((want is not None, ok))
            assert bool(g["bad"]) == (not ok), what
            if ok:
                split, mv, q = want
                assert g["split"] == split and g["fetched"] == (4 if split else 1), what
                assert np.array_equal(g["mv"], mv), what
                assert np.array_equal(g["q"][:q.size], q) and not g["q"][q.size:].any(), what
    assert verdicts == {(False, False), (True, False), (True, True)}
