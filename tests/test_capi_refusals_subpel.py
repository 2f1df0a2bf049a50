"""The refusal matrix of the chroma _ex entry points (capi_refusal_cases_subpel.py) against
golden/capi_refusals_subpel.json (record_capi_refusals_subpel.py next to it), and what ties it to
the recorded matrix of the base functions: at the inherited rules an _ex function says what its
base function says, under its own name.  Made-up addresses, so the library calls are for machines
without a GPU: the fixture that loads it skips where one is visible."""
import json
import os

import pytest

import capi_refusal_cases_subpel as table
from conftest import GOLDEN

CASES = table.cases()
with open(os.path.join(GOLDEN, "capi_refusals_subpel.json")) as _f:
    RECORDED = json.load(_f)
with open(os.path.join(GOLDEN, "capi_refusals.json")) as _f:
    RECORDED_BASE = json.load(_f)
FUNCTIONS = ("so_chroma_encode_frame_ex", "so_chroma_recon_frame_ex", "so_decode_chroma_frames_ex")


@pytest.fixture(scope="module")
def lib():
    import torch
    if torch.cuda.is_available():
        pytest.skip("made-up addresses: a case that slipped through validation would launch on this GPU")
    from streamoptima_amd import _lib, build
    build.build()
    return _lib.load()


def test_the_fixture_holds_exactly_the_cases():
    assert sorted(RECORDED) == sorted(cid for cid, _, _ in CASES)
    assert {fn for _, fn, _ in CASES} == set(FUNCTIONS) and len(CASES) > 150


def test_only_refusals_are_recorded():
    for cid, (rc, text) in RECORDED.items():
        assert rc in (0, -1, -2), cid
        if rc == 0:   # nothing to launch: the message of the refusal before it still stands
            assert text.startswith("so_set_option: option -1"), cid


def test_the_new_rule_and_its_place():
    for fn in FUNCTIONS:
        for bits in (0, 3, -1):
            rc, text = RECORDED[f"{fn}: mv_frac_bits {bits}"]
            assert rc == -1 and text.startswith(f"{fn}: mv_frac_bits {bits}"), (fn, bits, text)
        rc, text = RECORDED[f"{fn}: order: bs before mv_frac_bits"]
        assert rc == -2 and text.startswith(f"{fn}: block_size 8")
        for what in ("geometry", "qp", "qp_offset"):
            rc, text = RECORDED[f"{fn}: order: mv_frac_bits before {what}"]
            assert rc == -1 and "mv_frac_bits" in text, (fn, what, text)
    rc, text = RECORDED["so_decode_chroma_frames_ex: order: mv_frac_bits before nframes 0"]
    assert rc == -1 and "mv_frac_bits 0" in text
    assert RECORDED["so_decode_chroma_frames_ex: nframes 0"][0] == 0


def test_inherited_rules_read_as_the_base_functions_do():
    """A case of the same label in the recorded matrix of the base functions has the same code and
    the same text, the function's name apart."""
    shared = 0
    for cid, (rc, text) in RECORDED.items():
        fn, label = cid.split(": ", 1)
        for lab in (label, label.split(": ", 1)[1] if label.startswith("bits ") else None):
            old = RECORDED_BASE.get(f"{fn[:-3]}: {lab}") if lab else None
            if old is not None:
                assert [rc, text] == [old[0], old[1].replace(fn[:-3] + ":", fn + ":")], cid
                shared += 1
    assert shared > 100


@pytest.mark.parametrize("fn", FUNCTIONS)
def test_refusals(lib, fn):
    wrong = []
    for cid, f, args in CASES:
        if f == fn:
            got = list(table.run(lib, f, args))
            if got != RECORDED[cid]:
                wrong.append((cid, got, RECORDED[cid]))
    assert not wrong, wrong


def test_base_names_still_report_as_themselves(lib):
    """The three base functions forward with mv_frac_bits 1 and keep their own names."""
    import capi_refusal_cases as old
    n = 0
    for cid, f, args in old.cases():
        if f + "_ex" in FUNCTIONS:
            assert list(old.run(lib, f, args)) == RECORDED_BASE[cid], cid
            n += 1
    assert n > 60
