"""The refusal matrix: every case of capi_refusal_cases.py returns the code and leaves the
so_last_error() text recorded in golden/capi_refusals.json (record_capi_refusals.py next to it),
so a change to the C boundary's checks cannot move, reword, reorder or lose a refusal unseen.
The cases pass made-up addresses, so none may reach a launch: the module is for machines without
a GPU and skips itself where one is visible."""
import json
import os

import pytest

import capi_refusal_cases as table
from conftest import GOLDEN

CASES = table.cases()
with open(os.path.join(GOLDEN, "capi_refusals.json")) as _f:
    RECORDED = json.load(_f)


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
    assert len(CASES) > 900


def test_only_refusals_are_recorded():
    for cid, (rc, text) in RECORDED.items():
        assert rc in (0, -1, -2), cid
        if rc == 0:   # nothing to launch: the message of the refusal before it still stands
            assert text.startswith("so_set_option: option -1"), cid


@pytest.mark.parametrize("fn", sorted({fn for _, fn, _ in CASES}))
def test_refusals(lib, fn):
    wrong = []
    for cid, f, args in CASES:
        if f == fn:
            got = list(table.run(lib, f, args))
            if got != RECORDED[cid]:
                wrong.append((cid, got, RECORDED[cid]))
    assert not wrong, wrong


def test_default_p_rows_ex_reports_as_p_rows():
    rc, text = RECORDED["so_encode_p_rows_ex: defaults, bs 12: reported as so_encode_p_rows"]
    assert rc == -2 and text.startswith("so_encode_p_rows: block_size 12")
    rc, text = RECORDED["so_encode_p_rows_ex: bs 12"]
    assert rc == -2 and text.startswith("so_encode_p_rows_ex: block_size 12")
