"""The refusal matrix of so_deblock_yuv420 (capi_refusal_cases_deblock.py) against
golden/capi_refusals_deblock.json (record_capi_refusals_deblock.py next to it), and what the header
promises of it: the codes, the argument named, the order of the rules.  Made-up addresses, so the
library calls are for machines without a GPU: the fixture that loads it skips where one is visible."""
import json
import os

import pytest

import capi_refusal_cases_deblock as table
from conftest import GOLDEN

FN = table.FN
CASES = table.cases()
with open(os.path.join(GOLDEN, "capi_refusals_deblock.json")) as _f:
    RECORDED = json.load(_f)


def rec(label):
    return RECORDED[f"{FN}: {label}"]


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
    assert len(CASES) > 60


def test_only_refusals_are_recorded():
    ok = []
    for cid, (rc, text) in RECORDED.items():
        assert rc in (0, -1, -2), cid
        if rc == 0:   # nothing to launch: the message of the refusal before it still stands
            assert text.startswith("so_set_option: option -1"), cid
            ok.append(cid.split(": ", 1)[1])
        else:
            assert text.startswith(FN + ": "), cid
    assert sorted(ok) == ["W 120 is a multiple of 8", "nframes 0", "nframes 0 without arrays"]


def test_each_rule_names_its_argument():
    named = {"nframes -1": "nframes -1", "bs 12": "bs 12", "bs 0": "bs 0", "H 72": "H 72", "W 120": "W 120",
             "H 0": "H 0", "too large": "H 65536", "qp 21": "qp 21", "qp -1": "qp -1",
             "chroma_qp_offset 21": "chroma_qp_offset 21", "chroma_qp_offset -21": "chroma_qp_offset -21",
             "strength 4": "strength 4", "strength -4": "strength -4", "null sy": "sy is NULL", "null dy": "dy is NULL",
             "null sy[last]": "sy[1] is NULL", "null dy[0]": "dy[0] is NULL", "partial chroma: no sv": "sv is NULL",
             "partial chroma: only du": "su is NULL", "null dv[last]": "dv[1] is NULL", "null su[0]": "su[0] is NULL",
             "nframes 0, strength 4": "strength 4"}
    for label, text in named.items():
        rc, got = rec(label)
        assert rc == -1 and text in got, (label, got)
    for label in ("dy[0] is sy[0]", "dy[1] is sy[0]", "dy[0] inside sy[1]", "dy[0] ends inside sy[1]", "dy[0] is dy[1]",
                  "du[0] is sv[0]", "du[0] is dv[0]", "dv[1] overlaps du[1]", "dv[1] inside dy[0]", "du[0] inside sy[0]",
                  "luma only: dy[0] is sy[0]"):
        rc, got = rec(label)
        assert rc == -1 and "aliases" in got, (label, got)
    for label, text in {"chroma with bs 8": "chroma", "split[0] with bs 8": "split[0]",
                        "split[last] with bs 8": "split[1]"}.items():
        rc, got = rec(label)
        assert rc == -2 and text in got, (label, got)


def test_the_order_of_the_rules():
    first = {"order: nframes before bs": "nframes", "order: bs before geometry": "bs 12",
             "order: geometry before qp": "W 100", "order: qp before chroma_qp_offset": "qp 21",
             "order: chroma_qp_offset before strength": "chroma_qp_offset", "order: strength before NULL": "strength",
             "order: sy before dy": "sy is NULL", "order: luma pointers before the chroma set": "dy[1]",
             "order: partial chroma before aliasing": "su is NULL", "order: aliasing before bs 8 chroma": "aliases",
             "order: chroma before split with bs 8": "chroma"}
    for label, text in first.items():
        rc, got = rec(label)
        assert rc in (-1, -2) and text in got, (label, got)
    assert rec("order: aliasing before bs 8 chroma")[0] == -1
    assert rec("order: chroma before split with bs 8")[0] == -2


def test_refusals(lib):
    wrong = []
    for cid, f, args in CASES:
        got = list(table.run(lib, f, args))
        if got != RECORDED[cid]:
            wrong.append((cid, got, RECORDED[cid]))
    assert not wrong, wrong
