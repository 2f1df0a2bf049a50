"""Record tests/golden/capi_refusals_deblock.json: the return code and so_last_error() text of every
case of tests/capi_refusal_cases_deblock.py (so_deblock_yuv420).  The procedure is
record_capi_refusals.py's: on a machine WITHOUT a GPU, against the library whose behaviour is the
reference (SO_LIB_PATH, or the in-tree build); only refusals are recorded, and a case that reaches
the HIP runtime stops the recording and is named.

    python tests/golden/record_capi_refusals_deblock.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
FIXTURE = os.path.join(HERE, "capi_refusals_deblock.json")


def main() -> int:
    import torch
    if torch.cuda.is_available():
        print("a GPU is visible: a case that passed validation would launch on made-up addresses", file=sys.stderr)
        return 2
    import capi_refusal_cases_deblock as table
    from streamoptima_amd import _lib
    lib = _lib.load()
    rec, bad = {}, []
    for cid, fn, args in table.cases():
        rc, text = table.run(lib, fn, args)
        if rc not in (_lib.SO_OK, _lib.SO_E_INVALID, _lib.SO_E_UNSUPPORTED):
            bad.append(f"{cid}: returned {rc} ({text}): it reached the HIP runtime")
        rec[cid] = [rc, text]
    if bad:
        print("\n".join(bad), file=sys.stderr)
        print(f"{len(bad)} cases are not refusals; nothing written", file=sys.stderr)
        return 1
    with open(FIXTURE, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(rec)} cases -> {FIXTURE}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
