"""The fast 16-point transforms (so_dct.h: dct2_16_fast / dct3_16_fast) with the plain run's
certificates and fallback against the pocketfft sequence alone, on the host: tools/check_dct_fast.cpp
compiled for the CPU and run on its own corpus (1 M blocks, QP 0-12) plus the adversarial tie
blocks of tests/adversarial.py at every QP.  The flagged shares it prints are measurements
(DESIGN.md section 4), not thresholds.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import adversarial as adv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    pytest.fail("hipcc not found")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dct_fast")
    exe = str(tmp / "check_dct_fast")
    r = subprocess.run([_hipcc(), "-O2", "-ffp-contract=off", "-DSO_DEV=inline",
                        os.path.join(ROOT, "tools", "check_dct_fast.cpp"), "-o", exe, "-lpthread"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    blocks = np.concatenate([adv.run_blocks(f).reshape(-1, 16, 16) for f in (128, 0, 255)])
    ties = str(tmp / "ties.bin")
    blocks.astype("<i2").tofile(ties)
    r = subprocess.run([exe, "--file", ties], capture_output=True, text=True)
    print(r.stdout)
    return r, len(blocks)


def _line(out, key):
    m = re.search(rf"^{key} max_diff (\S+) bound_fast (\S+) bound_pocketfft (\S+) delta (\S+) accepted (\d+) fallback (\d+)$",
                  out, re.M)
    assert m, out[-2000:]
    return [float(v) for v in m.groups()[:4]] + [int(v) for v in m.groups()[4:]]


def test_fast_path_with_fallback_equals_pocketfft(report):
    r, nties = report
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = re.search(r"^blocks (\d+) vectors (\d+) mismatches (\d+)$", r.stdout, re.M)
    assert m and int(m.group(3)) == 0
    assert int(m.group(1)) >= 1_000_000 + 13 * nties and int(m.group(2)) >= 10_000_000
    assert f"file_blocks {nties}" in r.stdout


@pytest.mark.parametrize("direction", ["fwd", "inv"])
def test_bounds_thresholds_and_both_paths_ran(report, direction):
    r, _ = report
    diff, b_fast, b_pocket, delta, accepted, fallback = _line(r.stdout, direction)
    assert diff <= b_fast + b_pocket          # |fast - pocketfft| within the two derived bounds
    assert delta >= b_fast + b_pocket         # the flag threshold covers both errors
    assert accepted > 0 and fallback > 0      # neither path passes by never running
