"""kg_apply_lean.hpp (the packed apply's slot tests on the word's low half and its step) against the statements they replace, on the
host: tests/native/apply_lean_check.cc is built with hipcc (-x hip, so that it includes the real headers) and run on the CPU -- 1.3 M
slot words over cbits = 20 .. 32 (and remainders shorter than a word at cbits = 32): holds, taken / free, the step with its wrap."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_apply_lean_arithmetic_matches_plain_form(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "apply_lean_check")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "native", "apply_lean_check.cc"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "apply lean ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
