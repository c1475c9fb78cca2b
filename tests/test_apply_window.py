"""kg_apply_lean.hpp's window selection (ap_first_event: of the W slots a lane of the packed apply's drain reads per round trip, the first that is
free or holds the k-mer's remainder) against a plain loop over ap_holds / ap_taken, on the host: tests/native/apply_window_check.cc is built
with hipcc (-x hip, so that it includes the real headers) and run on the CPU -- W = 2 and 4, budgets 1 .. W + 1, cbits 20 .. 32, every
combination of free, foreign and own words in the window (own with remainder 0 too), and the wrap of the window's indices."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_window_selection_matches_plain_loop(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "apply_window_check")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", os.path.join(ROOT, "tests", "native", "apply_window_check.cc"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "apply window ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
