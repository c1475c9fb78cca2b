"""kg_exchange_layout.hpp (where the send list and the receive sets of the multi-GPU exchange lie in its buffer: kg_comm.hip's
exchange_bytes, split buffer and Exchange::plan) on the host: tests/native/exchange_layout_check.cc is built with hipcc (-x hip, as
tests/test_l1_lean.py builds its check) and run on the CPU -- every send list and set size from 0 to 4096 and a few large ones, both
shapes, both wire forms: the arrays in use are disjoint, aligned and inside the reported bytes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exchange_buffer_arrays_are_disjoint_aligned_and_inside(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = str(tmp_path / "exchange_layout_check")
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "native", "exchange_layout_check.cc"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "exchange layout ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
