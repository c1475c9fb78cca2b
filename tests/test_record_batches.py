"""kg_record_batches.hpp (where the batches of a per-record host form end, and the most bases of one: what for_record_batches walks and
what the gathered statistics size their buffers by) on the host: tests/native/record_batches_check.cc is a stand-alone program over the
header, built once plain and once with -fsanitize=address,undefined and run on the CPU -- every layout of at most 5 records x max_bases x
max_recs x three kinds of `joins`, 1.8 M cuts, each held against the rule restated as one loop over the records."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_record_batches_cut(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host compiler"
    exe = str(tmp_path / "record_batches_check")
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", *flags, os.path.join(ROOT, "tests", "native", "record_batches_check.cc"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "record batches ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
