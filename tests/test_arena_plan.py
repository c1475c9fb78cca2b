"""kg_arena_plan.hpp (the partition arena's arithmetic: bytes per k-mer of a round by shape, level 1's stride, the runs' capacity and base, a
pass's extent, a round's capacity per level-1 edition, round_starts) on the host: tests/native/arena_plan_check.cc is a stand-alone program
over the header, built once plain and once with -fsanitize=address,undefined and run on the CPU -- 1.4 M checks over P1 x P2 x level-1
workgroups x round sizes, and the rounds of the bench's default configuration."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "sanitized"])
def test_arena_plan_arithmetic(tmp_path, flags):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host compiler"
    exe = str(tmp_path / "arena_plan_check")
    r = subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", *flags, os.path.join(ROOT, "tests", "native", "arena_plan_check.cc"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-1500:])
    assert r.returncode == 0 and "arena plan ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
