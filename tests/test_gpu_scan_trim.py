"""The 5' trim on katgpu_count_files' fast paths -- the device record scan (kg_scan.hpp: k_line_len / k_emit take the trim) and the FASTQ
host strip -- against the oracle, under the hooks of tests/test_gpu_scan.py that make small files cross hundreds of batch and segment
cuts.  tests/scan_trim_cases.py holds the cases: its build() writes the files and the oracle's verdicts once for the session, its main()
runs in a subprocess per hook set.  Then the CLI: `katgpu hist --5ptrim` and `katgpu comp --d1_5ptrim / --d2_5ptrim` through the fast
paths write what they write through the streaming machine."""
import os
import subprocess
import sys

import pytest

from tests import scan_trim_cases

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "kat_amd", "bin", "katgpu")

SCAN_16K = {"KATGPU_TEST_SCAN_BATCH": "16384", "KATGPU_TEST_SCAN_SEGMENT": "4096", "KATGPU_TEST_SCAN_OVERLAP": "2048"}
STRIP_4K = {"KATGPU_TEST_STRIP_SEGMENT": "4096", "KATGPU_TEST_STRIP_OVERLAP": "2048", "KATGPU_TEST_SCAN_BATCH": "16384", "KATGPU_TEST_SCAN_OVERLAP": "2048"}
HOOK_SETS = {
    "scan_16k": SCAN_16K,
    "scan_5000_3_threads": {"KATGPU_TEST_SCAN_BATCH": "5000", "KATGPU_TEST_SCAN_SEGMENT": "1000", "KATGPU_TEST_SCAN_OVERLAP": "1500", "KATGPU_SCAN_THREADS": "3"},
    # the host machine from batch 3 on: on twoline.fa it starts right behind a header line as often as not (host_rest's start state)
    "scan_fail_at_3": {"KATGPU_TEST_SCAN_BATCH": "20000", "KATGPU_TEST_SCAN_SEGMENT": "20000", "KATGPU_TEST_SCAN_OVERLAP": "4096", "KATGPU_TEST_SCAN_FAIL_AT": "3"},
    "strip_4k": STRIP_4K,
    "strip_fail_at_5": {"KATGPU_TEST_STRIP_SEGMENT": "8192", "KATGPU_TEST_STRIP_OVERLAP": "4096", "KATGPU_TEST_STRIP_FAIL_AT": "5", "KATGPU_TEST_SCAN_BATCH": "20000", "KATGPU_TEST_SCAN_OVERLAP": "4096"},
}


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("scan_trim"))
    scan_trim_cases.build(tmp)
    return tmp


@pytest.mark.parametrize("hooks", list(HOOK_SETS))
def test_trimmed_files_through_the_fast_paths_match_the_oracle(cases, hooks):
    env = dict(os.environ)
    env.update(HOOK_SETS[hooks])
    env["KATGPU_TRACE"] = "1"
    r = subprocess.run([sys.executable, os.path.join(HERE, "scan_trim_cases.py"), cases], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "scan trim cases ok" in r.stdout


def _body(path):
    with open(path, "rb") as f:
        return [ln for ln in f.read().split(b"\n") if not ln.startswith(b"#")]


def _cli(args, hooks, cwd):
    env = dict(os.environ)
    env.update(hooks)
    env["KATGPU_TRACE"] = "1"
    r = subprocess.run([EXE] + args, env=env, capture_output=True, text=True, timeout=300, cwd=cwd)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stderr


STREAMING = {"KATGPU_DEVICE_SCAN": "0", "KATGPU_INGEST_MIN_BYTES": str(2 ** 60)}      # the machine alone, one reader thread per file


def test_cli_hist_5ptrim_takes_the_device_scan(cases, tmp_path):
    reads = os.path.join(cases, "reads.fq")
    err = _cli(["hist", "-m", "27", "--5ptrim", "5", "-o", "fast.hist", reads], SCAN_16K, str(tmp_path))
    assert "device scan of " + reads in err and not any(h in err for h in scan_trim_cases.HANDOVER), err[-3000:]
    slow = _cli(["hist", "-m", "27", "--5ptrim", "5", "-o", "slow.hist", reads], STREAMING, str(tmp_path))
    assert "device scan of" not in slow and "host strip of" not in slow and "by the team" not in slow, slow[-3000:]
    body = _body(tmp_path / "fast.hist")
    assert len(body) > 10 and body == _body(tmp_path / "slow.hist")


def test_cli_comp_5ptrim_lists_take_the_strip_and_the_scan(cases, tmp_path):
    reads, plainhdr, contigs = (os.path.join(cases, n) for n in ("reads.fq", "plainhdr.fq", "contigs.fa"))
    args = ["comp", "-m", "21", "--d1_5ptrim", "5,0", "--d2_5ptrim", "2"]
    err = _cli(args + ["-o", "fast", reads + " " + plainhdr, contigs], STRIP_4K, str(tmp_path))
    for line in ("host strip of " + reads, "host strip of " + plainhdr, "device scan of " + contigs):
        assert line in err, (line, err[-3000:])
    assert not any(h in err for h in scan_trim_cases.HANDOVER), err[-3000:]
    slow = _cli(args + ["-o", "slow", reads + " " + plainhdr, contigs], STREAMING, str(tmp_path))
    assert "device scan of" not in slow and "host strip of" not in slow, slow[-3000:]
    body = _body(tmp_path / "fast-main.mx")
    assert len(body) > 10 and body == _body(tmp_path / "slow-main.mx")
