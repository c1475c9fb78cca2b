"""`katgpu <mode> --gpus N -d`: the ranks' owned k-mers reach the one .jf file through katgpu_jf_dump_gathered -- ordered and packed on the
devices, gathered on rank 0's -- not through the host fallback and its .part files: the timing line of the new path is on stderr, the
file is the plain run's, and no .part file is left beside it.  Tiny inputs, as tests/test_gpu_cli.py has them, and ranges of 16 records."""
import os
import re
import subprocess

import pytest

from kat_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kat_amd", "bin", "katgpu")


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    d = tmp_path_factory.mktemp("tiny_dump")
    g = synth.genome(4000, seed=20261016)
    synth.write_fasta(str(d / "one.fa"), g[:50], contig_len=50)
    synth.write_fastq_pair(str(d / "pair_R1.fq"), str(d / "pair_R2.fq"), synth.reads(g, 0, 6, seed=3))
    return d


def _go(args, cwd, env):
    os.makedirs(cwd)
    r = subprocess.run([EXE] + args, cwd=cwd, capture_output=True, text=True, timeout=120, env=env)
    if r.returncode and "did not return within" in r.stderr and "KATGPU_COMM_INIT_TIMEOUT_S" in r.stderr:
        pytest.skip("RCCL's bootstrap did not come back on this box: " + r.stderr[-300:])
    assert r.returncode == 0, (args, r.stdout[-1500:], r.stderr[-3000:])
    return r


def _jf(path):
    """(header without its "time" and "pwd" fields, records); the runs' directories have names of one length, so the padding is the same."""
    b = open(path, "rb").read()
    h = int(b[:9])
    return re.sub(rb'"(time|pwd)":"[^"]*"', b"", b[9:9 + h]), b[9 + h:]


@pytest.mark.parametrize("mode,gpus,k,inputs,hashes", [
    ("hist", 2, 27, ["pair_R1.fq", "pair_R2.fq"], ["out-hash.jf27"]),
    ("comp", 3, 41, ["pair_R?.fq", "one.fa"], ["out-hash1.jf41", "out-hash2.jf41"])])
def test_gpus_dump_takes_the_device_path(tiny, tmp_path, mode, gpus, k, inputs, hashes):
    env = dict(os.environ, KATGPU_TESTING="1", KATGPU_TIMING="1", KATGPU_JF_RANGE_RECORDS="16", KATGPU_COMM_TRANSPORT="shm")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("KATGPU_COMM_INIT_TIMEOUT_S", "60")
    args = ["-d", "-m%d" % k, "-o", "out"] + [str(tiny / n) for n in inputs]
    _go([mode] + args, str(tmp_path / "plain"), env)
    r = _go([mode, "--gpus", str(gpus)] + args, str(tmp_path / "multi"), env)
    lines = re.findall(r'katgpu_timing \{"phase": "jf_dump_gathered".*"ranges": (\d+), "ranks": (\d+)', r.stderr)
    assert len(lines) == len(hashes), r.stderr[-3000:]                       # the new path ran for every hash, not the fallback
    assert all(int(ranks) == gpus for _, ranks in lines), lines
    assert max(int(ranges) for ranges, _ in lines) >= 2, lines               # (and range after range)
    for h in hashes:
        assert _jf(tmp_path / "plain" / h) == _jf(tmp_path / "multi" / h), h
    assert not [f for f in os.listdir(tmp_path / "multi") if f.endswith(".part")]
