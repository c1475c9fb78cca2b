"""`katgpu sect|cold --gpus N`: the hashes lie on the ranks by owner, every rank reads the sequence file, and the per-position counts
reach rank 0 through katgpu_table_profile_gathered_host -- which alone writes the outputs.  Every file of the multi run is the plain
run's, byte for byte (.jf hashes: their header's "time" and "pwd" apart), nothing else appears beside them, and rank 0's
profile_gathered timing lines are on stderr.  Tiny inputs, as tests/test_gpu_cli_dump_gathered.py has them; the ranks share the device
over /dev/shm, and batches of 1000 window starts put several batches on the 4000-base assembly."""
import os
import re
import subprocess

import numpy as np
import pytest

from kat_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kat_amd", "bin", "katgpu")
TIMING = re.compile(r'katgpu_timing \{"phase": "profile_gathered", "batches": (\d+), "ranks": (\d+), "records": (\d+), "wire_bytes": (\d+)\}')


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """A 4000-base genome, a 6x read pair off it, and the genome as an assembly of four contigs: a plain one, one shorter than any k
    here, one with runs of N, one partly in lowercase."""
    d = tmp_path_factory.mktemp("tiny_profile")
    g = synth.genome(4000, seed=20261019)
    synth.write_fastq_pair(str(d / "pair_R1.fq"), str(d / "pair_R2.fq"), synth.reads(g, 0, 160, seed=3))
    with_n = np.array(g[1500:2500])
    with_n[100:103] = ord("N")
    with_n[400:460] = ord("N")
    with_n[999] = ord("n")
    contigs = [g[:1500].tobytes(), g[1480:1500].tobytes(), with_n.tobytes(), g[2500:3200].tobytes() + g[3200:4000].tobytes().lower()]
    with open(d / "asm.fa", "wb") as f:
        for i, c in enumerate(contigs):
            f.write(b">contig%d some words\n" % i)
            for o in range(0, len(c), 80):
                f.write(c[o:o + 80] + b"\n")
    return d


def _go(args, cwd, env, expect=0):
    os.makedirs(cwd, exist_ok=True)
    r = subprocess.run([EXE] + args, cwd=cwd, capture_output=True, text=True, timeout=120, env=env)
    if r.returncode and "did not return within" in r.stderr and "KATGPU_COMM_INIT_TIMEOUT_S" in r.stderr:
        pytest.skip("RCCL's bootstrap did not come back on this box: " + r.stderr[-300:])
    assert r.returncode == expect, (args, r.stdout[-1500:], r.stderr[-3000:])
    return r


def _jf(path):
    """(header without its "time" and "pwd" fields, records); the runs' directories have names of one length, so the padding is the same."""
    b = open(path, "rb").read()
    h = int(b[:9])
    return re.sub(rb'"(time|pwd)":"[^"]*"', b"", b[9:9 + h]), b[9 + h:]


def _env():
    env = dict(os.environ, KATGPU_TESTING="1", KATGPU_TIMING="1", KATGPU_COMM_TRANSPORT="shm", KATGPU_TEST_GATHER_BATCH="1000")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("KATGPU_COMM_INIT_TIMEOUT_S", "60")
    return env


# mode, options, k, ranks, the timing lines a run must print (one per collective call: the assembly is one batch of records)
@pytest.mark.parametrize("mode,opts,k,gpus,calls", [
    ("sect", [], 27, 2, 1),
    ("sect", ["-n", "-g", "-E", "-F", "-M", "2", "-G", "5"], 27, 3, 1),
    ("sect", ["-N"], 27, 3, 1),
    ("sect", ["-d"], 27, 2, 1),
    ("sect", [], 41, 3, 1),
    ("cold", [], 27, 2, 2),
    ("cold", ["-d"], 27, 3, 2)])
def test_gpus_run_writes_the_plain_runs_bytes(tiny, tmp_path, mode, opts, k, gpus, calls):
    env = _env()
    args = opts + ["-m", str(k), "-o", "out", str(tiny / "asm.fa"), str(tiny / "pair_R1.fq"), str(tiny / "pair_R2.fq")]
    _go([mode] + args, str(tmp_path / "plain"), env)
    r = _go([mode, "--gpus", str(gpus)] + args, str(tmp_path / "multi"), env)
    lines = TIMING.findall(r.stderr)
    assert len(lines) == calls, r.stderr[-3000:]
    for batches, ranks, records, wire in lines:
        assert int(ranks) == gpus and int(batches) >= 4 and int(records) > 1000, lines
        assert 0 < int(wire) <= 12 * int(records), lines          # some of the windows' k-mers live on another rank than 0
    plain, multi = sorted(os.listdir(tmp_path / "plain")), sorted(os.listdir(tmp_path / "multi"))
    assert plain == multi, (plain, multi)                            # every output, and no stray file
    assert "out-stats.tsv" in plain and (mode == "cold" or "-n" in opts or "out-counts.cvg" in plain)
    assert len(plain) == 1 + (mode == "sect" and "-n" not in opts) + 3 * ("-E" in opts) + ("-d" in opts) * (2 if mode == "cold" else 1), plain
    for name in plain:
        a, b = tmp_path / "plain" / name, tmp_path / "multi" / name
        assert not os.path.islink(a) and not os.path.islink(b)
        if ".jf" in name:
            assert _jf(a) == _jf(b), name
        else:
            assert a.read_bytes() == b.read_bytes(), name
            assert a.stat().st_size > 0, name
    stats = (tmp_path / "multi" / "out-stats.tsv").read_text().splitlines()
    assert len(stats) == 5 and stats[2].split("\t")[1:3] == ["0", "0.00000"]       # (the contig shorter than k has no window)


def test_filter_is_still_refused(tiny, tmp_path):
    r = _go(["filter", "kmer", "--gpus", "2", str(tiny / "asm.fa")], str(tmp_path / "f"), _env(), expect=1)
    assert "--gpus applies to hist, gcp and comp" in r.stderr
    assert os.listdir(tmp_path / "f") == []
