"""`katgpu filter seq --gpus N`: the hash lies on the ranks by owner, every rank reads the sequence file(s) and cuts the same batches,
and the per-record hits are summed on rank 0 through katgpu_table_seq_hits_gathered_host -- which alone opens, decides and writes.
Every file of the multi run is the plain run's, byte for byte, nothing else appears beside them, and rank 0's seq_hits_gathered timing
line is on stderr.  Tiny inputs, as tests/test_gpu_cli_gathered_profile.py has them: the hash is counted from the first 1500 bases of a
4000-base genome, so reads from elsewhere score 0 and some reads are kept, some not.  The ranks share the device over /dev/shm, and
batches of 1000 bases put several batches on every input.  (-f is never used: it draws from random_device.)"""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

from kat_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kat_amd", "bin", "katgpu")
TIMING = re.compile(r'katgpu_timing \{"phase": "seq_hits_gathered", "batches": (\d+), "ranks": (\d+), "records": (\d+), "wire_bytes": (\d+)\}')
FOUND = re.compile(r"Found (\d+) / (\d+) to keep")
INPUTS = {"pair_R1.fq", "pair_R2.fq", "head.fa", "asm.fa", "jf/head-hash.jf27"}      # the fixture's files


def _env(**extra):
    env = dict(os.environ, KATGPU_TESTING="1", KATGPU_TIMING="1", KATGPU_COMM_TRANSPORT="shm", KATGPU_TEST_HITS_BATCH="1000")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("KATGPU_COMM_INIT_TIMEOUT_S", "60")
    env.update(extra)
    return env


def _go(args, cwd, env, expect=0):
    os.makedirs(cwd, exist_ok=True)
    r = subprocess.run([EXE] + args, cwd=cwd, capture_output=True, text=True, timeout=120, env=env)
    if r.returncode and "did not return within" in r.stderr and "KATGPU_COMM_INIT_TIMEOUT_S" in r.stderr:
        pytest.skip("RCCL's bootstrap did not come back on this box: " + r.stderr[-300:])
    assert r.returncode == expect, (args, r.stdout[-1500:], r.stderr[-3000:])
    return r


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    """A 4000-base genome, 160 read pairs off it, its first 1500 bases as the sequence the hash is counted from (and that hash as a
    .jf27 file, written by `hist -d`), and the genome as an assembly of five contigs: a plain one, one shorter than k, one with runs
    of N, one partly in lowercase, one of N alone."""
    d = tmp_path_factory.mktemp("tiny_filter_seq")
    g = synth.genome(4000, seed=20261019)
    synth.write_fastq_pair(str(d / "pair_R1.fq"), str(d / "pair_R2.fq"), synth.reads(g, 0, 320, seed=3))
    synth.write_fasta(str(d / "head.fa"), g[:1500], name="head")
    with_n = np.array(g[1500:2500])
    with_n[100:103] = ord("N")
    with_n[400:460] = ord("N")
    with_n[999] = ord("n")
    contigs = [g[:1500].tobytes(), g[1480:1500].tobytes(), with_n.tobytes(), g[2500:3200].tobytes() + g[3200:4000].tobytes().lower(), b"N" * 40]
    with open(d / "asm.fa", "wb") as f:
        for i, c in enumerate(contigs):
            f.write(b">contig%d some words\n" % i)
            for o in range(0, len(c), 80):
                f.write(c[o:o + 80] + b"\n")
    _go(["hist", "-d", "-m", "27", "-o", "head", str(d / "head.fa")], str(d / "jf"), _env())
    assert os.path.exists(d / "jf" / "head-hash.jf27")
    return d


def _same_files(plain, multi):
    a, b = sorted(os.listdir(plain)), sorted(os.listdir(multi))
    assert a == b, (a, b)                                            # every output, and no stray file
    for name in a:
        assert not os.path.islink(plain / name) and not os.path.islink(multi / name)
        assert (plain / name).read_bytes() == (multi / name).read_bytes(), name
    return a


# options (the inputs' names are completed below), ranks, the files a run leaves
@pytest.mark.parametrize("opts,gpus,transport,files", [
    (["--seq", "pair_R1.fq", "head.fa"], 2, "shm", ["out.in.fq"]),
    (["--seq", "pair_R1.fq", "--seq2", "pair_R2.fq", "-s", "--stats", "head.fa"], 3, "shm",
     ["out.in.R1.fq", "out.in.R2.fq", "out.out.R1.fq", "out.out.R2.fq", "out.stats"]),
    (["-i", "-T", "0.5", "--seq", "pair_R1.fq", "head.fa"], 2, "shm", ["out.in.fq"]),
    (["-m", "41", "--seq", "pair_R1.fq", "--stats", "head.fa"], 3, "shm", ["out.in.fq", "out.stats"]),
    (["--seq", "pair_R1.fq", "--stats", "jf/head-hash.jf27"], 2, "shm", ["out.in.fq", "out.stats"]),
    (["--seq", "asm.fa", "-s", "--stats", "head.fa"], 2, "shm", ["out.in.fa", "out.out.fa", "out.stats"]),
    (["--seq", "pair_R1.fq", "--seq2", "pair_R2.fq", "--stats", "head.fa"], 1, "rccl", ["out.in.R1.fq", "out.in.R2.fq", "out.stats"])])
def test_gpus_run_writes_the_plain_runs_bytes(tiny, tmp_path, opts, gpus, transport, files):
    env = _env(KATGPU_COMM_TRANSPORT=transport)
    args = ["-o", "out"] + [str(tiny / a) if a in INPUTS else a for a in opts]
    p = _go(["filter", "seq"] + args, str(tmp_path / "plain"), env)
    assert not TIMING.search(p.stderr)                                # (the plain run is katgpu_table_seq_hits_host's)
    keepers, total = map(int, FOUND.search(p.stdout).groups())
    assert 0 < keepers < total, p.stdout[-1000:]
    r = _go(["filter", "seq", "--gpus", str(gpus)] + args, str(tmp_path / "multi"), env)
    assert FOUND.search(r.stdout).groups() == FOUND.search(p.stdout).groups()
    lines = TIMING.findall(r.stderr)
    assert len(lines) == 1, r.stderr[-3000:]                          # one batch of entries: one collective call
    batches, ranks, records, wire = map(int, lines[0])
    paired = "--seq2" in opts
    assert ranks == gpus and batches >= 3 and records == total * (2 if paired else 1) and wire == 8 * records * (gpus - 1), lines
    assert _same_files(tmp_path / "plain", tmp_path / "multi") == files
    for name in files:
        assert (tmp_path / "multi" / name).stat().st_size > 0, name
    if "--stats" in opts:
        rows = [ln.split("\t") for ln in (tmp_path / "multi" / "out.stats").read_text().splitlines()[1:]]
        assert len(rows) == total and any(int(row[3]) > 0 for row in rows) and any(int(row[3]) == 0 and int(row[2]) > 0 for row in rows)
        if "asm.fa" in " ".join(opts):
            assert rows[1][1:] == ["20", "0", "0", "-nan"] and rows[4][1:] == ["40", "14", "0", "0"]      # shorter than k: 0 / 0; all N: no hit


@pytest.mark.parametrize("name,left", [("reads.xyz", []), ("reads.fq.gz", ["out.in.gz", "out.stats"])])
def test_unknown_extension_ends_every_rank_as_the_plain_run_ends(tiny, tmp_path, name, left):
    """A sequence extension nobody can place: exit 5 from a run of three ranks, within the timeout, and what the plain run leaves.
    reads.xyz stops every rank where it opens its input; reads.fq.gz is read, but names the outputs *.gz, which no rank can write: the
    plain run leaves the empty file it opened before it saw the name and the .stats header, and so does rank 0 -- alone."""
    os.makedirs(tmp_path / "in")
    raw = (tiny / "pair_R1.fq").read_bytes()
    (tmp_path / "in" / name).write_bytes(gzip.compress(raw) if name.endswith(".gz") else raw)
    args = ["-o", "out", "--stats", "--seq", str(tmp_path / "in" / name), str(tiny / "head.fa")]
    p = _go(["filter", "seq"] + args, str(tmp_path / "plain"), _env(), expect=5)
    r = _go(["filter", "seq", "--gpus", "3"] + args, str(tmp_path / "multi"), _env(), expect=5)
    assert "Unknown file extension" in p.stderr and "Unknown file extension" in r.stderr
    assert not TIMING.search(r.stderr)
    assert _same_files(tmp_path / "plain", tmp_path / "multi") == left
    if left:
        assert (tmp_path / "multi" / "out.in.gz").stat().st_size == 0
