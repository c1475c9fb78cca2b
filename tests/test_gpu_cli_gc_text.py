"""`katgpu sect -g` on one GPU where nothing per position is written (-n) or where the text comes from the device
(KATGPU_SECT_DEVICE_TEXT=1): the lines of -counts.gc are rendered on the device (katgpu_record_gc_text_host) and the run says how many
bytes of them it received.  -counts.gc and -stats.tsv are the oracle's, byte for byte; the plain path and --gpus 2, which keep making
the lines on the host, write the same bytes."""
import json
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kat_amd", "bin", "katgpu")
TIMING = re.compile(r'^katgpu_timing (\{"phase": "sect_coverage".*\})$', re.M)


@pytest.fixture(scope="module")
def inputs(refdata, tmp_path_factory):
    """Several thousand records (the reads of the reference's test data and pieces of them, some with N, some shorter than k, one
    empty) and one long contig, as FASTA (the recipe of tests/test_gpu_record_stats.py)."""
    from tests import filter_model as fm
    r1 = os.path.join(refdata, "ecoli_r1.1K.fastq")
    reads = [s for _, s, _ in fm.read_records(r1)]
    recs = []
    for i, s in enumerate(reads):
        recs += [("r%d" % i, s), ("h%d some words" % i, s[: len(s) // 2]), ("n%d" % i, s[:30] + "N" + s[31:70].lower()), ("t%d" % i, s[-(i % 60):] if i % 60 else "")]
    recs.insert(1500, ("contig", "".join(reads[:400]) + "NNNN" + "".join(reads[400:500])))
    fa = tmp_path_factory.mktemp("gc_text_cli") / "records.fa"
    with open(fa, "w") as f:
        for name, seq in recs:
            f.write(">" + name + "\n" + "".join(seq[i:i + 70] + "\n" for i in range(0, len(seq), 70)))
    assert len(recs) > 4000 and len(recs[1500][1]) > 40000
    return str(fa), r1, len(recs)


_WANT = {}


def _want(ko, inputs, tmp_path_factory, k, extract=False):
    """the oracle's files for the inputs at k: made once"""
    if (k, extract) not in _WANT:
        fa, r1, _ = inputs
        prefix = str(tmp_path_factory.mktemp("gc_text_want") / "want")
        table = (ko.WideTable(k, True) if k > 32 else ko.Table(k, True)).count_files([r1])
        ko.sect(table, fa, prefix, no_count_stats=True, output_gc_stats=True, extract_nr=extract, extract_r=extract, min_repeat=2, max_repeat=5 if extract else 0)
        _WANT[(k, extract)] = prefix
    return _WANT[(k, extract)]


def _run(args, cwd, **env):
    e = dict(os.environ, KATGPU_TESTING="1", KATGPU_TIMING="1", **env)
    os.makedirs(cwd, exist_ok=True)
    r = subprocess.run([EXE] + args, cwd=cwd, capture_output=True, text=True, timeout=300, env=e)
    assert r.returncode == 0, (args, r.stdout[-1500:], r.stderr[-3000:])
    return r


def _gc_text_bytes(r):
    lines = TIMING.findall(r.stderr)
    assert len(lines) == 1, r.stderr[-3000:]
    fields = json.loads(lines[0])
    assert "gc_text_bytes" in fields, fields
    return fields["gc_text_bytes"]


def _same(cwd, want, suffixes):
    for suffix in suffixes:
        got, exp = open(os.path.join(cwd, "out" + suffix), "rb").read(), open(want + suffix, "rb").read()
        assert len(exp) > 0 and got == exp, suffix


def _body_bytes(path, n_records):
    """the size of a -counts.gc without its ">name" lines"""
    lines = open(path, "rb").read().split(b"\n")
    names = [x for x in lines[0::2] if x.startswith(b">")]
    assert len(names) == n_records and lines[-1] == b"" and len(lines) == 2 * n_records + 1
    return sum(len(x) + 1 for x in lines[1::2])


@pytest.mark.parametrize("opts,k,extract,device_text", [
    (["-n", "-g"], 27, False, False),
    (["-n", "-g", "-m", "45"], 45, False, False),
    (["-n", "-g", "-E", "-F", "-M", "2", "-G", "5", "-t", "3"], 27, True, False),
    (["-g"], 27, False, True)], ids=["n", "wide", "EF_t3", "device_text"])
def test_gc_lines_come_from_the_device(ko, inputs, tmp_path_factory, tmp_path, opts, k, extract, device_text):
    fa, r1, n_records = inputs
    want = _want(ko, inputs, tmp_path_factory, k, extract)
    env = dict(KATGPU_TEST_FORBID_PROFILE_HOST="1")
    if device_text:
        env["KATGPU_SECT_DEVICE_TEXT"] = "1"
    cwd = str(tmp_path / "device")
    r = _run(["sect"] + opts + ["-H", "1000000", "-o", "out", fa, r1], cwd, **env)
    _same(cwd, want, ["-counts.gc", "-stats.tsv"] + (["-non_repetitive.fa", "-repetitive.fa"] if extract else []))
    body = _body_bytes(os.path.join(cwd, "out-counts.gc"), n_records)
    assert body > 500_000 and _gc_text_bytes(r) == body
    assert os.path.exists(os.path.join(cwd, "out-counts.cvg")) == device_text


def test_plain_and_gpus_paths_write_the_same_bytes(ko, inputs, tmp_path_factory, tmp_path):
    """Without -n and without the switch the lines are made on the host from the per-position walk, as before; so they are under --gpus."""
    fa, r1, _ = inputs
    want = _want(ko, inputs, tmp_path_factory, 27)
    r = _run(["sect", "-g", "-H", "1000000", "-o", "out", fa, r1], str(tmp_path / "plain"))
    assert _gc_text_bytes(r) == 0
    _same(str(tmp_path / "plain"), want, ["-counts.gc", "-stats.tsv"])
    env = {"KATGPU_COMM_TRANSPORT": "shm", "HSA_ENABLE_IPC_MODE_LEGACY": os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"),
           "KATGPU_COMM_INIT_TIMEOUT_S": os.environ.get("KATGPU_COMM_INIT_TIMEOUT_S", "60")}
    _run(["sect", "--gpus", "2", "-g", "-H", "1000000", "-o", "out", fa, r1], str(tmp_path / "gpus"), **env)
    _same(str(tmp_path / "gpus"), want, ["-counts.gc", "-stats.tsv"])
