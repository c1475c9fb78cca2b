"""CPU checks of tests/filter_model.py (the restatement of `kat filter`) and of the `katgpu filter` command-line rules that need no
device: routing, defaults, SeqAn's wrapping, the -nan record, pair concatenation, the dispatcher and the box errors."""
import os
import subprocess

import numpy as np
import pytest

from tests import filter_model as fm
from tests import independent

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "kat_amd", "bin", "katgpu")


def test_routing_truth_table():
    # src/filter_kmer.cc:262-281: without separate keep = in_bounds != invert; with separate invert is ignored
    want = {(True, False, False): "keep", (False, False, False): None, (True, True, False): None, (False, True, False): "keep",
            (True, False, True): "keep", (False, False, True): "drop", (True, True, True): "keep", (False, True, True): "drop"}
    for (inb, inv, sep), w in want.items():
        assert fm.route(inb, inv, sep) == w


def test_filter_kmer_model_counters_and_gc():
    k = 5
    keys = np.array([independent_key(s) for s in ("AAAAA", "CCCCC", "ACGTA", "TTTTT", "GGGCA")], np.uint64)
    counts = np.array([3, 20000, 5, 1, 7], np.uint64)
    assert list(fm.gc_of(keys, k)) == [0, 5, 2, 0, 4]
    keep, drop, ctr = fm.filter_kmer(keys, counts, k)                       # defaults: count 1..10000, GC 1..100
    assert list(keep) == [False, False, True, False, True] and not drop.any()
    assert ctr == dict(all_distinct=5, all_total=20016, keep_distinct=2, keep_total=12, drop_distinct=0, drop_total=0)
    keep, drop, ctr = fm.filter_kmer(keys, counts, k, invert=True, separate=True)   # invert ignored with separate
    assert list(keep) == [False, False, True, False, True] and list(drop) == [True, True, False, True, False]
    assert ctr["keep_total"] + ctr["drop_total"] == ctr["all_total"]
    assert fm.kmer_stdout_lines(ctr, True)[2] == "K-mers to discard : 3 distinct; 20004 total."


def independent_key(s):
    v = 0
    for ch in s:
        v = (v << 2) | "ACGT".index(ch)
    return v


def test_defaults_are_mains():
    assert fm.KMER_DEFAULTS == dict(output_prefix="kat.filter.kmer", low_count=1, high_count=10000, low_gc=1, high_gc=100, invert=False, separate=False)
    assert fm.SEQ_DEFAULTS["output_prefix"] == "kat.filter.kmer" and fm.SEQ_DEFAULTS["threshold"] == 0.1 and fm.SEQ_DEFAULTS["frequency"] == 0.0
    # the quirks these imply: an all-A/T k-mer (GC 0) and a k-mer counted more than 10000 times are dropped
    keep, _, _ = fm.filter_kmer(np.array([0, 0b0110], np.uint64), np.array([5, 10001], np.uint64), 2)
    assert not keep.any()


@pytest.mark.parametrize("n", [0, 69, 70, 71, 140])
def test_fasta_wrapping(n):
    seq = ("ACGT" * 40)[:n]
    rec = fm.fasta_record("r", seq)
    lines = rec.split("\n")[1:-1]
    assert rec.startswith(">r\n") and rec.endswith("\n")
    if n == 0:
        assert rec == ">r\n\n"                                              # an empty sequence still writes one line
    else:
        assert "".join(lines) == seq and all(len(x) == 70 for x in lines[:-1]) and 0 < len(lines[-1]) <= 70
        assert len(lines) == (n + 69) // 70
    assert fm.fastq_record("r", seq, "I" * n) == "@r\n" + seq + "\n+\n" + "I" * n + "\n"


def test_nan_record_is_never_kept():
    assert fm.fmt_ratio(0, 0) == "-nan"
    for inv in (False, True):
        assert not fm.keep_decision(0, 0, 0.0, inv)
    assert fm.fmt_ratio(1, 3) == "0.333333" and fm.fmt_ratio(3, 3) == "1"
    assert fm.keep_decision(1, 10, 0.1) and not fm.keep_decision(0, 10, 0.1) and fm.keep_decision(0, 10, 0.1, invert=True)
    assert not fm.keep_decision(5, 10, 0.1, frequency=0.5, u=0.7) and fm.keep_decision(5, 10, 0.1, frequency=0.5, u=0.3)


def test_pair_concatenation():
    # R1 has 2 hits of 4 windows, R2 0 of 6: the pair is 2 / 10 = 0.2 -- kept at T 0.15 though R2 alone would not be
    table = {"AAAA": (2, 4), "CCCCCC": (0, 6)}
    r1, r2 = [("p/1", "AAAA", "")], [("p/2", "CCCCCC", "")]
    res = fm.filter_seq(r1, r2, lambda s: table[s], False, threshold=0.15)
    assert res["keepers"] == 1 and res["in"] == ">p/1\nAAAA\n" and res["in2"] == ">p/2\nCCCCCC\n"
    assert res["stats"].splitlines()[1] == "0\t10\t10\t2\t0.2"
    res = fm.filter_seq(r2, None, lambda s: table[s], False, threshold=0.15, separate=True)
    assert res["keepers"] == 0 and res["out"] == ">p/2\nCCCCCC\n"


def test_gc_of_wide_matches_string_count():
    rng = np.random.default_rng(3)
    k = 45
    s = "".join(rng.choice(list("ACGT"), k))
    v = independent_key(s)
    hi, lo = np.array([v >> 64], np.uint64), np.array([v & ((1 << 64) - 1)], np.uint64)
    assert fm.gc_of((hi, lo), k)[0] == s.count("G") + s.count("C")
    assert independent.gc_count(np.array([independent_key(s[:20])], np.uint64), 20)[0] == s[:20].count("G") + s[:20].count("C")


# ---- the command line: what is decided before the device is opened ----

def _run(args, cwd):
    return subprocess.run([EXE] + args, cwd=cwd, capture_output=True, text=True, timeout=120)


def test_filter_dispatcher(tmp_path):
    r = _run(["filter"], tmp_path)
    assert r.returncode == 1 and "kmer" in r.stdout and "seq" in r.stdout
    r = _run(["filter", "x"], tmp_path)
    assert r.returncode == 1 and "Could not recognise mode string: x" in r.stderr
    r = _run(["filter", "kmer", "--gpus", "2", "a.fa"], tmp_path)
    assert r.returncode == 1 and "--gpus applies to hist, gcp and comp" in r.stderr
    r = _run(["--help"], tmp_path)
    assert "filter" in r.stdout


def test_filter_kmer_box_errors(tmp_path):
    r = _run(["filter", "kmer", "-c", "10", "-d", "5", "x.fa"], tmp_path)
    assert r.returncode == 4 and "High kmer count value must be >= to low kmer count value" in r.stderr
    r = _run(["filter", "kmer", "-g", "10", "-h", "5", "x.fa"], tmp_path)
    assert r.returncode == 4 and "High GC count value must be >= to low GC count value" in r.stderr
    r = _run(["filter", "seq", "x.jf27"], tmp_path)
    assert r.returncode == 4 and "You must specify at least one sequence file to filter" in r.stderr
    r = _run(["filter", "seq", "--seq", "nothere.fa", "x.jf27"], tmp_path)
    assert r.returncode == 4 and "Could not find input file at: nothere.fa; please check the path and try again." in r.stderr
