"""tests/record_stats_model.py -- the statement the GPU's per-record statistics are held to -- against the oracle's own end-to-end
answers (every column of the -stats.tsv that `kat sect -n` and `kat cold` write) and on hand-made records."""
import math
import os

import numpy as np

from tests import naive
from tests import record_stats_model as rm
from tests.test_oracle_sect import make_cases


def _model_of_file(ko, table, path, canonical=None):
    recs = naive.seqan_records(path)
    joined, st, ln = rm.join_records([s for _, s in recs])
    counts, _ = ko.profile(table, joined, canonical)
    return recs, rm.record_stats(joined, st, ln, table.k, counts)


def test_model_against_oracle_sect(ko, refdata, tmp_path):
    t = ko.Table.from_jf(os.path.join(refdata, "ecoli.header.jf27"))
    for name in ("sect_test.fa", "sect_length_test.fa"):
        p = os.path.join(refdata, name)
        ko.sect(t, p, str(tmp_path / name), no_count_stats=True)
        recs, stats = _model_of_file(ko, t, p)
        want = rm.SECT_HEADER + b"".join(rm.sect_row(n, len(s), 27, st) for (n, s), st in zip(recs, stats))
        assert (tmp_path / (name + "-stats.tsv")).read_bytes() == want
        assert not (tmp_path / (name + "-counts.cvg")).exists()


def test_model_against_oracle_cold(ko, refdata, tmp_path):
    paths, fa = make_cases(tmp_path)
    r1 = os.path.join(refdata, "ecoli_r1.1K.fastq")
    seen_nan = False
    for k, cr, ca in ((7, False, False), (15, True, False), (27, False, True)):
        reads = ko.Table(k, cr).count_files([r1, paths[2]])
        asm = ko.Table(k, ca).count_files([fa, os.path.join(refdata, "sect_test.fa")])
        for p in (paths[0], paths[3], os.path.join(refdata, "sect_test.fa")):
            ko.cold(reads, asm, p, str(tmp_path / "c"))
            recs, rs = _model_of_file(ko, reads, p)
            _, as_ = _model_of_file(ko, asm, p)
            want = rm.COLD_HEADER + b"".join(rm.cold_row(n, len(s), k, a, b) for (n, s), a, b in zip(recs, rs, as_))
            assert (tmp_path / "c-stats.tsv").read_bytes() == want, (k, p)
            seen_nan |= b"-nan" in want
    assert seen_nan                                   # the all-N and the empty record of make_cases


def _one(seq, counts, k):
    st = rm.one_record(rm.as_bytes(seq), np.array(counts, np.uint64), k)
    return tuple(int(st[f]) for f in rm.FIELDS)


def test_hand_cases():
    # (sum, median, non_zero, invalid, gc_bases, n_bases)
    assert _one(b"ACGTA", [3, 9], 4) == (12, 9, 2, 0, 2, 0)                     # nb == 2: sorted[1], the larger count
    assert _one(b"ACGTA", [9, 3], 4) == (12, 9, 2, 0, 2, 0)
    assert _one(b"ACGT", [7], 4) == (7, 7, 1, 0, 2, 0)                          # nb == 1
    assert _one(b"ACG", [], 4) == (0, 0, 0, 0, 2, 0)                            # shorter than k: the bases still count
    assert _one(b"", [], 4) == (0, 0, 0, 0, 0, 0)                               # empty
    assert _one(b"NNNNNN", [5, 5, 5], 4) == (0, 0, 0, 3, 0, 6)                  # all N: counts of invalid windows are ignored
    assert _one(b"acgtac", [1, 2, 3], 4) == (6, 2, 3, 0, 3, 0)                  # lower case
    # junk other than N: windows 0..2 hold the '-' and are invalid; it counts for neither G/C nor N
    assert _one(b"AC-TACGT", [9, 9, 9, 4, 6], 4) == (10, 0, 2, 3, 3, 0)
    assert _one(b"ACGTACGTA", [5, 1, 5, 5, 1, 9], 4) == (26, 5, 6, 0, 4, 0)     # ties around the median: 1 1 5 5 5 9 -> [3]
    assert _one(b"ACGTACG", [2, 2, 2, 2], 4)[1] == 2
    # the median is an invalid window's zero: counts 0 0 0 0 | 8 9 -> sorted[3] = 0 although every valid window is covered
    assert _one(b"ACGNACGTA", [7, 7, 7, 7, 8, 9], 4) == (17, 0, 2, 4, 4, 1)
    assert _one(b"ACGTA", [(1 << 63) + 1, (1 << 63) + 2], 4)[0] == 3            # the sum is a 64-bit word


def test_rows_and_nan():
    st = rm.one_record(rm.as_bytes(b"NNNNNN"), np.zeros(3, np.uint64), 4)
    assert rm.sect_row(b"x", 6, 4, st) == b"x\t0\t0.00000\t-nan\t6\t3\t3\t100.00000\t0\t0.00000\t0.00000\n"
    st = rm.one_record(rm.as_bytes(b"AC"), np.zeros(0, np.uint64), 4)
    assert rm.sect_row(b"s", 2, 4, st) == b"s\t0\t0.00000\t0.50000\t2\t%d\t0\t0.00000\t0\t0.00000\t0.00000\n" % (2 ** 32 - 1)
    assert math.isclose(float(rm.sect_row(b"y", 5, 4, rm.one_record(rm.as_bytes(b"ACGTA"), np.array([3, 9], np.uint64), 4)).split(b"\t")[2]), 6.0)


def test_record_stats_takes_windows_inside_records_only():
    bases = b"ACGTACGTTTGGCCAA"
    counts = np.arange(1, len(bases) - 4 + 2, dtype=np.uint64)                   # k = 4: 13 windows, count i + 1 at start i
    st = rm.record_stats(bases, [0, 6, 6, 11], [6, 0, 5, 5], 4, counts)          # adjacent records, an empty one between them
    assert [int(x) for x in st["sum"]] == [1 + 2 + 3, 0, 7 + 8, 12 + 13]
    assert [int(x) for x in st["median"]] == [2, 0, 8, 13]
