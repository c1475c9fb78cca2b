"""tests/record_regions_model.py -- the statement the GPU's count-range regions are held to -- against the oracle's own end-to-end
answers: its renderer's text, byte for byte, against the -non_repetitive.fa and -repetitive.fa that `kat sect -E -F` writes, on the
reference's test data and on a synthetic assembly with real repeats; and its intervals on hand-made records."""
import os

import numpy as np

from tests import naive
from tests import record_regions_model as gm
from tests import record_stats_model as rm


def _check_file(ko, table, path, tmp_path, min_repeat, max_repeat, canonical=None):
    """both .fa files of one oracle run against the model; returns how many regions each holds"""
    prefix = str(tmp_path / "o")
    ko.sect(table, path, prefix, canonical=canonical, no_count_stats=True, extract_nr=True, extract_r=True, min_repeat=min_repeat, max_repeat=max_repeat)
    recs = naive.seqan_records(path)
    joined, st, ln = rm.join_records([s for _, s in recs])
    counts, _ = ko.profile(table, joined, canonical)
    ranges = [(1, min_repeat), (min_repeat, max_repeat)]
    found = gm.regions(joined, st, ln, table.k, counts, ranges)
    for suffix, f, (lo, hi) in zip(("-non_repetitive.fa", "-repetitive.fa"), found, ranges):
        want = open(prefix + suffix, "rb").read()
        assert gm.render(recs, f, table.k, lo, hi) == want, (path, suffix, min_repeat, max_repeat)
        assert want.count(b"\n") == 2 * f.shape[0]
    return [f.shape[0] for f in found]


def test_renderer_against_oracle_on_the_reference_data(ko, refdata, tmp_path):
    r1 = os.path.join(refdata, "ecoli_r1.1K.fastq")
    tables = [ko.Table.from_jf(os.path.join(refdata, "ecoli.header.jf27")), ko.Table(27, True).count_files([r1]), ko.Table(11, False).count_files([r1])]
    seen = np.zeros(2, np.int64)
    for t in tables:
        for name in ("sect_test.fa", "sect_length_test.fa"):
            for min_repeat, max_repeat in ((2, 5), (2, 0), (1, 1), (3, 2)):
                seen += _check_file(ko, t, os.path.join(refdata, name), tmp_path, min_repeat, max_repeat)
    assert seen[0] > 10 and seen[1] > 10, seen


def _synthetic(tmp_path):
    """an assembly with real repeats: a unit that occurs two to six times, contigs that are one run, that end in a run, that hold N and
    lower case, one shorter than any k used, one empty"""
    rng = np.random.default_rng(7)
    seq = lambda n: bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))
    unit, unit2 = seq(300), seq(90)
    recs = [(b"two copies", seq(500) + unit + seq(40) + unit + seq(333)),
            (b"ends_in_a_repeat", seq(700) + unit),
            (b"all_repeat", unit),
            (b"starts_with_one", unit2 + seq(200) + unit2.lower() + seq(1)),
            (b"with_N", seq(100) + b"N" + unit2 + b"NN" + seq(150) + unit + b"n" + seq(80)),
            (b"unique", seq(1234)),
            (b"short", b"ACG"),
            (b"empty", b""),
            (b"tail", unit2 + unit2 + unit2)]
    fa = tmp_path / "asm.fa"
    with open(fa, "wb") as f:
        for name, s in recs:
            f.write(b">" + name + b"\n" + b"".join(s[i:i + 60] + b"\n" for i in range(0, len(s), 60)))
    return str(fa)


def test_renderer_against_oracle_on_repeats(ko, tmp_path):
    fa = _synthetic(tmp_path)
    seen = np.zeros(2, np.int64)
    for k, canonical in ((1, False), (2, True), (5, True), (21, True), (21, False), (32, True), (45, True)):
        t = (ko.WideTable(k, canonical) if k > 32 else ko.Table(k, canonical)).count_files([fa])
        for min_repeat, max_repeat in ((2, 5), (2, 0), (3, 4), (0, 3), (6, 6)):
            got = _check_file(ko, t, fa, tmp_path, min_repeat, max_repeat)
            if k >= 21:
                seen += got
    assert seen[0] > 50 and seen[1] > 50, seen


def _regions(bases, starts, lens, k, counts, ranges):
    return [f.tolist() for f in gm.regions(bases, starts, lens, k, np.array(counts, np.uint64), ranges)]


def test_hand_cases():
    b = b"ACGTACGTAC"                                           # k = 3: 8 windows
    c = [1, 2, 2, 0, 5, 5, 9, 1]
    assert _regions(b, [0], [10], 3, c, [(2, 5)]) == [[[0, 1, 3], [0, 4, 6]]]
    assert _regions(b, [0], [10], 3, c, [(1, 0)]) == [[[0, 0, 3], [0, 4, 8]]]              # max == 0: no upper bound; stop == nb
    assert _regions(b, [0], [10], 3, c, [(0, 0)]) == [[[0, 0, 8]]]                         # the whole record is one run
    assert _regions(b, [0], [10], 3, c, [(5, 2)]) == [[]]                                  # min > max > 0
    assert _regions(b, [0], [10], 3, c, [(9, 9), (1, 1)]) == [[[0, 6, 7]], [[0, 0, 1], [0, 7, 8]]]   # runs of length 1
    # an invalid window counts 0 whatever the array says: in range only when min == 0
    assert _regions(b"ACNTACG", [0], [7], 3, [7] * 5, [(1, 0), (0, 0), (0, 3)]) == [[[0, 3, 5]], [[0, 0, 5]], [[0, 0, 3]]]
    # records: windows inside a record only; starts and stops count from the record's first window
    assert _regions(b, [0, 5], [5, 5], 3, [1] * 8, [(1, 0)]) == [[[0, 0, 3], [1, 0, 3]]]
    assert _regions(b, [1, 4, 4, 9], [2, 0, 4, 1], 3, [1] * 8, [(1, 0)]) == [[[2, 0, 2]]]  # shorter than k, empty
    # touching records at k = 1: the last window of one and the first of the next are neighbours, and still two regions
    assert _regions(b"AAAAAA", [0, 3], [3, 3], 1, [4] * 6, [(1, 0)]) == [[[0, 0, 3], [1, 0, 3]]]
    assert _regions(b"AAAAAA", [0, 1, 2], [1, 1, 4], 1, [4] * 6, [(4, 4)]) == [[[0, 0, 1], [1, 0, 1], [2, 0, 4]]]


def test_render_quirks():
    seq = b"ACGTTGCAAT"                                          # k = 4: nb = 7
    # a run that ends inside the record: seq[1:3], then seq[4:6] -- the base at stop = 3 is skipped; length = end - start - 1
    assert gm.render_record(b"x y", seq, [(1, 3)], 4, 2, 5) == b">x y___region:1_length:4_pos:2:6_cov:2-5\nCGTG\n"
    # a run that reaches the last window: everything to the record's end
    assert gm.render_record(b"x", seq, [(5, 7)], 4, 1, 0) == b">x___region:1_length:4_pos:6:10_cov:1+\nGCAAT\n"
    assert gm.render_record(b"x", seq, [(0, 1), (5, 7)], 4, 1, 2).count(b"___region:2_") == 1
    # k = 1: end = stop, length = run - 1, nothing follows the run
    assert gm.render_record(b"x", b"ACGT", [(1, 2), (3, 4)], 1, 1, 2) == b">x___region:1_length:0_pos:2:2_cov:1-2\nC\n>x___region:2_length:0_pos:4:4_cov:1-2\nT\n"
    assert gm.render([(b"a", seq), (b"b", b""), (b"c", seq)], [[2, 5, 7]], 4, 1, 0) == b">c___region:1_length:4_pos:6:10_cov:1+\nGCAAT\n"
