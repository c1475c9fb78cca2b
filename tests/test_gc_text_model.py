"""tests/gc_text_model.py against the oracle's `kat sect -g`: on the reference's sect test files the model's lines, with the ">name"
lines between them, are the -counts.gc that ko.sect writes, byte for byte; and the widths a window's string can have.  No GPU."""
import os

import numpy as np
import pytest

from tests import gc_text_model as gm


def test_by_hand():
    # ten bytes at k = 2: records [0, 4) -> windows 0 .. 2; an empty one; one shorter than k; [5, 10) -> windows 5 .. 8; an empty one at the end
    gcs = np.array([0, 1, 2, 0, 0, -1, 2, 1, 0], np.int16)
    body, off = gm.text([0, 4, 4, 5, 10], [4, 0, 1, 5, 0], 2, gcs)
    assert body == b"0.0 50.0 100.0\n0.0\n0.0\n-0.1 100.0 50.0 0.0\n0.0\n"
    assert off.dtype == np.uint64 and off.tolist() == [0, 15, 19, 23, 43, 47]
    assert gm.record_text([], 7) == b"0.0\n" and gm.record_text([-1], 7) == b"-0.1\n" and gm.record_text([1, 2], 3) == b"33.3 66.7\n"
    assert gm.gc_file([b"a b", b"c"], [0, 4], [4, 0], 2, gcs) == b">a b\n0.0 50.0 100.0\n>c\n0.0\n"


def test_string_widths():
    for k in range(1, 64):
        for g in range(k + 1):
            s = gm.window_text(g, k)
            assert len(s) in (3, 4, 5) and (len(s) == 5) == (g == k), (k, g, s)
        assert gm.window_text(k, k) == b"100.0" and gm.window_text(0, k) == b"0.0" and gm.window_text(-1, k) == b"-0.1"


@pytest.mark.parametrize("name", ["sect_test.fa", "sect_length_test.fa"])
@pytest.mark.parametrize("k", [27, 45])
def test_model_is_the_oracles_counts_gc(ko, refdata, tmp_path, name, k):
    fa = os.path.join(refdata, name)
    names, seqs = gm.read_fasta(fa)
    b, st, ln = gm.joined(seqs)
    table = (ko.WideTable(k, True) if k > 32 else ko.Table(k, True)).count_bases(b)
    ko.sect(table, fa, str(tmp_path / "want"), output_gc_stats=True)
    want = (tmp_path / "want-counts.gc").read_bytes()
    assert want.count(b">") == len(names) and len(want) > 50
    assert gm.gc_file(names, st, ln, k, gm.oracle_gcs(ko, k, b)) == want
