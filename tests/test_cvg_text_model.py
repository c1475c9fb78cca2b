"""tests/cvg_text_model.py against the oracle's `kat sect`: on the reference's sect test files the model's lines, with the ">name" lines
between them, are the -counts.cvg that ko.sect writes for the same table, byte for byte.  No GPU."""
import os

import numpy as np
import pytest

from tests import cvg_text_model as cm


def test_by_hand():
    # ten bytes at k = 2: records [0, 4) -> windows 0 .. 2; an empty one; one shorter than k; [5, 10) -> windows 5 .. 8; an empty one at the end
    counts = np.array([0, 12, 3, 2 ** 64 - 1, 9, 7, 100, 5, 0], np.uint64)
    body, off = cm.text([0, 4, 4, 5, 10], [4, 0, 1, 5, 0], 2, counts)
    assert body == b"0 12 3\n0\n0\n7 100 5 0\n0\n"
    assert off.dtype == np.uint64 and off.tolist() == [0, 7, 9, 11, 21, 23]
    assert cm.record_text(np.array([2 ** 64 - 1], np.uint64)) == b"18446744073709551615\n"
    assert cm.record_text([]) == b"0\n"
    assert cm.cvg_file([b"a b", b"c"], [0, 4], [4, 0], 2, counts) == b">a b\n0 12 3\n>c\n0\n"


@pytest.mark.parametrize("name", ["sect_test.fa", "sect_length_test.fa"])
@pytest.mark.parametrize("k,canonical", [(5, True), (5, False), (27, True), (45, True)])
def test_model_is_the_oracles_counts_cvg(ko, refdata, tmp_path, name, k, canonical):
    fa = os.path.join(refdata, name)
    names, seqs = cm.read_fasta(fa)
    b, st, ln = cm.joined(seqs)
    table = (ko.WideTable(k, canonical) if k > 32 else ko.Table(k, canonical)).count_bases(b)
    counts, _ = ko.profile(table, b.tobytes(), canonical)
    ko.sect(table, fa, str(tmp_path / "want"))
    want = (tmp_path / "want-counts.cvg").read_bytes()
    assert want.count(b">") == len(names) and len(want) > 50
    assert cm.cvg_file(names, st, ln, k, counts) == want
