"""The periodic inputs of tests/query_at_size_case.py, at sizes the oracle and the numpy models can take directly: three copies of a
block, a giant record of two and a half periods.  The expectations built from one period must be identical to the oracle's profile
of the whole buffer and to tests/record_stats_model.py, tests/filter_model.py and tests/record_regions_model.py run on all of it --
per-position counts, statistics, hits and regions.  That is what makes the expectations of tests/test_gpu_query_at_size.py the
reference's and not the kernels'."""
import numpy as np
import pytest

from tests import filter_model as fm
from tests import query_at_size_case as case
from tests import record_regions_model as gm
from tests import record_stats_model as rm


def _direct_hits(ko, o, bases, st, ln, canonical):
    """every record profiled by itself, as FilterSeq does"""
    return np.array([fm.record_hits(*ko.profile(o, bases[int(s):int(s + n)].tobytes(), canonical)) for s, n in zip(st, ln)], np.uint64)


def _same_regions(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == np.uint64 and g.shape == w.shape and np.array_equal(g, w)


@pytest.mark.parametrize("build,k", [(case.tiled_mix, 21), (case.tiled_mix, 45), (case.tiled_regions, 21), (case.tiled_regions, 45),
                                     (case.tiled_reads, 17)])
def test_tiled_records(ko, build, k):
    P = 3
    c = build(ko, k)
    assert c.period % 2 == 1 and c.block.size == c.period and not gm._IS_BASE[c.block[-1]]
    bases = c.buffer(P)
    st, ln = c.records(P)
    assert bases.size == P * c.period and st.size == P * c.st.size and int(st[-1] + ln[-1]) <= bases.size
    o = case.oracle_table(ko, k, c.canonical, c.counted)
    counts, _ = ko.profile(o, bases.tobytes(), c.canonical)
    assert int(counts.max()) >= 2 and np.array_equal(c.want_counts(P), counts)
    assert np.array_equal(c.want_stats(P), rm.record_stats(bases, st, ln, k, counts))
    hits = c.want_hits(P)
    assert int(hits.max()) > 0 and np.array_equal(hits, _direct_hits(ko, o, bases, st, ln, c.canonical))
    want = c.want_regions(P)
    assert all(w.shape[0] >= 3 * 100 for w in want) and int(want[0][-1, 0]) >= 2 * c.st.size      # records of the third copy
    _same_regions(want, gm.regions(bases, st, ln, k, counts, c.ranges))


@pytest.mark.parametrize("k,variant", [(21, "plain"), (45, "plain"), (21, "ties"), (9, "big")])
def test_giant_record(ko, k, variant):
    c = case.Giant(ko, k, 5 * case.GIANT_PERIOD // 2, variant)
    bases, st, ln = c.bases, c.st, c.ln
    assert int(ln[0]) == 5 * c.g.size // 2 and int(ln[0]) % c.g.size and (~gm._IS_BASE[c.g]).sum() > 5
    assert np.array_equal(c.seq_of(0)[c.g.size:2 * c.g.size], c.g) and not gm._IS_BASE[bases[int(ln[0])]]
    o = case.oracle_table(ko, k, c.canonical, c.counted)
    if c.big:
        for key, n in zip(*c.big):
            o.add(int(key), int(n))
    counts, _ = ko.profile(o, bases.tobytes(), c.canonical)
    inside = np.zeros(counts.size, bool)
    for s, nb in zip(st.astype(np.int64), case.windows(ln, k)):
        inside[s:s + nb] = True
    assert np.array_equal(c.want_counts()[inside], counts[inside])
    want = c.want_stats()
    assert np.array_equal(want, rm.record_stats(bases, st, ln, k, counts))
    assert np.array_equal(want["non_zero"], _direct_hits(ko, o, bases, st, ln, c.canonical))
    if variant == "big":
        assert int(counts[inside].max()) > 1 << 34 and int(want["sum"][0]) > 1 << 34
    if variant == "ties":
        w = c.counts_of(0)
        assert (w == 1).mean() > 0.35 and (w == 2).mean() > 0.35 and ((w == 1) | (w == 2)).mean() > 0.95      # (the first half of G is there three times)
    for ranges in ([(0, 0), (2, 0)], [(2, 0), (0, 0)], [(1, 1), (3, 4)]):
        found = c.want_regions(ranges)
        _same_regions(found, gm.regions(bases, st, ln, k, counts, ranges))
        assert all(f.shape[0] > 0 for f in found)
