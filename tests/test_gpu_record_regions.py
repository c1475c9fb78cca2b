"""Count-range regions of records on the device: katgpu_table_record_regions_host / _device (kg_record_regions.hpp) against
tests/record_regions_model.py, exactly -- key widths and layouts, runs across lane, chunk and record seams, touching records, one and
two ranges, batch boundaries, the device form with too little room, counts beyond 32 bits, argument errors -- and
`katgpu sect -n -E -F` end to end with per-position profiles forbidden."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import kat_amd
from tests import record_regions_case as case
from tests import record_regions_model as gm
from tests import record_stats_case as stats_case
from tests.test_gpu_record_stats import EXE, _cli_inputs, _run

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_WANT = {}


def _oracle(ko, k, canonical, bases):
    return (ko.WideTable(k, canonical) if k > 32 else ko.Table(k, canonical)).count_bases(bases)


def _assert_equal(got, want, what=""):
    assert len(got) == len(want), what
    for q, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == np.uint64 and g.ndim == 2 and g.shape[1] == 3, (what, q, g.dtype, g.shape)
        assert g.shape == w.shape, (what, q, g.shape, w.shape)
        bad = np.nonzero((g != w).any(axis=1))[0]
        assert bad.size == 0, (what, q, bad[:5], g[bad[:5]], w[bad[:5]])


def _seam_case(ko, k):
    """the records of tests/record_regions_case.py, their counts and the model's regions for RANGES: computed once per k"""
    if k not in _WANT:
        b, st, ln = case.records(k)
        counts, _ = ko.profile(_oracle(ko, k, True, case.counted(k)), b.tobytes(), True)
        _WANT[k] = (b, st, ln, counts, gm.regions(b, st, ln, k, counts, case.RANGES))
    return _WANT[k]


@pytest.mark.parametrize("k,canonical", [(5, True), (5, False), (17, True), (17, False), (27, True), (27, False), (32, True), (32, False),
                                         (33, True), (51, False), (63, True)])
def test_key_widths_and_flags(engine, ko, k, canonical):
    b, st, ln = stats_case.mix(k)
    t = engine.table(k, canonical).count_bases(stats_case.counted(k))
    if k in (17, 27):
        assert t.slot_bytes() == (8 if k == 17 else 12)             # both layouts of a one-word table
    o = _oracle(ko, k, canonical, stats_case.counted(k))
    for canonicalise in (canonical, not canonical):
        counts, _ = ko.profile(o, b.tobytes(), canonicalise)
        m = int(np.median(counts[counts > 0]))                      # 1 or 2 from k = 17 on; in the hundreds at k = 5
        ranges = [(1, m), (m + 1, 0)]
        want = gm.regions(b, st, ln, k, counts, ranges)
        assert want[0].shape[0] > 100 and want[1].shape[0] > 100
        _assert_equal(t.record_regions(b, st, ln, ranges, canonicalise), want, (k, canonicalise))
    t.free()


@pytest.mark.parametrize("k", [21, 45])
def test_seams(engine, ko, k):
    b, st, ln, counts, want = _seam_case(ko, k)
    chunk = 4064 if k <= 32 else 4032
    nb = np.where(ln >= k, ln - np.uint64(k - 1), np.uint64(0))
    r = want[1]                                                     # the range (2, 0)
    rec, lo, hi = r[:, 0].astype(np.int64), (st[r[:, 0]] + r[:, 1]).astype(np.int64), (st[r[:, 0]] + r[:, 2]).astype(np.int64)   # buffer positions
    for m in (0, 15):
        assert (lo % 16 == m).any() and (hi % 16 == m).any() and ((hi - 1) % 16 == m).any()
    for seam in case.SEAM_RUNS:
        assert ((lo == seam[0]) & (hi == seam[1]) & (rec == 1)).any(), seam
    assert ((lo // chunk) != ((hi - 1) // chunk)).any() and ((hi - lo) > 2 * chunk).any()      # across a chunk's end; longer than two chunks
    assert (lo < 3 * 4064).any() and ((lo < 3 * 4064) & (hi > 3 * 4064)).any() and ((lo < 7 * 4032) & (hi > 7 * 4032)).any()
    assert (r[:, 2] == nb[r[:, 0]]).any() and (hi - lo == 1).any()                              # stop == nb; one window
    assert ((r[:, 1] == 0) & (r[:, 2] == nb[r[:, 0]]) & (nb[r[:, 0]] > 2000)).any()             # a record that is one run
    with_region = np.zeros(st.size, bool)
    with_region[rec] = True
    assert (~with_region & (nb > 0)).sum() > 100                                               # records with windows and no region
    assert ((ln > 0) & (nb == 0)).sum() >= 3 and (ln == 0).sum() >= 3000 and int(np.max(np.diff(np.nonzero(ln)[0]))) > 3000
    assert want[0].shape[0] >= 1000 and want[1].shape[0] >= 1000
    t = engine.table(k, True).count_bases(case.counted(k))
    _assert_equal(t.record_regions(b, st, ln, case.RANGES), want, k)
    t.free()


@pytest.mark.parametrize("k", [1, 2])
def test_touching_records(engine, ko, k):
    """Records with no byte between them.  At k = 1 the last window of a record and the first of the next are neighbouring positions."""
    rng = np.random.default_rng(5)
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), 13000, p=[0.4, 0.3, 0.2, 0.1])
    ln = rng.integers(1, 40, 600).astype(np.uint64)
    ln[100:110] = 1
    st = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64)
    assert int(st[-1] + ln[-1]) <= seq.size
    t = engine.table(k, False).count_bases(seq)
    counts, _ = ko.profile(_oracle(ko, k, False, seq), seq.tobytes(), False)
    common = int(np.max(counts))                                    # the count of A (k = 1) or AA (k = 2)
    ranges = [(1, 0), (common, common)]
    want = gm.regions(seq, st, ln, k, counts, ranges)
    # every record with a window is one run of (1, 0), and runs on both sides of a joint stay two regions
    assert want[0].shape[0] == int((ln >= k).sum()) and (want[0][:, 1] == 0).all()
    both = np.nonzero((st[want[1][1:, 0]] + want[1][1:, 1] == st[want[1][:-1, 0]] + want[1][:-1, 2] + np.uint64(k - 1)) & (want[1][1:, 1] == 0))[0]
    assert both.size > 5
    _assert_equal(t.record_regions(seq, st, ln, ranges, False), want, k)
    t.free()


def test_ranges(engine, ko):
    k = 21
    b, st, ln, counts, _ = _seam_case(ko, k)
    t = engine.table(k, True).count_bases(case.counted(k))
    pairs = [[(1, 1)], [(2, 0)], [(1, 1), (2, 0)], [(2, 2), (3, 3)], [(0, 0)], [(0, 1), (0, 0)], [(3, 2)], [(5, 2), (1, 0)], [(4, 0), (2, 0)]]
    got = {}
    for ranges in pairs:
        want = gm.regions(b, st, ln, k, counts, ranges)
        got[tuple(ranges)] = t.record_regions(b, st, ln, ranges)
        _assert_equal(got[tuple(ranges)], want, ranges)
    assert got[((3, 2),)][0].shape[0] == 0 and got[((5, 2), (1, 0))][0].shape[0] == 0           # min > max > 0: nothing
    # min == 0: invalid windows and uncounted stretches inside a record are in range -- every record with a window is one run
    assert got[((0, 0),)][0].shape[0] == int((ln >= k).sum()) and got[((0, 1), (0, 0))][0].shape[0] > 1000
    # two calls of one range each == one call of two
    for q in (0, 1):
        assert np.array_equal(got[((1, 1), (2, 0))][q], got[(((1, 1), (2, 0))[q],)][0])
    t.free()


def test_batches(ko, tmp_path):
    """Batches of 20000 bases: smaller than the genome record and the contig, larger than the reads; the 3000 empty records follow a
    batch's last read.  Records are numbered through the whole call."""
    k = 21
    b, st, ln, _, want = _seam_case(ko, k)
    out = str(tmp_path / "batches.npz")
    e = dict(os.environ)
    e["KATGPU_TEST_REGIONS_BATCH"] = "20000"
    r = subprocess.run([sys.executable, "-m", "tests.record_regions_case", str(k), "1", out], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    assert int(ln.max()) > 20000 and int(z["sections"]) >= 2 * 6       # the hook bites: the reads alone make six batches
    _assert_equal([z["r0"], z["r1"]], want)


def _device_call(engine, t, b, st, ln, ranges, cap, shift=0, guard=4):
    m = st.size
    db = engine.alloc(b.size + 64)
    db.upload(b, offset=shift)
    dr = engine.alloc(16 * m)
    dr.upload(st)
    dr.upload(ln, offset=8 * m)
    fill = np.full(3 * (cap + guard), 0xABABABABABABABAB, np.uint64)
    do = engine.alloc(fill.nbytes)
    do.upload(fill)
    n_out = t.record_regions_device(db.ptr + shift, b.size, dr.ptr, dr.ptr + 8 * m, m, ranges, do.ptr if cap else None, cap)
    engine.sync()
    out = do.download(np.uint64, fill.size).reshape(-1, 3)
    db.free(); dr.free(); do.free()
    return n_out, out


def test_device_form(engine, ko):
    k = 21
    b, st, ln, _, want = _seam_case(ko, k)
    t = engine.table(k, True).count_bases(case.counted(k))
    n0, n1 = want[0].shape[0], want[1].shape[0]
    both = np.concatenate(want)
    for shift in (0, 1, 16):                                        # (the aligned and the byte-wise loader)
        n_out, out = _device_call(engine, t, b, st, ln, case.RANGES, n0 + n1, shift)
        assert n_out == [n0, n1]
        assert np.array_equal(out[:n0 + n1], both) and (out[n0 + n1:] == 0xABABABABABABABAB).all(), shift
    for cap in (7, n0, n0 + 5):                                     # too little room: the first `cap` regions, nothing behind them, the true totals
        n_out, out = _device_call(engine, t, b, st, ln, case.RANGES, cap)
        assert n_out == [n0, n1]
        assert np.array_equal(out[:cap], both[:cap]) and (out[cap:] == 0xABABABABABABABAB).all(), cap
    n_out, out = _device_call(engine, t, b, st, ln, case.RANGES, 0)  # count only
    assert n_out == [n0, n1] and (out == 0xABABABABABABABAB).all()
    n_out, out = _device_call(engine, t, b, st, ln, case.RANGES[1:], n1)
    assert n_out == [n1] and np.array_equal(out[:n1], want[1])
    t.free()


def test_large_counts(engine, ko):
    """counts beyond 32 bits (tests/record_stats_case.py: three 9-mers of 2^33 + 5, 2^34 + 1, 2^32 + 7): the range test is 64 bits wide"""
    big = stats_case.BIG
    o = ko.Table(9, False)
    _, keys, counts = stats_case.big_keys(ko)
    for key, c in zip(keys, counts):
        o.add(key, c)
    b, st, ln = stats_case.big_records()
    prof, _ = ko.profile(o, b.tobytes(), False)
    t = engine.table(9, False)
    t.merge_host(np.array(keys, np.uint64), np.array(counts, np.uint64))
    for ranges in ([(big, big), ((1 << 32) + 7, (1 << 34))], [(big + 1, 0), (1, (1 << 32) + 6)], [(5, 7), (1 << 32, 0)]):
        want = gm.regions(b, st, ln, 9, prof, ranges)
        _assert_equal(t.record_regions(b, st, ln, ranges), want, ranges)
    assert gm.regions(b, st, ln, 9, prof, [(big, big)])[0].tolist() == [[0, 0, 1], [2, 0, 1], [3, 1, 2]]
    assert gm.regions(b, st, ln, 9, prof, [(5, 7)])[0].shape[0] == 0           # the low words alone would be in range
    t.free()


def test_argument_errors(engine):
    bases = b"ACGTACGTTGCATGCA"
    t = engine.table(9, True).count_bases(np.frombuffer(bases, np.uint8))
    err = kat_amd.binding.KatGpuError
    with pytest.raises(err, match="starts before record 0 ends") as ei:
        t.record_regions(bases, [0, 5], [10, 5], [(1, 0)])
    assert ei.value.code == 1
    with pytest.raises(err, match="starts before record 0 ends"):
        t.record_regions(bases, [8, 0], [4, 4], [(1, 0)])           # decreasing
    with pytest.raises(err, match="lies beyond the 16 bases") as ei:
        t.record_regions(bases, [0, 10], [5, 7], [(1, 0)])
    assert ei.value.code == 1
    for ranges in ([], [(1, 0), (2, 0), (3, 0)]):
        with pytest.raises(err, match="one or two count ranges") as ei:
            t.record_regions(bases, [0], [16], ranges)
        assert ei.value.code == 1
    with pytest.raises(err, match="one or two count ranges"):
        t.record_regions_device(0, 0, 0, 0, 0, [(1, 0)] * 3, None, 0)
    # NULL pointers
    L = engine.L
    b = np.frombuffer(bases, np.uint8)
    st, ln, rg = np.array([0], np.uint64), np.array([16], np.uint64), np.array([1, 0], np.uint64)
    p, n_out = C.c_void_p(), (C.c_size_t * 2)()
    good = [t.h, b.ctypes.data, b.size, st.ctypes.data, ln.ctypes.data, 1, 1, rg.ctypes.data, 1, C.byref(p), n_out]
    assert L.katgpu_table_record_regions_host(*good) == 0 and n_out[0] == 1
    L.katgpu_free_host(p)
    for i in (0, 1, 3, 4, 7, 9, 10):
        args = list(good)
        args[i] = None
        assert L.katgpu_table_record_regions_host(*args) == 1, i
    dev = [t.h, None, 0, None, None, 0, 1, rg.ctypes.data, 1, None, 0, n_out]
    assert L.katgpu_table_record_regions_device(*dev) == 0 and n_out[0] == 0
    for i, v in ((0, None), (7, None), (11, None), (2, 16), (5, 1), (10, 4)):
        args = list(dev)
        args[i] = v
        assert L.katgpu_table_record_regions_device(*args) == 1, i
    assert [x.shape for x in t.record_regions(bases, [], [], [(1, 0), (2, 0)])] == [(0, 3), (0, 3)]
    assert [x.shape for x in t.record_regions(b"", [0, 0], [0, 0], [(0, 0)])] == [(0, 3)]
    t.free()


# ---- the command line: regions without a per-position profile crossing the bus ----

def test_cli_regions_without_profiles(ko, refdata, tmp_path):
    fa = _cli_inputs(refdata, tmp_path)
    r1 = os.path.join(refdata, "ecoli_r1.1K.fastq")
    jf = os.path.join(refdata, "ecoli.header.jf27")
    reads = lambda: ko.Table(27, True).count_files([r1])
    both = dict(extract_nr=True, extract_r=True)
    seen = 0
    for tag, args, table, kw in (("sp", ["-E", "-F", fa, r1], reads, both),
                                 ("sg", ["-E", "-F", "-g", "-t", "3", fa, r1], reads, dict(output_gc_stats=True, **both)),
                                 ("sj", ["-E", "-F", fa, jf], lambda: ko.Table.from_jf(jf), both),
                                 ("sw", ["-E", "-F", "-m", "45", fa, r1], lambda: ko.WideTable(45, True).count_files([r1]), both),
                                 ("se", ["-E", fa, r1], reads, dict(extract_nr=True)),
                                 ("sf", ["-F", fa, r1], reads, dict(extract_r=True))):
        r = _run(["sect", "-n", "-M", "2", "-G", "5", "-H", "1000000", "-o", tag] + args, tmp_path)
        assert r.returncode == 0, r.stderr
        ko.sect(table(), fa, str(tmp_path / ("want_" + tag)), no_count_stats=True, min_repeat=2, max_repeat=5, **kw)
        suffixes = ["-stats.tsv"] + [s for s, flag in (("-non_repetitive.fa", "extract_nr"), ("-repetitive.fa", "extract_r"), ("-counts.gc", "output_gc_stats")) if kw.get(flag)]
        for suffix in suffixes:
            want = (tmp_path / ("want_" + tag + suffix)).read_bytes()
            assert (tmp_path / (tag + suffix)).read_bytes() == want, (tag, suffix)
            seen += want.count(b"___region:") if tag == "sp" else 0
        for suffix in ("-counts.cvg", "-non_repetitive.fa", "-repetitive.fa", "-counts.gc"):
            assert (tmp_path / (tag + suffix)).exists() == (suffix in suffixes), (tag, suffix)
    assert seen > 1000
    # without -n the counts are needed for the .cvg file and the regions come from them, as before: all six files (with the test hook
    # that has Sect::save() write the contamination matrix)
    e = dict(os.environ)
    e["KATGPU_SECT_SAVE"] = "1"
    r = subprocess.run([EXE, "sect", "-E", "-F", "-g", "-M", "2", "-G", "5", "-H", "1000000", "-o", "full", fa, r1], cwd=tmp_path, capture_output=True,
                       text=True, timeout=300, env=e)
    assert r.returncode == 0, r.stderr
    ko.sect(reads(), fa, str(tmp_path / "want_full"), output_gc_stats=True, min_repeat=2, max_repeat=5, save=True, **both)
    for suffix in ("-counts.cvg", "-stats.tsv", "-counts.gc", "-non_repetitive.fa", "-repetitive.fa", "-contamination.mx"):
        assert (tmp_path / ("full" + suffix)).read_bytes() == (tmp_path / ("want_full" + suffix)).read_bytes(), suffix
