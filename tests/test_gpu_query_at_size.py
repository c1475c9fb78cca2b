"""The query kernels at the sizes of a genome, with the library's default batch sizes: katgpu_table_profile_*, _seq_hits_*,
_record_stats_* and _record_regions_* on tens of millions of bases, exactly, against the periodic inputs of
tests/query_at_size_case.py (tests/test_query_at_size_model.py shows that their expectations are the oracle's and the models').
What only these sizes reach: the second turn of every grid-stride loop (the grids stop at 8 blocks per CU), the second round of
k_regions_scan, host batches of 32 Mi bases and of 2^20 records, the statistics' cut at 8 Mi long windows, mask blocks in which every
position opens a run.  Every test first asserts, from the device's CU count and its expectations, that its input gets there."""
import ctypes as C

import numpy as np
import pytest

from tests import query_at_size_case as case
from tests import record_regions_model as gm
from tests import record_stats_model as rm
from tests.test_gpu_record_regions import _assert_equal as _same_regions
from tests.test_gpu_record_regions import _device_call as _regions_device
from tests.test_gpu_record_stats import _assert_equal as _same_stats

pytestmark = pytest.mark.gpu

TILE = 3072                                    # bytes a block of k_rstats_short owns per turn
SEL_CHUNK = 4096                               # counts a block of k_rstats_hist takes per turn
SHORT_WINDOWS = 960                            # the short / long limit of the statistics
GUARD = 0xABABABABABABABAB
HIP_ATTR_MULTIPROCESSOR_COUNT = 63                # hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h)
_BUILT = {}


def _built(key, make):
    if key not in _BUILT:
        _BUILT[key] = make()
    return _BUILT[key]


def _grid(engine):
    """the most blocks a query kernel is launched with: eight per CU.  The engine does not report its CUs and torch brings a HIP
    runtime of its own, which sees no device in a process where the library's holds it: the library's runtime is asked."""
    cus = C.c_int(0)
    assert engine.L.hipDeviceGetAttribute(C.byref(cus), HIP_ATTR_MULTIPROCESSOR_COUNT, 0) == 0 and cus.value > 0
    return 8 * cus.value


def _chunk(k):
    return 4064 if k <= 32 else 4032


def _tiles(n, per):
    return -(-n // per)


def _sections(engine):
    return engine.profile()["profile"]["launches"]


class _Tiled:
    """a Tiled case at P copies: the buffer, the records, the expectations"""

    def __init__(self, c, P, n_rec=None):
        self.c, self.k = c, c.k
        self.st, self.ln = c.records(P)
        self.bases = c.buffer(P)
        self.stats, self.hits, self.regions = c.want_stats(P), c.want_hits(P), c.want_regions(P)
        if n_rec is not None:                                       # the first n_rec records only
            self.st, self.ln, self.stats, self.hits = self.st[:n_rec], self.ln[:n_rec], self.stats[:n_rec], self.hits[:n_rec]
            self.bases = self.bases[:int(self.st[-1] + self.ln[-1])]
            self.regions = [r[r[:, 0] < n_rec] for r in self.regions]


def _mix(ko, k):
    def make():
        c = case.tiled_mix(ko, k)
        return _Tiled(c, c.copies(case.MIN_BASES))
    return _built(("mix", k), make)


def _regions(ko, k):
    def make():
        c = case.tiled_regions(ko, k)
        return _Tiled(c, c.copies(case.MIN_BASES))
    return _built(("regions", k), make)


def _giant(ko, k, variant):
    def make():
        c = case.Giant(ko, k, case.GIANT_LENGTH, variant)
        c.stats = c.want_stats()
        return c
    return _built(("giant", k, variant), make)


def _upload(engine, bases, shift, *words):
    """the bases `shift` bytes into a buffer, and a second buffer of 64-bit arrays one behind the other"""
    db = engine.alloc(bases.size + 64)
    db.upload(bases, offset=shift)
    dw = engine.alloc(8 * sum(w.size for w in words))
    at = []
    for w in words:
        at.append(dw.ptr + 8 * sum(x.size for x in words[:len(at)]))
        dw.upload(w, offset=at[-1] - dw.ptr)
    return db, dw, at


# ---- 1 ----

@pytest.mark.parametrize("k", [21, 45])
def test_profile_at_size(engine, ko, k):
    m = _mix(ko, k)
    want = m.c.want_counts(m.bases.size // m.c.period)
    n, n_out = m.bases.size, m.bases.size - k + 1
    assert n >= case.MIN_BASES and want.size == n_out
    assert _tiles(n_out, _chunk(k)) > _grid(engine)                 # k_profile takes a second turn
    assert n_out > case.BATCH                                       # the host form a second batch
    t = engine.table(k, True).count_bases(m.c.counted)
    engine.profile_reset()
    got = t.profile(m.bases)
    assert _sections(engine) == 2
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:5]
    del got
    poison = np.full(n_out + 2, GUARD, np.uint64)
    for shift in (0, 1):                                            # the aligned and the byte-wise loader
        db, dc, (at,) = _upload(engine, m.bases, shift, poison)
        t.profile_device(db.ptr + shift, n, at)
        engine.sync()
        got = dc.download(np.uint64, n_out + 2)
        db.free(); dc.free()
        assert np.array_equal(got[:n_out], want) and (got[n_out:] == GUARD).all(), (shift, np.nonzero(got[:n_out] != want)[0][:5])
    t.free()


# ---- 2 ----

@pytest.mark.parametrize("k", [21, 45])
def test_hits_and_stats_at_size(engine, ko, k):
    m = _mix(ko, k)
    grid, chunk, n = _grid(engine), _chunk(k), m.bases.size
    st, nb = m.st.astype(np.int64), case.windows(m.ln, k)
    assert _tiles(n, TILE) > grid and _tiles(n, chunk) > grid
    full = (m.stats["sum"] > 0) & (m.stats["median"] > 0) & (m.hits > 0)
    short, long_ = (nb > 0) & (nb <= SHORT_WINDOWS), nb > SHORT_WINDOWS
    assert (short & full & (st // TILE >= grid)).sum() > 1000       # records of k_rstats_short's second turn
    assert (short & full & (st // chunk >= grid)).sum() > 1000      # and of k_seq_hits'
    assert (long_ & full & (st // chunk < grid)).any() and (long_ & full & (st // chunk >= grid)).any()     # k_rstats_long: both turns
    cut = case.batches(m.st, m.ln, long_windows=(k, SHORT_WINDOWS, case.BATCH // 4))
    assert len(cut) == 2 and int(m.st[cut[0][1]] - m.st[0]) < case.BATCH - (1 << 20)     # the host form's first batch ends at 8 Mi long windows
    assert all(long_[a:b].any() for a, b in cut)
    t = engine.table(k, True).count_bases(m.c.counted)
    hits = t.seq_hits(m.bases, m.st, m.ln)
    assert np.array_equal(hits, m.hits), np.nonzero(hits != m.hits)[0][:5]
    engine.profile_reset()
    got = t.record_stats(m.bases, m.st, m.ln)
    assert _sections(engine) == 2 * 2                                # two batches, long records in both
    _same_stats(got, m.stats, "host")
    r = m.st.size
    for shift in (0, 1):
        db, dw, (ds, dl, dh, do) = _upload(engine, m.bases, shift, m.st, m.ln, np.full(r, GUARD, np.uint64), np.full(6 * r, GUARD, np.uint64))
        t.seq_hits_device(db.ptr + shift, n, ds, dl, r, dh)
        t.record_stats_device(db.ptr + shift, n, ds, dl, r, do)
        engine.sync()
        hits, got = dw.download(np.uint64, r, offset=dh - dw.ptr), dw.download(np.uint64, 6 * r, offset=do - dw.ptr).view(rm.DTYPE)
        db.free(); dw.free()
        assert np.array_equal(hits, m.hits), (shift, np.nonzero(hits != m.hits)[0][:5])
        _same_stats(got, m.stats, shift)
    t.free()


# ---- 3 ----

@pytest.mark.parametrize("k,variant", [(21, "plain"), (45, "plain"), (21, "ties"), (9, "big")])
def test_stats_of_giant_records(engine, ko, k, variant):
    c = _giant(ko, k, variant)
    nb = case.windows(c.ln, k)
    grid = _grid(engine)
    assert int(nb[nb > SHORT_WINDOWS].sum()) > grid * SEL_CHUNK     # k_rstats_hist takes a second turn
    assert _tiles(c.bases.size, _chunk(k)) > grid                   # and k_rstats_long
    assert int(nb[0]) > case.BATCH // 4 and nb[1] > SHORT_WINDOWS and c.bases.size < case.BATCH      # the cut at 8 Mi long windows, not at 32 Mi bases
    assert (nb[2:] <= SHORT_WINDOWS).all() and (nb[2:] > 0).sum() >= 3
    w = c.counts_of(0)
    if variant == "ties":
        assert (w == 1).mean() > 0.4 and (w == 2).mean() > 0.4 and int(c.stats["median"][0]) in (1, 2)
    if variant == "big":
        assert int((w > 1 << 32).sum()) > 100 and int(c.stats["sum"][0]) > 1 << 40 and 0 < int(c.stats["median"][0]) < 1 << 32
    else:
        assert int(w.max()) < 1 << 16                               # (the upper six digit passes find nothing to do)
    assert int(c.stats["invalid"][0]) > 1000 and len(set(c.stats["median"][:2].tolist()) | {0}) >= 2
    t = c.table(engine)
    engine.profile_reset()
    got = t.record_stats(c.bases, c.st, c.ln)
    assert _sections(engine) == 4                                    # two batches, long records in both
    _same_stats(got, c.stats, "host")
    r = c.st.size
    for shift in (0, 1):
        db, dw, (ds, dl, do) = _upload(engine, c.bases, shift, c.st, c.ln, np.full(6 * r, GUARD, np.uint64))
        t.record_stats_device(db.ptr + shift, c.bases.size, ds, dl, r, do)
        engine.sync()
        got = dw.download(np.uint64, 6 * r, offset=do - dw.ptr).view(rm.DTYPE)
        db.free(); dw.free()
        _same_stats(got, c.stats, shift)
    t.free()


# ---- 4 ----

@pytest.mark.parametrize("k", [21, 45])
def test_regions_at_size(engine, ko, k):
    m = _regions(ko, k)
    grid, n = _grid(engine), m.bases.size
    cut = case.batches(m.st, m.ln)
    first = int(m.st[cut[0][1] - 1] + m.ln[cut[0][1] - 1])          # the bases of the first batch (the first record starts at 0)
    assert n >= case.MIN_BASES and len(cut) == 2 and int(m.st[0]) == 0
    assert _tiles(_tiles(first, 64), 256) == 2048 == 2 * 1024       # full: two rounds of k_regions_scan
    assert _tiles(n, case.MASK_BLOCK) > grid and _tiles(n, _chunk(k)) > grid      # k_regions_count / _emit and k_regions_mask take a second turn
    for q, found in enumerate(m.regions):
        lo, hi = case.buffer_runs(m.st, found)
        last = hi - 1
        assert len(set((lo % 64).tolist())) == 64 and len(set((last % 64).tolist())) == 64 and len(set((hi % 64).tolist())) == 64, q
        assert len(set((lo % 16).tolist())) == 16 and len(set((last % 16).tolist())) == 16, q
        assert ((lo % case.MASK_BLOCK >= case.MASK_BLOCK - 64) & (last // case.MASK_BLOCK == lo // case.MASK_BLOCK + 1)).any(), q
        assert ((lo >= first) & (found[:, 0] >= cut[1][0])).any(), q
    lo, hi = case.buffer_runs(m.st, np.concatenate(m.regions))
    assert ((lo < case.SCAN_ROUND) & (hi > case.SCAN_ROUND)).any() and case.SCAN_ROUND < first
    t = engine.table(k, True).count_bases(m.c.counted)
    engine.profile_reset()
    got = t.record_regions(m.bases, m.st, m.ln, m.c.ranges)
    assert _sections(engine) == 2 * 2                                # per batch: masks and offsets, then the regions
    _same_regions(got, m.regions, "host")
    del got
    n0, n1 = m.regions[0].shape[0], m.regions[1].shape[0]
    both = np.concatenate(m.regions)
    for shift in (0, 1):
        n_out, out = _regions_device(engine, t, m.bases, m.st, m.ln, m.c.ranges, n0 + n1, shift)
        assert n_out == [n0, n1]
        bad = np.nonzero((out[:n0 + n1] != both).any(axis=1))[0]
        assert bad.size == 0 and (out[n0 + n1:] == GUARD).all(), (shift, bad[:5], out[bad[:5]], both[bad[:5]])
    n_out, out = _regions_device(engine, t, m.bases, m.st, m.ln, m.c.ranges, 0)
    assert n_out == [n0, n1] and (out == GUARD).all()
    # too little room, the last region written one of range 0 in the second round of the scan
    lo, _ = case.buffer_runs(m.st, m.regions[0])
    cap = int(np.searchsorted(lo, case.SCAN_ROUND)) + 1000
    assert cap < n0 and lo[cap - 1] > case.SCAN_ROUND
    n_out, out = _regions_device(engine, t, m.bases, m.st, m.ln, m.c.ranges, cap)
    assert n_out == [n0, n1]
    assert np.array_equal(out[:cap], both[:cap]) and (out[cap:] == GUARD).all()
    t.free()


# ---- 5 ----

@pytest.mark.parametrize("k", [21, 45])
def test_regions_of_a_giant_record(engine, ko, k):
    c = _giant(ko, k, "plain")
    nb = case.windows(c.ln, k)
    n = c.bases.size
    assert _tiles(_tiles(n, 64), 256) > 1024 and _tiles(n, _chunk(k)) > _grid(engine)
    t = c.table(engine)
    for ranges in ([(0, 0), (2, 0)], [(2, 0), (0, 0)]):
        want = _built(("giant regions", k, tuple(ranges)), lambda: c.want_regions(ranges))
        whole, many = (want[0], want[1]) if ranges[0] == (0, 0) else (want[1], want[0])
        # every record with a window is one run of (0, 0); the giant's opens in the scan's first round and closes in its second
        assert whole.tolist() == [[r, 0, int(nb[r])] for r in range(nb.size) if nb[r]] and int(nb[0]) > 17_000_000 > case.SCAN_ROUND
        assert many.shape[0] > 20_000 and int((many[:, 0] == 0).sum()) > 20_000 and (many[:, 0] == 1).any()
        _same_regions(t.record_regions(c.bases, c.st, c.ln, ranges), want, ("host", ranges))
        n0, n1 = want[0].shape[0], want[1].shape[0]
        for shift in (0, 1):
            n_out, out = _regions_device(engine, t, c.bases, c.st, c.ln, ranges, n0 + n1, shift)
            assert n_out == [n0, n1], (ranges, shift)
            assert np.array_equal(out[:n0 + n1], np.concatenate(want)) and (out[n0 + n1:] == GUARD).all(), (ranges, shift)
    t.free()


# ---- 6 ----

def test_more_records_than_a_batch_holds(engine, ko):
    k = 17
    def make():
        c = case.tiled_reads(ko, k)
        return _Tiled(c, -(-case.MANY_RECORDS // c.st.size), case.MANY_RECORDS)
    m = _built(("reads", k), make)
    cut = case.BATCH_RECS
    assert m.st.size == case.MANY_RECORDS and m.bases.size < case.BATCH
    assert case.batches(m.st, m.ln) == [(0, cut), (cut, m.st.size)]  # the record limit ends the first batch
    assert 20 <= int(m.ln[m.ln > 0].min()) and int(m.ln.max()) <= 40 and (m.ln == 0).sum() > 10_000
    assert (m.st[1:] == m.st[:-1] + m.ln[:-1]).sum() > 100_000       # touching
    for q, found in enumerate(m.regions):
        rec = found[:, 0].astype(np.int64)
        assert ((rec >= cut - 20) & (rec < cut)).any() and ((rec >= cut) & (rec < cut + 20)).any() and (rec > cut + 4000).any(), q
    for f in ("sum", "median", "non_zero", "invalid", "gc_bases"):
        assert m.stats[f][cut - 50:cut].any() and m.stats[f][cut:].any() and len(set(m.stats[f][cut:].tolist())) > 2, f
    assert m.hits[cut:].any() and cut % m.c.st.size                  # (the cut lies inside a copy)
    t = engine.table(k, True).count_bases(m.c.counted)
    engine.profile_reset()
    hits = t.seq_hits(m.bases, m.st, m.ln)
    assert _sections(engine) == 2
    assert np.array_equal(hits, m.hits), np.nonzero(hits != m.hits)[0][:5]
    engine.profile_reset()
    got = t.record_stats(m.bases, m.st, m.ln)
    assert _sections(engine) == 2                                    # (no long records)
    _same_stats(got, m.stats)
    engine.profile_reset()
    got = t.record_regions(m.bases, m.st, m.ln, m.c.ranges)
    assert _sections(engine) == 2 * 2
    _same_regions(got, m.regions)
    t.free()


# ---- 7 ----

def test_densest_masks(engine, ko):
    k = 1
    seq, st, ln = case.dense()
    o = ko.Table(k, False).count_bases(seq)
    counts, _ = ko.profile(o, seq.tobytes(), False)
    common = int(counts.max())
    ranges = [(1, 0), (common, common)]
    want = gm.regions(seq, st, ln, k, counts, ranges)
    # one region per record: 64 opens and 64 closes in every mask word, 16384 in each of the four full mask blocks
    assert seq.size > 4 * case.MASK_BLOCK and want[0].tolist() == [[r, 0, 1] for r in range(st.size)]
    assert want[1].shape[0] > 40_000 and (want[1][:case.MASK_BLOCK, 0] == np.arange(case.MASK_BLOCK)).all() and want[1].shape[0] < st.size
    t = engine.table(k, False).count_bases(seq)
    _same_regions(t.record_regions(seq, st, ln, ranges, False), want, "host")
    n0, n1 = want[0].shape[0], want[1].shape[0]
    for shift in (0, 1):
        n_out, out = _regions_device(engine, t, seq, st, ln, ranges, n0 + n1, shift)
        assert n_out == [n0, n1]
        assert np.array_equal(out[:n0 + n1], np.concatenate(want)) and (out[n0 + n1:] == GUARD).all(), shift
    t.free()
