"""Per-record statistics and count-range regions from a dense array of counts: katgpu_record_stats_from_counts_device and
katgpu_record_regions_from_counts_device (the CountsDense instantiations of K11, K12 and K14) against tests/record_stats_model.py and
tests/record_regions_model.py, exactly, field by field.  The counts are a seeded generator's, not a table's: mostly 0..3, some up to
5000, a few beyond 2^33, and all-ones on every invalid window and every window that lies in no record -- a count read where none may
be read shows in a sum, a median or a region.  The bases and records are tests/record_stats_case.py's mix(k): both statistics kernels
run.  One process; the load-time hook KATGPU_TEST_STATS_SHORT in children (tests/record_from_counts_case.py)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import kat_amd
from tests import record_from_counts_case as case
from tests import record_regions_model as gm
from tests import record_stats_case as stats_case
from tests import record_stats_model as sm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
_WANT = {}


def _inputs(k):
    """mix(k), the generator's counts, and what the two models make of them: computed once per k"""
    if k not in _WANT:
        b, st, ln = stats_case.mix(k)
        counts, poisoned = case.counts_for(k, b, st, ln)
        assert poisoned > 1000 and int((counts[counts != case.POISON] > U64(1 << 33)).sum()) > 10
        nb = np.where(ln >= k, ln - U64(k) + U64(1), U64(0))
        assert int((nb > 960).sum()) >= 3 and int(((nb > 0) & (nb <= 960)).sum()) > 2000 and {0, k - 1, k, k + 1} <= set(ln.tolist())
        _WANT[k] = (b, st, ln, counts, sm.record_stats(b, st, ln, k, counts), gm.regions(b, st, ln, k, counts, case.RANGES))
    return _WANT[k]


def _assert_stats(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for f in sm.FIELDS:
        bad = np.flatnonzero(got[f] != want[f])
        assert bad.size == 0, (what, f, bad[:5], got[f][bad[:5]], want[f][bad[:5]])


def _assert_regions(rows, totals, want, what=""):
    assert list(totals) == [w.shape[0] for w in want], (what, totals)
    both = np.concatenate(want)
    assert rows.shape[0] >= both.shape[0]
    bad = np.flatnonzero((rows[:both.shape[0]] != both).any(axis=1))
    assert bad.size == 0, (what, bad[:5], rows[bad[:5]], both[bad[:5]])


@pytest.mark.parametrize("k", case.KS)
def test_statistics_and_regions_are_the_models(engine, k):
    b, st, ln, counts, want_s, want_r = _inputs(k)
    n0, n1 = want_r[0].shape[0], want_r[1].shape[0]
    assert n0 > 100 and n1 > 100 and int(want_s["sum"].max()) > (1 << 33)
    for shift in (0, 1):                                            # 1: one byte past a 16-byte boundary -- the byte-wise loader's instantiation
        stats, n_out, rows = case.device_call(engine, k, b, counts, st, ln, case.RANGES, n0 + n1, shift)
        _assert_stats(stats, want_s, (k, shift))
        _assert_regions(rows, n_out, want_r, (k, shift))
        assert (rows[n0 + n1:] == 0xABABABABABABABAB).all()


def test_one_range_and_too_little_room(engine):
    k = 27
    b, st, ln, counts, _, want_r = _inputs(k)
    n0, n1 = want_r[0].shape[0], want_r[1].shape[0]
    both = np.concatenate(want_r)
    for q in (0, 1):
        _, n_out, rows = case.device_call(engine, k, b, counts, st, ln, case.RANGES[q:q + 1], want_r[q].shape[0])
        _assert_regions(rows, n_out, want_r[q:q + 1], q)
    for cap in (7, n0, n0 + 5):                                     # the first `cap` regions, nothing behind them, the true totals
        _, n_out, rows = case.device_call(engine, k, b, counts, st, ln, case.RANGES, cap)
        assert n_out == [n0, n1]
        assert np.array_equal(rows[:cap], both[:cap]) and (rows[cap:] == 0xABABABABABABABAB).all(), cap
    _, n_out, rows = case.device_call(engine, k, b, counts, st, ln, case.RANGES, 0)      # count only
    assert n_out == [n0, n1] and (rows == 0xABABABABABABABAB).all()


@pytest.mark.parametrize("short", [0, 100])
def test_all_long_and_mixed(tmp_path, short):
    """KATGPU_TEST_STATS_SHORT = 0: every record with a window goes the long way (K12 / K13); 100: the reads divide between the two."""
    out = str(tmp_path / "out.npz")
    env = dict(os.environ, KATGPU_TESTING="1", KATGPU_TEST_STATS_SHORT=str(short))
    r = subprocess.run([sys.executable, "-m", "tests.record_from_counts_case", out] + [str(k) for k in case.KS], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(out)
    for k in case.KS:
        _, _, ln, _, want_s, want_r = _inputs(k)
        nb = np.where(ln >= k, ln - U64(k) + U64(1), U64(0))
        assert short == 0 or (int(((nb > 0) & (nb <= short)).sum()) > 300 and int((nb > short).sum()) > 300)
        _assert_stats(z["stats_%d" % k], want_s, (short, k))
        _assert_regions(z["regions_%d" % k], z["totals_%d" % k].tolist(), want_r, (short, k))


@pytest.mark.parametrize("k", [27, 41])
def test_the_two_sources_agree(engine, k):
    """Table.profile_device into a buffer, the from-counts calls from it: what Table.record_stats and Table.record_regions return."""
    b, st, ln = stats_case.mix(k)
    t = engine.table(k, True).count_bases(stats_case.counted(k))
    ranges = [(1, 2), (3, 0)]
    want_s, want_r = t.record_stats(b, st, ln), t.record_regions(b, st, ln, ranges)
    assert want_r[0].shape[0] > 100 and want_r[1].shape[0] > 100
    db, dc = engine.alloc(b.size + 64), engine.alloc(8 * (b.size - k + 1))
    db.upload(b)
    t.profile_device(db, b.size, dc)
    engine.sync()
    counts = dc.download(U64)
    db.free(); dc.free()
    stats, n_out, rows = case.device_call(engine, k, b, counts, st, ln, ranges, sum(w.shape[0] for w in want_r))
    _assert_stats(stats, want_s, k)
    _assert_regions(rows, n_out, want_r, k)
    t.free()


def test_argument_errors(engine):
    err = kat_amd.binding.KatGpuError
    k = 9
    b = np.frombuffer(b"ACGTACGTTGCATGCANNGC", np.uint8)
    st, ln = np.array([0, 16], U64), np.array([16, 4], U64)
    counts = np.arange(1, b.size - k + 2, dtype=U64)
    db, dc, dr, ds = engine.alloc(64), engine.alloc(8 * counts.size + 8), engine.alloc(32), engine.alloc(96)
    db.upload(b); dc.upload(counts); dr.upload(st); dr.upload(ln, offset=16)
    L, rg, n_out = engine.L, np.array([1, 0], U64), (C.c_size_t * 2)()
    good_s = [engine.h, k, db.ptr, b.size, dc.ptr, dr.ptr, dr.ptr + 16, 2, ds.ptr]
    good_r = [engine.h, k, db.ptr, b.size, dc.ptr, dr.ptr, dr.ptr + 16, 2, rg.ctypes.data, 1, None, 0, n_out]
    assert L.katgpu_record_stats_from_counts_device(*good_s) == 0
    assert L.katgpu_record_regions_from_counts_device(*good_r) == 0 and n_out[0] == 1
    engine.sync()
    got = ds.download(np.uint8, 96).view(kat_amd.binding.RECORD_STATS)
    _assert_stats(got, sm.record_stats(b, st, ln, k, counts))
    assert got["gc_bases"].tolist() == [8, 2] and got["n_bases"].tolist() == [0, 2]       # (a record shorter than k has its base classes)
    for bad_k in (0, 64):                                           # KATGPU_ERR_K, with a message
        with pytest.raises(err, match="unsupported") as ei:
            engine.record_stats_from_counts_device(bad_k, db, b.size, dc, dr.ptr, dr.ptr + 16, 2, ds)
        assert ei.value.code == 6
        with pytest.raises(err, match="unsupported") as ei:
            engine.record_regions_from_counts_device(bad_k, db, b.size, dc, dr.ptr, dr.ptr + 16, 2, [(1, 0)], None, 0)
        assert ei.value.code == 6
    for off in (1, 4):                                              # counts that are not 8-byte aligned
        with pytest.raises(err, match="8-byte aligned") as ei:
            engine.record_stats_from_counts_device(k, db, b.size, dc.ptr + off, dr.ptr, dr.ptr + 16, 2, ds)
        assert ei.value.code == 1
        with pytest.raises(err, match="8-byte aligned") as ei:
            engine.record_regions_from_counts_device(k, db, b.size, dc.ptr + off, dr.ptr, dr.ptr + 16, 2, [(1, 0)], None, 0)
        assert ei.value.code == 1
    for i in (0, 2, 4, 5, 6, 8):                                    # NULL where a pointer is needed
        args = list(good_s)
        args[i] = None
        assert L.katgpu_record_stats_from_counts_device(*args) == 1, i
    for i, v in ((0, None), (2, None), (4, None), (5, None), (6, None), (8, None), (12, None), (11, 4), (9, 3), (9, 0)):
        args = list(good_r)
        args[i] = v
        assert L.katgpu_record_regions_from_counts_device(*args) == 1, i
    # no records: nothing happens, with or without pointers
    assert L.katgpu_record_stats_from_counts_device(engine.h, k, None, 0, None, None, None, 0, None) == 0
    n_out[0] = 5
    assert L.katgpu_record_regions_from_counts_device(engine.h, k, None, 0, None, None, None, 0, rg.ctypes.data, 1, None, 0, n_out) == 0 and n_out[0] == 0
    # a buffer shorter than k: no counts are needed, the base classes are still made
    short_ln = np.array([5, 3], U64)
    dr.upload(np.array([0, 5], U64)); dr.upload(short_ln, offset=16)
    ds.upload(np.full(12, 0xAB, U64))
    assert L.katgpu_record_stats_from_counts_device(engine.h, k, db.ptr, 8, None, dr.ptr, dr.ptr + 16, 2, ds.ptr) == 0
    engine.sync()
    got = ds.download(np.uint8, 96).view(kat_amd.binding.RECORD_STATS)
    _assert_stats(got, sm.record_stats(b[:8], [0, 5], [5, 3], k, np.zeros(0, U64)))
    assert got["gc_bases"].tolist() == [2, 2] and not got["sum"].any() and not got["invalid"].any()
    n_out[0] = 5
    assert L.katgpu_record_regions_from_counts_device(engine.h, k, db.ptr, 8, None, dr.ptr, dr.ptr + 16, 2, rg.ctypes.data, 1, None, 0, n_out) == 0 and n_out[0] == 0
    for x in (db, dc, dr, ds):
        x.free()
