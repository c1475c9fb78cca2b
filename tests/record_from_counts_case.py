"""Inputs of tests/test_gpu_record_from_counts.py, and -- run as a program -- katgpu_record_stats_from_counts_device and
katgpu_record_regions_from_counts_device on them in a process of its own, because the library reads KATGPU_TEST_STATS_SHORT once, when
it is loaded:
    python -m tests.record_from_counts_case <out.npz> <k> [<k> ...]
The bases and records are tests/record_stats_case.py's mix(k); the counts come from a seeded generator, not from a table."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import record_stats_case as stats_case  # noqa: E402

U64 = np.uint64
POISON = U64(2 ** 64 - 1)                 # what a count that must never be read holds
KS = (5, 27, 32, 33, 63)
RANGES = [(1, 2), (2, 0)]                 # they overlap at 2: a window may lie in both
_IS_BASE = np.zeros(256, bool)
_IS_BASE[list(b"ACGTacgt")] = True


def counts_for(k, b, st, ln):
    """One count per window start of b: mostly 0..3 (ties, zeros), one in 50 up to 5000, one in 2000 beyond 2^33; all-ones on every
    invalid window and on every window that lies in no record.  Returns (counts, how many were poisoned)."""
    rng = np.random.default_rng(77000 + k)
    n_out = b.size - k + 1
    c = rng.integers(0, 4, n_out, dtype=U64)
    some = rng.random(n_out) < 0.02
    c[some] = rng.integers(4, 5001, int(some.sum()), dtype=U64)
    few = rng.random(n_out) < 0.0005
    c[few] = (U64(1) << U64(33)) + rng.integers(1, 1 << 20, int(few.sum()), dtype=U64)
    bad = np.concatenate([[0], np.cumsum(~_IS_BASE[b])])
    invalid = (bad[k:] - bad[:-k]) > 0
    in_record = np.zeros(n_out, bool)
    for s, n in zip(st.tolist(), ln.tolist()):
        if n >= k:
            in_record[s:s + n - k + 1] = True
    poison = invalid | ~in_record
    c[poison] = POISON
    return c, int(poison.sum())


def device_call(eng, k, b, counts, st, ln, ranges=None, cap=None, shift=0, guard=4):
    """The two from-counts calls on device copies of the inputs, the bases `shift` bytes past an aligned address.  Returns
    (stats, totals per range, the region words: cap + guard rows, 0xAB.. where nothing was written)."""
    from kat_amd.binding import RECORD_STATS
    m = st.size
    db = eng.alloc(b.size + 64)
    db.upload(b, offset=shift)
    dc = eng.alloc(max(counts.nbytes, 8))
    if counts.size:
        dc.upload(counts)
    dr = eng.alloc(16 * max(m, 1))
    if m:
        dr.upload(st)
        dr.upload(ln, offset=8 * m)
    ds = eng.alloc(48 * max(m, 1))
    eng.record_stats_from_counts_device(k, db.ptr + shift, b.size, dc.ptr, dr.ptr, dr.ptr + 8 * m, m, ds.ptr)
    eng.sync()
    stats = ds.download(np.uint8, 48 * m).view(RECORD_STATS)
    n_out, out = None, None
    if ranges is not None:
        fill = np.full(3 * (cap + guard), 0xABABABABABABABAB, U64)
        do = eng.alloc(fill.nbytes)
        do.upload(fill)
        n_out = eng.record_regions_from_counts_device(k, db.ptr + shift, b.size, dc.ptr, dr.ptr, dr.ptr + 8 * m, m, ranges, do.ptr if cap else None, cap)
        eng.sync()
        out = do.download(U64, fill.size).reshape(-1, 3)
        do.free()
    for x in (db, dc, dr, ds):
        x.free()
    return stats, n_out, out


def main(out, ks):
    import kat_amd
    eng = kat_amd.Engine(0)
    res = {}
    for k in ks:
        b, st, ln = stats_case.mix(k)
        counts, _ = counts_for(k, b, st, ln)
        _, n_out, _ = device_call(eng, k, b, counts, st, ln, RANGES, 0)
        stats, n_out2, rows = device_call(eng, k, b, counts, st, ln, RANGES, sum(n_out))
        assert n_out == n_out2
        res["stats_%d" % k] = stats
        res["totals_%d" % k] = np.array(n_out, U64)
        res["regions_%d" % k] = rows[:sum(n_out)]
    np.savez(out, **res)
    eng.close()


if __name__ == "__main__":
    main(sys.argv[1], [int(x) for x in sys.argv[2:]])
