"""Run in a subprocess by tests/test_gpu_key_widths.py with KATGPU_TEST_REGION_SLOTS=256 (small tables of several regions; the one-word
ones become packed): `python key_widths_case.py K CANONICAL`.  One scenario through the kernels that are one body for both key widths
(k_regrow, k_merge, k_partition, k_get, k_filter, k_export's and k_partition's exports) and their entry points, against the oracle,
kat_amd.dist's owner functions and tests/filter_model.py.  A record is (key columns, count): one key column for k <= 32, (hi, lo) beyond."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kat_amd  # noqa: E402
from kat_amd import dist, synth  # noqa: E402
from oracle import koracle as ko  # noqa: E402
from tests import filter_model as fm  # noqa: E402

ERR_K = 6
# what the entry point of the other key width answers (the texts of kg_host.hpp's NARROW_ONLY / WIDE_ONLY)
NARROW_ON_WIDE = {
    "get": "katgpu_table_get: use katgpu_table_get_wide; is not available for k > 32 (k = %u)",
    "export": "katgpu_table_export: use katgpu_table_export_wide; is not available for k > 32 (k = %u)",
    "merge_host": "katgpu_table_merge_host: use katgpu_table_merge_host_wide; is not available for k > 32 (k = %u)",
    "partition": "katgpu_table_partition is not available for k > 32 (k = %u)",
    "merge_device": "katgpu_table_merge_device is not available for k > 32 (k = %u)",
}
WIDE_ON_NARROW = {
    "get": "katgpu_table_get_wide is for k > 32 tables (k = %u): use katgpu_table_get",
    "export": "katgpu_table_export_wide is for k > 32 tables (k = %u): use katgpu_table_export",
    "merge_host": "katgpu_table_merge_host_wide is for k > 32 tables (k = %u): use katgpu_table_merge_host",
    "partition": "katgpu_table_partition_wide is for k > 32 tables (k = %u): use katgpu_table_partition",
    "merge_device": "katgpu_table_merge_device_wide is for k > 32 tables (k = %u): use katgpu_table_merge_device",
}


def dump(t):
    """(key columns, counts) of a device or oracle table, sorted by key."""
    d = t.dump_sorted()
    return tuple(d[:-1]), d[-1]


def sort_records(cols, counts):
    order = np.lexsort(tuple(reversed(cols)))
    return tuple(c[order] for c in cols), counts[order]


def same(a, b):
    return len(a[0]) == len(b[0]) and all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and np.array_equal(a[1], b[1])


def select(rec, mask):
    return tuple(c[mask] for c in rec[0]), rec[1][mask]


def main(k, canonical):
    wide = k > 32
    nk = 2 if wide else 1                                               # key columns
    eng = kat_amd.Engine(0)
    g = synth.genome(3000, seed=k)
    stream = np.concatenate([synth.reads(g, 0, 2000, read_len=100, frag_len=200, err_ppm=500, seed=5),
                             np.frombuffer(b"A" * 100 + b"N" + b"T" * 100 + b"N", np.uint8)])
    t = eng.table(k, canonical).count_bases(stream)
    o = (ko.WideTable if wide else ko.Table)(k, canonical).count_bases(stream)
    want = dump(o)
    n = want[1].size
    assert 2000 <= n <= 30000, n                                       # a few thousand distinct k-mers
    assert t.stats()["capacity"] >= 4 * 256                            # several regions
    if k == 21:
        assert t.slot_bytes() == 8                                      # packed
    if k == 32:
        assert t.slot_bytes() == 12                                     # KV12 ...
        assert not canonical and want[0][0][-1] == np.uint64(2 ** 64 - 1)    # ... whose all-ones k-mer (the poly-T read's) lives in CTR_ONES

    # (a) export
    assert same(dump(t), want)

    # (b) partition sizes and partition, 3 owners
    P = 3
    owner = dist.owner_of_wide(want[0][0], want[0][1], k, P) if wide else dist.owner_of(want[0][0], k, P)
    sizes = t.partition_sizes(P)
    assert np.array_equal(sizes.astype(np.int64), np.bincount(owner, minlength=P))
    off = np.concatenate([[0], np.cumsum(sizes.astype(np.int64))])
    bufs = [eng.alloc(8 * n) for _ in range(nk + 1)]
    (t.partition_wide if wide else t.partition)(P, off[:P].astype(np.uint64), *[b.ptr for b in bufs])
    cols = [b.download(np.uint64, n) for b in bufs]
    for p in range(P):
        part = sort_records(tuple(c[off[p]:off[p + 1]] for c in cols[:nk]), cols[nk][off[p]:off[p + 1]])
        assert same(part, select(want, owner == p)), p

    # (c) merge the parts into a table that has to grow; a second time: every count doubled
    m = eng.table(k, canonical, size_hint=64)
    for rnd in (1, 2):
        for p in range(P):
            (m.merge_device_wide if wide else m.merge_device)(*[b.ptr + 8 * int(off[p]) for b in bufs], int(sizes[p]))
        assert same(dump(m), (want[0], want[1] * np.uint64(rnd))), rnd
    assert m.regrows >= 1

    # (d) counts beyond 32 bits and lookups
    i = n // 2
    key = tuple(c[i:i + 1] for c in want[0])
    big = np.array([(1 << 32) + 5], np.uint64)
    get = m.get_wide if wide else m.get
    for _ in range(2):
        (m.merge_host_wide if wide else m.merge_host)(*key, big)
    total = 2 * int(want[1][i]) + 2 * ((1 << 32) + 5)
    assert int(get(*key)[0]) == total
    rc = dist._revcomp_wide(key[0], key[1], k) if wide else (dist._revcomp(key[0], k),)
    present = set(zip(*[c.tolist() for c in want[0]]))
    if canonical:                                                       # (k is odd: the reverse complement is another k-mer, and not stored)
        assert tuple(int(c[0]) for c in rc) not in present
        assert int(get(*rc, canonicalise=True)[0]) == total
        assert int(get(*rc)[0]) == 0
    head, last = tuple(int(c[0]) for c in key[:-1]), int(key[-1][0])
    absent = next(c for c in (head + (last ^ d,) for d in range(1, 1 << 20)) if c not in present)      # other last bases, until no stored k-mer
    assert int(get(*[np.array([x], np.uint64) for x in absent])[0]) == 0

    # (e) filter: a count x GC box that splits the set
    box = dict(low_count=2, high_count=10000, low_gc=(2 * k) // 5, high_gc=(3 * k) // 5)
    keep, drop, ctr = t.filter(separate=True, **box)
    mk, md, mctr = fm.filter_kmer(want[0] if wide else want[0][0], want[1], k, separate=True, **box)
    assert 0 < mctr["keep_distinct"] < n and mctr["drop_distinct"] > 0
    assert ctr == mctr
    got_keep, got_drop = dump(keep), dump(drop)
    assert same(got_keep, select(want, mk)) and same(got_drop, select(want, md))
    union = sort_records(tuple(np.concatenate([a, b]) for a, b in zip(got_keep[0], got_drop[0])), np.concatenate([got_keep[1], got_drop[1]]))
    assert same(union, want)

    # (f) the entry points of the other key width refuse, in the words they always had
    one = np.array([1], np.uint64)
    ptrs = [b.ptr for b in bufs]
    if wide:
        calls = {"get": lambda: t.get(one), "export": t.export, "merge_host": lambda: t.merge_host(one, one),
                 "partition": lambda: t.partition(1, one, ptrs[0], ptrs[1]), "merge_device": lambda: t.merge_device(ptrs[0], ptrs[1], 1)}
        texts = NARROW_ON_WIDE
    else:
        extra = eng.alloc(8)
        calls = {"get": lambda: t.get_wide(one, one), "export": t.export_wide, "merge_host": lambda: t.merge_host_wide(one, one, one),
                 "partition": lambda: t.partition_wide(1, one, ptrs[0], ptrs[1], extra.ptr),
                 "merge_device": lambda: t.merge_device_wide(ptrs[0], ptrs[1], extra.ptr, 1)}
        texts = WIDE_ON_NARROW
    for name, call in calls.items():
        try:
            call()
        except kat_amd.KatGpuError as e:
            assert e.code == ERR_K and e.message == texts[name] % k, (name, e.code, e.message)
        else:
            raise AssertionError(name + " did not refuse")
    assert same(dump(t), want)                                          # (and left the table as it was)
    print("key widths ok: k = %d, %d records" % (k, n))


if __name__ == "__main__":
    main(int(sys.argv[1]), sys.argv[2] == "1")
