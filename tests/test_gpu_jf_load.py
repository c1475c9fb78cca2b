"""Packed .jf records added to a table on the device (katgpu_table_add_jf_records_device) and the load built on it
(katgpu_jf_load, katgpu_jf_load_part): the table equals the numpy model of tests/jf_load_model.py, the reference's own reader
(the oracle's Table.from_jf, k <= 32) and the load through the host reader and katgpu_table_merge_host[_wide]."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kat_amd
from tests import jf_load_model as model
from tests.test_gpu_jf_dump import CASES, make_table, reads
from tests.test_gpu_parity import assert_same_table
from tests.test_jf_load_model import records

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
# (k, counter_len) -> record bytes: each a different way for a record to straddle the 4- and 16-byte words it is read from
ROWS = [(1, 1, 2), (5, 4, 6), (16, 4, 8), (21, 4, 10), (27, 4, 11), (31, 8, 16), (32, 1, 9), (33, 4, 13), (48, 4, 16), (63, 5, 21)]
NS = [0, 1, 2, 255, 256, 257, 1024, 1025, 5000]       # around the workgroup (256 lanes) and its tile (1024 records); 5000: five tiles, the last short
OFFSETS = [0, 1, 3, 15]


def table_is(t, hi, lo, count):
    got = t.dump_sorted()
    if t.k > 32:
        want = (hi, lo, count)
    else:
        assert not np.asarray(hi).any()
        want = (lo, count)
    assert got[0].size == want[0].size, "distinct differs: table %d model %d" % (got[0].size, want[0].size)
    for x, y in zip(got, want):
        assert np.array_equal(x, y)
    assert t.stats()["distinct"] == want[0].size


def packed(k, n, counter_len, seed):
    """n records of distinct keys with non-zero counts that fit counter_len bytes: (their bytes, what a table holds after them)."""
    hi, lo, counts = records(k, n, seed)
    counts = (counts << U64(31) if counter_len == 8 else counts) & U64((1 << (8 * counter_len)) - 1)
    counts[counts == 0] = U64(1)
    raw = np.frombuffer(model.pack(hi, lo, counts, 2 * k, counter_len), np.uint8)
    return raw, model.combine(*model.decode(raw, 2 * k, counter_len))


@pytest.mark.parametrize("k,counter_len,rb", ROWS)
def test_entry_point(engine, k, counter_len, rb):
    assert model.record_bytes(2 * k, counter_len) == rb
    for n in NS:
        raw, want = packed(k, n, counter_len, 1000 * k + n)
        assert raw.size == min(n, 4 ** k) * rb and want[0].size == min(n, 4 ** k)
        for off in OFFSETS:
            t = engine.table(k, False, size_hint=1 << 14)
            t.add_jf_records(raw, 2 * k, counter_len, offset=off)
            table_is(t, *want)
            t.free()


@pytest.mark.parametrize("k,hint,slot", [(27, 1 << 23, 8), (32, 1 << 14, 12)])
def test_slot_layouts(engine, k, hint, slot):
    raw, want = packed(k, 5000, 4, k)
    for off in OFFSETS:
        t = engine.table(k, False, size_hint=hint)
        assert t.slot_bytes() == slot
        t.add_jf_records(raw, 2 * k, 4, offset=off)
        table_is(t, *want)
        t.add_jf_records(raw, 2 * k, 4, offset=off)           # and once more into the table as it stands: every count doubles
        table_is(t, want[0], want[1], want[2] * U64(2))
        t.free()


def get(t, hi, lo):
    if t.k > 32:
        return list(map(int, t.get_wide(np.array(hi, U64), np.array(lo, U64))))
    return list(map(int, t.get(np.array(lo, U64))))


@pytest.mark.parametrize("k,hint,slot", [(27, 1 << 23, 8), (32, 1 << 14, 12), (33, 1 << 14, 20)])
def test_semantics(engine, k, hint, slot):
    t = engine.table(k, False, size_hint=hint)
    assert t.slot_bytes() == slot
    h = 1 if k > 32 else 0
    # one key in three records: the sum; a zero count: no key; 3 x (2^32 - 1): beyond any slot's field, exact from the side table
    hi = [h, 0, h, 0, h, 0, 0, 0]
    lo = [77, 5, 77, 123456, 77, 9, 9, 9]
    counts = [10, 1, 20, 0, 30, 2**32 - 1, 2**32 - 1, 2**32 - 1]
    t.add_jf_records(np.frombuffer(model.pack(hi, lo, counts, 2 * k, 4), np.uint8), 2 * k, 4, offset=3)
    assert get(t, [h, 0, 0, 0], [77, 5, 123456, 9]) == [60, 1, 0, 3 * (2**32 - 1)]
    assert t.stats()["distinct"] == 3
    # 8-byte counters: 2^40 in one record
    t.add_jf_records(np.frombuffer(model.pack([h, 0], [4242, 5], [2**40, 2**40 + 1], 2 * k, 8), np.uint8), 2 * k, 8, offset=1)
    assert get(t, [h, 0], [4242, 5]) == [2**40, 2**40 + 2]
    table_is(t, *model.combine(np.array([h, 0, 0, h], U64), np.array([77, 5, 9, 4242], U64), np.array([60, 2**40 + 2, 3 * (2**32 - 1), 2**40], U64)))
    t.free()


@pytest.mark.parametrize("k", [32, 16])
def test_all_ones_kmer(engine, k):
    ones = (1 << (2 * k)) - 1
    t = engine.table(k, False, size_hint=1 << 14)
    raw = np.frombuffer(model.pack([0, 0, 0], [ones, 5, ones], [3, 4, 2**33], 2 * k, 8), np.uint8)
    t.add_jf_records(raw, 2 * k, 8, offset=15)
    assert get(t, [0, 0], [ones, 5]) == [2**33 + 3, 4]
    table_is(t, np.zeros(2, U64), np.array([5, ones], U64), np.array([4, 2**33 + 3], U64))
    t.free()


@pytest.mark.parametrize("k", [27, 33])
def test_junk_above_the_key_is_ignored(engine, k):
    kb = (2 * k + 7) // 8
    raw, want = packed(k, 700, 4, 5 * k)
    rec = raw.reshape(-1, kb + 4).copy()
    junk = (0xFF << (2 * k - 8 * (kb - 1))) & 0xFF
    assert junk and not (rec[:, kb - 1] & junk).any()
    rec[::2, kb - 1] |= junk
    rec[1::4, kb - 1] |= junk & 0x40
    t = engine.table(k, False, size_hint=1 << 14)
    t.add_jf_records(rec.ravel(), 2 * k, 4, offset=1)
    table_is(t, *want)
    for x, y in zip(model.combine(*model.decode(rec.tobytes(), 2 * k, 4)), want):
        assert np.array_equal(x, y)
    t.free()


def test_arguments(engine):
    for k in (27, 33):
        t = engine.table(k, False, size_hint=1 << 14)
        none = np.zeros(0, np.uint8)
        for key_len in (2 * k - 2, 2 * k + 2, 2):
            with pytest.raises(kat_amd.binding.KatGpuError) as e:
                t.add_jf_records(none, key_len, 4)
            assert e.value.code == 9
        for counter_len in (0, 9):
            with pytest.raises(kat_amd.binding.KatGpuError) as e:
                t.add_jf_records(none, 2 * k, counter_len)
            assert e.value.code == 1
        t.add_jf_records(none, 2 * k, 4, offset=5)              # no records: nothing happens
        assert t.stats()["distinct"] == 0
        t.free()


@pytest.mark.parametrize("k", [27, 33])
def test_growth(engine, k):
    raw, want = packed(k, 20000, 4, 7 * k)
    t = engine.table(k, False, size_hint=1 << 12)
    t.add_jf_records(raw, 2 * k, 4, offset=3)
    assert t.regrows > 0
    table_is(t, *want)
    t.free()
    t = engine.table(k, False, size_hint=1 << 12, disable_grow=True)
    with pytest.raises(kat_amd.binding.KatGpuError, match="Hash full") as e:
        t.add_jf_records(raw, 2 * k, 4)
    assert e.value.code == 7
    t.free()


# ---- katgpu_jf_load ----

def old_route(engine, path):
    """The load as it was: the host reader's arrays merged into a fresh table."""
    k, canonical, hi, lo, counts = kat_amd.jf_read_records_wide(path)
    t = engine.table(k, canonical, size_hint=max(int(lo.size / 0.6) + 1024, 1 << 16))
    if k > 32:
        t.merge_host_wide(hi, lo, counts)
    else:
        t.merge_host(lo, counts)
    return t


def check_load(engine, ko, path, ko_too=True):
    t = engine.load_jf(path)
    k, canonical, hi, lo, counts = model.load(path)
    assert (t.k, t.canonical) == (k, canonical)
    table_is(t, hi, lo, counts)
    old = old_route(engine, path)
    for x, y in zip(t.dump_sorted(), old.dump_sorted()):
        assert np.array_equal(x, y)
    old.free()
    if k <= 32 and ko_too:
        assert_same_table(t, ko.Table.from_jf(path))
    return t


@pytest.fixture(scope="module")
def files(engine, tmp_path_factory):
    """(k, canonical) -> a dump of the table test_gpu_jf_dump counts for it; k = 33 and k = 51 besides."""
    d = tmp_path_factory.mktemp("jfload")
    out = {}
    for (k, canonical) in list(CASES) + [(33, True), (51, False)]:
        t = make_table(engine, k, canonical) if (k, canonical) in CASES else engine.table(k, canonical, size_hint=1 << 14).count_bases(reads())
        out[(k, canonical)] = str(d / ("t%d.jf" % k))
        t.dump_jf(out[(k, canonical)])
        t.free()
    return out


@pytest.mark.parametrize("k,canonical", list(CASES) + [(33, True), (51, False)])
def test_load_dumped(engine, ko, files, k, canonical):
    t = check_load(engine, ko, files[(k, canonical)])
    assert t.stats()["distinct"] > (1000 if k > 5 else 100)
    t.free()


@pytest.mark.parametrize("k", [27, 33])
@pytest.mark.parametrize("counter_len", [2, 8])
def test_load_other_counter_widths(engine, ko, tmp_path, k, counter_len):
    hi, lo, counts = records(k, 3000, 11 * k + counter_len)
    counts = (counts << U64(31)) if counter_len == 8 else (counts & U64(0xFFFF)) | U64(1)
    p = model.write(str(tmp_path / "c.jf"), k, True, hi, lo, counts, counter_len)
    t = check_load(engine, ko, p)
    if counter_len == 8:
        assert int(t.dump_sorted()[-1].max()) >= 2**32
    t.free()


def test_load_edges(engine, ko, tmp_path):
    p = str(tmp_path / "e.jf")
    none = np.zeros(0, U64)
    for k in (27, 33):
        kat_amd.jf_write_records_wide(p, k, True, none, none, none)            # the header alone
        assert model.split(p)[2] == b""
        t = check_load(engine, ko, p)
        assert t.stats()["distinct"] == 0
        t.free()
        kat_amd.jf_write_records_wide(p, k, False, np.array([int(k > 32)], U64), np.array([123456789], U64), np.array([7], U64))
        t = check_load(engine, ko, p)
        assert t.stats()["distinct"] == 1 and not t.canonical
        t.free()
    # a body that is no whole number of records
    kat_amd.jf_write_records(p, 27, True, np.array([1, 2, 3], U64), np.array([4, 5, 6], U64))
    with open(p, "ab") as f:
        f.write(b"\0\0\0")
    with pytest.raises(kat_amd.binding.KatGpuError, match=r"Size of database \(36\) must be a multiple of the length of a record \(11\)") as e:
        engine.load_jf(p)
    assert e.value.code == 3
    with pytest.raises(kat_amd.binding.KatGpuError, match="Could not find input file at: ") as e:
        engine.load_jf(str(tmp_path / "missing.jf"))
    assert e.value.code == 2


CHILD = """
import sys
import numpy as np
import kat_amd
eng = kat_amd.Engine(0)
t = eng.load_jf(sys.argv[1])
keys, counts = t.dump_sorted()
np.savez(sys.argv[2], keys=keys, counts=counts)
t.free()
eng.close()
"""


@pytest.mark.parametrize("chunk", [1, 7, 4096])
def test_chunks(engine, files, tmp_path, chunk):
    """The hook is read when the library loads: a fresh process per value.  One record a chunk on a small file, 7 and 4096 on the
    k = 27 dump: every chunk but the last is whole, and the two buffers are gone round many times."""
    path = files[(27, True)]
    if chunk == 1:
        hi, lo, counts = records(27, 700, 3)
        path = model.write(str(tmp_path / "small.jf"), 27, True, hi, lo, counts, 4)
    n = len(model.split(path)[2]) // 11
    assert n <= 1000 if chunk == 1 else n > 2 * 4096
    out = str(tmp_path / "got.npz")
    env = dict(os.environ, KATGPU_TESTING="1", KATGPU_JF_LOAD_RECORDS=str(chunk), KATGPU_TIMING="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", CHILD, path, out], capture_output=True, text=True, timeout=300, env=env, cwd=os.getcwd())
    assert r.returncode == 0, r.stderr
    m = re.search(r'katgpu_timing \{"phase": "jf_load", "records": (\d+), "chunks": (\d+), "read_s": [\d.]+, "copy_s": [\d.]+, "device_s": [\d.]+, "total_s": [\d.]+\}', r.stderr)
    assert m, r.stderr
    assert int(m.group(1)) == n and int(m.group(2)) == -(-n // chunk) > 2
    t = engine.load_jf(path)
    got = np.load(out)
    keys, counts = t.dump_sorted()
    assert np.array_equal(got["keys"], keys) and np.array_equal(got["counts"], counts)
    t.free()


def geometry(t):
    if t.k > 32:                                                # (katgpu_table_geometry serves the region-ordered exchange, which wide tables do not take)
        return t.stats(want_total=False)["capacity"], t.slot_bytes()
    g = t.geometry()
    return tuple(getattr(g, f) for f, _ in g._fields_)


@pytest.mark.parametrize("k,canonical", [(27, True), (33, True)])
def test_parts(engine, files, k, canonical):
    path = files[(k, canonical)]
    whole = engine.load_jf(path)
    parts = [engine.load_jf_part(path, p, 3) for p in range(3)]
    assert len({geometry(t) for t in parts}) == 1
    n = whole.stats()["distinct"]
    assert [t.stats()["distinct"] for t in parts] == [n * (p + 1) // 3 - n * p // 3 for p in range(3)]
    union = engine.table(k, canonical, size_hint=1 << 16)
    for t in parts:
        if k > 32:
            union.merge_host_wide(*t.export_wide())
        else:
            union.merge_host(*t.export())
        t.free()
    for x, y in zip(union.dump_sorted(), whole.dump_sorted()):
        assert np.array_equal(x, y)
    union.free()
    whole.free()


def test_parts_edges(engine, tmp_path):
    p = str(tmp_path / "two.jf")
    kat_amd.jf_write_records(p, 27, True, np.array([10, 20], U64), np.array([1, 2], U64))
    parts = [engine.load_jf_part(p, i, 3) for i in range(3)]
    assert sorted(t.stats()["distinct"] for t in parts) == [0, 1, 1]
    assert len({geometry(t) for t in parts}) == 1
    got = sorted((int(k), int(c)) for t in parts for k, c in zip(*t.export()))
    assert got == sorted(zip(*(map(int, x) for x in kat_amd.jf_read_records(p)[2:])))
    for t in parts:
        t.free()
    for part, n_parts in ((3, 3), (1, 1), (0, 0), (7, 2)):
        with pytest.raises(kat_amd.binding.KatGpuError) as e:
            engine.load_jf_part(p, part, n_parts)
        assert e.value.code == 1
