""".jf dumps whose records are ordered and packed on the device (katgpu_table_jf_records_device, katgpu_jf_dump for k <= 32):
the file equals the host writer's byte for byte (the header's time apart) and the numpy model of tests/jf_order_model.py."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kat_amd
from kat_amd import synth
from tests import jf_order_model as model
from tests.test_gpu_parity import assert_same_table

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (k, canonical) -> size hint, slot bytes the table must have (None: whatever the geometry gives)
CASES = {(27, True): (1 << 23, 8), (21, False): (0, 8), (32, False): (1 << 14, 12), (13, True): (0, None), (5, True): (0, None)}
_reads = {}


def reads():
    if "r" not in _reads:
        _reads["r"] = synth.reads(synth.genome(20000, seed=3), 0, 2000, seed=1)
    return _reads["r"]


def make_table(engine, k, canonical):
    hint, _ = CASES[(k, canonical)]
    return engine.table(k, canonical, size_hint=hint).count_bases(reads())


def whole(path):
    hdr, head, body = model.split(path)
    return hdr, model.blank_time(head), body


def host_file(table, path):
    keys, counts = table.export()
    kat_amd.jf_write_records(path, table.k, table.canonical, keys, counts)
    return keys, counts


@pytest.fixture(scope="module")
def dumped(engine, tmp_path_factory):
    """Per case, once: the table, its export, the host writer's file (a) and the dump (b)."""
    d = tmp_path_factory.mktemp("jf")
    out = {}
    for (k, canonical) in CASES:
        t = make_table(engine, k, canonical)
        a, b = str(d / ("a%d.jf" % k)), str(d / ("b%d.jf" % k))
        keys, counts = host_file(t, a)
        t.dump_jf(b)
        out[(k, canonical)] = (t, keys, counts, a, b)
    return out


@pytest.mark.parametrize("k,canonical", list(CASES))
def test_bytes(dumped, k, canonical):
    t, keys, counts, a, b = dumped[(k, canonical)]
    want_slot = CASES[(k, canonical)][1]
    if want_slot:
        assert t.slot_bytes() == want_slot
    hdr, head_b, body_b = whole(b)
    _, head_a, body_a = whole(a)
    assert head_a == head_b
    assert len(body_b) == keys.size * ((2 * k + 7) // 8 + 4)
    assert body_a == body_b
    r, cols = model.matrix(hdr)
    want, pos = model.record_bytes(k, keys, counts, cols, r)
    assert body_b == want
    if k in (21, 27):                                       # r < 2k: equal positions, so the order inside a run is exercised
        assert r < 2 * k
        same = np.diff(pos) == 0
        assert (same[1:] & same[:-1]).any(), "no run of three equal positions"
    if k == 5:
        assert r == 2 * k and not (np.diff(pos) == 0).any() # a bijective position


CHILD = """
import sys
import kat_amd
from kat_amd import synth
eng = kat_amd.Engine(0)
t = eng.table(27, True).count_bases(synth.reads(synth.genome(20000, seed=3), 0, 2000, seed=1))
t.dump_jf(sys.argv[1])
eng.close()
"""


@pytest.mark.parametrize("range_records", [1, 7, 4096])
def test_ranges(dumped, tmp_path, range_records):
    """The hook is read when the library loads: a fresh process per value.  At 1 every occupied position is a range of its own and the
    stretches between them are empty ranges' worth of positions."""
    _, keys, _, _, b = dumped[(27, True)]
    out = str(tmp_path / "ranged.jf")
    env = dict(os.environ, KATGPU_TESTING="1", KATGPU_JF_RANGE_RECORDS=str(range_records), KATGPU_TIMING="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", CHILD, out], capture_output=True, text=True, timeout=300, env=env, cwd=os.getcwd())
    assert r.returncode == 0, r.stderr
    m = re.search(r'katgpu_timing \{"phase": "jf_dump".*"ranges": (\d+)', r.stderr)
    assert m, r.stderr
    assert int(m.group(1)) >= keys.size // max(range_records, 3) // 2 > 1
    assert whole(out)[1:] == whole(b)[1:]


def test_entry_point(engine, dumped):
    t, keys, counts, _, b = dumped[(27, True)]
    hdr, _, body = whole(b)
    r, cols = model.matrix(hdr)
    size = 1 << r
    assert t.jf_records(r, cols).tobytes() == body
    cuts = [0, size // 7, size // 3 + 1, size - 5, size]
    parts = [t.jf_records(r, cols, lo, hi).tobytes() for lo, hi in zip(cuts, cuts[1:])]
    for (lo, hi), p in zip(zip(cuts, cuts[1:]), parts):
        assert p == model.record_bytes(27, keys, counts, cols, r, lo, hi)[0]
    assert b"".join(parts) == body
    ns = [t.jf_records(r, cols, lo, hi, count_only=True) for lo, hi in zip(cuts, cuts[1:])]
    assert sum(ns) == keys.size == t.stats()["distinct"] and [n * 11 for n in ns] == [len(p) for p in parts]
    assert t.jf_records(r, cols, 17, 17).size == 0 and t.jf_records(r, cols, size, size, count_only=True) == 0
    for bad in (dict(r=0), dict(r=55), dict(pos_lo=5, pos_hi=4), dict(pos_hi=size + 1)):
        kw = dict(r=r, cols=cols)
        kw.update(bad)
        with pytest.raises(kat_amd.binding.KatGpuError) as e:
            t.jf_records(**kw)
        assert e.value.code == 1


@pytest.mark.parametrize("n", [1000, 2500])
def test_one_position_for_all(engine, n):
    """A matrix that sends every key to position 5: one run of n records, more than the LDS tile a bucket is sorted in, so the
    order comes from the ranking path through global memory.  It must be by key."""
    k, r = 16, 10
    c = 2 * k
    cols = np.zeros(c, np.uint64)
    for i in range(r):
        cols[c - 1 - i] = np.uint64(1 << i)
    rng = np.random.default_rng(n)
    keys = ((rng.permutation(4 * n)[:n].astype(np.uint64)) << np.uint64(r)) | np.uint64(5)
    counts = rng.integers(1, 1 << 16, size=n, dtype=np.uint64)
    t = engine.table(k, False)
    t.merge_host(keys, counts)
    assert (model.positions(keys, cols, r) == 5).all()
    got = t.jf_records(r, cols)
    want, _ = model.record_bytes(k, keys, counts, cols, r)
    assert got.tobytes() == want
    rec = got.reshape(n, 8)
    assert (np.diff(rec[:, :4].copy().view("<u4")[:, 0].astype(np.int64)) > 0).all()
    assert t.jf_records(r, cols, 5, 6).tobytes() == want and t.jf_records(r, cols, 6, 1 << r).size == 0
    t.free()


def test_skewed_matrix_is_refused(engine):
    """A zero matrix sends the whole table to position 0.  Beyond 2^16 records in one bucket the entry refuses (the ranking path is
    quadratic) and says how many records the range holds; the dump of the same table, whose own matrix spreads it, is unaffected."""
    k, r, n = 16, 10, (1 << 16) + 1
    keys = np.arange(n, dtype=np.uint64) * np.uint64(3)
    t = engine.table(k, False)
    t.merge_host(keys, np.ones(n, np.uint64))
    cols = np.zeros(2 * k, np.uint64)
    assert t.jf_records(r, cols, count_only=True) == n
    with pytest.raises(kat_amd.binding.KatGpuError, match="does not spread") as e:
        t.jf_records(r, cols)
    assert e.value.code == 1
    t.free()


@pytest.mark.parametrize("k,hint,slot", [(21, 0, 8), (32, 1 << 14, 12)])
def test_counts(engine, tmp_path, k, hint, slot):
    """Counts beyond the slot's own field live in the overflow side table; beyond 32 bits they are written saturated."""
    t = engine.table(k, False, size_hint=hint)
    keys = np.array([11, 22, 33, 44, 55], np.uint64)
    counts = np.array([2**32 - 1, 2**32, 2**40, 2**29 + 3, 1], np.uint64)
    t.merge_host(keys, counts)
    assert t.slot_bytes() == slot
    assert list(map(int, t.get(keys))) == list(map(int, counts))
    b = str(tmp_path / "c.jf")
    t.dump_jf(b)
    hdr, _, body = whole(b)
    kb = (2 * k + 7) // 8
    rec = np.frombuffer(body, np.uint8).reshape(5, kb + 4)
    by_key = {int.from_bytes(bytes(x[:kb]), "little"): bytes(x[kb:]) for x in rec}
    assert by_key[11] == by_key[22] == by_key[33] == b"\xff\xff\xff\xff"
    assert by_key[44] == (2**29 + 3).to_bytes(4, "little") and by_key[55] == (1).to_bytes(4, "little")
    r, cols = model.matrix(hdr)
    assert body == model.record_bytes(k, keys, counts, cols, r)[0]
    t.free()


def test_edges(engine, tmp_path):
    a, b = str(tmp_path / "a.jf"), str(tmp_path / "b.jf")
    # an empty table: the header alone
    t = engine.table(27, True)
    host_file(t, a)
    t.dump_jf(b)
    assert whole(a)[1:] == whole(b)[1:] and whole(b)[2] == b""
    # one record
    t.merge_host(np.array([123456789], np.uint64), np.array([7], np.uint64))
    host_file(t, a)
    t.dump_jf(b)
    assert whole(a)[1:] == whole(b)[1:] and len(whole(b)[2]) == 11
    t.free()
    # a table that has regrown
    t = engine.table(27, True, size_hint=1 << 12).count_bases(reads())
    assert t.regrows > 0
    host_file(t, a)
    t.dump_jf(b)
    assert whole(a)[1:] == whole(b)[1:]
    t.free()
    # the all-ones 32-mer lives beside the slots
    t = engine.table(32, False, size_hint=1 << 14)
    t.merge_host(np.array([2**64 - 1, 5, 2**63], np.uint64), np.array([3, 4, 5], np.uint64))
    host_file(t, a)
    t.dump_jf(b)
    assert whole(a)[1:] == whole(b)[1:] and len(whole(b)[2]) == 36
    t.free()
    # k = 33: not this entry's, and the dump goes the way it always went
    w = engine.table(33, True, size_hint=1 << 14).count_bases(reads())
    with pytest.raises(kat_amd.binding.KatGpuError) as e:
        w.jf_records(10, np.zeros(66, np.uint64))
    assert e.value.code == 6
    w.dump_jf(b)
    back = engine.load_jf(b)
    for x, y in zip(back.dump_sorted(), w.dump_sorted()):
        assert np.array_equal(x, y)
    w.free()


@pytest.mark.parametrize("k,canonical", [(27, True), (32, False)])
def test_round_trip(engine, ko, dumped, k, canonical):
    t, _, _, _, b = dumped[(k, canonical)]
    back = engine.load_jf(b)
    for x, y in zip(back.dump_sorted(), t.dump_sorted()):
        assert np.array_equal(x, y)
    assert_same_table(t, ko.Table.from_jf(b))
    assert_same_table(back, ko.Table.from_jf(b))
    back.free()
