""".jf dumps of two-word tables (33 <= k <= 63) whose records are ordered and packed on the device (katgpu_table_jf_records_device_wide,
katgpu_jf_dump): the file equals the host writer's byte for byte (the header's time apart) and the numpy model of
tests/jf_order_model_wide.py, which tests/test_jf_order_model_wide.py pins to the host writer and to the reference's reader."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import kat_amd
from kat_amd import synth
from tests import jf_order_model_wide as model
from tests.test_gpu_wide import assert_same_wide

pytestmark = pytest.mark.gpu

U64 = np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (k, canonical) -> size hint (2^14: the table regrows while it counts)
CASES = {(33, True): 0, (36, False): 0, (47, True): 1 << 14, (63, False): 0}
_reads = {}


def reads():
    if "r" not in _reads:
        _reads["r"] = synth.reads(synth.genome(20000, seed=3), 0, 2000, seed=1)
    return _reads["r"]


def whole(path):
    hdr, head, body = model.split(path)
    return hdr, model.blank_time(head), body


def host_file(table, path):
    hi, lo, counts = table.export_wide()
    kat_amd.jf_write_records_wide(path, table.k, table.canonical, hi, lo, counts)
    return hi, lo, counts


def wide_table(engine, k, hi, lo, counts):
    t = engine.table(k, False)
    t.merge_host_wide(np.asarray(hi, U64), np.asarray(lo, U64), np.asarray(counts, U64))
    return t


def words(raw, k):
    """(hi, lo, the 4 count bytes) of packed records."""
    kb = (2 * k + 7) // 8
    rec = np.frombuffer(bytes(raw), np.uint8).reshape(-1, kb + 4)
    lo = rec[:, :8].copy().view("<u8")[:, 0]
    hi8 = np.zeros((rec.shape[0], 8), np.uint8)
    hi8[:, :kb - 8] = rec[:, 8:kb]
    return hi8.view("<u8")[:, 0], lo, rec[:, kb:]


@pytest.fixture(scope="module")
def dumped(engine, tmp_path_factory):
    """Per case, once: the table, its export, the host writer's file (a) and the dump (b)."""
    d = tmp_path_factory.mktemp("jfw")
    out = {}
    for (k, canonical), hint in CASES.items():
        t = engine.table(k, canonical, size_hint=hint).count_bases(reads())
        a, b = str(d / ("a%d.jf" % k)), str(d / ("b%d.jf" % k))
        hi, lo, counts = host_file(t, a)
        t.dump_jf(b)
        out[(k, canonical)] = (t, hi, lo, counts, a, b)
    return out


@pytest.mark.parametrize("k,canonical", list(CASES))
def test_bytes(dumped, k, canonical):
    t, hi, lo, counts, a, b = dumped[(k, canonical)]
    assert t.slot_bytes() == 20
    if CASES[(k, canonical)]:
        assert t.regrows > 0
    hdr, head_b, body_b = whole(b)
    _, head_a, body_a = whole(a)
    assert head_a == head_b
    assert lo.size > 10000 and len(body_b) == lo.size * ((2 * k + 7) // 8 + 4)
    assert body_a == body_b
    r, cols = model.matrix(hdr)
    want, pos, shi, slo = model.record_bytes(k, hi, lo, counts, cols, r)
    assert body_b == want
    assert r < 2 * k
    same = np.diff(pos) == 0
    assert (same[1:] & same[:-1]).any(), "no run of three equal positions"
    # a sort that compared lo before hi would turn such neighbours round
    assert (same & (shi[1:] > shi[:-1]) & (slo[1:] < slo[:-1])).any(), "no run ordered by hi against lo"


CHILD = """
import sys
import kat_amd
from kat_amd import synth
eng = kat_amd.Engine(0)
t = eng.table(47, True, size_hint=1 << 14).count_bases(synth.reads(synth.genome(20000, seed=3), 0, 2000, seed=1))
t.dump_jf(sys.argv[1])
eng.close()
"""


@pytest.mark.parametrize("range_records", [1, 7, 4096])
def test_ranges(dumped, tmp_path, range_records):
    """The hook is read when the library loads: a fresh process per value."""
    b = dumped[(47, True)][5]
    out = str(tmp_path / "ranged.jf")
    env = dict(os.environ, KATGPU_TESTING="1", KATGPU_JF_RANGE_RECORDS=str(range_records), KATGPU_TIMING="1", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", CHILD, out], capture_output=True, text=True, timeout=300, env=env, cwd=os.getcwd())
    assert r.returncode == 0, r.stderr
    m = re.search(r'katgpu_timing \{"phase": "jf_dump".*"ranges": (\d+)', r.stderr)
    assert m, r.stderr
    assert int(m.group(1)) > 1
    assert whole(out)[1:] == whole(b)[1:]


def test_entry_point(engine, dumped):
    t, hi, lo, counts, _, b = dumped[(47, True)]
    hdr, _, body = whole(b)
    r, cols = model.matrix(hdr)
    size = 1 << r
    assert t.jf_records_wide(r, cols).tobytes() == body
    cuts = [0, size // 7, size // 3 + 1, size // 2, size - 5, size]
    parts = [t.jf_records_wide(r, cols, a, z).tobytes() for a, z in zip(cuts, cuts[1:])]
    for (a, z), p in zip(zip(cuts, cuts[1:]), parts):
        assert p == model.record_bytes(47, hi, lo, counts, cols, r, a, z)[0]
    assert b"".join(parts) == body
    ns = [t.jf_records_wide(r, cols, a, z, count_only=True) for a, z in zip(cuts, cuts[1:])]
    assert sum(ns) == lo.size == t.stats()["distinct"] and [n * 16 for n in ns] == [len(p) for p in parts]
    assert t.jf_records_wide(r, cols, 17, 17).size == 0 and t.jf_records_wide(r, cols, size, size, count_only=True) == 0
    for bad in (dict(r=0), dict(r=64), dict(pos_lo=5, pos_hi=4), dict(pos_hi=size + 1)):
        kw = dict(r=r, cols=cols)
        kw.update(bad)
        with pytest.raises(kat_amd.binding.KatGpuError) as e:
            t.jf_records_wide(**kw)
        assert e.value.code == 1
    n = engine.table(27, True).count_bases(reads())
    with pytest.raises(kat_amd.binding.KatGpuError) as e:
        n.jf_records_wide(10, np.zeros(54, U64))
    assert e.value.code == 6
    n.free()


def test_position_from_high_word(engine):
    """Only the columns of key bits 64 .. 73 are set: the position is the low ten bits of hi, whatever lo is."""
    k, r, n = 40, 10, 5000
    c = 2 * k
    cols = np.zeros(c, U64)
    for j in range(r):
        cols[c - 1 - (64 + j)] = U64(1 << j)
    rng = np.random.default_rng(40)
    v = rng.permutation(1 << 16)[:n].astype(U64)            # distinct (hi, lo) pairs: 4096 values of hi, four to a position
    hi, lo = v & U64(0x0FFF), (v >> U64(12)) * U64(0x9E3779B97F4A7C15)
    counts = rng.integers(1, 1 << 16, size=n, dtype=U64)
    assert np.unique(np.stack([hi, lo], 1), axis=0).shape[0] == n and np.unique(hi).size < n - 1000
    pos = model.positions(hi, lo, cols, r)
    assert np.array_equal(pos, hi & U64(1023)) and np.unique(pos).size > 900
    t = wide_table(engine, k, hi, lo, counts)
    want, _, shi, slo = model.record_bytes(k, hi, lo, counts, cols, r)
    assert ((shi[1:] == shi[:-1]) & (slo[1:] > slo[:-1])).any()
    assert t.jf_records_wide(r, cols).tobytes() == want
    t.free()


@pytest.mark.parametrize("n", [1000, 2500])
def test_one_position_for_all(engine, n):
    """A matrix that sends every key to position 5: one run of n records, more than the LDS tile a bucket is sorted in, so the
    order comes from the ranking path through global memory.  It must be by (hi, lo)."""
    k, r = 40, 10
    c = 2 * k
    cols = np.zeros(c, U64)
    for i in range(r):
        cols[c - 1 - i] = U64(1 << i)
    rng = np.random.default_rng(n)
    v = rng.permutation(4 * n)[:n].astype(U64)
    q = v >> U64(2)                                         # up to four records share a value of lo; their hi differ in the low bits
    lo = (q << U64(50)) | (q << U64(r)) | U64(5)
    hi = ((v * U64(2654435761)) & U64(0xFFFC)) | (v & U64(3))
    counts = rng.integers(1, 1 << 16, size=n, dtype=U64)
    assert np.unique(lo).size < n - 8 and np.unique(hi).size > n // 2
    assert (model.positions(hi, lo, cols, r) == 5).all()
    t = wide_table(engine, k, hi, lo, counts)
    got = t.jf_records_wide(r, cols)
    want = model.record_bytes(k, hi, lo, counts, cols, r)[0]
    assert got.tobytes() == want
    ghi, glo, _ = words(got, k)
    assert ((ghi[1:] > ghi[:-1]) | ((ghi[1:] == ghi[:-1]) & (glo[1:] > glo[:-1]))).all()
    assert t.jf_records_wide(r, cols, 5, 6).tobytes() == want and t.jf_records_wide(r, cols, 6, 1 << r).size == 0
    t.free()


def test_skewed_matrix_is_refused(engine, tmp_path):
    """A zero matrix sends the whole table to position 0.  Beyond 2^16 records in one bucket the entry refuses (the ranking path is
    quadratic); the dump of the same table, whose own matrix spreads it, is unaffected."""
    k, r, n = 40, 10, (1 << 16) + 1
    lo = np.arange(n, dtype=U64) * U64(3)
    hi = np.arange(n, dtype=U64) & U64(0xFF)
    counts = np.ones(n, U64)
    t = wide_table(engine, k, hi, lo, counts)
    cols = np.zeros(2 * k, U64)
    assert t.jf_records_wide(r, cols, count_only=True) == n
    with pytest.raises(kat_amd.binding.KatGpuError, match="does not spread") as e:
        t.jf_records_wide(r, cols)
    assert e.value.code == 1
    a, b = str(tmp_path / "a.jf"), str(tmp_path / "b.jf")
    host_file(t, a)
    t.dump_jf(b)
    assert whole(a)[1:] == whole(b)[1:] and len(whole(b)[2]) == n * 14
    t.free()


@pytest.mark.parametrize("k", [33, 63])
def test_counts(engine, tmp_path, k):
    """Counts beyond the slot's own field live in the overflow side table; beyond 32 bits they are written saturated."""
    hi = np.array([1, 2, 3, 0, 1], U64)
    lo = np.array([11, 22, 33, 44, 55], U64)
    counts = np.array([2**32 - 1, 2**32, 2**40, 2**29 + 3, 1], U64)
    t = wide_table(engine, k, hi, lo, counts)
    assert list(map(int, t.get_wide(hi, lo))) == list(map(int, counts))
    b = str(tmp_path / "c.jf")
    t.dump_jf(b)
    hdr, _, body = whole(b)
    ghi, glo, gcnt = words(body, k)
    by_key = {(int(h), int(l)): bytes(c) for h, l, c in zip(ghi, glo, gcnt)}
    assert by_key[(1, 11)] == by_key[(2, 22)] == by_key[(3, 33)] == b"\xff\xff\xff\xff"
    assert by_key[(0, 44)] == (2**29 + 3).to_bytes(4, "little") and by_key[(1, 55)] == (1).to_bytes(4, "little")
    r, cols = model.matrix(hdr)
    assert body == model.record_bytes(k, hi, lo, counts, cols, r)[0]
    t.free()


def test_edges(engine, tmp_path):
    a, b = str(tmp_path / "a.jf"), str(tmp_path / "b.jf")
    # an empty table: the header alone
    t = engine.table(33, True)
    host_file(t, a)
    t.dump_jf(b)
    assert whole(a)[1:] == whole(b)[1:] and whole(b)[2] == b""
    # one record at either end of the key widths
    t.merge_host_wide(np.array([2], U64), np.array([123456789], U64), np.array([7], U64))
    host_file(t, a)
    t.dump_jf(b)
    assert whole(a)[1:] == whole(b)[1:] and len(whole(b)[2]) == 13
    t.free()
    t = wide_table(engine, 63, [1 << 40], [987654321], [7])
    host_file(t, a)
    t.dump_jf(b)
    assert whole(a)[1:] == whole(b)[1:] and len(whole(b)[2]) == 20
    t.free()
    # the all-T 63-mer sits in a slot like any other (its first 63-bit half is not the empty marker), and so does the top key bit alone
    hi, lo, counts = [2**62 - 1, 1 << 61, 5], [2**64 - 1, 0, 2**63], [3, 4, 5]
    t = wide_table(engine, 63, hi, lo, counts)
    host_file(t, a)
    t.dump_jf(b)
    hdr, _, body = whole(b)
    r, cols = model.matrix(hdr)
    assert whole(a)[1:] == whole(b)[1:] and body == model.record_bytes(63, hi, lo, counts, cols, r)[0] and len(body) == 60
    assert t.jf_records_wide(r, cols).tobytes() == body
    t.free()


@pytest.mark.parametrize("k,canonical", [(33, True), (63, False)])
def test_round_trip(engine, ko, dumped, k, canonical):
    """The oracle's Table.from_jf reads one-word keys only, so the oracle's side of the round trip is its WideTable counted from the
    same reads: the table the dump must give back."""
    t, _, _, _, _, b = dumped[(k, canonical)]
    back = engine.load_jf(b)
    assert (back.k, back.canonical) == (k, canonical)
    for x, y in zip(back.dump_sorted(), t.dump_sorted()):
        assert np.array_equal(x, y)
    ot = ko.WideTable(k, canonical).count_bases(reads())
    assert_same_wide(t, ot)
    assert_same_wide(back, ot)
    rk, _, rhi, rlo, rcounts = kat_amd.jf_read_records_wide(b)
    order = np.lexsort((rlo, rhi))
    assert rk == k
    for x, y in zip((rhi[order], rlo[order], rcounts[order]), t.dump_sorted()):
        assert np.array_equal(x, y)
    back.free()
