"""The -counts.cvg text of records on the device: katgpu_table_record_cvg_text_host / _device (kg_cvg_text.hpp) against
tests/cvg_text_model.py, exactly -- key widths and layouts, counts of one to twenty digits, records across tile and chunk seams,
thousands of records without a window, touching records, batch boundaries, the device form with too little room, argument errors."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import kat_amd
from tests import cvg_text_case as cvg_case
from tests import cvg_text_model as cm
from tests import record_regions_case as case
from tests import record_stats_case as stats_case
from tests.record_text_checks import assert_equal as _assert_equal, device_call as _device_call

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 4096                                                         # positions per tile of the text kernels
_WANT = {}


def _oracle(ko, k, canonical, bases):
    return (ko.WideTable(k, canonical) if k > 32 else ko.Table(k, canonical)).count_bases(bases)


def _seam_case(ko, k):
    """the records of tests/record_regions_case.py, their counts and the model's text: computed once per k"""
    if k not in _WANT:
        b, st, ln = case.records(k)
        counts, _ = ko.profile(_oracle(ko, k, True, case.counted(k)), b.tobytes(), True)
        _WANT[k] = (b, st, ln, cm.text(st, ln, k, counts))
    return _WANT[k]


@pytest.mark.parametrize("k,canonical", [(5, True), (5, False), (17, True), (17, False), (27, True), (27, False), (32, True), (32, False),
                                         (33, True), (33, False), (51, True), (51, False), (63, True), (63, False)])
def test_key_widths_and_flags(engine, ko, k, canonical):
    b, st, ln = stats_case.mix(k)
    t = engine.table(k, canonical).count_bases(stats_case.counted(k))
    if k in (17, 27):
        assert t.slot_bytes() == (8 if k == 17 else 12)             # both layouts of a one-word table
    o = _oracle(ko, k, canonical, stats_case.counted(k))
    for canonicalise in (canonical, not canonical):
        counts, _ = ko.profile(o, b.tobytes(), canonicalise)
        want = cm.text(st, ln, k, counts)
        if k == 5:
            assert int(counts.max()) >= 100                        # three digits
        assert len(want[0]) > 2 * int(st.size) + 100_000
        _assert_equal(t.record_cvg_text(b, st, ln, canonicalise), want, (k, canonicalise))
    t.free()


def test_digit_widths(engine, ko):
    k = cvg_case.WIDTH_K
    s, b, st, ln = cvg_case.width_case()
    keys = [ko.encode(s[i:i + k].decode()) for i, c in enumerate(cvg_case.WIDTH_COUNTS) if c]
    amounts = [c for c in cvg_case.WIDTH_COUNTS if c]
    o = ko.Table(k, False)
    for key, c in zip(keys, amounts):
        o.add(key, c)
    counts, _ = ko.profile(o, b.tobytes(), False)
    assert counts[:len(cvg_case.WIDTH_COUNTS)].tolist() == cvg_case.WIDTH_COUNTS
    want = cm.text(st, ln, k, counts)
    lines = want[0].split(b"\n")
    assert lines[0] == b" ".join(b"%d" % c for c in cvg_case.WIDTH_COUNTS)                  # side by side
    assert [line.split(b" ")[-1] for line in lines[1:-1]] == [b"%d" % c for c in cvg_case.WIDTH_COUNTS]   # each before a newline
    numbers = set(want[0].split())
    assert any(len(x) == 20 for x in numbers) and any(len(x) == 13 for x in numbers)
    assert {len(x) for x in numbers} >= {1, 2, 3, 10, 13, 19, 20}
    t = engine.table(k, False)
    t.merge_host(np.array(keys, np.uint64), np.array(amounts, np.uint64))
    _assert_equal(t.record_cvg_text(b, st, ln, False), want)
    t.free()


@pytest.mark.parametrize("k", [21, 45])
def test_seams(engine, ko, k):
    b, st, ln, want = _seam_case(ko, k)
    chunk = 4064 if k <= 32 else 4032
    s, n = st.astype(np.int64), ln.astype(np.int64)
    nb = np.where(n >= k, n - (k - 1), 0)
    has = n > 0
    assert ((s[has] // chunk) != ((s[has] + n[has] - 1) // chunk)).any() and (n > 2 * chunk).any()   # across a chunk's end; longer than two chunks
    assert int(np.max(np.diff(np.nonzero(n)[0]))) > 3000 and (n == 0).sum() >= 3000             # over 3000 empty records in a row
    assert ((n > 0) & (n < k)).sum() >= 3 and (n == k).sum() >= 3                               # 0 < len < k; exactly k bases: one window
    win = nb > 0
    assert ((s[win] // TILE) != ((s[win] + nb[win] - 1) // TILE)).any()                          # a text that starts in one tile and ends in a later one
    assert (nb > 2 * TILE).any()                                                                # ... and one over more than two tiles
    assert want[1][-1] == len(want[0]) > 500_000
    t = engine.table(k, True).count_bases(case.counted(k))
    _assert_equal(t.record_cvg_text(b, st, ln), want, k)
    t.free()


@pytest.mark.parametrize("k", [1, 2])
def test_touching_records(engine, ko, k):
    """Records with no byte between them (the case of tests/test_gpu_record_regions.py): at k = 1 the last window of a record and the
    first of the next are neighbouring positions, and a newline stands between their counts."""
    rng = np.random.default_rng(5)
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), 13000, p=[0.4, 0.3, 0.2, 0.1])
    ln = rng.integers(1, 40, 600).astype(np.uint64)
    ln[100:110] = 1
    st = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64)
    assert int(st[-1] + ln[-1]) <= seq.size
    t = engine.table(k, False).count_bases(seq)
    counts, _ = ko.profile(_oracle(ko, k, False, seq), seq.tobytes(), False)
    want = cm.text(st, ln, k, counts)
    assert want[0].count(b"\n") == 600 and (b"\n0\n" in want[0]) == (k == 2)
    _assert_equal(t.record_cvg_text(seq, st, ln, False), want, k)
    t.free()


def test_batches(ko, tmp_path):
    """Batches of 5000 bases: the genome record, the contig and the run record are longer and batches of their own, the reads make
    many, the 3000 empty records follow a batch's last read.  The offsets count through the whole call."""
    k = 21
    b, st, ln, want = _seam_case(ko, k)
    out = str(tmp_path / "batches.npz")
    e = dict(os.environ)
    e["KATGPU_TEST_CVG_BATCH"] = "5000"
    r = subprocess.run([sys.executable, "-m", "tests.cvg_text_case", str(k), out], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    assert int(ln.max()) > 5000 and int(z["sections"]) >= 2 * 15       # the hook bites: the reads alone make fifteen batches
    _assert_equal((z["text"].tobytes(), z["off"]), want)


def test_device_form(engine, ko):
    k = 21
    b, st, ln, (wtext, woff) = _seam_case(ko, k)
    w = np.frombuffer(wtext, np.uint8)
    t = engine.table(k, True).count_bases(case.counted(k))
    _assert_equal(t.record_cvg_text(b, st, ln), (wtext, woff))
    for shift in (0, 1, 16):                                        # (the aligned and the byte-wise loader of the lookups)
        total, out, off = _device_call(engine, t.record_cvg_text_device, b, st, ln, w.size, shift)
        assert total == w.size and np.array_equal(off, woff), shift
        assert np.array_equal(out[:w.size], w) and (out[w.size:] == 0xAB).all(), shift
    for cap in (1, 7, 100_001, w.size - 1):                         # too little room: the first `cap` bytes, nothing behind them, the true total
        total, out, off = _device_call(engine, t.record_cvg_text_device, b, st, ln, cap)
        assert total == w.size and np.array_equal(off, woff), cap
        assert np.array_equal(out[:cap], w[:cap]) and (out[cap:] == 0xAB).all(), cap
    total, out, off = _device_call(engine, t.record_cvg_text_device, b, st, ln, 0)         # size only: the offsets all the same
    assert total == w.size and np.array_equal(off, woff) and (out == 0xAB).all()
    t.free()


def test_argument_errors(engine, ko):
    bases = b"ACGTACGTTGCATGCA"
    t = engine.table(9, True).count_bases(np.frombuffer(bases, np.uint8))
    counts, _ = ko.profile(ko.Table(9, True).count_bases(bases), bases, True)
    err = kat_amd.binding.KatGpuError
    with pytest.raises(err, match="starts before record 0 ends") as ei:
        t.record_cvg_text(bases, [0, 5], [10, 5])                   # overlapping
    assert ei.value.code == 1
    with pytest.raises(err, match="starts before record 0 ends") as ei:
        t.record_cvg_text(bases, [8, 0], [4, 4])                    # decreasing
    assert ei.value.code == 1
    with pytest.raises(err, match="lies beyond the 16 bases") as ei:
        t.record_cvg_text(bases, [0, 10], [5, 7])
    assert ei.value.code == 1
    text, off = t.record_cvg_text(bases, [], [])
    assert text == b"" and off.dtype == np.uint64 and off.tolist() == [0]
    text, off = t.record_cvg_text(b"", [0, 0], [0, 0])
    assert text == b"0\n0\n" and off.tolist() == [0, 2, 4]
    text, off = t.record_cvg_text(bases, [0, 16], [16, 0])          # a record that starts where the bases end
    assert text == cm.record_text(counts) + b"0\n" and off.tolist() == [0, 16, 18] and counts.size == 8
    # NULL pointers
    L = engine.L
    b = np.frombuffer(bases, np.uint8)
    st, ln, off = np.array([0], np.uint64), np.array([16], np.uint64), np.zeros(2, np.uint64)
    p, total = C.c_void_p(), C.c_uint64()
    good = [t.h, b.ctypes.data, b.size, st.ctypes.data, ln.ctypes.data, 1, 1, C.byref(p), off.ctypes.data]
    assert L.katgpu_table_record_cvg_text_host(*good) == 0 and off.tolist() == [0, 16] and p.value
    L.katgpu_free_host(p)
    for i in (0, 1, 3, 4, 7, 8):
        args = list(good)
        args[i] = None
        assert L.katgpu_table_record_cvg_text_host(*args) == 1, i
    p = C.c_void_p()
    assert L.katgpu_table_record_cvg_text_host(t.h, None, 0, None, None, 0, 1, C.byref(p), off.ctypes.data) == 0 and p.value and off[0] == 0
    L.katgpu_free_host(p)
    d_off = engine.alloc(16)
    d_off.upload(np.full(2, 7, np.uint64))
    dev = [t.h, None, 0, None, None, 0, 1, None, 0, d_off.ptr, C.byref(total)]
    assert L.katgpu_table_record_cvg_text_device(*dev) == 0 and total.value == 0
    assert d_off.download(np.uint64, 2).tolist() == [0, 7]
    for i, v in ((0, None), (9, None), (10, None), (2, 16), (5, 1), (8, 4)):
        args = list(dev)
        args[i] = v
        assert L.katgpu_table_record_cvg_text_device(*args) == 1, i
    d_off.free()
    t.free()
