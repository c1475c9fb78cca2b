"""The -counts.gc text of records on the device: katgpu_record_gc_text_host / _device (kg_gc_text.hpp) against tests/gc_text_model.py fed
with the oracle's per-position G+C counts, exactly -- key widths from one bit to 63 bits across two mask words, strings of every width
side by side, every byte class, records across tile seams and a tile's halo, thousands of records without a window, touching records,
batch boundaries, the device form with too little room, argument errors."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import kat_amd
from tests import gc_text_case as gc_case
from tests import gc_text_model as gm
from tests import record_stats_case as stats_case
from tests.record_text_checks import assert_equal as _assert_equal, device_call as _device_call

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = gc_case.TILE
_WANT = {}


def _seam_case(ko, k):
    """the seam records and the model's text: computed once per k"""
    if k not in _WANT:
        b, st, ln = gc_case.seam_records(k)
        _WANT[k] = (b, st, ln, gm.text(st, ln, k, gm.oracle_gcs(ko, k, b)))
    return _WANT[k]


@pytest.mark.parametrize("k", [1, 2, 5, 17, 27, 31, 32, 33, 51, 63])
def test_key_widths(engine, ko, k):
    b, st, ln = stats_case.mix(k)
    want = gm.text(st, ln, k, gm.oracle_gcs(ko, k, b))
    strings = set(want[0].split())
    assert b"-0.1" in strings and {len(s) for s in strings} >= {3, 4}
    assert len(want[0]) > 3 * int(st.size) + 100_000
    _assert_equal(engine.record_gc_text(k, b, st, ln), want, k)


def test_widths_and_byte_classes(engine, ko):
    k = gc_case.WIDTH_K
    b, st, ln = gc_case.width_case()
    want = gm.text(st, ln, k, gm.oracle_gcs(ko, k, b))
    text = want[0]
    for pair in (b"0.0 0.0", b"0.0 10.0", b"10.0 0.0", b"80.0 90.0", b"90.0 100.0", b"100.0 100.0", b"100.0 90.0", b"100.0 -0.1", b"-0.1 100.0",
                 b"0.0 -0.1", b"-0.1 0.0", b"-0.1 -0.1", b"100.0\n0.0", b"0.0\n100.0", b"-0.1\n100.0", b"100.0\n", b"0.0\n", b"-0.1\n", b"\n0.0\n0.0\n"):
        assert pair in text, pair                                   # every width before and behind every separator
    lines = text.split(b"\n")
    assert lines[0] == b" ".join([b"100.0"] * 5) and lines[1] == b" ".join([b"0.0"] * 5) and lines[2] == b" ".join([b"10.0"] * 16)
    assert all(b"-0.1" not in line and len(line) > 10 for line in lines[3:6])                    # lower case is valid
    junk = lines[12:12 + 3 * len(gc_case.JUNK)]
    for i, line in enumerate(junk):                                 # 16 windows: the first, the ten in the middle or the last invalid
        flags = [s == b"-0.1" for s in line.split(b" ")]
        first, last = {0: (0, 1), 1: (3, 13), 2: (15, 16)}[i % 3]
        assert flags == [first <= j < last for j in range(16)], (i, line)
    tail = lines[-7:-1]                                             # 0, 1, k - 1, k, k + 1 and 0 bases
    assert ln[-6:].tolist() == [0, 1, k - 1, k, k + 1, 0] and tail[:3] == [b"0.0"] * 3 and tail[3] == b"50.0" and tail[4].count(b" ") == 1 and tail[5] == b"0.0"
    _assert_equal(engine.record_gc_text(k, b, st, ln), want)


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
    # the two crafted records: the invalid byte a tile's first, and the last of a tile's k - 1 halo -- the windows that hold it, no other, are invalid
    for r, at in ((-2, 100), (-1, 100 + k - 2)):
        assert (int(s[r]) + at) % TILE == (0 if r == -2 else k - 2) and b[int(s[r]) + at] in b"Nn"
        flags = [x == b"-0.1" for x in want[0][int(want[1][r - 1]):int(want[1][r - 1 + 1]) - 1].split(b" ")]
        assert len(flags) == 300 - k + 1 and flags == [at - k < j <= at for j in range(len(flags))], r
    _assert_equal(engine.record_gc_text(k, b, st, ln), want, k)


@pytest.mark.parametrize("k", [1, 2])
def test_touching_records(engine, ko, k):
    """Records with no byte between them: at k = 1 the last window of a record and the first of the next are neighbouring positions,
    and a newline stands between their strings."""
    rng = np.random.default_rng(5)
    seq = rng.choice(np.frombuffer(b"ACGT", np.uint8), 13000, p=[0.4, 0.3, 0.2, 0.1])
    ln = rng.integers(1, 40, 600).astype(np.uint64)
    ln[100:110] = 1
    st = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.uint64)
    assert int(st[-1] + ln[-1]) <= seq.size
    want = gm.text(st, ln, k, gm.oracle_gcs(ko, k, seq))
    assert want[0].count(b"\n") == 600 and (k == 1 or b"\n0.0\n0.0\n" in want[0])    # (k = 2: the ten records of one base have no window)
    _assert_equal(engine.record_gc_text(k, seq, st, ln), want, k)


def test_batches(ko, tmp_path):
    """Batches of 5000 bases: the genome record, the contig and the run record are longer and batches of their own, the reads make
    many, the 3000 empty records follow a batch's last read.  The offsets count through the whole call."""
    k = 21
    b, st, ln, want = _seam_case(ko, k)
    out = str(tmp_path / "batches.npz")
    e = dict(os.environ)
    e["KATGPU_TEST_GC_BATCH"] = "5000"
    r = subprocess.run([sys.executable, "-m", "tests.gc_text_case", str(k), out], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    assert int(ln.max()) > 5000 and int(z["sections"]) >= 2 * 15       # the hook bites: two timed sections a batch, the reads alone make fifteen batches
    assert z["off"][-1] == len(want[0]) and (np.diff(z["off"].astype(np.int64)) >= 4).all()    # the offsets count through the whole call
    _assert_equal((z["text"].tobytes(), z["off"]), want)


def test_device_form(engine, ko):
    k = 21
    b, st, ln, (wtext, woff) = _seam_case(ko, k)
    w = np.frombuffer(wtext, np.uint8)
    gc_text_device = functools.partial(engine.record_gc_text_device, k)
    for shift in (0, 1, 16):                                        # (the aligned and the byte-wise loader)
        total, out, off = _device_call(engine, gc_text_device, b, st, ln, w.size, shift)
        assert total == w.size and np.array_equal(off, woff), shift
        assert np.array_equal(out[:w.size], w) and (out[w.size:] == 0xAB).all(), shift
    for cap in (1, 7, 100_001, w.size - 1):                         # too little room: the first `cap` bytes, nothing behind them, the true total
        total, out, off = _device_call(engine, gc_text_device, b, st, ln, cap)
        assert total == w.size and np.array_equal(off, woff), cap
        assert np.array_equal(out[:cap], w[:cap]) and (out[cap:] == 0xAB).all(), cap
    total, out, off = _device_call(engine, gc_text_device, b, st, ln, 0)         # size only: the offsets all the same
    assert total == w.size and np.array_equal(off, woff) and (out == 0xAB).all()


def test_argument_errors(engine, ko):
    bases = b"ACGTACGTTGCATGCA"
    k = 9
    gcs = gm.oracle_gcs(ko, k, bases)
    err = kat_amd.binding.KatGpuError
    with pytest.raises(err, match="starts before record 0 ends") as ei:
        engine.record_gc_text(k, bases, [0, 5], [10, 5])             # overlapping
    assert ei.value.code == 1
    with pytest.raises(err, match="starts before record 0 ends") as ei:
        engine.record_gc_text(k, bases, [8, 0], [4, 4])              # decreasing
    assert ei.value.code == 1
    with pytest.raises(err, match="lies beyond the 16 bases") as ei:
        engine.record_gc_text(k, bases, [0, 10], [5, 7])
    assert ei.value.code == 1
    text, off = engine.record_gc_text(k, bases, [], [])
    assert text == b"" and off.dtype == np.uint64 and off.tolist() == [0]
    text, off = engine.record_gc_text(k, b"", [0, 0], [0, 0])
    assert text == b"0.0\n0.0\n" and off.tolist() == [0, 4, 8]
    text, off = engine.record_gc_text(k, bases, [0, 16], [16, 0])    # a record that starts where the bases end
    line = gm.record_text(gcs, k)
    assert gcs.size == 8 and text == line + b"0.0\n" and off.tolist() == [0, len(line), len(line) + 4]
    for bad_k in (0, 64):
        with pytest.raises(err, match="k = %d unsupported" % bad_k) as ei:
            engine.record_gc_text(bad_k, bases, [0], [16])
        assert ei.value.code == 6                                   # KATGPU_ERR_K
    # NULL pointers
    L = engine.L
    b = np.frombuffer(bases, np.uint8)
    st, ln, off = np.array([0], np.uint64), np.array([16], np.uint64), np.zeros(2, np.uint64)
    p, total = C.c_void_p(), C.c_uint64()
    good = [engine.h, k, b.ctypes.data, b.size, st.ctypes.data, ln.ctypes.data, 1, C.byref(p), off.ctypes.data]
    assert L.katgpu_record_gc_text_host(*good) == 0 and off.tolist() == [0, len(line)] and p.value
    L.katgpu_free_host(p)
    for i in (0, 2, 4, 5, 7, 8):
        args = list(good)
        args[i] = None
        assert L.katgpu_record_gc_text_host(*args) == 1, i
    p = C.c_void_p()
    assert L.katgpu_record_gc_text_host(engine.h, k, None, 0, None, None, 0, C.byref(p), off.ctypes.data) == 0 and p.value and off[0] == 0
    L.katgpu_free_host(p)
    d_off = engine.alloc(16)
    d_off.upload(np.full(2, 7, np.uint64))
    dev = [engine.h, k, None, 0, None, None, 0, None, 0, d_off.ptr, C.byref(total)]
    assert L.katgpu_record_gc_text_device(*dev) == 0 and total.value == 0
    assert d_off.download(np.uint64, 2).tolist() == [0, 7]
    for i, v in ((0, None), (9, None), (10, None), (3, 16), (6, 1), (8, 4)):   # no context, offsets or total; bases, records or text wanted and NULL
        args = list(dev)
        args[i] = v
        assert L.katgpu_record_gc_text_device(*args) == 1, i
    for bad_k in (0, 64):
        args = list(dev)
        args[1] = bad_k
        assert L.katgpu_record_gc_text_device(*args) == 6, bad_k
    d_off.free()
