"""tests/jf_load_model.py against the project's host reader (katgpu_jf_read_records_wide), on files of the host writer and on files
the model's own writer made from them with other counter widths.  No device."""
import numpy as np
import pytest

import kat_amd
from tests import jf_load_model as model

U64 = np.uint64
KS = [5, 27, 32, 33, 63]


def records(k, n, seed):
    """n distinct random k-mers (hi, lo) and counts below 2^32."""
    rng = np.random.default_rng(seed)
    n = min(n, 4 ** k)
    if 2 * k <= 20:
        lo = rng.permutation(4 ** k)[:n].astype(U64)
    else:
        lo = np.unique(rng.integers(0, 1 << min(2 * k, 64), size=2 * n, dtype=U64))[:n]
        rng.shuffle(lo)
    hi = rng.integers(0, 1 << (2 * k - 64), size=lo.size, dtype=U64) if k > 32 else np.zeros(lo.size, U64)
    return hi, lo, rng.integers(1, 1 << 32, size=lo.size, dtype=U64)


def read_sorted(path):
    k, canonical, hi, lo, counts = kat_amd.jf_read_records_wide(path)
    order = np.lexsort((lo, hi))
    return k, canonical, hi[order], lo[order], counts[order]


def same(a, b):
    assert a[:2] == b[:2]
    for x, y in zip(a[2:], b[2:]):
        assert x.dtype == y.dtype == U64 and np.array_equal(x, y)


@pytest.mark.parametrize("k", KS)
def test_host_writer_files(tmp_path, k):
    hi, lo, counts = records(k, 3000, k)
    p = str(tmp_path / "a.jf")
    kat_amd.jf_write_records_wide(p, k, k % 2 == 1, hi, lo, counts)
    got = model.load(p)
    same(got, read_sorted(p))
    order = np.lexsort((lo, hi))
    same(got, (k, k % 2 == 1, hi[order], lo[order], counts[order]))


@pytest.mark.parametrize("counter_len", [1, 2, 5, 8])
@pytest.mark.parametrize("k", KS)
def test_rewritten_files(tmp_path, k, counter_len):
    hi, lo, counts = records(k, 1000, 100 + k)
    if counter_len == 8:
        counts = counts << U64(31)
    counts &= U64((1 << (8 * counter_len)) - 1)
    counts[counts == 0] = U64(1)
    p = model.write(str(tmp_path / "b.jf"), k, True, hi, lo, counts, counter_len)
    hdr, head, body = model.split(p)
    assert hdr["counter_len"] == counter_len and hdr["key_len"] == 2 * k and len(head) % 8 == 0
    assert len(body) == lo.size * model.record_bytes(2 * k, counter_len)
    got = model.load(p)
    same(got, read_sorted(p))
    order = np.lexsort((lo, hi))
    same(got, (k, True, hi[order], lo[order], counts[order]))


def test_combine_and_mask():
    # equal keys are summed, a zero count leaves no key, sums are taken modulo 2^64
    hi = np.array([0, 0, 0, 1, 0], U64)
    lo = np.array([7, 9, 7, 7, 3], U64)
    c = np.array([2**40, 5, 2**63, 0, 1], U64)
    h, l, s = model.combine(hi, lo, c)
    assert list(map(int, h)) == [0, 0, 0] and list(map(int, l)) == [3, 7, 9] and list(map(int, s)) == [1, 2**40 + 2**63, 5]
    # bits of the last key byte above key_len are not part of the key: k = 27 (54 bits in 7 bytes), k = 33 (66 bits in 9 bytes)
    for k, kb in ((27, 7), (33, 9)):
        body = bytes([0xFF] * kb) + (3).to_bytes(4, "little")
        h, l, s = model.decode(body, 2 * k, 4)
        assert int(l[0]) == (1 << min(2 * k, 64)) - 1 and int(h[0]) == ((1 << (2 * k - 64)) - 1 if k > 32 else 0) and int(s[0]) == 3
    # pack is decode's inverse
    hi, lo, counts = records(63, 50, 9)
    assert all(np.array_equal(x, y) for x, y in zip(model.decode(model.pack(hi, lo, counts, 126, 5), 126, 5), (hi, lo, counts & U64((1 << 40) - 1))))
