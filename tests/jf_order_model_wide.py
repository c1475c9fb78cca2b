"""tests/jf_order_model.py for two-word k-mers (33 <= k <= 63): a key is (hi, lo), the upper and lower 64 bits of the 2k-bit word.
The records are ordered by ((M * kmer) & (size - 1), hi, lo) and packed as ceil(2k/8) key bytes -- the 8 of lo, then the low ones
of hi -- + 4 saturated count bytes, little endian.  The header helpers (split, blank_time, matrix) are the narrow model's."""
import numpy as np

from tests.jf_order_model import blank_time, matrix, split  # noqa: F401

U64 = np.uint64


def positions(hi, lo, cols, r):
    """XOR of the columns the key's bits select: bit i of the 2k-bit k-mer selects column c-1-i, bits 64 and up come from hi."""
    hi, lo = np.asarray(hi, U64), np.asarray(lo, U64)
    c = cols.size
    pos = np.zeros(lo.size, U64)
    for i in range(c):
        bit = (lo >> U64(i)) & U64(1) if i < 64 else (hi >> U64(i - 64)) & U64(1)
        pos ^= np.where(bit, cols[c - 1 - i], U64(0)).astype(U64)
    return pos & U64((1 << r) - 1)


def record_bytes(k, hi, lo, counts, cols, r, pos_lo=0, pos_hi=None):
    """(the bytes, and the positions, hi and lo words of the records in file order)."""
    hi, lo, counts = np.asarray(hi, U64), np.asarray(lo, U64), np.asarray(counts, U64)
    pos = positions(hi, lo, cols, r)
    if pos_hi is not None or pos_lo:
        sel = (pos >= U64(pos_lo)) & (pos < U64((1 << r) if pos_hi is None else pos_hi))
        hi, lo, counts, pos = hi[sel], lo[sel], counts[sel], pos[sel]
    order = np.lexsort((lo, hi, pos))
    kb = (2 * k + 7) // 8
    assert 8 < kb <= 16
    out = np.zeros((lo.size, kb + 4), np.uint8)
    out[:, :8] = lo[order].astype("<u8").view(np.uint8).reshape(-1, 8)
    out[:, 8:kb] = hi[order].astype("<u8").view(np.uint8).reshape(-1, 8)[:, :kb - 8]
    out[:, kb:] = np.minimum(counts[order], U64(0xFFFFFFFF)).astype("<u4").view(np.uint8).reshape(-1, 4)
    return out.tobytes(), pos[order], hi[order], lo[order]
