"""A numpy restatement of what loading a Jellyfish binary/sorted file puts into a table: every record's key (ceil(key_len/8) bytes,
bits above key_len ignored) and count (counter_len bytes), both little endian, added up per key; keys whose sum is zero are absent.
Also a writer of such files for any counter_len, on a header of the project's host writer."""
import re

import numpy as np

import kat_amd
from tests.jf_order_model import split

U64 = np.uint64


def record_bytes(key_len, counter_len):
    return (key_len + 7) // 8 + counter_len


def _mask(bits):
    return U64((1 << min(max(bits, 0), 64)) - 1)


def decode(body, key_len, counter_len):
    """(hi, lo, count) per record, in file order.  key_len <= 126, counter_len 1..8."""
    assert 0 < key_len <= 126 and 1 <= counter_len <= 8
    kb, rb = (key_len + 7) // 8, record_bytes(key_len, counter_len)
    raw = np.frombuffer(bytes(body), np.uint8)
    assert raw.size % rb == 0
    rec = raw.reshape(-1, rb)
    key = np.zeros((rec.shape[0], 16), np.uint8)
    key[:, :kb] = rec[:, :kb]
    words = key.view("<u8")
    cnt = np.zeros((rec.shape[0], 8), np.uint8)
    cnt[:, :counter_len] = rec[:, kb:]
    lo = words[:, 0].astype(U64) & _mask(key_len)
    hi = words[:, 1].astype(U64) & _mask(key_len - 64)
    return hi, lo, cnt.view("<u8")[:, 0].astype(U64)


def combine(hi, lo, count):
    """Equal keys summed (mod 2^64, as 64-bit adds are), zero sums dropped, ascending by (hi, lo)."""
    hi, lo, count = (np.asarray(x, U64) for x in (hi, lo, count))
    order = np.lexsort((lo, hi))
    hi, lo, count = hi[order], lo[order], count[order]
    if not hi.size:
        return hi, lo, count
    first = np.ones(hi.size, bool)
    first[1:] = (hi[1:] != hi[:-1]) | (lo[1:] != lo[:-1])
    starts = np.flatnonzero(first)
    sums = np.add.reduceat(count, starts)
    keep = sums != 0
    return hi[starts][keep], lo[starts][keep], sums[keep]


def load(path):
    """(k, canonical, hi, lo, count): what a table loaded from `path` holds, sorted."""
    hdr, _, body = split(path)
    hi, lo, count = combine(*decode(body, hdr["key_len"], hdr["counter_len"]))
    return hdr["key_len"] // 2, bool(hdr["canonical"]), hi, lo, count


def pack(hi, lo, count, key_len, counter_len):
    """The records' bytes, in the order given; counts are cut to counter_len bytes (the caller saturates if it wants to)."""
    hi, lo, count = (np.asarray(x, U64) for x in (hi, lo, count))
    kb = (key_len + 7) // 8
    out = np.zeros((lo.size, kb + counter_len), np.uint8)
    key = np.zeros((lo.size, 16), np.uint8)
    key[:, :8] = lo.astype("<u8").view(np.uint8).reshape(-1, 8)
    key[:, 8:] = hi.astype("<u8").view(np.uint8).reshape(-1, 8)
    out[:, :kb] = key[:, :kb]
    out[:, kb:] = count.astype("<u8").view(np.uint8).reshape(-1, 8)[:, :counter_len]
    return out.tobytes()


def write(path, k, canonical, hi, lo, count, counter_len):
    """A file of these records, in the order given, with counters of counter_len bytes: the header is the host writer's for the same
    records, with its counter_len and its 9-digit length rewritten."""
    hi, lo, count = (np.asarray(x, U64) for x in (hi, lo, count))
    kat_amd.jf_write_records_wide(path, k, canonical, hi, lo, count)
    _, head, _ = split(path)
    js = head[9:].rstrip(b"\0")
    js, n = re.subn(rb'"counter_len":\d+', b'"counter_len":%d' % counter_len, js)
    assert n == 1
    js += b"\0" * (-(9 + len(js)) % 8)
    with open(path, "wb") as f:
        f.write(b"%09d" % len(js) + js + pack(hi, lo, count, 2 * k, counter_len))
    return path
