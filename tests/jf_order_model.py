"""A numpy restatement of what a Jellyfish binary/sorted file holds after its header: the records ordered by
((M * kmer) & (size - 1), kmer) and packed as ceil(2k/8) key bytes + 4 saturated count bytes, little endian.
M, r and size are read back from the header, so the model knows nothing of how the writer made them."""
import json
import re

import numpy as np

U64 = np.uint64


def split(path):
    """(header dict, header bytes incl. the 9 digits and the padding, record bytes)."""
    raw = open(path, "rb").read()
    hlen = int(raw[:9])
    js = raw[9:9 + hlen].rstrip(b"\0")
    return json.loads(js), raw[:9 + hlen], raw[9 + hlen:]


def blank_time(header_bytes):
    out, n = re.subn(rb'"time":"[^"]*"', b'"time":""', header_bytes)
    assert n == 1
    return out


def matrix(hdr):
    m = hdr["matrix1"]
    assert m["c"] == hdr["key_len"] and len(m["columns"]) == m["c"] and hdr["size"] == 1 << m["r"]
    return m["r"], np.array(m["columns"], U64)


def positions(keys, cols, r):
    """XOR of the columns the key's bits select: bit i of the k-mer selects column c-1-i."""
    keys = np.asarray(keys, U64)
    c = cols.size
    pos = np.zeros(keys.size, U64)
    for i in range(min(c, 64)):
        pos ^= np.where((keys >> U64(i)) & U64(1), cols[c - 1 - i], U64(0)).astype(U64)
    return pos & U64((1 << r) - 1)


def record_bytes(k, keys, counts, cols, r, pos_lo=0, pos_hi=None):
    keys, counts = np.asarray(keys, U64), np.asarray(counts, U64)
    pos = positions(keys, cols, r)
    if pos_hi is not None or pos_lo:
        sel = (pos >= U64(pos_lo)) & (pos < U64((1 << r) if pos_hi is None else pos_hi))
        keys, counts, pos = keys[sel], counts[sel], pos[sel]
    order = np.lexsort((keys, pos))
    kb = (2 * k + 7) // 8
    out = np.zeros((keys.size, kb + 4), np.uint8)
    out[:, :kb] = keys[order].astype("<u8").view(np.uint8).reshape(-1, 8)[:, :kb]
    out[:, kb:] = np.minimum(counts[order], U64(0xFFFFFFFF)).astype("<u4").view(np.uint8).reshape(-1, 4)
    return out.tobytes(), pos[order]
