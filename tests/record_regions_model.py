"""katgpu_table_record_regions_* restated in numpy: the maximal runs of window starts whose count lies in a range, per record, from
the bases, the records, k and the per-position counts (oracle.koracle.profile over the same bases); and the text `katgpu sect -E / -F`
prints from them (Sect::printRegions, src/sect.cc:373-424, with its quirks)."""
import numpy as np

_IS_BASE = np.zeros(256, bool)
_IS_BASE[list(b"ACGTacgt")] = True


def as_bytes(bases):
    if isinstance(bases, str):
        bases = bases.encode()
    return np.frombuffer(bases, np.uint8) if isinstance(bases, (bytes, bytearray)) else np.ascontiguousarray(bases, np.uint8)


def windows(length, k):
    return length - k + 1 if length >= k else 0


def in_range(c, lo, hi):
    """the test of printRegions: count >= min and (count <= max or max == 0)"""
    c = np.asarray(c, np.uint64)
    return (c >= np.uint64(lo)) & ((c <= np.uint64(hi)) if hi else np.ones(c.shape, bool))


def runs(flags):
    """(start, stop) of every maximal run of True in a 1-d array: flags[start:stop] all True"""
    edge = np.diff(np.concatenate([[0], np.asarray(flags, np.int8), [0]]))
    return np.nonzero(edge == 1)[0], np.nonzero(edge == -1)[0]


def regions(bases, rec_start, rec_len, k, counts, ranges):
    """One (m, 3) u64 array of (record, start, stop) per range, sorted by (record, start).  counts[i] = the count of the window that
    starts at bases[i] (any value where the window is invalid: those count 0 here); every record is looked at by itself, so a run
    cannot cross from one into the next."""
    b = as_bytes(bases)
    counts = np.asarray(counts, np.uint64)
    bad = np.concatenate([[0], np.cumsum(~_IS_BASE[b])])
    out = [[] for _ in ranges]
    for r, (s, n) in enumerate(zip(rec_start, rec_len)):
        s, nb = int(s), windows(int(n), k)
        if not nb:
            continue
        invalid = (bad[s + k:s + k + nb] - bad[s:s + nb]) > 0
        c = np.where(invalid, np.uint64(0), counts[s:s + nb])
        for q, (lo, hi) in enumerate(ranges):
            a, z = runs(in_range(c, lo, hi))
            if a.size:
                out[q].append(np.stack([np.full(a.size, r, np.uint64), a.astype(np.uint64), z.astype(np.uint64)], axis=1))
    return [np.concatenate(x) if x else np.zeros((0, 3), np.uint64) for x in out]


def render_record(name, seq, intervals, k, lo, hi):
    """The bytes printRegions writes for one record whose runs are `intervals` ((start, stop) pairs in order).  Its quirks: `length:`
    is end - start - 1 in 32 bits with end = stop + k - 1; a run that ends inside the record prints seq[start:stop] and then
    seq[stop + 1:stop + k - 1] -- the base at `stop` is skipped; one that reaches the last window prints seq[start:nb + k - 1]."""
    nb = windows(len(seq), k)
    cov = b"_cov:%d" % lo + (b"-%d" % hi if hi > 0 else b"+")
    out = []
    for i, (start, stop) in enumerate(intervals):
        start, stop = int(start), int(stop)
        end = (stop + k - 1) & 0xFFFFFFFF
        out.append(b">" + name + b"___region:%d_length:%d_pos:%d:%d" % (i + 1, (end - start - 1) & 0xFFFFFFFF, start + 1, end) + cov + b"\n")
        out.append(seq[start:stop] + (seq[nb:end] if stop == nb else seq[stop + 1:end]) + b"\n")
    return b"".join(out)


def render(records, found, k, lo, hi):
    """The whole -non_repetitive.fa / -repetitive.fa of `records` ((name, seq) byte strings) from one range's (m, 3) array."""
    found = np.asarray(found, np.uint64).reshape(-1, 3)
    first = np.searchsorted(found[:, 0], np.arange(len(records) + 1, dtype=np.uint64))
    return b"".join(render_record(name, seq, found[first[r]:first[r + 1], 1:], k, lo, hi) for r, (name, seq) in enumerate(records))
