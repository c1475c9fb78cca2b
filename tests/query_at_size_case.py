"""Inputs of tests/test_gpu_query_at_size.py with their expected answers: buffers of tens of millions of bases whose exact per-position
counts, per-record statistics, hits and regions follow from the oracle's and the numpy models' answer on one period, so nothing loops
over the big buffer in Python.  tests/test_query_at_size_model.py shows, at a few periods, that what is built here equals the oracle's
profile and the two models run directly on the whole buffer.

Tiled      P copies of one block of records, each followed by non-base bytes; the period is odd, so the copies meet the 16-base lanes,
           the 64-bit mask words, the 3072 / 4032 / 4064 chunks and the 16384 mask blocks at ever-changing phases.  A window that
           reaches into the separator is invalid, so the counts of one period are the block's profile and k - 1 zeros.
Giant      one record of any length whose content repeats a period G (random bases, a little junk), a second long record and a few
           short ones behind it, all cut from the same periodic stream.  A window's count depends on its content alone: the counts of
           a record are the profile of G + G[:k - 1], read round and round from the record's phase."""
import numpy as np

from tests import record_regions_case as regions_case
from tests import record_regions_model as gm
from tests import record_stats_case as stats_case
from tests import record_stats_model as rm

N = ord("N")
BATCH = 32 << 20                               # bases per batch of the statistics and regions host forms, window starts per batch of profile_host
BATCH_RECS = 1 << 20                           # records per batch of the host forms
MASK_BLOCK = 256 * 64                          # positions per block of k_regions_count / k_regions_emit
SCAN_ROUND = 1024 * MASK_BLOCK                 # positions per round of k_regions_scan
MIN_BASES = 34_000_000                         # a tiled buffer: more than a batch, more than 2048 mask blocks
GIANT_PERIOD = 250_007
GIANT_LENGTH = 17_500_000 + 4321
MANY_RECORDS = BATCH_RECS + 5000
STATS_RANGES = [(1, 1), (2, 0)]


def oracle_table(ko, k, canonical, bases):
    return (ko.WideTable(k, canonical) if k > 32 else ko.Table(k, canonical)).count_bases(bases)


def windows(ln, k):
    ln = np.asarray(ln, np.int64)
    return np.where(ln >= k, ln - (k - 1), 0)


def record_hits(st, ln, k, counts):
    """the windows of every record that are valid and counted, from per-position counts that are 0 where a window is invalid"""
    cs = np.concatenate([[0], np.cumsum(np.asarray(counts) > 0)])
    nb = windows(ln, k)
    s = np.minimum(np.asarray(st, np.int64), len(counts))
    return (cs[np.where(nb > 0, s + nb, s)] - cs[s]).astype(np.uint64)


def batches(st, ln, max_bases=BATCH, max_recs=BATCH_RECS, long_windows=None):
    """[r0, r1) of every batch for_record_batches (kg_host.hpp) cuts: at most max_recs records, and the bases from the first record's
    start to the last one's end at most max_bases; a batch holds at least one record.  long_windows = (k, limit, most): the cut of the
    statistics' host form as well -- the records of more than `limit` windows of a batch have at most `most` windows between them."""
    st, ln = np.asarray(st, np.int64), np.asarray(ln, np.int64)
    ends = st + ln                                                   # (never decreasing: the records are in order and disjoint)
    if long_windows:
        k, limit, most = long_windows
        w = windows(ln, k)
        w = np.where(w > limit, w, 0)
        upto = np.cumsum(w)
    out, r0 = [], 0
    while r0 < st.size:
        r1 = min(int(np.searchsorted(ends, st[r0] + max_bases, "right")), r0 + max_recs)
        if long_windows:
            r1 = min(r1, int(np.searchsorted(upto, upto[r0] - w[r0] + most, "right")))
        r1 = max(r0 + 1, r1)
        out.append((r0, r1))
        r0 = r1
    return out


def buffer_runs(st, found):
    """(first position, position behind the last) in the buffer of every region of one (m, 3) array"""
    s = np.asarray(st, np.int64)[found[:, 0].astype(np.int64)]
    return s + found[:, 1].astype(np.int64), s + found[:, 2].astype(np.int64)


class Tiled:
    def __init__(self, ko, k, canonical, records, counted, ranges):
        self.k, self.canonical, self.ranges, self.counted = k, canonical, ranges, counted
        self.b, self.st, self.ln = records
        prof, _ = ko.profile(oracle_table(ko, k, canonical, counted), self.b.tobytes(), canonical)
        self.prof = prof
        self.stats = rm.record_stats(self.b, self.st, self.ln, k, prof)
        self.hits = record_hits(self.st, self.ln, k, prof)
        self.regions = gm.regions(self.b, self.st, self.ln, k, prof, ranges)
        self.min_sep = 1 if self.b.size % 2 == 0 else 2
        self.set_sep(self.min_sep)

    def set_sep(self, n_sep):
        self.period = self.b.size + n_sep
        assert self.period % 2 == 1 and n_sep >= 1
        self.block = np.concatenate([self.b, np.full(n_sep, N, np.uint8)])
        self.per = np.concatenate([self.prof, np.zeros(self.period - self.prof.size, np.uint64)])

    def copies(self, n_bases):
        return -(-n_bases // self.period)

    def buffer(self, P):
        return np.tile(self.block, P)

    def records(self, P):
        st = (np.arange(P, dtype=np.uint64)[:, None] * np.uint64(self.period) + self.st[None, :]).ravel()
        return st, np.tile(self.ln, P)

    def want_counts(self, P):
        return np.tile(self.per, P)[:P * self.period - self.k + 1]

    def want_stats(self, P):
        return np.tile(self.stats, P)

    def want_hits(self, P):
        return np.tile(self.hits, P)

    def want_regions(self, P):
        out = []
        for found in self.regions:
            r = np.tile(found, (P, 1))
            r[:, 0] += np.repeat(np.arange(P, dtype=np.uint64) * np.uint64(self.st.size), found.shape[0])
            out.append(r)
        return out


def tiled_mix(ko, k):
    """blocks of tests/record_stats_case.py: mix -- reads, contigs, the whole genome"""
    return Tiled(ko, k, True, stats_case.mix(k), stats_case.counted(k), STATS_RANGES)


def first_batch_bases(c):
    """the bases of the first batch of BATCH bases over a Tiled buffer of more than BATCH bases"""
    ends = c.st.astype(np.int64) + c.ln.astype(np.int64)
    copy, off = divmod(BATCH, c.period)
    j = int(np.searchsorted(ends, off, "right"))
    return copy * c.period + int(ends[j - 1]) if j else (copy - 1) * c.period + int(ends[-1])


def crosses_scan_round(c):
    """a run of one of the ranges holds the positions SCAN_ROUND - 1 and SCAN_ROUND of a Tiled buffer that long"""
    off = SCAN_ROUND % c.period
    for found in c.regions:
        lo, hi = buffer_runs(c.st, found)
        if ((lo < off) & (hi > off)).any():
            return True
    return False


def tiled_regions(ko, k):
    """blocks of tests/record_regions_case.py.  The period grows by two separator bytes at a time until a run lies across the end of
    the first round of k_regions_scan and the first host batch ends in the last of its 2048 mask blocks."""
    c = Tiled(ko, k, True, regions_case.records(k), regions_case.counted(k), regions_case.RANGES)
    for extra in range(0, 2000, 2):
        c.set_sep(c.min_sep + extra)
        if crosses_scan_round(c) and first_batch_bases(c) > BATCH - MASK_BLOCK:
            return c
    raise AssertionError("no period puts a run across position %d and the first batch's end into its last mask block" % SCAN_ROUND)


def tiled_reads(ko, k=17):
    """blocks of three thousand reads of 20 .. 40 bases -- a third touch the read before them, some hold junk, some are empty -- over a
    genome of which two fifths is counted twice"""
    rng = np.random.default_rng(3000 + k)
    g = regions_case.random_seq(rng, 60_000)
    sep = np.frombuffer(b"N", np.uint8)
    parts = [g] + [g[a:a + 60] for a in range(0, g.size - 60, 150)]
    counted = np.concatenate([x for part in parts for x in (part, sep)])
    parts, starts, lens, pos = [], [], [], 0
    for i in range(3000):
        n = 0 if i % 50 == 49 else int(rng.integers(20, 41))
        s0 = int(rng.integers(0, g.size - 40))
        s = g[s0:s0 + n].copy()
        if i % 10 == 0:
            s[rng.integers(0, n)] = N
        if i % 3:
            parts.append(rng.choice(np.frombuffer(b"ACGTN", np.uint8), 1)); pos += 1
        starts.append(pos); lens.append(n)
        parts.append(s); pos += n
    return Tiled(ko, k, True, (np.concatenate(parts), np.array(starts, np.uint64), np.array(lens, np.uint64)), counted, STATS_RANGES)


def dense(n=40_000):
    """k = 1: n touching one-base records of A and n of mixed bases -- every position opens and closes a run of the range (1, 0)"""
    rng = np.random.default_rng(7)
    seq = np.concatenate([np.full(n, ord("A"), np.uint8), rng.choice(np.frombuffer(b"ACGT", np.uint8), n, p=[0.1, 0.2, 0.3, 0.4])])
    return seq, np.arange(2 * n, dtype=np.uint64), np.ones(2 * n, np.uint64)


# ---- giant records ----

def record_runs(seq, counts, k, ranges):
    """record_regions_model.regions for one record: (starts, stops) of its runs, per range"""
    nb = seq.size - k + 1 if seq.size >= k else 0
    if not nb:
        return [(np.zeros(0, np.int64), np.zeros(0, np.int64)) for _ in ranges]
    bad = np.concatenate([[0], np.cumsum(~gm._IS_BASE[seq])])
    c = np.where((bad[k:] - bad[:-k]) > 0, np.uint64(0), np.asarray(counts[:nb], np.uint64))
    return [gm.runs(gm.in_range(c, lo, hi)) for lo, hi in ranges]


class Giant:
    """variant: "plain" -- hundreds of short stretches of G counted two or three times and a few long ones: counts from 1 to 6;
    "ties" -- half of G counted twice: most windows count 1 or 2 and the median lies where the two meet;
    "big" -- k = 9, not canonical, with the three 9-mers of record_stats_case.big_keys, whose counts lie beyond 2^32, planted in G."""

    def __init__(self, ko, k, length, variant="plain"):
        self.k, self.variant, self.canonical = k, variant, variant != "big"
        rng = np.random.default_rng(500 + k)
        g = stats_case.random_seq(rng, GIANT_PERIOD, junk=0.0001)
        if variant == "big":
            assert k == 9
            for at in (1000, 77_777, 123_456, 200_001, GIANT_PERIOD - 5):      # (the last one wraps round the period's end)
                word = np.frombuffer(b"ACGTTGCAATG", np.uint8)
                g[np.arange(at, at + word.size) % g.size] = word
        self.g = g
        wrapped = np.concatenate([g, g[:k - 1]])
        short = [(600 * i + 17, 600 * i + 17 + k + i % 25, 2 if i % 3 == 0 else 1) for i in range(400)]
        stretches = {"plain": short + [(100_000, 130_000, 1), (110_000, 120_000, 3), (200_000, 200_700, 2)],
                     "ties": short[:50] + [(0, g.size // 2 + 37, 1)], "big": []}[variant]
        sep = np.frombuffer(b"N", np.uint8)
        parts = [wrapped] + [g[a:b] for a, b, copies in stretches for _ in range(copies)]
        self.counted = np.concatenate([x for part in parts for x in (part, sep)])
        o = oracle_table(ko, k, self.canonical, self.counted)
        self.big = None
        if variant == "big":
            _, keys, counts = stats_case.big_keys(ko)
            for key, c in zip(keys, counts):
                o.add(key, c)
            self.big = (np.array(keys, np.uint64), np.array(counts, np.uint64))
        self.per, _ = ko.profile(o, wrapped.tobytes(), self.canonical)       # per[i]: the count of the window that starts at phase i
        assert self.per.size == g.size
        # (phase, length, bytes of no record before it): the giant, a second long record, short ones -- two touch, one is empty
        layout = [(0, length, 0), (123_457, g.size + g.size // 3, 1), (5000, 150, 2), (70_001, 40, 0), (9, k - 1, 0), (0, 0, 2), (31, k, 0),
                  (249_900, 300, 1)]
        parts, pos = [], 0
        self.phase, st, ln = [], [], []
        for phase, n, gap in layout:
            parts.append(np.full(gap, N, np.uint8)); pos += gap
            st.append(pos); ln.append(n); self.phase.append(phase)
            parts.append(self.stream(phase, n)); pos += n
        self.bases, self.st, self.ln = np.concatenate(parts), np.array(st, np.uint64), np.array(ln, np.uint64)

    def table(self, engine):
        t = engine.table(self.k, self.canonical).count_bases(self.counted)
        if self.big:
            t.merge_host(*self.big)
        return t

    def stream(self, phase, n):
        return np.tile(self.g, (phase + n) // self.g.size + 1)[phase:phase + n]

    def counts_of(self, r):
        nb = int(windows(self.ln[r], self.k))
        return np.tile(self.per, (self.phase[r] + nb) // self.per.size + 1)[self.phase[r]:self.phase[r] + nb]

    def seq_of(self, r):
        return self.bases[int(self.st[r]):int(self.st[r] + self.ln[r])]

    def want_counts(self):
        """per-position counts of the whole buffer, right on the windows inside records (0 elsewhere)"""
        out = np.zeros(self.bases.size - self.k + 1, np.uint64)
        for r in range(self.st.size):
            c = self.counts_of(r)
            out[int(self.st[r]):int(self.st[r]) + c.size] = c
        return out

    def want_stats(self):
        out = np.zeros(self.st.size, rm.DTYPE)
        for r in range(self.st.size):
            out[r] = rm.one_record(self.seq_of(r), self.counts_of(r), self.k)
        return out

    def want_regions(self, ranges):
        out = [[] for _ in ranges]
        for r in range(self.st.size):
            for q, (a, z) in enumerate(record_runs(self.seq_of(r), self.counts_of(r), self.k, ranges)):
                out[q].append(np.stack([np.full(a.size, r, np.uint64), a.astype(np.uint64), z.astype(np.uint64)], axis=1))
        return [np.concatenate(x) for x in out]
