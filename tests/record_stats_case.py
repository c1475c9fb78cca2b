"""Inputs of tests/test_gpu_record_stats.py, and -- run as a program -- one katgpu_table_record_stats_host call on them in a process of
its own, because the library reads KATGPU_TEST_STATS_SHORT / KATGPU_TEST_STATS_BATCH once, when it is loaded:
    python -m tests.record_stats_case <mix|reads|big> <k> <canonical 0|1> <out.npy>
(<out.npy>.sections: how many timed sections the call added to the profile kernel class)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BIG = (1 << 33) + 5


def random_seq(rng, n, junk=0.01):
    s = rng.choice(np.frombuffer(b"ACGTacgt", np.uint8), n)
    bad = rng.random(n) < junk
    s[bad] = rng.choice(np.frombuffer(b"NnRY-\n\x00", np.uint8), int(bad.sum()))
    return s


def genome(k):
    return random_seq(np.random.default_rng(k), 200_000)


def counted(k):
    """what the tables are counted from: the genome and stretches of it again, so that coverage runs from 1 to 9 along a record"""
    g = genome(k)
    sep = np.frombuffer(b"N", np.uint8)
    parts = [g, g[:100_000], g[:50_000]] + [g[20_000:30_000]] * 5 + [g[150_000:150_700]] * 2
    return np.concatenate([x for part in parts for x in (part, sep)])


def mix(k, contigs=True, empties=0):
    """(bases u8, starts, lengths): thousands of 30..300-base reads cut from the genome, shuffled ones, contigs of 5 k, 70 k and the
    whole genome, records of length 0, k - 1, k and k + 1, in random order; between two records nothing (adjacent), or a few bytes
    that belong to no record."""
    rng = np.random.default_rng(1000 + k)
    g = genome(k)
    recs = []
    for _ in range(2500):
        n = int(rng.integers(30, 301))
        s0 = int(rng.integers(0, g.size - n))
        recs.append(g[s0:s0 + n])
    for _ in range(250):
        recs.append(random_seq(rng, int(rng.integers(30, 301)), 0.0))
    for n in (0, k - 1, k, k + 1) * 3:
        recs.append(g[777:777 + n])
    if contigs:
        recs += [g[1000:6000], g[100_000:170_000], g]
    order = rng.permutation(len(recs))
    recs = [recs[i] for i in order] + [g[:0]] * empties
    parts, starts, pos = [], [], 0
    for s in recs:
        gap = int(rng.integers(0, 4)) if rng.random() < 0.5 else 0
        if gap:
            parts.append(rng.choice(np.frombuffer(b"ACGTN", np.uint8), gap)); pos += gap
        starts.append(pos)
        parts.append(s); pos += s.size
    return np.concatenate(parts), np.array(starts, np.uint64), np.array([s.size for s in recs], np.uint64)


def big_keys(ko):
    """k = 9, not canonical: three overlapping 9-mers of one 11-base string, counts beyond 32 bits"""
    s = "ACGTTGCAATG"
    return s, [ko.encode(s[i:i + 9]) for i in range(3)], [BIG, (1 << 34) + 1, (1 << 32) + 7]


def big_records():
    """over `big_keys`: the 2^33 + 5 k-mer as the median of three windows; a record whose two counts are both beyond 2^32; the first
    k-mer alone; one with a window that is not in the table"""
    s = b"ACGTTGCAATG"
    recs = [s, s[1:], s[:9], b"T" + s[:10]]
    joined = b"N".join(recs)
    starts = np.cumsum([0] + [len(r) + 1 for r in recs[:-1]]).astype(np.uint64)
    return np.frombuffer(joined, np.uint8), starts, np.array([len(r) for r in recs], np.uint64)


def main(kind, k, canonical, out):
    import kat_amd
    from oracle import koracle as ko
    eng = kat_amd.Engine(0)
    if kind == "big":
        t = eng.table(9, False)
        _, keys, counts = big_keys(ko)
        t.merge_host(np.array(keys, np.uint64), np.array(counts, np.uint64))
        b, st, ln = big_records()
    else:
        t = eng.table(k, canonical).count_bases(counted(k))
        b, st, ln = mix(k, contigs=kind == "mix", empties=5000 if kind == "mix" else 0)
    eng.profile_reset()
    np.save(out, t.record_stats(b, st, ln))
    with open(out + ".sections", "w") as f:                        # timed sections of the profile class: one per batch, one more where a batch has long records
        f.write(str(eng.profile()["profile"]["launches"]))
    t.free()
    eng.close()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), bool(int(sys.argv[3])), sys.argv[4])
