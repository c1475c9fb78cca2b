"""Inputs of tests/test_gpu_record_regions.py, and -- run as a program -- one katgpu_table_record_regions_host call on them in a process
of its own, because the library reads KATGPU_TEST_REGIONS_BATCH once, when it is loaded:
    python -m tests.record_regions_case <k> <canonical 0|1> <out.npz>
(the arrays of the two RANGES, and `sections`: how many timed sections the call added to the profile kernel class)

The layout puts runs of the range (2, 0) where the kernels' seams are.  A stretch [a, b) of the genome that is counted twice gives the
windows a .. b - k a count of 2: the run [a, b - k + 1) of the record that holds the whole genome.  That record starts at byte BIG_AT of
the buffer, and the seams are in buffer positions: a lane owns 16 of them, a chunk 4064 (4032 for k > 32)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GENOME = 170_000
BIG_AT = 43                                    # the first record is 40 bases, three bytes of no record follow
RANGES = [(1, 1), (2, 0)]
# runs of (2, 0) in the big record, in buffer positions [from, to): lane seams (0 and 15 mod 16 at either end), across 3 x 4064 and
# 7 x 4032, longer than two chunks, one window; the last runs to the record's end
SEAM_RUNS = [(1600, 1615), (1695, 1712), (1840, 1841), (3 * 4064 - 100, 3 * 4064 + 50), (7 * 4032 - 7, 7 * 4032 + 1), (30_000, 39_000),
             (41_007, 41_008)]
MANY_FROM, MANY_STEP, MANY = 45_000, 100, 1150      # and 1150 short runs, every third of them counted three times


def random_seq(rng, n):
    return rng.choice(np.frombuffer(b"ACGT", np.uint8), n)


def genome(k):
    return random_seq(np.random.default_rng(100 + k), GENOME)


def stretches(k):
    """(a, b, copies): the stretches of the genome that are counted again"""
    out = [(lo - BIG_AT, hi - BIG_AT + k - 1, 1) for lo, hi in SEAM_RUNS]
    out += [(MANY_FROM + MANY_STEP * i, MANY_FROM + MANY_STEP * i + k + i % 25, 2 if i % 3 == 0 else 1) for i in range(MANY)]
    out.append((GENOME - 500, GENOME, 1))
    return out


def counted(k):
    g = genome(k)
    sep = np.frombuffer(b"N", np.uint8)
    parts = [g] + [g[a:b] for a, b, copies in stretches(k) for _ in range(copies)]
    return np.concatenate([x for part in parts for x in (part, sep)])


def records(k):
    """(bases u8, starts, lengths): a read, the whole genome, a record that is one run of (2, 0), reads of 30 .. 300 bases -- some with
    junk, some that touch their neighbour --, records of length 0, k - 1, k, k + 1, three thousand empty records in a row, a contig"""
    rng = np.random.default_rng(2000 + k)
    g = genome(k)
    recs = [g[500:540], g, g[31_000 - BIG_AT:34_000 - BIG_AT]]
    gaps = [0, 3, 0]
    for i in range(600):
        n = int(rng.integers(30, 301))
        s0 = int(rng.integers(0, g.size - n))
        s = g[s0:s0 + n].copy()
        if i % 7 == 0:
            s[rng.integers(0, n, 2)] = rng.choice(np.frombuffer(b"Nn-\n", np.uint8), 2)
        recs.append(s)
        gaps.append(int(rng.integers(0, 4)) if i % 2 else 0)
    for n in (0, k - 1, k, k + 1) * 3:
        recs.append(g[777:777 + n]); gaps.append(int(rng.integers(0, 3)))
    recs += [g[:0]] * 3000
    gaps += [0] * 3000
    recs.append(g[60_000:75_000]); gaps.append(0)
    parts, starts, pos = [], [], 0
    for s, gap in zip(recs, gaps):
        if gap:
            parts.append(rng.choice(np.frombuffer(b"ACGTN", np.uint8), gap)); pos += gap
        starts.append(pos)
        parts.append(s); pos += s.size
    assert starts[1] == BIG_AT
    return np.concatenate(parts), np.array(starts, np.uint64), np.array([s.size for s in recs], np.uint64)


def main(k, canonical, out):
    import kat_amd
    eng = kat_amd.Engine(0)
    t = eng.table(k, canonical).count_bases(counted(k))
    b, st, ln = records(k)
    eng.profile_reset()
    got = t.record_regions(b, st, ln, RANGES)
    np.savez(out, r0=got[0], r1=got[1], sections=np.array(eng.profile()["profile"]["launches"]))
    t.free()
    eng.close()


if __name__ == "__main__":
    main(int(sys.argv[1]), bool(int(sys.argv[2])), sys.argv[3])
