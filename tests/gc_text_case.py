"""Inputs of tests/test_gpu_gc_text.py that it shares, and -- run as a program -- one katgpu_record_gc_text_host call on the seam case
in a process of its own, because the library reads KATGPU_TEST_GC_BATCH once, when it is loaded:
    python -m tests.gc_text_case <k> <out.npz>
(`text` as u8, `off`, and `sections`: how many timed sections the call added to the profile kernel class)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import record_regions_case as case  # noqa: E402

TILE = 4096                                                         # positions per tile of the text kernels
WIDTH_K = 10
JUNK = [b"N", b"n", b"R", b"U", b"-", b"*", b" ", b"\n", b"\x00", b"\x80", b"\xff"]


def _lay(recs, gaps):
    """(bases u8, starts, lengths): the records one after another, gaps[i] bytes of no record in front of record i"""
    parts, starts, pos = [], [], 0
    for s, gap in zip(recs, gaps):
        parts.append(b"A" * gap); pos += gap
        starts.append(pos)
        parts.append(s); pos += len(s)
    return np.frombuffer(b"".join(parts), np.uint8), np.array(starts, np.uint64), np.array([len(s) for s in recs], np.uint64)


def width_case():
    """(bases u8, starts, lengths) at k = WIDTH_K = 10: strings of every width side by side -- "0.0", "10.0" / "90.0" / "-0.1",
    "100.0" --, every byte class at the first, a middle and the last position of a record, lower case, records of 0, 1, k - 1, k and
    k + 1 bases; every third record has a byte of no record in front of it, the others touch."""
    k = WIDTH_K
    rng = np.random.default_rng(10)
    recs = [b"GCGCCGGCGCGCCG", b"ATTATATAATTTAA", b"AAAAAAAAAG" * 2 + b"AAAAA", b"acgtacgtttgacca", b"AcGtaCgTTgacCAgt", b"ggccggccgcgc",
            b"A" * 11 + b"G" * 12 + b"A" * 11,                     # 0.0 0.0 10.0 ... 90.0 100.0 100.0 100.0 90.0 ... 10.0 0.0 0.0
            b"G" * 11 + b"N" + b"G" * 11, b"A" * 11 + b"N" + b"A" * 11, b"G" * 10 + b"N", b"C" * 10, b"T" * 10]
    for junk in JUNK:
        for at in (0, 12, 24):                                      # first, middle, last of 25
            s = bytearray(rng.choice(np.frombuffer(b"ACGTacgt", np.uint8), 25).tobytes())
            s[at:at + 1] = junk
            recs.append(bytes(s))
    recs += [b"", b"G", b"ACGTACGTA", b"ACGTACGTAC", b"ACGTACGTACG", b""]
    return _lay(recs, [1 if i % 3 == 2 else 0 for i in range(len(recs))])


def seam_records(k):
    """(bases u8, starts, lengths): the records of tests/record_regions_case.py, and behind them two records of 300 bases across a
    tile's end: one whose only invalid byte is the first byte of a tile, one whose only invalid byte is the last byte of a tile's
    k - 1 halo (the bytes behind the tile that its last windows reach into)"""
    b, st, ln = case.records(k)
    rng = np.random.default_rng(3000 + k)
    t0 = (b.size // TILE + 2) * TILE                                # a tile's first byte, beyond the case
    pad = case.random_seq(rng, t0 + 2 * TILE + 400 - b.size)
    ext = np.concatenate([b, pad])
    ext[t0] = ord("N")
    ext[t0 + TILE + k - 2] = ord("n")
    st = np.concatenate([st, [t0 - 100, t0 + TILE - 100]]).astype(np.uint64)
    ln = np.concatenate([ln, [300, 300]]).astype(np.uint64)
    return ext, st, ln


def main(k, out):
    import kat_amd
    eng = kat_amd.Engine(0)
    b, st, ln = seam_records(k)
    eng.profile_reset()
    text, off = eng.record_gc_text(k, b, st, ln)
    np.savez(out, text=np.frombuffer(text, np.uint8), off=off, sections=np.array(eng.profile()["profile"]["launches"]))
    eng.close()


if __name__ == "__main__":
    main(int(sys.argv[1]), sys.argv[2])
