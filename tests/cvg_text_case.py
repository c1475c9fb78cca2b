"""Inputs of tests/test_gpu_cvg_text.py that it shares, and -- run as a program -- one katgpu_table_record_cvg_text_host call on the
seam case of tests/record_regions_case.py in a process of its own, because the library reads KATGPU_TEST_CVG_BATCH once, when it is
loaded:
    python -m tests.cvg_text_case <k> <out.npz>
(`text` as u8, `off`, and `sections`: how many timed sections the call added to the profile kernel class)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import record_regions_case as case  # noqa: E402

# one to twenty digits: nothing, the ends of one, two and three digits, of 32 bits, a 13-digit number, the ends of 19 and 20 digits
WIDTH_COUNTS = [0, 9, 10, 99, 100, 2 ** 32 - 1, 2 ** 32, 2 ** 40, 10 ** 19 - 1, 10 ** 19]
WIDTH_K = 9


def width_case():
    """(sequence, bases u8, starts, lengths): 18 bases whose ten 9-mers are distinct; window i is to carry WIDTH_COUNTS[i].  Record 0
    is the whole sequence -- the counts side by side --, record 1 + i its first 9 + i bases, whose last window is window i."""
    rng = np.random.default_rng(9)
    while True:
        s = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), WIDTH_K + len(WIDTH_COUNTS) - 1))
        if len({s[i:i + WIDTH_K] for i in range(len(WIDTH_COUNTS))}) == len(WIDTH_COUNTS):
            break
    recs = [s] + [s[:WIDTH_K + i] for i in range(len(WIDTH_COUNTS))]
    starts = np.cumsum([0] + [len(r) + 1 for r in recs[:-1]]).astype(np.uint64)
    return s, np.frombuffer(b"N".join(recs), np.uint8), starts, np.array([len(r) for r in recs], np.uint64)


def main(k, out):
    import kat_amd
    eng = kat_amd.Engine(0)
    t = eng.table(k, True).count_bases(case.counted(k))
    b, st, ln = case.records(k)
    eng.profile_reset()
    text, off = t.record_cvg_text(b, st, ln)
    np.savez(out, text=np.frombuffer(text, np.uint8), off=off, sections=np.array(eng.profile()["profile"]["launches"]))
    t.free()
    eng.close()


if __name__ == "__main__":
    main(int(sys.argv[1]), sys.argv[2])
