"""Inputs of the many-batch tests of katgpu_table_seq_hits_host (tests/test_gpu_filter.py) and katgpu_table_profile_host
(tests/test_gpu_sect.py), and -- run as a program -- one such call on them in a process of its own, because the library reads
KATGPU_TEST_HITS_BATCH / KATGPU_TEST_PROFILE_BATCH once, when it is loaded:
    python -m tests.host_batch_case <hits|profile> <k> <canonical 0|1> <canonicalise 0|1> <bases: 0 = all> <out.npy>
(<out.npy>.sections: how many timed sections the call added to the profile kernel class -- one per batch that has a window)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from kat_amd import synth  # noqa: E402


def counted():
    """what the tables are counted from: reads of a 30 000-base genome"""
    return synth.reads(synth.genome(30000, seed=11), 0, 600, seed=5)


def hits_records(k):
    """(joined bases, starts, lengths, the records as strings): the record set of tests/test_gpu_filter.py, one after the other"""
    from tests.test_gpu_filter import _records
    recs = _records(np.random.default_rng(k), k)
    starts = np.cumsum([0] + [len(s) for s in recs[:-1]]).astype(np.uint64)
    return "".join(recs).encode(), starts, np.array([len(s) for s in recs], np.uint64), recs


def profile_sequence():
    """the 30 000 bases of that genome, about 1 % of them replaced by bytes that are no base"""
    rng = np.random.default_rng(29)
    s = synth.genome(30000, seed=11).copy()
    bad = rng.random(s.size) < 0.01
    s[bad] = rng.choice(np.frombuffer(b"NnRY-\n\x00", np.uint8), int(bad.sum()))
    return s


def main(kind, k, canonical, canonicalise, n_bases, out):
    import kat_amd
    eng = kat_amd.Engine(0)
    t = eng.table(k, canonical).count_bases(counted())
    if kind == "hits":
        b, st, ln, _ = hits_records(k)
        eng.profile_reset()
        res = t.seq_hits(b, st, ln, canonicalise)
    else:
        s = profile_sequence()
        eng.profile_reset()
        res = t.profile(s[:n_bases] if n_bases else s, canonicalise)
    np.save(out, res)
    with open(out + ".sections", "w") as f:
        f.write(str(eng.profile()["profile"]["launches"]))
    t.free()
    eng.close()


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]), bool(int(sys.argv[3])), bool(int(sys.argv[4])), int(sys.argv[5]), sys.argv[6])
