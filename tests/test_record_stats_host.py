"""kat_amd/csrc/host/record_stats_host.hpp -- a record's katgpu_record_stats from its bases and per-position counts, on the host: what
Sect::processSeq does with the device's counts and Cold::processSeqFile with the counts gathered under --gpus -- against
tests/record_stats_model.py.  tests/native/record_stats_host_check.cc is built with -fsanitize=address,undefined and run as a program
of its own on vectors written here: records shorter than k, of exactly k, empty, all N, lowercase, other junk bytes, counts that need
all 64 bits (their sum wraps, as the model's does) and garbage at invalid windows, which must not count."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import record_stats_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64


def _vectors(k, seed):
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"ACGTACGTACGTacgtNnX-\n", np.uint8)
    lengths = [0, 1, k - 1, k, k + 1, 2 * k, 2 * k + 1, 300, 301, 1000] + rng.integers(0, 400, size=30).tolist()
    recs = []
    for i, n in enumerate(lengths):
        if i % 7 == 3:
            seq = np.full(n, ord("N"), np.uint8)
        elif i % 7 == 5:
            seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=n)]         # no invalid window
        else:
            seq = alphabet[rng.integers(0, alphabet.size, size=n)] if i % 2 else np.frombuffer(b"ACGTacgtN", np.uint8)[rng.integers(0, 9, size=n) % (9 if i % 4 else 8)]
        nb = max(0, n - k + 1)
        cnt = rng.integers(0, 6, size=nb, dtype=U64)                                   # many zeros and ties around the median
        if i % 3 == 0:
            cnt = rng.integers(0, 2 ** 64, size=nb, dtype=U64)
        elif i % 3 == 1 and nb:
            cnt[rng.integers(0, nb)] = 2 ** 40
        bad = np.concatenate([[0], np.cumsum(~model._IS_BASE[seq])])
        invalid = (bad[k:] - bad[:-k]) > 0 if nb else np.zeros(0, bool)
        cnt[invalid] = U64(0xDEADBEEFDEADBEEF)                                         # garbage where the window is invalid
        recs.append((seq, cnt, model.one_record(seq, cnt, k)))
    return recs


@pytest.mark.parametrize("k", [5, 27, 41])
def test_host_record_stats_match_the_model_under_sanitizers(tmp_path, k):
    recs = _vectors(k, 20261019 + k)
    assert any(int(st["invalid"]) for _, _, st in recs) and any(int(st["median"]) > 2 ** 32 for _, _, st in recs)
    vec = tmp_path / "vectors.bin"
    with open(vec, "wb") as f:
        f.write(struct.pack("<II", k, len(recs)))
        for seq, cnt, st in recs:
            f.write(struct.pack("<Q", seq.size) + seq.tobytes() + cnt.tobytes())
            f.write(struct.pack("<6Q", *[int(st[name]) for name in ("sum", "median", "non_zero", "invalid", "gc_bases", "n_bases")]))
    exe = str(tmp_path / "record_stats_host_check")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "kat_amd", "csrc", "host"),
                        os.path.join(ROOT, "tests", "native", "record_stats_host_check.cc"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, str(vec)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "record stats host ok: %d records at k = %d" % (len(recs), k) in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
