"""katgpu_table_profile_gathered_host: after the exchange a k-mer lives on one rank; every rank looks up the windows whose k-mer it
owns (k_profile_owned), the runs of (window, count) travel to rank 0, which scatters them into the dense per-position array
(k_profile_scatter).  tests/profile_gather_rank.py is one rank; the ranks share one device over /dev/shm.

The expected array owes nothing to the code under test: a Python dictionary of the plan's k-mers (strings), probed window by window
with tests/naive.py's reverse complement -- 0 for a window with a byte outside ACGTacgt and for an absent k-mer, the inserted count
(2^40 for one of them: the side table) otherwise.  Equality is exact.  With KATGPU_TEST_GATHER_BATCH=64 a sequence of ~3000 bases is
some fifty batches: a window lost or doubled at a seam shows in the array, and the timing line's records and wire bytes are the
plan's."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import naive
from tests import profile_gather_rank as pr
from tests.test_gpu_comm import fake_rccl  # noqa: F401  (the RCCL stand-in, built once per module)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
U64 = np.uint64
TIMING = re.compile(r'katgpu_timing (\{"phase": "profile_gathered".*\})')
BASES = set("ACGTacgt")


def _launch(tmp_path, world, k, mode, env_extra):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("KATGPU_COMM_INIT_TIMEOUT_S", "60")
    env.setdefault("KATGPU_COMM_TIMEOUT_S", "20")       # a rank that dies ends the others through the communicator's liveness checks
    env.update(KATGPU_TESTING="1", KATGPU_TIMING="1", KATGPU_COMM_TRANSPORT="shm")
    env.update(env_extra)
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "profile_gather_rank.py"), str(r), str(world), str(tmp_path / "id.bin"), str(tmp_path), str(k), mode],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=120)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        if p.returncode:                                 # one rank failed: the others would wait for it
            for q in procs:
                if q.poll() is None:
                    q.kill()
    if any(p.returncode for p in procs) and any("did not return within" in o and "KATGPU_COMM_INIT_TIMEOUT_S" in o for o in outs):
        pytest.skip("RCCL's bootstrap did not come back on this box: " + next(o for o in outs if "did not return within" in o)[-300:])    # the box's, not the code's
    assert all(p.returncode == 0 for p in procs), "\n----\n".join(o[-3000:] for o in outs)
    return outs


def _expected(seq, k, counts, canonicalise):
    """counts: {k-mer string: count}.  The window's k-mer as it stands, or the smaller of it and its reverse complement (A < C < G < T)."""
    out = np.zeros(max(0, len(seq) - k + 1), U64)
    for i in range(out.size):
        w = seq[i:i + k]
        if BASES.issuperset(w):
            u = w.upper()
            out[i] = counts.get(min(u, naive.revcomp(u)) if canonicalise else u, 0)
    return out


def _check(tmp_path, world, k, canonical, batch, out0):
    S, cases = pr.plans(k, world, canonical)
    lines, slot_bytes, pending = {}, set(), []
    for ln in out0.splitlines():                         # rank 0's output: one profile_gathered line before every "plan" line
        m = TIMING.search(ln)
        if m:
            pending.append(m.group(1))
        m = re.match(r"plan (\d+) (\w+) slot_bytes (\d+)", ln)
        if m:
            assert len(pending) == 1, (ln, pending)
            lines[int(m.group(1))] = json.loads(pending.pop())
            slot_bytes.add(int(m.group(3)))
    assert sorted(lines) == list(range(len(cases))), out0[-3000:]
    saw_big = lopsided_batch = False
    for ci, (name, plan, chosen) in enumerate(cases):
        counts = {}
        for strings, cnt in plan:
            for s, c in zip(strings, cnt.tolist()):
                assert s not in counts                   # (disjoint across ranks: the union is their sum)
                counts[s] = c
        assert set(counts) == set(chosen)
        seq, rc_only = pr.sequence(k, S, chosen, canonical)
        assert 2500 < len(seq) < 4000 and "N" * pr.N_RUN in seq and "\n" in seq and any(c.islower() for c in seq)
        records = seq.split("\n")
        assert any(0 < len(r) < k for r in records) and any(len(r) == k for r in records)
        want = _expected(seq, k, counts, canonical)
        got = np.load(tmp_path / ("case_%02d.npy" % ci))
        assert got.dtype == U64 and got.shape == want.shape, (name, got.shape, want.shape)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (name, bad[:10], got[bad[:10]], want[bad[:10]])
        # the k-mer that is in the sequence as its reverse complement only: a hit in a canonical table, a miss in the other
        at = seq.index("\n" + rc_only + "\n") + 1
        assert rc_only not in counts and naive.revcomp(rc_only) in (counts if chosen else S)
        if chosen:
            assert int(want[at]) == (counts[naive.revcomp(rc_only)] if canonical else 0), (name, want[at])
            saw_big = saw_big or bool((want == U64(pr.BIG)).any())
        # the timing line: the batches, and the records and wire bytes that follow from who owns what
        hits = np.flatnonzero(want)
        own = pr.owner([seq[i:i + k].upper() for i in hits], k, world) if hits.size else np.zeros(0, np.int64)
        t = lines[ci]
        n_batches = -(-want.size // batch)
        assert t == {"phase": "profile_gathered", "batches": n_batches, "ranks": world, "records": int(hits.size), "wire_bytes": 12 * int((own != 0).sum())}, (name, t)
        if batch == 64:
            assert n_batches > 40
            per = np.zeros((n_batches, world), np.int64)
            np.add.at(per, (hits // 64, own), 1)
            lopsided_batch = lopsided_batch or bool(((per == 0).any(axis=1) & (per != 0).any(axis=1)).any()) or (world == 1 and bool((per == 0).any()))
    assert saw_big                                       # a count of 2^40 came back whole
    if batch == 64:
        assert lopsided_batch                            # a batch in which a rank's run was empty (while another's was not, where there is another)
    return cases, slot_bytes


# world, transport, k, mode, batch (window starts; 0: the default, one batch), size hint, the slot bytes it makes (0: whatever)
@pytest.mark.parametrize("world,transport,k,mode,batch,hint,slot", [
    (1, "shm", 27, "plans", 64, 1 << 16, 12), (2, "shm", 5, "plans", 64, 1 << 16, 0), (2, "shm", 27, "plans_nc", 64, 1 << 16, 12),
    (3, "shm", 41, "plans", 64, 1 << 16, 20), (3, "shm", 27, "plans", 64, 1 << 23, 8), (3, "shm", 27, "plans_nc", 64, 1 << 23, 8),
    (8, "shm", 27, "plans", 64, 1 << 16, 12), (3, "shm", 5, "plans", 64, 1 << 16, 0), (2, "shm", 41, "plans", 64, 1 << 16, 20),
    (2, "shm", 27, "plans", 0, 1 << 16, 12), (3, "rccl", 27, "plans", 64, 1 << 16, 12)])
def test_gathered_profile_is_the_dictionarys(tmp_path, fake_rccl, world, transport, k, mode, batch, hint, slot):  # noqa: F811
    """Worlds 1, 2, 3 and 8 (9 processes hold the GPU), k = 5 (all 512 canonical 5-mers), 27 and 41 (wide), canonical and non-canonical
    tables at k = 27, both one-word layouts (8-byte packed slots at a size hint of 2^23, 12-byte ones below), every ownership plan of
    tests/profile_gather_rank.py; batches of 64 window starts, the default once (one batch), and once through the RCCL branch."""
    env = {"KATGPU_COMM_TRANSPORT": transport, "PROFILE_GATHER_SIZE_HINT": str(hint)}
    if batch:
        env["KATGPU_TEST_GATHER_BATCH"] = str(batch)
    if transport == "rccl":
        env["KATGPU_RCCL_LIB"] = fake_rccl
    outs = _launch(tmp_path, world, k, mode, env)
    assert "transport: %s" % transport in outs[0], outs[0][-2000:]
    cases, slot_bytes = _check(tmp_path, world, k, mode == "plans", batch or (32 << 20), outs[0])
    assert {"even", "all_on_rank0", "all_on_last", "nothing"} <= {c[0] for c in cases}
    if world > 2:
        assert "rank1_empty" in {c[0] for c in cases}
    if slot:
        assert slot_bytes == {slot}, slot_bytes


@pytest.mark.parametrize("world,k", [(2, 27), (3, 41)])
def test_shorter_than_k_writes_nothing(tmp_path, world, k):
    """n < k (0, 1, k - 1): every rank returns OK and rank 0's array is untouched (asserted in the rank script)."""
    outs = _launch(tmp_path, world, k, "short", {})
    for r, o in enumerate(outs):
        assert "short ok rank %d" % r in o, o[-2000:]
    assert not any("profile_gathered" in o for o in outs)


@pytest.mark.parametrize("world,k", [(2, 41), (3, 27)])
def test_ranks_that_disagree_on_n_all_get_invalid_arg(tmp_path, world, k):
    """The last rank passes one base fewer: KATGPU_ERR_INVALID_ARG on every rank, nothing written, an all-reduce on the same
    communicator still works (asserted in the rank script) -- and so does the call itself: its array is the dictionary's."""
    outs = _launch(tmp_path, world, k, "mismatch", {"KATGPU_TEST_GATHER_BATCH": "64"})
    for r, o in enumerate(outs):
        assert "mismatch ok rank %d" % r in o, o[-2000:]
    S, cases = pr.plans(k, world, True)
    name, plan, chosen = cases[0]
    counts = {s: c for strings, cnt in plan for s, c in zip(strings, cnt.tolist())}
    seq, _ = pr.sequence(k, S, chosen, True)
    assert np.array_equal(np.load(tmp_path / "after_mismatch.npy"), _expected(seq, k, counts, True))


@pytest.mark.parametrize("world,k,who", [(2, 27, 1), (3, 41, 0)])
def test_no_memory_is_collective(tmp_path, world, k, who):
    """KATGPU_TEST_GATHER_NOMEM: one rank reports that it could not allocate -- every rank returns KATGPU_ERR_NOMEM naming it, and the
    communicator carries an all-reduce afterwards (asserted in the rank script)."""
    outs = _launch(tmp_path, world, k, "nomem", {"KATGPU_TEST_GATHER_NOMEM": str(who)})
    for r, o in enumerate(outs):
        assert "nomem ok rank %d" % r in o, o[-2000:]
    assert not any("profile_gathered" in o for o in outs)
