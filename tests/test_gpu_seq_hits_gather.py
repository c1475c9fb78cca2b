"""katgpu_table_seq_hits_gathered_host: after the exchange a k-mer lives on one rank; every rank counts, per record, the hits among the
windows whose k-mer it owns (k_seq_hits_owned), the other ranks' 8 bytes per record travel to rank 0, which adds them to its own
(k_hits_sum).  tests/seq_hits_gather_rank.py is one rank; the ranks share one device over /dev/shm.

The expected array owes nothing to the code under test: a Python dictionary of the plan's k-mers (strings); hits[r] is the number of
windows inside record r that are all ACGTacgt and whose k-mer (for canonical tables: the smaller of it and its reverse complement) is
in the dictionary.  Equality is exact.  With KATGPU_TEST_HITS_BATCH=256 a sequence of ~3000 bases is more than ten batches, and a
record longer than 256 bases is a batch of its own; the timing line's batches, records and wire bytes are the plan's."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import naive
from tests import profile_gather_rank as pr
from tests import seq_hits_gather_rank as hr
from tests.test_gpu_comm import fake_rccl  # noqa: F401  (the RCCL stand-in, built once per module)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
U64 = np.uint64
TIMING = re.compile(r'katgpu_timing (\{"phase": "seq_hits_gathered".*\})')
BASES = set("ACGTacgt")
DEFAULT_BATCH, DEFAULT_RECS = 64 << 20, 1 << 20


def _launch(tmp_path, world, k, mode, env_extra):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("KATGPU_COMM_INIT_TIMEOUT_S", "60")
    env.setdefault("KATGPU_COMM_TIMEOUT_S", "20")       # a rank that dies ends the others through the communicator's liveness checks
    env.update(KATGPU_TESTING="1", KATGPU_TIMING="1", KATGPU_COMM_TRANSPORT="shm")
    env.update(env_extra)
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "seq_hits_gather_rank.py"), str(r), str(world), str(tmp_path / "id.bin"), str(tmp_path), str(k), mode],
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


def _expected(bases, starts, lens, k, counts, canonicalise):
    """counts: {k-mer string: count}.  Per record, the windows inside it whose k-mer -- as it stands, or the smaller of it and its
    reverse complement (A < C < G < T) -- the dictionary holds."""
    out = np.zeros(len(starts), U64)
    for r, (s, n) in enumerate(zip(starts.tolist(), lens.tolist())):
        rec = bases[s:s + n]
        for i in range(len(rec) - k + 1):
            w = rec[i:i + k]
            if BASES.issuperset(w):
                u = w.upper()
                out[r] += (min(u, naive.revcomp(u)) if canonicalise else u) in counts
    return out


def _n_batches(starts, lens, max_bases, max_recs):
    """The cut of for_record_batches (kg_host.hpp): a batch takes records while it stays within both limits; its first record always joins."""
    st, ln = starts.tolist(), lens.tolist()
    n, r0 = 0, 0
    while r0 < len(st):
        r1 = r0 + 1
        while r1 < len(st) and r1 - r0 < max_recs and st[r1] + ln[r1] - st[r0] <= max_bases:
            r1 += 1
        n, r0 = n + 1, r1
    return n


def _counts_of(plan):
    counts = {}
    for strings, cnt in plan:
        for s, c in zip(strings, cnt.tolist()):
            assert s not in counts                       # (disjoint across ranks: the union is their sum)
            counts[s] = c
    return counts


def _check(tmp_path, world, k, canonical, max_bases, max_recs, out0):
    S, cases = pr.plans(k, world, canonical)
    lines, slot_bytes, pending = {}, set(), []
    for ln in out0.splitlines():                         # rank 0's output: one seq_hits_gathered line before every "plan" line
        m = TIMING.search(ln)
        if m:
            pending.append(m.group(1))
        m = re.match(r"plan (\d+) (\w+) slot_bytes (\d+)", ln)
        if m:
            assert len(pending) == 1, (ln, pending)
            lines[int(m.group(1))] = json.loads(pending.pop())
            slot_bytes.add(int(m.group(3)))
    assert sorted(lines) == list(range(len(cases))), out0[-3000:]
    saw_big = False
    for ci, (name, plan, chosen) in enumerate(cases):
        counts = _counts_of(plan)
        assert set(counts) == set(chosen)
        seq, rc_only = pr.sequence(k, S, chosen, canonical)
        starts, lens = hr.records(seq)
        assert 2500 < len(seq) < 4000 and starts.size == seq.count("\n") + 1 and (lens == k).any() and ((lens > 0) & (lens < k)).any()
        want = _expected(seq, starts, lens, k, counts, canonical)
        got = np.load(tmp_path / ("case_%02d.npy" % ci))
        assert got.dtype == U64 and got.shape == want.shape, (name, got.shape, want.shape)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (name, bad[:10], got[bad[:10]], want[bad[:10]])
        assert (got[lens < k] == 0).all() and (got[lens == k] <= 1).all()
        if not chosen:
            assert not got.any()
        # the k-mer that is in the sequence as its reverse complement only, a record of its own: a hit in a canonical table, a miss in the other
        at = seq.index("\n" + rc_only + "\n") + 1
        r = int(np.flatnonzero(starts == at)[0])
        assert int(lens[r]) == k and rc_only not in counts and naive.revcomp(rc_only) in (counts if chosen else S)
        if chosen:
            assert int(got[r]) == (1 if canonical else 0), (name, got[r])
            # the k-mer counted 2^40 times (its count lies in the side table) is a hit: without it the dictionary finds fewer
            big = [s for s, c in counts.items() if c == pr.BIG]
            assert len(big) == 1
            less = _expected(seq, starts, lens, k, {s: c for s, c in counts.items() if s != big[0]}, canonical)
            saw_big = saw_big or bool((less < want).any())
        # the timing line: the batches cut from the records, 8 bytes per record and rank other than 0
        n_batches = _n_batches(starts, lens, max_bases, max_recs)
        t = lines[ci]
        assert t == {"phase": "seq_hits_gathered", "batches": n_batches, "ranks": world, "records": int(starts.size), "wire_bytes": 8 * int(starts.size) * (world - 1)}, (name, t)
        if max_bases == 256:
            assert n_batches > 10 and (k < 27 or (lens > 256).any())
        elif max_recs == 7:
            assert n_batches == -(-int(starts.size) // 7) and n_batches > 3      # the record limit alone cuts
        else:
            assert n_batches == 1
    assert saw_big
    return cases, slot_bytes


# world, transport, k, mode, bases per batch (0: the default, one batch), records per batch (0: the default), size hint, the slot bytes it makes (0: whatever)
@pytest.mark.parametrize("world,transport,k,mode,batch,recs,hint,slot", [
    (1, "shm", 27, "plans", 256, 0, 1 << 16, 12), (2, "shm", 5, "plans", 256, 0, 1 << 16, 0), (2, "shm", 27, "plans_nc", 256, 0, 1 << 16, 12),
    (3, "shm", 41, "plans", 256, 0, 1 << 16, 20), (3, "shm", 27, "plans", 256, 0, 1 << 23, 8), (8, "shm", 27, "plans", 256, 0, 1 << 16, 12),
    (2, "shm", 27, "plans", 0, 0, 1 << 16, 12), (3, "rccl", 27, "plans", 256, 0, 1 << 16, 12), (2, "shm", 27, "plans", 0, 7, 1 << 16, 12)])
def test_gathered_hits_are_the_dictionarys(tmp_path, request, world, transport, k, mode, batch, recs, hint, slot):
    """Worlds 1, 2, 3 and 8 (9 processes hold the GPU), k = 5, 27 and 41 (wide), canonical and non-canonical tables at k = 27, both
    one-word layouts (8-byte packed slots at a size hint of 2^23, 12-byte ones below), every ownership plan of
    tests/profile_gather_rank.py; batches of 256 bases, the default once (one batch), once through the RCCL branch, and once with
    batches of 7 records (KATGPU_TEST_HITS_RECS: the record limit cuts, not the base limit)."""
    env = {"KATGPU_COMM_TRANSPORT": transport, "PROFILE_GATHER_SIZE_HINT": str(hint)}
    if batch:
        env["KATGPU_TEST_HITS_BATCH"] = str(batch)
    if recs:
        env["KATGPU_TEST_HITS_RECS"] = str(recs)
    if transport == "rccl":
        env["KATGPU_RCCL_LIB"] = request.getfixturevalue("fake_rccl")
    outs = _launch(tmp_path, world, k, mode, env)
    assert "transport: %s" % transport in outs[0], outs[0][-2000:]
    cases, slot_bytes = _check(tmp_path, world, k, mode == "plans", batch or DEFAULT_BATCH, recs or DEFAULT_RECS, outs[0])
    assert {"even", "all_on_rank0", "all_on_last", "nothing"} <= {c[0] for c in cases}
    if world > 2:
        assert "rank1_empty" in {c[0] for c in cases}
    if slot:
        assert slot_bytes == {slot}, slot_bytes


def _first_case(k, world):
    S, cases = pr.plans(k, world, True)
    name, plan, chosen = cases[0]
    seq, _ = pr.sequence(k, S, chosen, True)
    return seq, _counts_of(plan)


@pytest.mark.parametrize("world,k", [(2, 27), (3, 41)])
def test_more_records_in_a_chunk_than_lds_bins(tmp_path, world, k):
    """2100 empty records between two real ones: the second one's hits are added beyond the 2048 LDS bins of its chunk, straight to memory."""
    outs = _launch(tmp_path, world, k, "empties", {})
    for r, o in enumerate(outs):
        assert "empties ok rank %d" % r in o, o[-2000:]
    seq, counts = _first_case(k, world)
    flat, starts, lens = hr.with_empties(seq)
    want = _expected(flat, starts, lens, k, counts, True)
    assert want.size == hr.N_EMPTY + 2 > 2048 + 2 and want[0] > 0 and want[-1] > 0 and not want[1:-1].any()
    assert np.array_equal(np.load(tmp_path / "empties.npy"), want)
    t = [json.loads(m.group(1)) for m in map(TIMING.search, outs[0].splitlines()) if m]
    assert t == [{"phase": "seq_hits_gathered", "batches": 1, "ranks": world, "records": want.size, "wire_bytes": 8 * want.size * (world - 1)}]


@pytest.mark.parametrize("world,k", [(2, 41), (3, 27)])
def test_ranks_that_disagree_on_the_records_all_get_invalid_arg(tmp_path, world, k):
    """The last rank passes one record fewer: KATGPU_ERR_INVALID_ARG on every rank with a message naming it, nothing written, an
    all-reduce on the same communicator still works (asserted in the rank script) -- and so does the call itself."""
    outs = _launch(tmp_path, world, k, "mismatch", {"KATGPU_TEST_HITS_BATCH": "256"})
    for r, o in enumerate(outs):
        assert "mismatch ok rank %d" % r in o, o[-2000:]
    seq, counts = _first_case(k, world)
    starts, lens = hr.records(seq)
    assert np.array_equal(np.load(tmp_path / "after_mismatch.npy"), _expected(seq, starts, lens, k, counts, True))


@pytest.mark.parametrize("world,k,who", [(2, 27, 1), (3, 41, 0)])
def test_no_memory_is_collective(tmp_path, world, k, who):
    """KATGPU_TEST_HITS_GATHER_NOMEM: one rank reports that it could not allocate -- every rank returns KATGPU_ERR_NOMEM naming it, and
    the communicator carries an all-reduce afterwards (asserted in the rank script)."""
    outs = _launch(tmp_path, world, k, "nomem", {"KATGPU_TEST_HITS_GATHER_NOMEM": str(who)})
    for r, o in enumerate(outs):
        assert "nomem ok rank %d" % r in o, o[-2000:]
    assert not any("seq_hits_gathered" in o for o in outs)


@pytest.mark.parametrize("world,k", [(2, 27)])
def test_no_records_is_ok_and_silent(tmp_path, world, k):
    """n_rec == 0, with and without bases: KATGPU_OK on every rank, nothing written, no timing line."""
    outs = _launch(tmp_path, world, k, "zero", {})
    for r, o in enumerate(outs):
        assert "zero ok rank %d" % r in o, o[-2000:]
    assert not any("seq_hits_gathered" in o for o in outs)
