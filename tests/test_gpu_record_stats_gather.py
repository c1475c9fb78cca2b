"""katgpu_table_record_stats_gathered_host: after the exchange a k-mer lives on one rank; per batch of records the ranks' runs of
(window, count) are gathered into one dense array on rank 0's device, and rank 0 reduces it there -- the statistics of every record
and the regions of one or two count ranges from the same gather (the CountsDense kernels), 48 bytes per record and 24 per region back.
tests/record_stats_gather_rank.py is one rank; the ranks share one device over /dev/shm.

The expected values owe nothing to the code under test: the per-position array from a Python dictionary of the plan's k-mers, as
tests/test_gpu_profile_gather.py builds it, then tests/record_stats_model.py and tests/record_regions_model.py over the records the
sequence's "\\n" bytes cut it into.  Equality is exact.  The timing lines: one profile_gathered and one record_stats_gathered per
call, the first with the records and wire bytes that follow from the dictionary and the owners."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import profile_gather_rank as pr
from tests import record_regions_model as gm
from tests import record_stats_gather_rank as rr
from tests import record_stats_model as sm
from tests.test_gpu_profile_gather import _expected

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
U64 = np.uint64
GATHER = re.compile(r'katgpu_timing (\{"phase": "profile_gathered".*\})')
STATS = re.compile(r'katgpu_timing (\{"phase": "record_stats_gathered".*\})')


def _launch(tmp_path, world, k, mode, env_extra):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("KATGPU_COMM_INIT_TIMEOUT_S", "60")
    env.setdefault("KATGPU_COMM_TIMEOUT_S", "20")       # a rank that dies ends the others through the communicator's liveness checks
    env.update(KATGPU_TESTING="1", KATGPU_TIMING="1", KATGPU_COMM_TRANSPORT="shm", KATGPU_TEST_GATHER_BATCH="64")
    env.update(env_extra)
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "record_stats_gather_rank.py"), str(r), str(world), str(tmp_path / "id.bin"), str(tmp_path), str(k), mode],
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
    assert all(p.returncode == 0 for p in procs), "\n----\n".join(o[-3000:] for o in outs)
    return outs


def _want(seq, k, counts, canonical):
    """the dictionary's per-position array, the records, and what the two models make of them"""
    prof = _expected(seq, k, counts, canonical)
    st, ln = rr.records(seq)
    b = seq.encode()
    full = np.zeros(len(b), U64)                          # (the models index counts by base position)
    full[:prof.size] = prof
    return prof, st, ln, sm.record_stats(b, st, ln, k, full), gm.regions(b, st, ln, k, full, rr.RANGES)


def _assert_case(path, want_s, want_r, what):
    z = np.load(path)
    got = z["stats"]
    assert got.shape == want_s.shape, (what, got.shape, want_s.shape)
    for f in sm.FIELDS:
        bad = np.flatnonzero(got[f] != want_s[f])
        assert bad.size == 0, (what, f, bad[:5], got[f][bad[:5]], want_s[f][bad[:5]])
    for q in (0, 1):
        g, w = z["r%d" % q], want_r[q]
        assert g.dtype == U64 and g.shape == w.shape, (what, q, g.shape, w.shape)
        assert np.array_equal(g, w), (what, q)


# world, k, mode, size hint, the slot bytes it makes (0: whatever), hooks beside KATGPU_TEST_GATHER_BATCH=64
@pytest.mark.parametrize("world,k,mode,hint,slot,hooks", [
    (1, 27, "plans", 1 << 16, 12, {}),
    (2, 27, "plans_nc", 1 << 16, 12, {}),
    (3, 41, "plans", 1 << 16, 20, {"KATGPU_TEST_STATS_SHORT": "20"}),           # records of more than 20 windows go the long way
    (3, 27, "plans", 1 << 23, 8, {"KATGPU_TEST_STATS_BATCH": "700"}),           # several record batches per call
    (2, 5, "plans", 1 << 16, 0, {}),
    (2, 27, "plans", 1 << 16, 12, {"KATGPU_TEST_STATS_SHORT": "20", "KATGPU_TEST_STATS_BATCH": "700"})])   # the long records' window budget ends batches (last: the rows above keep their ids)
def test_gathered_statistics_and_regions_are_the_models(tmp_path, world, k, mode, hint, slot, hooks):
    canonical = mode == "plans"
    outs = _launch(tmp_path, world, k, mode, dict(hooks, PROFILE_GATHER_SIZE_HINT=str(hint)))
    for o in outs[1:]:
        assert "katgpu_timing" not in o, o[-2000:]
    S, cases = pr.plans(k, world, canonical)
    lines, slot_bytes, pending = {}, set(), []
    for ln_ in outs[0].splitlines():                     # rank 0's output: the two lines of a call before every "plan" line
        for rx in (GATHER, STATS):
            m = rx.search(ln_)
            if m:
                pending.append(json.loads(m.group(1)))
        m = re.match(r"plan (\d+) (\w+) slot_bytes (\d+)", ln_)
        if m:
            assert [p["phase"] for p in pending] == ["profile_gathered", "record_stats_gathered"], (ln_, pending)
            lines[int(m.group(1))] = pending
            pending = []
            slot_bytes.add(int(m.group(3)))
    assert sorted(lines) == list(range(len(cases))), outs[0][-3000:]
    if slot:
        assert slot_bytes == {slot}, slot_bytes
    saw_big = saw_long = False
    for ci, (name, plan, chosen) in enumerate(cases):
        counts = {s: c for strings, cnt in plan for s, c in zip(strings, cnt.tolist())}
        seq, _ = pr.sequence(k, S, chosen, canonical)
        prof, st, ln, want_s, want_r = _want(seq, k, counts, canonical)
        assert any(0 < n < k for n in ln.tolist()) and k in ln.tolist() and "N" * pr.N_RUN in seq and any(c.islower() for c in seq)
        _assert_case(tmp_path / ("case_%02d.npz" % ci), want_s, want_r, name)
        if chosen:
            assert want_r[0].shape[0] > 5 and want_r[1].shape[0] > 5, name
            saw_big = saw_big or int(want_s["sum"].max()) >= pr.BIG
        saw_long = saw_long or int(ln.max()) - k + 1 > 20
        # the gather's line: the records and wire bytes follow from who owns what; the statistics' line from the models
        hits = np.flatnonzero(prof)
        own = pr.owner([seq[i:i + k].upper() for i in hits], k, world) if hits.size else np.zeros(0, np.int64)
        g, t = lines[ci]
        assert g["batches"] >= 40 and {x: g[x] for x in ("ranks", "records", "wire_bytes")} == \
            {"ranks": world, "records": int(hits.size), "wire_bytes": 12 * int((own != 0).sum())}, (name, g)
        n_regions = want_r[0].shape[0] + want_r[1].shape[0]
        assert {x: t[x] for x in ("ranks", "records", "regions", "back_bytes")} == \
            {"ranks": world, "records": int(st.size), "regions": n_regions, "back_bytes": 48 * int(st.size) + 24 * n_regions}, (name, t)
        assert t["batches"] >= 4 if "KATGPU_TEST_STATS_BATCH" in hooks else t["batches"] == 1, (name, t)
    assert saw_big and saw_long                           # a count of 2^40 came back whole in a sum; a record the hook sends the long way


@pytest.mark.parametrize("world,k", [(2, 41), (3, 27)])
def test_ranks_that_disagree_on_the_records_all_get_invalid_arg(tmp_path, world, k):
    """The last rank passes one record fewer: KATGPU_ERR_INVALID_ARG on every rank, nothing written, an all-reduce on the same
    communicator still works (asserted in the rank script) -- and so does the call itself."""
    outs = _launch(tmp_path, world, k, "mismatch", {})
    for r, o in enumerate(outs):
        assert "mismatch ok rank %d" % r in o, o[-2000:]
    S, cases = pr.plans(k, world, True)
    name, plan, chosen = cases[0]
    counts = {s: c for strings, cnt in plan for s, c in zip(strings, cnt.tolist())}
    seq, _ = pr.sequence(k, S, chosen, True)
    _, _, _, want_s, want_r = _want(seq, k, counts, True)
    _assert_case(tmp_path / "after_mismatch.npz", want_s, want_r, "after the mismatch")


@pytest.mark.parametrize("world,k,who", [(2, 27, 1), (3, 41, 0)])
def test_no_memory_is_collective(tmp_path, world, k, who):
    """KATGPU_TEST_GATHER_NOMEM: one rank reports that it could not allocate -- every rank returns KATGPU_ERR_NOMEM naming it, and the
    communicator carries an all-reduce afterwards (asserted in the rank script)."""
    outs = _launch(tmp_path, world, k, "nomem", {"KATGPU_TEST_GATHER_NOMEM": str(who)})
    for r, o in enumerate(outs):
        assert "nomem ok rank %d" % r in o, o[-2000:]
    assert not any("katgpu_timing" in o for o in outs)


def test_no_records(tmp_path):
    outs = _launch(tmp_path, 2, 27, "empty", {})
    for r, o in enumerate(outs):
        assert "empty ok rank %d" % r in o, o[-2000:]
    assert not any("profile_gathered" in o for o in outs)


@pytest.mark.parametrize("world,k", [(2, 27), (3, 41)])
def test_shorter_than_k_gathers_nothing(tmp_path, world, k):
    """k - 1 bases holding two records: their gc_bases and n_bases are right, everything else is 0, there is no region, and no gather ran."""
    outs = _launch(tmp_path, world, k, "short", {})
    for r, o in enumerate(outs):
        assert "short ok rank %d" % r in o, o[-2000:]
    assert not any("profile_gathered" in o for o in outs)
    b, st, ln = rr.short_case(k)
    want_s = sm.record_stats(b, st, ln, k, np.zeros(len(b), U64))
    assert int(want_s["gc_bases"].sum()) > 5 and int(want_s["n_bases"].sum()) > 2
    _assert_case(tmp_path / "short.npz", want_s, [np.zeros((0, 3), U64)] * 2, "short")
