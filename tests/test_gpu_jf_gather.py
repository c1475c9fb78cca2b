"""katgpu_jf_dump_gathered: the ranks' tables, after the exchange, in the one .jf file rank 0 writes -- runs ordered and packed on every
rank's device, gathered on rank 0's and ordered there from the packed runs (k_jf_select_runs), range of positions by range.
tests/jf_gather_rank.py is one rank.  The independent side is the host writer (katgpu_jf_write_records[_wide], pinned to the
reference's reader by tests/test_jf.py) on the summed records: the gathered file's record bytes are its record bytes; the header, its
"time" apart, is that of a single process's katgpu_jf_dump of one table holding the union.

A stretch of positions without records is absorbed by the range before it (the "gap" plan leaves a quarter of the positions without a
k-mer), but the LAST range can be empty on every rank: a stretch that alone holds more than the target is closed by the empty stretch
behind it, and if nothing follows, what is left up to 2^r holds no record.  The "empty_tail" plan builds that at 64 records a range
(tests/jf_gather_rank.py), and the timing line must count the empty range.  "all_on_last" leaves rank 0's own run empty in every
range, "all_on_rank0" every remote one."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from tests import jf_gather_rank as jr
from tests.test_gpu_comm import fake_rccl  # noqa: F401  (the RCCL stand-in, built once per module)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
U64 = np.uint64
BIG = 1 << 30                                           # a KATGPU_JF_RANGE_RECORDS larger than any table here: one range
EVEN_TOTAL = {64: 1500, 700: 7000, BIG: 3000}           # the "even" plan's records: at least 8 ranges at 64 and at 700 records a range
# the "even" plan makes at least 8 ranges everywhere but here: one range by design, and the 512 canonical 5-mers are one range of 700
SINGLE_RANGE = {(32, BIG), (63, BIG), (5, 700)}
TIMING = re.compile(r'katgpu_timing (\{"phase": "jf_dump_gathered".*\})')


def _launch(tmp_path, world, k, mode, env_extra, even_total):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("KATGPU_COMM_INIT_TIMEOUT_S", "60")
    env.setdefault("KATGPU_COMM_TIMEOUT_S", "20")       # a rank that dies ends the others through the communicator's liveness checks
    env.update(KATGPU_TESTING="1", KATGPU_TIMING="1", JF_GATHER_EVEN_TOTAL=str(even_total))
    env.update(env_extra)
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "jf_gather_rank.py"), str(r), str(world), str(tmp_path / "id.bin"), str(tmp_path), str(k), mode],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=240)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    if any(p.returncode for p in procs) and any("did not return within" in o and "KATGPU_COMM_INIT_TIMEOUT_S" in o for o in outs):
        pytest.skip("RCCL's bootstrap did not come back on this box: " + next(o for o in outs if "did not return within" in o)[-300:])    # the box's, not the code's
    assert all(p.returncode == 0 for p in procs), "\n----\n".join(o[-3000:] for o in outs)
    return outs


def _split(path):
    """(header bytes without the "time" field, record bytes)."""
    b = open(path, "rb").read()
    h = int(b[:9])
    return re.sub(rb'"time":"[^"]*"', b"", b[9:9 + h]), b[9 + h:]


def _implied_ranges(P, k, host_file, want):
    """The records of every range the cuts make of these k-mers under the file's matrix: stretches of 2^(r - min(r, 16)) positions, a
    new range where the next stretch would take the range past `want` records, the last one up to 2^r.  No record: no range."""
    if not len(P):
        return []
    r, cols = jr.header_matrix(host_file)
    cb = min(r, 16)
    bins = np.bincount((jr.positions(P, cols, r) >> U64(r - cb)).astype(np.int64), minlength=1 << cb)
    sizes, acc = [], 0
    for b in bins.tolist():
        if acc and acc + b > want:
            sizes.append(acc)
            acc = 0
        acc += b
    return sizes + [acc]


def _check(tmp_path, world, k, want, out0):
    P, cases = jr.plans(k, world, EVEN_TOTAL[want], str(tmp_path))
    # rank 0's output: one jf_dump_gathered line before every "plan" line
    lines, pending = {}, []
    for ln in out0.splitlines():
        m = TIMING.search(ln)
        if m:
            pending.append(m.group(1))
        m = re.match(r"plan (\d+) (\w+)", ln)
        if m:
            assert len(pending) == 1, (ln, pending)
            lines[int(m.group(1))] = pending.pop()
    assert sorted(lines) == list(range(len(cases))), out0[-3000:]
    kb = (2 * k + 7) // 8
    for ci, (name, plan) in enumerate(cases):
        idx = np.concatenate([p[0] for p in plan])
        cnt = np.concatenate([p[1] for p in plan])
        host = str(tmp_path / ("case_%02d.host.jf" % ci))
        jr.write_host(host, k, P[idx], cnt)                                   # (disjoint across ranks: the sum of the records is their union)
        got_h, got_r = _split(tmp_path / ("case_%02d.jf" % ci))
        assert got_r == _split(host)[1], (name, len(got_r), idx.size)
        assert len(got_r) == idx.size * (kb + 4)
        one_h, one_r = _split(tmp_path / ("case_%02d.single.jf" % ci))
        assert got_h == one_h, name
        assert got_r == one_r, name
        t = json.loads(lines[ci])
        assert t["ranks"] == world and t["records"] == idx.size, (name, t)
        sizes = _implied_ranges(P[idx], k, host, want)
        assert t["ranges"] == len(sizes), (name, t, sizes)
        if name == "even" and (k, want) not in SINGLE_RANGE:
            assert t["ranges"] >= 8, (name, t)                                # the streaming ran: range after range
        if name == "empty_tail" and want == 64:                               # a range without a record on any rank, and it is counted
            assert sizes == [jr.TAIL_TOTAL - jr.TAIL_PILE, jr.TAIL_PILE, 0], sizes
        if name == "even":                                                    # 2^32 - 1, 2^32 and 2^40 all read 0xFFFFFFFF
            recs = np.frombuffer(got_r, np.uint8).reshape(-1, kb + 4)
            sat = int((recs[:, kb:] == 255).all(axis=1).sum())
            assert sat == len(jr.SATURATING), sat
    return cases


@pytest.mark.parametrize("world,transport,k,want", [
    (2, "shm", 27, 64), (3, "shm", 33, 700), (2, "rccl", 63, 64), (3, "rccl", 27, 700),
    (3, "shm", 5, 64), (2, "rccl", 5, 700), (2, "rccl", 32, BIG), (2, "shm", 45, 700),
    (3, "rccl", 45, 64), (3, "shm", 63, BIG), (2, "rccl", 33, 64), (3, "shm", 32, 64),
    (8, "shm", 27, 64)])                                                      # 8: the node's world size (9 processes hold the GPU)
def test_gathered_dump_is_the_host_writers_file(tmp_path, fake_rccl, world, transport, k, want):  # noqa: F811
    """2, 3 and 8 ranks over /dev/shm and through the RCCL branch (the stand-in library: one GPU), every record width (k = 5: all 512
    canonical 5-mers, r capped at 2k; 27: 11-byte records, every run after the first unaligned; 32; 33; 45; 63: 20 bytes), ranges of
    64 and 700 records and a single one, every ownership plan of tests/jf_gather_rank.py."""
    env = {"KATGPU_COMM_TRANSPORT": transport, "KATGPU_JF_RANGE_RECORDS": str(want)}
    if transport == "rccl":
        env["KATGPU_RCCL_LIB"] = fake_rccl
    outs = _launch(tmp_path, world, k, "plans", env, EVEN_TOTAL[want])
    assert "transport: %s" % transport in outs[0], outs[0][-2000:]
    cases = _check(tmp_path, world, k, want, outs[0])
    assert {"even", "all_on_rank0", "all_on_last", "nothing", "single"} <= {n for n, _ in cases}
    if k != 5:                                                                # (512 5-mers cannot pile 66 onto one position)
        assert {"gap", "empty_tail"} <= {n for n, _ in cases}
    if world > 2:
        assert "rank1_empty" in {n for n, _ in cases}


@pytest.mark.parametrize("k,want", [(27, 64), (45, 700)])
def test_gathered_dump_single_rank_over_rccl(tmp_path, k, want):
    """One rank over real RCCL: the file katgpu_jf_dump writes."""
    outs = _launch(tmp_path, 1, k, "plans", {"KATGPU_COMM_TRANSPORT": "rccl", "KATGPU_JF_RANGE_RECORDS": str(want)}, EVEN_TOTAL[want])
    assert "transport: rccl" in outs[0], outs[0][-2000:]
    _check(tmp_path, 1, k, want, outs[0])


@pytest.mark.parametrize("world,transport,k,who", [(2, "shm", 27, 1), (3, "rccl", 45, 0), (3, "shm", 33, 2)])
def test_no_go_is_collective_and_leaves_no_file(tmp_path, fake_rccl, world, transport, k, who):  # noqa: F811
    """KATGPU_TEST_JF_GATHER_NOMEM: one rank reports that it could not allocate -- every rank returns KATGPU_ERR_NOMEM naming it, nothing
    exists at the path, and the communicator carries an all-reduce afterwards (asserted in the rank script)."""
    env = {"KATGPU_COMM_TRANSPORT": transport, "KATGPU_JF_RANGE_RECORDS": "64", "KATGPU_TEST_JF_GATHER_NOMEM": str(who)}
    if transport == "rccl":
        env["KATGPU_RCCL_LIB"] = fake_rccl
    outs = _launch(tmp_path, world, k, "nomem", env, 1500)
    for r, o in enumerate(outs):
        assert "nomem ok rank %d" % r in o, o[-2000:]
    assert not (tmp_path / "nomem.jf").exists()
    assert not any("jf_dump_gathered" in o for o in outs)


@pytest.mark.parametrize("world,transport,k", [(2, "shm", 27), (3, "rccl", 45)])
def test_unopenable_output_is_collective_and_leaves_no_file(tmp_path, fake_rccl, world, transport, k):  # noqa: F811
    """Rank 0's path lies in a directory that does not exist: every rank returns KATGPU_ERR_IO -- rank 0 naming the path, its peers
    rank 0 -- none hangs (a rank that reaches _launch's time limit fails the test), nothing exists at the path, and the communicator
    carries an all-reduce afterwards (asserted in the rank script).  50 to 60 k-mers a rank at 64 records a range: more than one range."""
    env = {"KATGPU_COMM_TRANSPORT": transport, "KATGPU_JF_RANGE_RECORDS": "64"}
    if transport == "rccl":
        env["KATGPU_RCCL_LIB"] = fake_rccl
    outs = _launch(tmp_path, world, k, "noopen", env, 120 if world == 2 else 150)
    for r, o in enumerate(outs):
        assert "noopen ok rank %d" % r in o, o[-2000:]
    assert not (tmp_path / "no_such_dir").exists()
    assert not any("jf_dump_gathered" in o for o in outs)


@pytest.mark.parametrize("k", [27, 45])
def test_records_of_a_table_are_what_they_were(engine, tmp_path, k):
    """katgpu_table_jf_records_device[_wide], whose range producer now takes its records from a table or from packed runs: the bytes of
    a narrow and of a wide table, whole and range by range, are the host writer's."""
    P = jr.pool(k)[:5000]
    cnt = np.random.default_rng(5).integers(1, 1 << 34, size=len(P), dtype=U64)
    t = engine.table(k, True, size_hint=1 << 16)
    if k > 32:
        t.merge_host_wide(P[:, 0], P[:, 1], cnt)
    else:
        t.merge_host(P[:, 1], cnt)
    host = str(tmp_path / "host.jf")
    jr.write_host(host, k, P, cnt)
    r, cols = jr.header_matrix(host)
    want = _split(host)[1]
    rec = t.jf_records_wide if k > 32 else t.jf_records
    cols = np.array(cols, U64)
    assert rec(r, cols, count_only=True) == len(P)
    assert bytes(rec(r, cols)) == want
    cuts = [0, 1, (1 << r) // 3, (1 << r) // 3, (1 << r) - 5, 1 << r]
    assert b"".join(bytes(rec(r, cols, lo, hi)) for lo, hi in zip(cuts, cuts[1:])) == want
    t.free()
