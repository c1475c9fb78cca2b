"""The native exchange (kg_comm.hip) at exact small sizes: every rank's tables are filled from a plan (tests/comm_plan_rank.py), so that
send lists, receive sets and chunks hold none, one, 31, 32, 33 ... records, everything belongs to one rank, every rank has the same keys,
or a rank's only records travel out of band.  Against a plain numpy reference of the same records: the exact sums per key split by
owner, rank by rank, and the oracle's hist / gcp / comp of the summed tables for the all-reduced results."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_comm import fake_rccl  # noqa: F401  (the RCCL stand-in, built once per module)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
K = {"packed": 27, "wire12": 27, "mixed": 27, "xs": 29, "wide": 45}
FORM_ENV = {"packed": {"KATGPU_TEST_REGION_SLOTS": "128"}, "wire12": {"KATGPU_TEST_REGION_SLOTS": "128", "KATGPU_COMM_PACKED_RECORDS": "0"},
            "mixed": {}, "xs": {"KATGPU_TEST_REGION_SLOTS": "128"}, "wide": {}}


def _run(tmp_path, world, form, shape, env_extra):
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("KATGPU_COMM_INIT_TIMEOUT_S", "60")
    env.update(FORM_ENV[form], KATGPU_TESTING="1", KATGPU_TEST_EXCHANGE_CHUNKS="6")
    env.update(env_extra)
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "comm_plan_rank.py"), str(r), str(world), str(tmp_path / "id.bin"), str(tmp_path), form, shape],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True) for r in range(world)]
    outs = []
    for p in procs:
        try:
            outs.append(p.communicate(timeout=400)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    if any(p.returncode for p in procs) and any("did not return within" in o and "KATGPU_COMM_INIT_TIMEOUT_S" in o for o in outs):
        pytest.skip("RCCL's bootstrap did not come back on this box: " + next(o for o in outs if "did not return within" in o)[-300:])    # the box's, not the code's
    assert all(p.returncode == 0 for p in procs), "\n----\n".join(o[-3000:] for o in outs)
    return outs[0]


def _summed(ko, k, records):
    """{key: exact sum} over (keys, counts) pairs, and the oracle table holding it."""
    total = {}
    for keys, counts in records:
        for key, c in zip(keys, counts.tolist()):
            total[key] = total.get(key, 0) + int(c)
    o = (ko.WideTable if k > 32 else ko.Table)(k, True)
    for key, c in total.items():
        o.add(key, c)
    return total, o


def _as_ints(keys, k):
    if k > 32:
        return [(int(h) << 64) | int(lo) for h, lo in keys.reshape(-1, 2).tolist()] if keys.size else []
    return [int(x) for x in keys.tolist()]


def _check(ko, tmp_path, world, form):
    from kat_amd import dist as kdist
    k = K[form]
    n_cases = len([f for f in os.listdir(tmp_path) if f.startswith("case_") and f.endswith(".rank0.npz")])
    assert n_cases >= 13, n_cases
    for ci in range(n_cases):
        got = [np.load(tmp_path / ("case_%02d.rank%d.npz" % (ci, r))) for r in range(world)]
        total, o1 = _summed(ko, k, [(_as_ints(g["ins"], k), g["ins_counts"]) for g in got])
        _, o2 = _summed(ko, k, [(_as_ints(g["ins2"], k), g["ins2_counts"]) for g in got])
        keys = sorted(total)
        if k > 32:
            hi = np.array([x >> 64 for x in keys], np.uint64)
            lo = np.array([x & ((1 << 64) - 1) for x in keys], np.uint64)
            own = kdist.owner_of_wide(hi, lo, k, world) if keys else np.zeros(0, np.int64)
        else:
            own = kdist.owner_of(np.array(keys, np.uint64), k, world) if keys else np.zeros(0, np.int64)
        for r, g in enumerate(got):
            want = [x for x, w in zip(keys, own.tolist()) if w == r]
            if k > 32:
                have = [(int(h) << 64) | int(lo) for h, lo in zip(g["got_hi"].tolist(), g["got_lo"].tolist())]
            else:
                have = [int(x) for x in g["got_keys"].tolist()]
            assert have == want, (ci, r, len(have), len(want))
            assert [int(c) for c in g["got_counts"].tolist()] == [total[x] for x in want], (ci, r)
            if form in ("packed", "xs"):
                assert bool(g["packed"]), (ci, r)                                      # 9-byte records on the wire
            elif form in ("wire12", "mixed"):
                assert not bool(g["packed"]), (ci, r)
        mx, cc, sp = ko.comp(o1, o2, 1.0, 1.0, 201, 101)
        h, gm = o1.hist(1, 300, 1), o1.gcp(1.0, 100)
        for r, g in enumerate(got):
            assert np.array_equal(g["h"], h) and np.array_equal(g["gm"], gm), (ci, r)
            assert np.array_equal(g["mx"], mx) and np.array_equal(g["cc"], cc) and np.array_equal(g["sp"], sp), (ci, r)
    if form == "xs":
        assert int(np.load(tmp_path / "case_00.rank0.npz")["xs"]) > 0          # (the case of counts past 32 - xs bits ran)


@pytest.mark.parametrize("world,transport,form,shape,extra", [
    (2, "shm", "packed", "pipelined", {}),
    (3, "shm", "packed", "split", {"KATGPU_TEST_LAZY_MIN_SLOTS": "1024"}),      # (lazy: the emptied table is not cleared, the merge is its first sweep)
    (2, "rccl", "packed", "split", {"KATGPU_TEST_EXCHANGE_NO_SPLIT": "1"}),      # split refused: the pipelined shape inside begin
    (3, "rccl", "packed", "pipelined", {"KATGPU_TEST_LAZY_MIN_SLOTS": "1024"}),
    (2, "shm", "wire12", "split", {}),
    (3, "rccl", "wire12", "pipelined", {}),
    (2, "rccl", "mixed", "split", {}),
    (3, "shm", "mixed", "pipelined", {}),
    (2, "shm", "xs", "split", {}),
    (3, "rccl", "xs", "pipelined", {}),
    (3, "shm", "wide", "pipelined", {}),
    (2, "rccl", "wide", "split", {})])
def test_exchange_at_exact_small_sizes(ko, tmp_path, fake_rccl, world, transport, form, shape, extra):  # noqa: F811
    """2 and 3 ranks on the /dev/shm transport and on the RCCL branch (the stand-in library: one GPU), every wire form and shape."""
    env = dict(extra, KATGPU_COMM_TRANSPORT=transport)
    if transport == "rccl":
        env["KATGPU_RCCL_LIB"] = fake_rccl
    out = _run(tmp_path, world, form, shape, env)
    assert "transport: %s" % transport in out, out[-2000:]
    _check(ko, tmp_path, world, form)


@pytest.mark.parametrize("form,shape", [("packed", "pipelined"), ("packed", "split"), ("wide", "pipelined")])
def test_exchange_at_exact_small_sizes_single_rank_over_rccl(ko, tmp_path, form, shape):
    """One rank over real RCCL: the whole protocol on the rank's own records."""
    out = _run(tmp_path, 1, form, shape, {"KATGPU_COMM_TRANSPORT": "rccl"})
    assert "transport: rccl" in out, out[-2000:]
    _check(ko, tmp_path, 1, form)
