"""katgpu_hist and katgpu_gcp through every kernel form they dispatch (kat_amd/csrc/kg_reduce.hip), at the edges of their arguments,
against two witnesses: the model of tests/reducer_forms_model.py and the oracle.

The forms: k_hist<false> (KV12 and wide tables) and k_hist<true> (packed), each with all its buckets in LDS and with global ones;
k_gcp<false,false>, k_gcp_pk and k_gcp<true,false>, each with global atomics and with the LDS increments of the environment (plain, or
aggregated per wave under KATGPU_COMP_PLAIN_INC=0), with and without side-table counts; k_gcp_pk's second region per wave and its
second round of quads.  The tables are crafted (merge_host / merge_host_wide of explicit records next to a counted stream): twins of
the same keys, one whose counts all stay in their slots and one with counts on both sides of the slot's limit and far beyond it.  A
child per environment and region size (tests/reducer_forms_case.py: the hooks are read when the library loads) compares every result
exactly and every call's "reducer form:" trace line with the model's dispatch; this module asserts that every reachable form was seen.

The records, the stream and both witnesses' results are made once per module, on the CPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import reducer_forms_model as rf

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
COMMON = {"KATGPU_TESTING": "1", "KATGPU_TRACE": "1"}
M64 = (1 << 64) - 1


def sparse(out, name, a):
    flat = np.ascontiguousarray(a, np.uint64).ravel()
    idx = np.flatnonzero(flat)
    out[name + "_idx"], out[name + "_val"] = idx, flat[idx]


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    from oracle import koracle as ko
    d = tmp_path_factory.mktemp("reducer_forms")
    np.save(d / "stream.npy", rf.stream())
    for la in rf.LAYOUTS:
        out = {}
        for twin in ("a", "b"):
            crafted = rf.crafted(la.name)[twin]
            out[twin + "_hi"] = np.array([key >> 64 for key, _ in crafted], np.uint64)
            out[twin + "_lo"] = np.array([key & M64 for key, _ in crafted], np.uint64)
            out[twin + "_counts"] = np.array([c for _, c in crafted], np.uint64)
            o = (ko.WideTable if la.k > 32 else ko.Table)(la.k, False)
            for key, c in crafted:
                o.add(key, c)
            o.count_bases(rf.stream())
            m = rf.Multiset(la.k, rf.records(la.name, twin))
            out[twin + "_distinct"] = np.uint64(m.distinct)
            for i, (low, high, inc) in enumerate(rf.HIST_TRIPLES):
                sparse(out, "%s_hist%d_model" % (twin, i), rf.hist_model(m, *rf.hist_geometry(low, high)[:2], inc, rf.hist_geometry(low, high)[2]))
                sparse(out, "%s_hist%d_oracle" % (twin, i), o.hist(low, high, inc))
            for i, (scale, bins) in enumerate(rf.gcp_args(la.k, twin)):
                sparse(out, "%s_gcp%d_model" % (twin, i), rf.gcp_model(m, la.k, scale, bins))
                sparse(out, "%s_gcp%d_oracle" % (twin, i), o.gcp(scale, bins))
        np.savez(d / (la.name + ".npz"), **out)
    return str(d)


def child(reference, env, region_slots, names):
    r = subprocess.run([sys.executable, os.path.join(HERE, "reducer_forms_case.py"), reference] + names,
                       env=dict(os.environ, **COMMON, KATGPU_TEST_REGION_SLOTS=str(region_slots), **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "reducer forms ok: " + " ".join(names) in r.stdout, "exit %d\n" % r.returncode + r.stdout[-3000:] + r.stderr[-6000:]
    print(r.stdout)
    line = next(x for x in r.stdout.splitlines() if x.startswith("forms seen: "))
    calls = int(r.stdout.rsplit(", ", 1)[1].split()[0])
    return {tuple(f) for f in json.loads(line[len("forms seen: "):])}, calls


@pytest.mark.parametrize("env", [
    {},                                                                     # packed tables where the geometry allows; plain LDS increments
    {"KATGPU_COMP_PLAIN_INC": "0"},                                         # gcp's LDS increments aggregated per wave
    {"KATGPU_NO_PACKED": "1"},                                              # KV12 slots at every k <= 32
    {"KATGPU_TEST_LAZY_MIN_SLOTS": "1"}],                                   # packed tables are left uncleared for their first sweep
    ids=["default", "aggregated", "no_packed", "lazy"])
def test_reducer_forms_match_model_and_oracle(reference, env):
    seen, calls = set(), 0
    for region_slots in sorted({la.region_slots for la in rf.LAYOUTS}):
        s, n = child(reference, env, region_slots, [la.name for la in rf.LAYOUTS if la.region_slots == region_slots])
        seen |= s
        calls += n
    packed = "KATGPU_NO_PACKED" not in env
    want = rf.reachable_forms({8, 12, 20} if packed else {12, 20}, env.get("KATGPU_COMP_PLAIN_INC", "1") != "0")
    if packed:
        want |= {("gcp", "pk", what, ovf) for what in ("second region per wave", "second round of quads") for ovf in (False, True)}
    print("%d calls, %d forms:\n" % (calls, len(seen)) + "\n".join(str(f) for f in sorted(seen, key=str)))
    assert not want - seen, sorted(want - seen, key=str)
