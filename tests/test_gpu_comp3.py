"""katgpu_comp3 -- k_comp3_pass1<W>, k_comp3_pass3 -- and the k = 32 tails of k_comp and k_comp_join (kat_amd/csrc/kg_reduce.hip) at
their edges, against two witnesses: the model of tests/comp_model.py and the oracle.

What the cases reach (tests/test_comp_model.py asserts it from the model): the third table's count deciding ends / middle / mixed,
in and beside the 64 x 64 LDS tile, both column clamps, probes that only hit when canonicalised and only when not, side-table counts
in each of the three tables, the all-ones 32-mer in each table (the virtual slot `cap`, the join's one-lane tail, table_get's short
cut, poly-A found through the canonicalised probe), empty and new tables, table 3 on a grid of its own.  A child per layout and
hook set (tests/comp3_case.py: the hooks are read when the library loads) compares every result exactly and every call's "reducer
form:" trace lines with the model's dispatch; test_every_form_was_seen asserts the union over the runs.

The records and both witnesses' results are made once per module, on the CPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import comp_model as cm
from tests.test_gpu_reducer_forms import sparse

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
COMMON = {"KATGPU_TESTING": "1", "KATGPU_TRACE": "1", "KATGPU_TEST_REGION_SLOTS": str(cm.REGION_SLOTS)}
NAMES = ("main", "ends", "middle", "mixed", "counters", "spectra")
SEEN = {}


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    d = tmp_path_factory.mktemp("comp3")
    for la in cm.LAYOUTS:
        for case in cm.cases(la.name):
            out = {}
            for t, rec in enumerate(cm.records(case)):
                out["rec%d_hi" % (t + 1)] = np.array([key >> 64 for key, _ in rec], np.uint64)
                out["rec%d_lo" % (t + 1)] = np.array([key & cm.M64 for key, _ in rec], np.uint64)
                out["rec%d_counts" % (t + 1)] = np.array([c for _, c in rec], np.uint64)
            out["ones"] = np.array([cm.table_of(rec).get(cm.ALL_ONES, 0) if la.k == 32 else 0 for rec in cm.records(case)], np.uint64)
            for i, (_, m3, o3, m2, o2) in enumerate(cm.witnesses(case)):
                for who, r3, r2 in (("model", m3, m2), ("oracle", o3, o2)):
                    for name, a in zip(NAMES, r3):
                        if name == "counters":
                            out["%s_%d_counters" % (who, i)] = a
                        else:
                            sparse(out, "%s_%d_%s" % (who, i, name), a)
                    out["%s_%d_comp_counters" % (who, i)] = r2[1]
            np.savez(d / ("%s-%s.npz" % (la.name, case.name)), **out)
    return str(d)


@pytest.mark.parametrize("name,hooks", cm.RUNS, ids=["-".join([name] + [h[7:].lower() for h in hooks]) for name, hooks in cm.RUNS])
def test_comp3_matches_model_and_oracle(reference, name, hooks):
    env = dict(os.environ, **COMMON, **cm.LAYOUT[name].hooks, **hooks)
    r = subprocess.run([sys.executable, os.path.join(HERE, "comp3_case.py"), reference, name], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "comp3 cases ok: " + name in r.stdout, "exit %d\n" % r.returncode + r.stdout[-3000:] + r.stderr[-6000:]
    print(r.stdout)
    line = next(x for x in r.stdout.splitlines() if x.startswith("forms seen: "))
    SEEN[name, tuple(hooks)] = {tuple(f) for f in json.loads(line[len("forms seen: "):])}


def test_every_form_was_seen():
    """The union over the runs above: every form of the "reducer form: comp" line these layouts reach, comp3 on every slot layout
    with side-table counts in none and in each of the tables, the slot-less key in every place that looks for it."""
    assert set(SEEN) == {(name, tuple(hooks)) for name, hooks in cm.RUNS}, "a run above failed"
    seen = set().union(*SEEN.values())
    want = {("comp",) + f for f in cm.REACHABLE_COMP_FORMS}
    want |= {("comp", "join tail of pass 1 with the all-ones key"), ("comp", "virtual slot of pass 1 with the all-ones key"),
             ("comp3", "virtual slot of pass 1 with the all-ones key"), ("comp3", "virtual slot of pass 3 with the all-ones key")}
    want |= {("comp3", layout, "side tables " + t) for layout in ("kv12", "packed", "wide") for t in ("", "1", "2", "3")}
    want |= {("comp3", "rounds of pass %d" % p, n) for p in (1, 3) for n in (1, 2)}
    print("\n".join(str(f) for f in sorted(seen, key=str)))
    assert not want - seen, sorted(want - seen, key=str)
