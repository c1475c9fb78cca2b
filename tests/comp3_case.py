"""Run in a subprocess by tests/test_gpu_comp3.py with KATGPU_* hooks in the environment: katgpu_comp3 and katgpu_comp on the tables of
one layout of tests/comp_model.py (crafted records through merge_host / merge_host_wide), every argument tuple of every case, every
result equal to both the model's and the oracle's (made once by the parent: argv[1]).  Every call's "reducer form:" trace lines must
name what the model's dispatch says; the forms seen are printed for the parent's coverage check.

argv: the reference directory, then the layout to run."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kat_amd  # noqa: E402
from tests import comp_model as cm  # noqa: E402
from tests.reducer_forms_case import Trace, dense  # noqa: E402

HOOKS = {h: os.environ[h] for h in ("KATGPU_NO_PACKED", "KATGPU_NO_JOIN", "KATGPU_NO_FUSED", "KATGPU_NO_SEEN", "KATGPU_NO_FOLD", "KATGPU_TEST_LAZY_MIN_SLOTS") if h in os.environ}
assert int(os.environ["KATGPU_TEST_REGION_SLOTS"]) == cm.REGION_SLOTS
NAMES = ("main", "ends", "middle", "mixed", "counters", "spectra")


def fields(words):
    return {w.split("=")[0]: w.split("=")[1] for w in words if "=" in w}


def make_table(eng, la, canonical, hint, ref, t, like=None):
    tab = eng.table(la.k, canonical, size_hint=hint, like=like if la.k <= 32 else None)
    hi, lo, counts = (ref["rec%d_%s" % (t, x)] for x in ("hi", "lo", "counts"))
    if counts.size:
        if la.k > 32:
            tab.merge_host_wide(hi, lo, counts)
        else:
            tab.merge_host(lo, counts)
    n_regions, cbits = cm.geometry(la, hint, HOOKS)
    assert tab.slot_bytes() == (20 if la.k > 32 else 8 if cbits else 12), (la.name, t, tab.slot_bytes())
    st = tab.stats(want_total=False)
    assert (st["capacity"], tab.regrows, st["distinct"]) == (n_regions * cm.REGION_SLOTS, 0, counts.size), (la.name, t, st, tab.regrows)
    return tab, st["capacity"]


def expected(ref, who, i, name, shape):
    if name == "counters":
        return ref["%s_%d_counters" % (who, i)]
    return dense(ref, "%s_%d_%s" % (who, i, name), shape)


def run_case(eng, trace, refdir, la, case, seen):
    ref = np.load(os.path.join(refdir, "%s-%s.npz" % (la.name, case.name)))
    n_calls = 0
    for like in case.likes:
        t1, cap1 = make_table(eng, la, case.strands[0], case.hints[0], ref, 1)
        t2, _ = make_table(eng, la, case.strands[1], cm.hint2(case, like), ref, 2, like=t1 if like else None)
        t3, cap3 = make_table(eng, la, case.strands[2], case.hints[2], ref, 3)
        if la.k <= 32:
            g1, g2, g3 = t1.geometry(), t2.geometry(), t3.geometry()
            assert ((g1.p1, g1.p2) == (g2.p1, g2.p2)) == like and (g3.p1, g3.p2) != (g1.p1, g1.p2), (case.name, like)     # table 3's grid is never table 1's
        cbits1 = cm.geometry(la, case.hints[0], HOOKS)[1]
        want_forms = cm.comp_forms(la, case.strands, like, HOOKS, cbits1)
        ones = [int(ref["ones"][t]) for t in range(3)]
        trace.take()
        for i, args in enumerate(cm.ARGS):
            d1b, d2b = args[2:]
            shapes = {"main": (d1b, d2b), "ends": (d1b, d2b), "middle": (d1b, d2b), "mixed": (d1b, d2b), "counters": (13,), "spectra": (4, min(d1b, d2b))}
            got3 = kat_amd.comp3(t1, t2, t3, *args)
            lines = trace.take()
            assert [w[0] for w in lines] == ["comp", "comp3"], lines
            got2 = kat_amd.comp(t1, t2, *args)
            lines += trace.take()
            assert [w[0] for w in lines] == ["comp", "comp3", "comp"], lines
            for words in (lines[0], lines[2]):
                f = fields(words)
                assert (f["pass1"], f["pass2"]) == want_forms, (case.name, like, words, want_forms)
                assert (int(f["pk"]), int(f["wide"]), int(f["fold"])) == (int(cbits1 != 0), int(la.k > 32), cm.fold(args, HOOKS)), (case.name, words)
                assert (int(f["n_ovf1"]) != 0, int(f["n_ovf2"]) != 0) == cm.side_tables(case)[:2] and (int(f["ones1"]), int(f["ones2"])) == tuple(ones[:2]), (case.name, words)
                seen.add(("comp", f["pass1"], f["pass2"]))
                if la.slot_bytes == 12 and f["pass1"] == "join" and ones[0]:
                    seen.add(("comp", "join tail of pass 1 with the all-ones key"))
                if la.k == 32 and f["pass1"] == "probe" and ones[0]:
                    seen.add(("comp", "virtual slot of pass 1 with the all-ones key"))
            f = fields(lines[1])
            assert tuple(int(f["n_ovf%d" % t]) != 0 for t in (1, 2, 3)) == cm.side_tables(case), (case.name, lines[1])
            assert (int(f["wide"]), int(f["ones1"]), int(f["ones3"])) == (int(la.k > 32), ones[0], ones[2]), (case.name, lines[1])
            grid1, grid3 = int(f["grid1"]), int(f["grid3"])
            assert 1 <= grid1 <= -(-(cap1 + 1) // 256) and 1 <= grid3 <= -(-(cap3 + 1) // 256), (case.name, lines[1])
            rounds1, rounds3 = -(-(cap1 + 1) // (grid1 * 256)), -(-(cap3 + 1) // (grid3 * 256))
            seen.add(("comp3", "wide" if la.k > 32 else "packed" if cbits1 else "kv12", "side tables " + "".join(str(t + 1) for t in range(3) if cm.side_tables(case)[t])))
            seen.add(("comp3", "rounds of pass 1", min(rounds1, 2)))
            seen.add(("comp3", "rounds of pass 3", min(rounds3, 2)))
            if ones[0]:
                seen.add(("comp3", "virtual slot of pass 1 with the all-ones key"))
            if ones[2]:
                seen.add(("comp3", "virtual slot of pass 3 with the all-ones key"))
            for who in ("model", "oracle"):
                for name, got in zip(NAMES, got3):
                    assert np.array_equal(got, expected(ref, who, i, name, shapes[name])), (la.name, case.name, like, args, who, name)
                cc2 = ref["%s_%d_comp_counters" % (who, i)]
                for name, got, want in zip(("main", "counters", "spectra"), got2, (expected(ref, who, i, "main", shapes["main"]), cc2, expected(ref, who, i, "spectra", shapes["spectra"]))):
                    assert np.array_equal(got, want), (la.name, case.name, like, args, who, "comp " + name)
            n_calls += 2
        for t in (t1, t2, t3):
            t.free()
    return n_calls


def run_new_tables(eng, la):
    """comp3 and comp as the very first calls on new tables (under KATGPU_TEST_LAZY_MIN_SLOTS=1 a packed one is still uncleared)."""
    for first in ("comp3", "comp"):
        t1 = eng.table(la.k, True, size_hint=cm.HINT1)
        t2 = eng.table(la.k, True, size_hint=cm.HINT1, like=t1 if la.k <= 32 else None)
        t3 = eng.table(la.k, True, size_hint=cm.HINT3)
        cbits = cm.geometry(la, cm.HINT1, HOOKS)[1]
        assert t1.slot_bytes() == (20 if la.k > 32 else 8 if cbits else 12)
        out = kat_amd.comp3(t1, t2, t3, 1.0, 1.0, 201, 101) if first == "comp3" else kat_amd.comp(t1, t2, 1.0, 1.0, 201, 101)
        assert not any(a.any() for a in out), first
        out = kat_amd.comp(t1, t2, 0.5, 0.5, 300, 130) if first == "comp3" else kat_amd.comp3(t1, t2, t3, 0.5, 0.5, 300, 130)
        assert not any(a.any() for a in out), first
        for t in (t1, t2, t3):
            t.free()
    return 4


def main():
    refdir, name = sys.argv[1], sys.argv[2]
    la = cm.LAYOUT[name]
    assert all(os.environ.get(h) == v for h, v in la.hooks.items()), la
    trace = Trace()
    done = False
    t0 = time.time()
    try:
        eng = kat_amd.Engine(0)
        seen = set()
        n = run_new_tables(eng, la)
        for case in cm.cases(name):
            n += run_case(eng, trace, refdir, la, case, seen)
        done = True
    finally:
        trace.restore(show=not done)
    print("forms seen: " + json.dumps(sorted((list(f) for f in seen), key=str)))
    print("comp3 cases ok: %s, %d cases, %.1f s, %d calls" % (name, len(cm.cases(name)), time.time() - t0, n))


if __name__ == "__main__":
    main()
