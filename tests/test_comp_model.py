"""The model of tests/comp_model.py against the oracle on every case of its lists, integer for integer, and the conditions under which
the cases reach every branch of k_comp3_pass1, k_comp3_pass3 and the k = 32 tails of k_comp / k_comp_join -- computed from the model
alone, and asserted: the device test (tests/test_gpu_comp3.py) runs the same cases."""
import numpy as np
import pytest

from tests import comp_model as cm

NAMES = ("main", "ends", "middle", "mixed", "counters", "spectra")
TILE = cm.COMP_TILE


@pytest.mark.parametrize("name", [la.name for la in cm.LAYOUTS])
def test_model_matches_oracle(name):
    for case in cm.cases(name):
        for args, m3, o3, m2, o2 in cm.witnesses(case):
            for what, a, b in zip(NAMES, m3, o3):
                assert a.shape == b.shape and np.array_equal(a, b), (case.name, args, what)
            for what, a, b in zip(("main", "counters", "spectra"), m2, o2):
                assert a.shape == b.shape and np.array_equal(a, b), (case.name, args, "comp " + what)
            # the three-input form restates the two-input one, and adds counters 2 and 5
            assert np.array_equal(m2[0], m3[0]) and np.array_equal(m2[2], m3[5])
            rest = [i for i in range(13) if i not in (cm.H3_TOTAL, cm.H3_DISTINCT)]
            assert np.array_equal(m2[1][rest], m3[4][rest]) and not m2[1][[cm.H3_TOTAL, cm.H3_DISTINCT]].any()
            recs = cm.records(case)
            t3 = cm.table_of(recs[2])
            assert (int(m3[4][cm.H3_TOTAL]), int(m3[4][cm.H3_DISTINCT])) == (sum(t3.values()), len(t3))
            if case.empty == 1:                                     # every matrix zero; counters 2 and 5 still set
                assert not any(m.any() for m in m3[1:4]) and m3[4][cm.H3_DISTINCT] > 0
            if case.empty == 3:
                assert m3[4][cm.H3_DISTINCT] == 0 and not m3[3].any()          # nothing is "mixed" without a count in 3


def strand_cases(name):
    return [c for c in cm.cases(name) if c.name.startswith("strands-")]


def kmers(case, args):
    recs = cm.records(case)
    return list(cm.comp3_kmers(recs[0], recs[1], recs[2], cm.LAYOUT[case.layout].k, case.strands[1], case.strands[2], *args))


@pytest.mark.parametrize("name", [la.name for la in cm.LAYOUTS])
def test_cases_reach_every_branch_of_pass1(name):
    d1_bins, d2_bins = cm.REACH_ARGS[2:]
    assert d1_bins > TILE and d2_bins > TILE
    for case in strand_cases(name):
        ms = kmers(case, cm.REACH_ARGS)
        quadrants = lambda which: {(m.s1 >= TILE, m.s3 >= TILE) for m in ms if m.which == which}
        assert len(quadrants(0)) == 4 and len(quadrants(2)) == 4, (case.name, quadrants(0), quadrants(2))      # ends, mixed: in the tile, beside it, below it, beyond both
        assert {m.s1 >= TILE for m in ms if m.which == 1} == {False, True}, case.name                           # middle (column 0): rows in and below the tile
        # ends only because the clamp makes s2 and s3 equal
        assert any(m.which == 0 and m.u2 != m.u3 and m.c2 and m.c3 for m in ms), case.name
        # both clamps bind
        assert any(m.u1 >= d1_bins for m in ms) and any(m.u3 >= d2_bins for m in ms) and any(m.u2 >= d2_bins for m in ms), case.name
        # the s3 > 0 branch both ways among the k-mers whose s2 and s3 differ
        assert {m.s3 > 0 for m in ms if m.s2 != m.s3} == {False, True}, case.name
        # ends only because the scale makes s2 and s3 equal (3 and 4 at 0.5), below every clamp
        half = kmers(case, cm.HALF_ARGS)
        assert any(m.which == 0 and m.c2 != m.c3 and m.u2 == m.u3 < cm.HALF_ARGS[3] - 1 for m in half), case.name
        # the clamp lands exactly on the tile's edge: column 63 (64 bins) and column 64 (65 bins), row 63 and row 64
        for args in (cm.ARGS[2], cm.ARGS[3]):
            e = kmers(case, args)
            assert any(m.u1 >= args[2] for m in e) and any(m.u3 >= args[3] for m in e), (case.name, args)
            assert {(m.s1 >= TILE, m.s3 >= TILE) for m in e} == ({(False, False), (False, True)} if args[3] > TILE else {(False, False), (True, False)}), (case.name, args)


def probes(case):
    """Every probe the comparison makes: (the stored key it starts from, the table it looks into, is the probe canonicalised?)."""
    la = cm.LAYOUT[case.layout]
    recs = cm.records(case)
    t = [cm.table_of(r) for r in recs]
    _, canon2, canon3 = case.strands
    for key in t[0]:
        yield key, t[1], canon2, la.k
        yield key, t[2], canon3, la.k
    for key in t[1]:
        yield key, t[0], True, la.k


@pytest.mark.parametrize("name", [la.name for la in cm.LAYOUTS])
def test_cases_tell_canonicalised_probes_from_plain_ones(name):
    """A k-mer that a probe finds only when canonicalised, and one it finds only when not, wherever the strands allow one.
    "Only when canonicalised" needs a stored key that is not canonical, so a non-canonical table among the three: table 1 (passes 1
    and 3) or table 2 (pass 2).  "Only when not" needs the probed table to hold a non-canonical key as well: table 1 and one of the
    others non-canonical.  With all three canonical every stored key is its own canonical form and the two probes are one."""
    for case in strand_cases(name):
        s1, s2, s3 = case.strands
        only_canonical = only_plain = 0
        differ_taken = 0
        for key, table, canon, k in probes(case):
            plain, can = table.get(key, 0), table.get(cm.canonical(key, k), 0)
            only_canonical += bool(can and not plain)
            only_plain += bool(plain and not can)
            differ_taken += bool((can != plain) and (can if canon else plain))          # the probe the library must make decides the hit
        assert (only_canonical > 0) == (not (s1 and s2)), (case.name, only_canonical)
        assert (only_plain > 0) == (not s1 and not (s2 and s3)), (case.name, only_plain)
        if not (s1 and s2 and s3):
            assert differ_taken > 0, case.name
        for rec, canon in zip(cm.records(case), case.strands):                            # a canonical table gets canonical keys
            assert not canon or all(key == cm.canonical(key, k) for key, _ in rec), case.name
    if cm.LAYOUT[name].k % 2 == 0:
        k = cm.LAYOUT[name].k
        pal = cm.palindromes(k)
        assert len(pal) >= 3 and all(cm.revcomp(x, k) == x for x in pal)
        assert all(x in cm.table_of(cm.records(c)[0]) for c in strand_cases(name) for x in pal)


@pytest.mark.parametrize("name", [la.name for la in cm.LAYOUTS])
def test_side_table_and_all_ones_cases(name):
    la = cm.LAYOUT[name]
    by_name = {c.name: c for c in cm.cases(name)}
    plain = cm.records(by_name["strands-" + cm.strand_name(cm.base_strands(la))])
    for case in (c for c in cm.cases(name) if c.side):
        recs = cm.records(case)
        t = case.side - 1
        cbits = cm.cbits_of(case, case.side, case.likes[0], la.hooks)
        limit = (1 << (cbits - 1)) if cbits else (1 << 32) - 1              # what a slot keeps by itself (kg_device.hpp: table_add_pk)
        over = [c for _, c in recs[t] if c > limit]
        assert len(over) >= 3 and max(over) == (1 << 53) + 1, (case.name, over)
        for u in range(3):                                                   # the other tables are unchanged, and stay inside their slots
            if u != t:
                assert recs[u] == plain[u], (case.name, u)
        # the large counts are seen: as s1, or through a probe that finds them
        ms = kmers(case, cm.REACH_ARGS)
        assert sum((m.c1, m.c2, m.c3)[t] > limit for m in ms) == len(over), case.name
    for case in cm.cases(name):
        if not case.side:
            for t, rec in enumerate(cm.records(case)):
                cbits = cm.cbits_of(case, t + 1, True, la.hooks)
                cbits = min(cbits, cm.cbits_of(case, t + 1, False, la.hooks)) if cbits else 0
                assert all(c <= ((1 << (cbits - 1)) if cbits else (1 << 32) - 1) for _, c in rec), (case.name, t)
        assert max(float(c) * 4.0 for rec in cm.records(case) for _, c in rec or [(0, 0)]) < 2.0 ** 63      # (the reference's cast is undefined beyond)
    if la.k == 32:
        seen = set()
        for case in (c for c in cm.cases(name) if any(c.ones)):
            assert not case.strands[0]
            recs = [cm.table_of(r) for r in cm.records(case)]
            seen.add(tuple(bool(r.get(cm.ALL_ONES)) for r in recs))
            assert {r.get(cm.ALL_ONES, 0) for r in recs} <= {0} | set(cm.ONES_COUNTS)
        assert {(True, False, False), (False, True, False), (False, False, True), (True, True, True)} <= seen
        # poly-T in table 1, poly-A in a canonical table: the canonicalised probe finds it
        for cname, t in (("polya-2", 1), ("polya-3", 2)):
            case = by_name[cname]
            assert case.strands[t] and not case.strands[0]
            (m,) = [m for m in kmers(case, cm.REACH_ARGS) if m.key == cm.ALL_ONES]
            assert (m.c2, m.c3)[t - 1] == case.polya[t] > 0 and cm.canonical(cm.ALL_ONES, 32) == 0
    else:
        assert not any(any(c.ones) or any(c.polya) for c in cm.cases(name))


def test_dispatch_reaches_every_form():
    """The forms the cases can reach under the hook sets of tests/test_gpu_comp3.py, by the model of katgpu_comp's choice."""
    seen = set()
    for name, hooks in cm.RUNS:
        la = cm.LAYOUT[name]
        env = dict(la.hooks, **hooks)
        for case in cm.cases(name):
            for like in case.likes:
                seen.add(cm.comp_forms(la, case.strands, like, env, cm.geometry(la, case.hints[0], env)[1]))
    assert seen == cm.REACHABLE_COMP_FORMS, seen ^ cm.REACHABLE_COMP_FORMS
