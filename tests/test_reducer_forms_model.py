"""tests/reducer_forms_model.py against the oracle, on the CPU: for every table and argument of the reducer-form cases the model's
histogram and GC matrix equal those of ko.Table / ko.WideTable filled by add (so that on the device the model is a second,
independent witness), the sums are the distinct counts, and the case lists hold the edges they are named for -- an edit to the lists
cannot lose one quietly."""
import numpy as np
import pytest

from oracle import koracle as ko
from tests import reducer_forms_model as rf

TABLES = [(la.name, twin) for la in rf.LAYOUTS for twin in ("a", "b")]


def oracle_table(name, twin):
    """The oracle's table of a case: every record through add, the stream through the oracle's own counting."""
    la = rf.LAYOUT[name]
    o = (ko.WideTable if la.k > 32 else ko.Table)(la.k, False)
    for key, c in rf.crafted(name)[twin]:
        o.add(key, c)
    return o.count_bases(rf.stream())


@pytest.fixture(scope="module")
def tables():
    return {(name, twin): (oracle_table(name, twin), rf.Multiset(rf.LAYOUT[name].k, rf.records(name, twin))) for name, twin in TABLES}


def expected_cbits(la):
    return rf.table_geometry(la.k, la.size_hint, la.region_slots)[1]


@pytest.mark.parametrize("name,twin", TABLES)
def test_model_equals_oracle(tables, name, twin):
    o, m = tables[name, twin]
    k = rf.LAYOUT[name].k
    assert m.distinct == o.distinct
    dropped = int((m.gc == k).sum())
    assert dropped >= 1                                                   # the all-G k-mer
    for low, high, inc in rf.HIST_TRIPLES:
        base, ceil, nb = rf.hist_geometry(low, high)
        assert (base, ceil, nb) == ko.hist_geometry(low, high)
        h = rf.hist_model(m, base, ceil, inc, nb)
        assert np.array_equal(h, o.hist(low, high, inc)), (low, high, inc)
        assert int(h.sum()) == m.distinct
    for scale, bins in rf.gcp_args(k, twin):
        g = rf.gcp_model(m, k, scale, bins)
        assert np.array_equal(g, o.gcp(scale, bins)), (scale, bins)
        assert int(g.sum()) == m.distinct - dropped
        assert max(m.table.values()) * scale < 2.0 ** 63                  # (the reference's cast is undefined beyond)


def test_models_take_plain_record_lists():
    """... with a key that comes twice, at both key widths, next to the oracle; the vector column is the scalar one."""
    for k, table in ((32, ko.Table), (63, ko.WideTable)):
        top = (1 << (2 * k)) - 1
        recs = [(0, 1), (top, 5), (top - 1, 1 << 40), (int("10" * k, 2), 9), (0, 2), (12345, (1 << 53) + 1)]
        o = table(k, False)
        for key, c in recs:
            o.add(key, c)
        assert np.array_equal(rf.hist_model(recs, 2, 7, 2, 6), o.hist(3, 6, 2))
        for scale in (1.0, 0.37, 1000.0):
            assert np.array_equal(rf.gcp_model(recs, k, scale, 50), o.gcp(scale, 50))
    for scale in (1.0, 0.37, 0.5, 3.0, 1000.0, 5000.0):
        for c in rf.edge_counts(27) + [(1 << 32) - 1, 1 << 32, (1 << 40) + 3]:
            for bins in (100, 1000):
                col = int(np.minimum(np.ceil(np.float64(np.uint64(c)) * np.float64(scale)), float(bins)))
                assert col == rf.column(c, scale, bins)
    assert rf.column(0, 0.37, 10) == 0 and rf.column(1, 0.37, 10) == 1 and rf.column(2001, 0.5, 1000) == 1000 and rf.column(1999, 0.5, 1000) == 1000
    assert rf.gc_count(int("10" * 51, 2), 51) == 51 and rf.gc_count((1 << 102) - 1, 51) == 0 and rf.gc_count(0b0110, 2) == 2


def test_layouts_are_what_they_are_named_for():
    geo = {la.name: rf.table_geometry(la.k, la.size_hint, la.region_slots) for la in rf.LAYOUTS}
    assert geo["kv12"][1] == 0 and rf.LAYOUT["kv12"].k == 32
    assert geo["pk32"][1] == 32
    assert 20 <= geo["pk22"][1] <= 22 and geo["pk22"][0] >= 1 << 10
    assert geo["pkmany"][0] > rf.MANY_REGIONS and geo["pkmany"][1]
    assert rf.LAYOUT["pk512"].region_slots // 4 > 64 and geo["pk512"][1]                    # more quads per region than a wave has lanes
    assert rf.LAYOUT["wide"].k > 32 and geo["wide"][1] == 0
    for la in rf.LAYOUTS:
        assert la.slot_bytes == (20 if la.k > 32 else 8 if geo[la.name][1] else 12)
        assert rf.table_geometry(la.k, la.size_hint, la.region_slots, packed=False)[1] == 0
        assert la.region_slots == (512 if la.name == "pk512" else rf.REGION_SLOTS)
        # the table does not grow under the cases' records (the fill limit of small regions, kg_table.hip: load_limit): its count bits stay
        starts = rf.stream().size + rf.N_CRAFTED + 8
        assert starts <= max(0.25, 0.7 - 3.0 / la.region_slots ** 0.5) * la.size_hint


def test_hist_edges_are_hit():
    """Per triple and table: k-mers below the base, on it, on both sides of the first bucket's end, on the ceiling and above it, and in
    the last LDS bucket and the first global one."""
    kinds = set()
    for name, twin in TABLES:
        m = rf.Multiset(None, rf.crafted(name)[twin])
        have = set(int(c) for c in m.counts)
        for low, high, inc in rf.HIST_TRIPLES:
            base, ceil, nb = rf.hist_geometry(low, high)
            lb = rf.hist_lds_bins(nb)
            want = {base, base + inc - 1, base + inc, ceil, ceil + 1}
            if base > 1:
                want.add(base - 1)
            assert want <= have, (name, twin, low, high, inc, sorted(want - have))
            h = rf.hist_model(m, base, ceil, inc, nb)
            assert h[0] and h[nb - 1]
            if nb > lb and base + inc * lb <= ceil:                        # either side of the LDS / global boundary
                assert h[lb] and h[lb - 1], (name, low, high, inc)
                assert base + inc * lb - 1 in have and base + inc * lb in have
                kinds.add("boundary")
            elif nb > lb:                                                  # (inc > 1: the buckets from (ceil - base) // inc + 1 on stay empty but for the last,
                assert (ceil - base) // inc < lb - 1 and inc > 1           # which is a global one; no count can land on the boundary)
                kinds.add("global catch-all")
            else:
                assert h[lb - 1]                                           # all in LDS: the catch-all is the last LDS bucket
                kinds.add("lds")
    assert kinds == {"boundary", "global catch-all", "lds"}
    nbs = [rf.hist_geometry(lo, hi)[2] for lo, hi, _ in rf.HIST_TRIPLES]
    assert nbs[:3] == [16383, 16384, 16385] and [rf.hist_lds_bins(nb) for nb in nbs[:3]] == [16383, 16384, 16384] and 3 in nbs


def test_gcp_args_sit_on_the_thresholds():
    exact = {32: [511, 512, 599, 600, 1199, 1200], 15: [None, None, 1279, 1280, 2559, 2560]}
    for la in rf.LAYOUTS:
        k = la.k
        tb = rf.threshold_bins(k)
        for i, t in enumerate(rf.THRESHOLDS):
            under, over = rf.gcp_lds(k, tb[2 * i]), rf.gcp_lds(k, tb[2 * i + 1])
            assert under <= t < over and over - under == 4 * k             # the nearest pair on either side
            if t % (4 * k) == 0:
                assert under == t
        for i, b in enumerate(exact.get(k, [])):
            assert b is None or tb[i] == b
        for twin in ("a", "b"):
            args = rf.gcp_args(k, twin)
            for plain in (True, False):
                forms = [rf.dispatch(k, la.slot_bytes, bins, plain) for _, bins in args]
                assert {f.use_lds for f in forms} == {0, 2 if plain else 1}
                assert {f.per_cu for f in forms if f.use_lds} == {1, 2}
                assert any(f.use_lds and f.lds <= rf.LDS_ATTR for f in forms) and any(f.use_lds and f.lds > rf.LDS_ATTR for f in forms)
            for b in tb:
                assert (1.0, b) in args and any(s != 1.0 and bb == b for s, bb in args)
            assert {s for s, _ in args} == set(rf.SCALES) | {rf.BIG_SCALE[twin]}
            assert {s for s, b in args if b == rf.GLOBAL_BINS} >= {1.0, 0.37, 0.5, rf.BIG_SCALE[twin]}
    assert sorted(rf.gcp_lds(32, b) for b in (511, 599, 1199)) == list(rf.THRESHOLDS)
    assert rf.dispatch(32, 12, 1199, True) == rf.Form("flat", 2, 1, 153600) and rf.dispatch(32, 12, 1200, True) == rf.Form("flat", 0, 2, 153728)
    assert rf.dispatch(15, 8, 1279, False) == rf.Form("pk", 1, 2, 76800) and rf.dispatch(15, 8, 1280, False).per_cu == 1
    assert rf.dispatch(51, 20, 320, True).lds <= 65536 < rf.dispatch(51, 20, 321, True).lds


def test_counts_and_keys_of_the_twins():
    for la in rf.LAYOUTS:
        cbits = expected_cbits(la)
        limit = rf.limit_in_slot(cbits)
        a, b = (rf.Multiset(la.k, rf.records(la.name, twin)) for twin in ("a", "b"))
        assert a.keys == b.keys                                               # twins: the same keys
        ca, cb = set(int(c) for c in a.counts), set(int(c) for c in b.counts)
        assert max(ca) == limit and limit - 1 in ca                           # twin a: everything stays in the slot, under either layout
        assert limit <= (1 << 32) - 1
        want_b = {(1 << 32) - 1, 1 << 32, (1 << 40) + 3, (1 << 53) + 1}
        if cbits:
            want_b |= {limit + 1, (1 << cbits) - 1, 1 << cbits}
        assert want_b <= cb
        sp = rf.special_keys(la.k)
        assert [rf.gc_count(sp[n], la.k) for n in ("all_a", "gc1", "gc_k_minus_1", "all_g")] == [0, 1, la.k - 1, la.k]
        assert all(key in a.table for key in sp.values())
        assert b.table[sp["gc_k_minus_1"]] > 1 << 32                          # a row found for a count that lies in the side table
        # scale 0.5 on even and odd counts around twice the bins: exactly integral products at the last columns
        assert set(range(2 * rf.HALF_BINS - 3, 2 * rf.HALF_BINS + 2)) <= ca
        # the large scale takes a count below 2^32 beyond 2^32
        for twin, cs in (("a", ca), ("b", cb)):
            assert any(c < 1 << 32 and c * rf.BIG_SCALE[twin] > 1 << 32 for c in cs)
        if la.k == 32:
            ones = sp["all_ones"]
            assert ones == (1 << 64) - 1 and rf.gc_count(ones, 32) == 0
            seen = set()
            for table in (a, b):
                c = table.table[ones]
                for low, high, _ in rf.HIST_TRIPLES:
                    base, ceil, _ = rf.hist_geometry(low, high)
                    seen.add("below" if c < base else "above" if c > ceil else "inside")
            assert seen == {"below", "inside", "above"}
            assert any(inc > 1 and rf.hist_geometry(lo, hi)[0] <= b.table[ones] <= hi for lo, hi, inc in rf.HIST_TRIPLES)
    # no crafted key of twin a can meet a k-mer of the stream and leave its slot, but the special ones, whose counts are small
    for la in rf.LAYOUTS:
        crafted = {key for key, _ in rf.crafted(la.name)["a"]} - set(rf.special_keys(la.k).values())
        assert not crafted & {key for key, _ in rf.stream_records(la.k)}


def test_reachable_forms():
    f = rf.reachable_forms({8, 12, 20}, True)
    assert len(f) == 24 and ("gcp", "pk", 2, False) in f and ("gcp", "pk", 0, True) in f and ("hist", "wide", "global", True) in f
    assert {x[2] for x in rf.reachable_forms({12, 20}, False) if x[0] == "gcp"} == {0, 1}
