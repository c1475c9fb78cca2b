"""tests/partition_forms.py on its own, without a GPU: its restatement of the partitioned counter's dispatch reaches exactly the labels
written down here by hand, its case table covers them, and every case is one the device test can rely on (the label it claims, every k,
both strand modes, a table that does not grow in mid-call)."""
import numpy as np
import pytest

from tests import partition_forms as pf

# Every reachable "<level 1> <items> hb <hb> <layout>", from reading kg_count.hip (plan_level1, launch_l2_hb, launch_apply) and kg_table.hip
# (alloc_dev_table) -- not from the model.  With p2 = 2^l2 <= 1024 the power of two >= sqrt(regions), p1 <= p2 (and > p2 / 4 beyond two
# regions), n1 = 2k - floor(log2 p1), rb = n1 - l2; packed iff rb <= 44 and more than one region:
LABELS = {
    # the block edition: lean, p1 <= 512, 41 <= n1 <= 47, so rb = 31 .. 47 (31 takes l2 = 10: a 257 .. 511 x 1024 grid at k = 24 .. 25) -- and
    # rb >= 45 only where l2 <= 2: a dozen regions
    "Blocks Blocks hb 0 packed", "Blocks Blocks hb 1 packed", "Blocks Blocks hb 2 packed", "Blocks Blocks hb 2 KV12",
    # the lean sweep, p1 <= 512: groups are n1 = 32 .. 40, rb <= 38; wide groups n1 >= 48, rb >= 38
    "Lean512 Groups hb 0 packed", "Lean512 Groups hb 1 packed",
    "Lean512 WideGroups hb 1 packed", "Lean512 WideGroups hb 2 packed", "Lean512 WideGroups hb 2 KV12", "Lean512 WideGroups hb 4 KV12",
    # the lean sweep, p1 > 512: l2 = 10 and n1 = 2k - 9 = 33 .. 53 (k = 21 .. 31), rb = 23 .. 43: always packed
    "Lean1024 Groups hb 0 packed", "Lean1024 Groups hb 1 packed", "Lean1024 WideGroups hb 1 packed", "Lean1024 WideGroups hb 2 packed",
    # the plain sweep, p1 > 512: k <= 20 (n1 = 2k - 9 < 32) or k = 32 (n1 = 55, or 54 at p1 = 1024: rb = 45 or 44)
    "Plain1024 Groups hb 0 packed", "Plain1024 WideGroups hb 2 packed", "Plain1024 WideGroups hb 2 KV12",
    # the plain sweep, p1 <= 512: n1 < 32 (groups, rb <= 31) or k = 32 (n1 >= 55, rb >= 45) -- and a table of one level-1 digit (one or two regions:
    # n1 = 2k is no less than 2k, never lean), whose remainder has 2k or 2k - 1 bits: anything
    "Plain512 Groups hb 0 packed", "Plain512 WideGroups hb 2 KV12", "Plain512 WideGroups hb 4 KV12",
    "Plain512 Groups hb 0 KV12", "Plain512 Groups hb 1 KV12", "Plain512 Groups hb 2 KV12", "Plain512 Groups hb 1 packed", "Plain512 Groups hb 2 packed",
}
# KATGPU_NO_PACKED: the same level 1 and level 2 (hb no longer stops at 2, but every packed rb was <= 44 anyway) in front of the KV12 apply
LABELS_NO_PACKED = {
    "Blocks Blocks hb 0 KV12", "Blocks Blocks hb 1 KV12",
    "Lean512 Groups hb 0 KV12", "Lean512 Groups hb 1 KV12", "Lean512 WideGroups hb 1 KV12",
    "Lean1024 Groups hb 0 KV12", "Lean1024 Groups hb 1 KV12", "Lean1024 WideGroups hb 1 KV12", "Lean1024 WideGroups hb 2 KV12",
    "Plain1024 Groups hb 0 KV12",
}


@pytest.fixture(scope="module")
def reachable():
    return set(pf.enumerate_labels(False)), set(pf.enumerate_labels(True))


def test_the_model_reaches_the_hand_written_labels_and_no_other(reachable):
    natural, no_packed = reachable
    assert natural == LABELS, (sorted(natural - LABELS), sorted(LABELS - natural))
    assert all(label.endswith("KV12") for label in no_packed)
    assert no_packed - natural == LABELS_NO_PACKED, (sorted(no_packed - natural - LABELS_NO_PACKED), sorted(LABELS_NO_PACKED - (no_packed - natural)))


def test_the_grids_of_the_enumeration_are_alloc_dev_tables():
    """The enumeration's short cut through the capacities (one per grid) against every number of regions, at one region size."""
    rs, grids = 1024, set()
    for nr in range(2, (1 << 26) // rs + 1):
        p2 = 1
        while p2 * p2 < nr:
            p2 += 1                                                  # (as alloc_dev_table does it: the root, then the power of two)
        q = 1
        while q < p2:
            q *= 2
        grids.add((-(-nr // q), q))
    assert {(pf.Form(32, rs, cap).p1, pf.Form(32, rs, cap).p2) for cap in pf.grid_caps(rs, 1 << 26) if cap > rs} == grids


def test_the_table_covers_every_label():
    assert {r.label for r in pf.ROWS if not r.no_packed} == LABELS
    assert {r.label for r in pf.ROWS if r.no_packed} >= LABELS_NO_PACKED
    # ... with the segmented level 1, but for the labels that only a table of one level-1 digit reaches
    assert {r.label for r in pf.ROWS if r.seg} == (LABELS | LABELS_NO_PACKED) - pf.LABELS_SHORT_ONLY
    assert pf.LABELS_SHORT_ONLY == {"Plain512 Groups hb 1 KV12", "Plain512 Groups hb 2 KV12", "Plain512 Groups hb 1 packed", "Plain512 Groups hb 2 packed"}
    assert {r.k for r in pf.ROWS} >= set(range(12, 33))
    assert {r.canonical for r in pf.ROWS if not r.no_packed and not r.short} == {True, False}
    # the all-ones k-mer (k = 32, both strands) in packed and in KV12 slots
    assert {r.form.packed for r in pf.ROWS if r.k == 32 and not r.canonical} == {True, False}


@pytest.mark.parametrize("row", pf.ROWS, ids=repr)
def test_a_row_is_what_it_claims(row):
    f = row.form
    assert f.partitioned and f.label() == row.label, f.label()
    assert 64 <= f.region_slots <= 8192 and f.cap <= 1 << 26
    assert pf.label_of_trace(f.trace(2, 2, True)) == row.label                  # a round's trace line, and back
    assert (pf.FAST in row.settings()) == row.seg and (pf.EXACT_L1 in row.settings()) == row.short
    assert (pf.MIXED in row.settings()) == (f.blocks and row.seg and not row.no_packed)
    assert (pf.EXACT in row.settings()) == (not row.no_packed or not row.seg)


def test_every_row_runs_in_exactly_the_children_of_its_settings():
    ran = {}
    for _, env, st, rows in pf.groups():
        assert 1 <= len(rows) <= 4
        for i in rows:
            r = pf.ROWS[i]
            assert int(env["KATGPU_TEST_REGION_SLOTS"]) == r.rs and ("KATGPU_NO_PACKED" in env) == r.no_packed
            assert (int(env["KATGPU_L1_FAST"]), int(env["KATGPU_P2_FAST"])) == st
            assert int(env["KATGPU_TEST_ROUND_ITEMS"]) == (pf.ROUND_ITEMS_LONG if r.long else pf.ROUND_ITEMS)
            ran.setdefault(i, []).append(st)
    assert {i: sorted(v) for i, v in ran.items()} == {i: sorted(r.settings()) for i, r in enumerate(pf.ROWS)}
    assert len({g[0] for g in pf.groups()}) == len(pf.groups())


@pytest.fixture(scope="module")
def streams():
    s = {"stream": pf.stream(), "long": pf.stream(long=True)}
    s["short"] = np.ascontiguousarray(s["stream"][:pf.SHORT_BASES])
    return s


def test_the_streams_are_what_the_rows_need(streams):
    for which, round_items in (("stream", pf.ROUND_ITEMS), ("long", pf.ROUND_ITEMS_LONG)):
        text = streams[which].tobytes()
        assert len(text) % 16 == 5
        assert b"N" + b"A" * 3000 + b"N" + b"T" * 2000 + b"N" in text
        assert any(c in text for c in b"acgt")
        assert round_items < len(text) < 2 * round_items * 0.98                # two rounds (kg_count.hip: round_starts)
    assert 900_000 <= streams["stream"].size <= 950_000
    assert streams["short"].tobytes().isupper()


ORACLE = {}                                                                  # the oracle's (distinct, total), per (k, strand mode, stream)


def oracle(row, streams):
    from oracle import koracle as ko
    key = (row.k, row.canonical, row.which())
    if key not in ORACLE:
        o = ko.Table(row.k, row.canonical).count_bases(streams[row.which()], threads=1 if row.short else 4)
        ORACLE[key] = (o.distinct, o.total)
    return ORACLE[key]


@pytest.mark.parametrize("row", pf.ROWS, ids=repr)
def test_a_rows_table_has_room(row, streams):
    """load_limit x capacity >= distinct + window starts: what ensure_room asks before spilled k-mers go in.  A table that grows in mid-call
    keeps its grid but not its region size, and the row would test another form than it claims."""
    distinct, _ = oracle(row, streams)
    f = row.form
    assert pf.load_limit(f.region_slots, f.n_regions) * f.cap >= distinct + (streams[row.which()].size - row.k + 1), distinct
    assert 0.6 * f.cap >= distinct                                           # (count_partitioned doubles the table beyond this)


@pytest.mark.parametrize("row", pf.ROWS, ids=repr)
def test_a_rows_segments_hold_iff_it_says_so(row, streams):
    """The k-mers a level-1 workgroup meets for a bucket (the stream's own share of k-mers among its window starts) against its segment, for a
    round of half the stream.  Where they do not fit, no stream that the row's table has room for makes them: the round's share of a segment grows
    with the stream no faster than the workgroup's tiles do."""
    _, total = oracle(row, streams)
    starts = streams[row.which()].size - row.k + 1
    fill, cap = pf.segment_fill(row.form, starts if row.short else starts // 2, total / starts)
    assert (fill <= cap) == row.seg, (fill, cap)
