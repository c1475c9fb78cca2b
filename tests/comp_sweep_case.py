"""Run in a subprocess by tests/test_gpu_comp_sweep.py with KATGPU_TEST_REGION_SLOTS in the environment (the hook is read when the library
loads): the fused comparison's sweep of the resident region (kat_amd/csrc/kg_reduce_kernels.hpp: k_comp_fused), whose k-mers of count 1 that
the other table lacks are tallied per lane and never reach the wave's queue.  Two packed tables of one grid hold constructed k-mers:

  - only in table A at counts 1, 2, 63, 64, 65 and 1000; shared ones at those counts; k-mers only in table B;
  - four regions of A in which the 64 slots [64, 128) -- what one wave of the sweep reads at once -- are all occupied (placed with
    kat_amd.binding.place_keys; the occupied slots of a linear-probing region do not depend on the order of insertion): all of them count 1 and
    absent from B, none of them so (count 2, or shared), one in three so, and a region of which B holds every k-mer (all marked);
  - with and without a poly-A run of 600 K copies in A, or in B: more than the 20 count bits of a slot of this grid hold in their lower
    half, so its count continues in the side table and the side-table instantiation runs -- swept (A) or only streamed (B).

comp(A, B) has A resident as hash 1 (the sweep is pass 1's "only hash 1 has it"), comp(B, A) has A resident as hash 2 (the sweep is all of
pass 2).  Default scales (the spectra fold into the tile), scales for which count 1 lands in another tile cell than (1, 0) or outside the
tile, and matrices too small to fold.  Matrix, the 13 counters and the spectra equal the oracle's, integer for integer.

  comp_sweep_case.py <region slots>"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kat_amd  # noqa: E402
from kat_amd.binding import place_keys  # noqa: E402
from oracle import koracle as ko  # noqa: E402

K = 27
COUNTS = (1, 2, 63, 64, 65, 1000)
WINDOW = (64, 128)                       # the slots of a region that lanes 0 .. 63 of the sweep's wave 1 read together


def canonical_kmers(n, seed):
    """n random canonical K-mers (distinct, sorted)"""
    rng = np.random.default_rng(seed)
    key = rng.integers(0, 1 << (2 * K), n, dtype=np.uint64)
    rc = np.zeros(n, np.uint64)
    x = key.copy()
    for _ in range(K):
        rc = (rc << np.uint64(2)) | (np.uint64(3) - (x & np.uint64(3)))
        x >>= np.uint64(2)
    return np.unique(np.minimum(key, rc))


def occupied(homes, slots):
    """the slots a linear-probing region of `slots` slots has occupied once k-mers with these home slots are in (any order)"""
    occ = np.zeros(slots, bool)
    for h in homes:
        while occ[h]:
            h = (h + 1) % slots
        occ[h] = True
    return occ


def main():
    rs = int(sys.argv[1])
    assert int(os.environ["KATGPU_TEST_REGION_SLOTS"]) == rs
    eng = kat_amd.Engine(0)
    probe = eng.table(K, True, size_hint=1024 * rs)
    geo = probe.geometry()
    assert geo.region_slots == rs and geo.n_regions >= 1024 and probe.packed_records(), (geo.region_slots, geo.n_regions)
    p1, p2 = geo.p1, geo.p2
    probe.free()

    cand = canonical_kmers(4_000_000, seed=rs)
    d1, d2, _, back, rb, home = place_keys(K, p1, int(p2).bit_length() - 1, cand, region_slots=rs)
    assert rb <= 44 and (back == cand).all()
    region = d1.astype(np.int64) * p2 + d2

    # the four constructed regions: the most populous ones; up to two k-mers per home slot from just below the window to its end fill it and more
    per_region = np.bincount(region, minlength=p1 * p2)
    special = np.argsort(per_region)[-4:]
    lo, hi = WINDOW
    windows = []
    for r in special:
        in_r = np.flatnonzero(region == r)
        idx = np.concatenate([in_r[home[in_r] == h][:2] for h in range(lo - 4, hi)])
        occ = occupied(home[idx].tolist(), rs)
        assert occ[lo:hi].all(), ("region", int(r), "window not full", int(occ[lo:hi].sum()), idx.size)
        windows.append(cand[idx])
    used = np.isin(region, special)
    rest = cand[~used]
    all_hot, none_hot, mixed, all_marked = windows

    a_keys, a_counts, b_keys, b_counts = [], [], [], []

    def put(keys, ca, cb):
        keys = np.asarray(keys, np.uint64)
        if ca:
            a_keys.append(keys); a_counts.append(np.full(keys.size, ca, np.uint64))
        if cb:
            b_keys.append(keys); b_counts.append(np.full(keys.size, cb, np.uint64))

    at = 0
    for c in COUNTS:                                       # only in A; shared at (c, 1) and (1, c)
        put(rest[at:at + 3000], c, 0); at += 3000
        put(rest[at:at + 500], c, 1); at += 500
        put(rest[at:at + 500], 1, c); at += 500
    put(rest[at:at + 6000], 0, 1); at += 6000              # only in B
    put(rest[at:at + 1000], 0, 70); at += 1000
    put(all_hot, 1, 0)
    put(none_hot[0::2], 2, 0); put(none_hot[1::2], 1, 3)
    put(mixed[0::3], 1, 0); put(mixed[1::3], 1, 1); put(mixed[2::3], 3, 0)
    put(all_marked, 1, 2)
    a_keys, a_counts, b_keys, b_counts = (np.concatenate(x) for x in (a_keys, a_counts, b_keys, b_counts))
    assert a_keys.size > b_keys.size                       # A has more k-mers: it is the resident table either way round

    poly_a = np.frombuffer(b"N" + b"A" * (600_000 + K - 1) + b"N", np.uint8)
    n = 0
    for ovf in ("none", "A", "B"):
        ta = eng.table(K, True, size_hint=1024 * rs)
        tb = eng.table(K, True, size_hint=1024 * rs, like=ta)
        oa, ob = ko.Table(K, True), ko.Table(K, True)
        ta.merge_host(a_keys, a_counts); tb.merge_host(b_keys, b_counts)
        for o, keys, counts in ((oa, a_keys, a_counts), (ob, b_keys, b_counts)):
            for key, c in zip(keys.tolist(), counts.tolist()):
                o.add(key, c)
        if ovf == "A":
            ta.count_bases(poly_a); oa.count_bases(poly_a)
        if ovf == "B":
            tb.count_bases(poly_a); ob.count_bases(poly_a)
        for t in (ta, tb):
            g = t.geometry()
            assert t.regrows == 0 and (g.p1, g.p2, g.region_slots) == (p1, p2, rs) and t.packed_records()
        for t, o in ((ta, oa), (tb, ob)):
            gk, gc = t.dump_sorted()
            wk, wc = o.dump_sorted()
            assert np.array_equal(gk, wk) and np.array_equal(gc, wc), (rs, ovf, "the tables differ before any comparison")
        eng.profile_reset()
        for (t1, t2, o1, o2), way in (((ta, tb, oa, ob), "A resident as hash 1"), ((tb, ta, ob, oa), "A resident as hash 2")):
            for bins, s1, s2 in (((1001, 1001), 1.0, 1.0), ((40, 50), 1.0, 1.0), ((1001, 1001), 2.5, 2.5), ((1001, 1001), 2.5, 1.0), ((1001, 1001), 1.0, 2.5),
                                 ((1001, 1001), 100.0, 100.0), ((1001, 1001), 0.5, 0.5)):
                want = ko.comp(o1, o2, s1, s2, *bins)
                got = kat_amd.comp(t1, t2, s1, s2, *bins)
                for gg, ww, name in zip(got, want, ("main", "counters", "spectra")):
                    assert np.array_equal(gg, ww), (rs, ovf, way, bins, s1, s2, name, int((np.asarray(gg) != np.asarray(ww)).sum()))
                n += 1
        prof = eng.profile()
        assert prof["comp_pass1"]["launches"] == 14 and prof["comp_pass2"]["launches"] == 0, (prof["comp_pass1"], prof["comp_pass2"])     # the fused kernel is pass 1 and 2
        ta.free(); tb.free()
    print("comp sweep ok:", rs, n)


if __name__ == "__main__":
    main()
