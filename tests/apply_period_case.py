"""Run in a subprocess by tests/test_gpu_apply_period.py (the hooks are read when the library loads): the packed apply's region loop
(kat_amd/csrc/kg_partition.hpp: k_p3_apply_pk) -- the next region's loads leaving with the wave that has finished the run's last segment,
the fill from registers, the write-back -- over runs of chosen lengths in regions whose neighbours are empty, some of them followed on their
workgroup's stride by further runs behind empty regions.

The scenes are tests/apply_lean_case.py's first four (the three kernel shapes: B=512 KP=4 at 256 and 4096 slots, B=512 KP=10 at 4100,
B=1024 KP=5 at 9700).  With CH = 256 UG k-mers per chunk (UG = 1: what the host launches) and NW = 8 or 16 waves, regions 3, 40, 77, ... (37
apart: no two of them share a workgroup's stride for any grid that is a multiple of 256, and the special regions below are chosen off their
strides) receive runs of exactly

    0, 1, CH - 1, CH, CH + 1, CH / 2, CH / 2 - 1, CH / 2 + 1, (NW - 1) CH, NW CH, NW CH + 1 and 2 NW CH + CH / 2 + 3

items, made of up to half a region's slots of distinct k-mers (place_keys says which region a k-mer belongs to; each k-mer is a record
of its own, so a run is exactly its k-mers in a round).  Nearly every other region of the table stays empty: the kernel's skip over
regions without a run, the loads for a region far ahead and the end of a workgroup's regions behind a loaded one all happen.
Four of the chosen regions r -- the ones with 0, 1, CH and NW CH items -- are FOLLOWED on their stride: regions r + n / 4 and r + 3 n / 4 (modulo n) of
the table's n hold runs of CH + 1 and 3 items, the regions between and behind them nothing.  With the grids the kernel takes (256, 512 or 1024
workgroups) a workgroup that has walked r, or skipped it, goes on to a loaded region one or two strides on: at the KP = 10 scene (2048
regions, two workgroups per CU: 512 on 256 CUs) r + 512 follows r, r + 1024 is skipped and r + 1536 is the stride's last.  In the second call
these regions are loaded, so the words that the early loads bring are the ones the next fill needs: loads of the wrong region show in the dump.

Table 2 takes two count calls, each in ONE round.  The first is its first sweep (the slots are cleared by the kernel: every region is
visited and written; inline claims).  The second finds it loaded (the steady shape: claims through the waves' queues) and brings the same
run lengths, half of each run's k-mers new, and in regions of their own
  - new k-mers three and six times in a row (several lanes of a chunk meet the same free slot: one claim wins, the others find the winner),
  - two different new k-mers with one home slot, side by side,
  - a new k-mer whose home is the region's last slot, taken since the first call (the probe wraps to slot 0),
  - 256-slot scenes: the 40 k-mers that fill a region to its last slot, three times each (claims that meet a region filling up; nothing
    may spill: the table has room for exactly these),
and both calls hold a poly-A run of more than half the count range in the scene with 20 count bits: the walk goes in segments and the LAST
one lifts the counter above half, so the write-back hands the excess to the side table.

  apply_period_case.py one     as above
  apply_period_case.py seg     walks in segments of 4096 k-mers (KATGPU_TEST_AP_SEG): the longest runs take two and three, with the sweep between
  apply_period_case.py spill   KATGPU_TEST_SPILL_MOD = 5: a fifth of the k-mers leave the walk for the direct path (the hooked shape, B=1024 KP=5)

After every call: the trace's "partition forms" line, the dump and the statistics against the oracle, and comp(table 1, table 2) --
matrix, counters, spectra -- against the oracle's, exactly."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from apply_lean_case import ROOT, SCENES, canonical_kmers, count_of, forms_lines, records, same  # noqa: E402  (its capture of the trace comes with it)

import kat_amd  # noqa: E402
from kat_amd import synth  # noqa: E402
from kat_amd.binding import place_keys  # noqa: E402
from oracle import koracle as ko  # noqa: E402

assert ROOT == os.path.dirname(HERE)
UG = 1                                    # groups a lane takes per chunk (k_p3_apply_pk's last template argument: the host launches 1)
CH = 256 * UG                             # k-mers per chunk: 64 lanes x 4 UG
FOLLOWED = (0, 1, 3, 9)                   # the chosen regions (by their place in run_lengths) with further runs on their stride
STEP = 37                                 # between the chosen regions


def run_lengths(nw):
    return [0, 1, CH - 1, CH, CH + 1, CH // 2, CH // 2 - 1, CH // 2 + 1, (nw - 1) * CH, nw * CH, nw * CH + 1, 2 * nw * CH + CH // 2 + 3]


def build_streams(k, p1, p2, S, cbits, nw):
    """the two calls' k-mers (records come later), and what was constructed"""
    l2 = int(p2).bit_length() - 1
    cand = canonical_kmers(k, 1_000_000, seed=300 + k + S)
    d1, d2, rem, back, _, home = place_keys(k, p1, l2, cand, region_slots=S)
    assert (back == cand).all()
    region = d1.astype(np.int64) * p2 + d2
    order = np.argsort(region, kind="stable")
    starts = np.searchsorted(region[order], np.arange(p1 * p2 + 1))

    def pool(r):
        return order[starts[r]:starts[r + 1]]             # indices into cand of region r's candidates

    lengths = run_lengths(nw)
    first, second, made = [], [], {"runs": []}
    for i, n in enumerate(lengths):
        r = 3 + STEP * i
        idx = pool(r)
        d = min(n, S // 2, idx.size * 2 // 3)
        assert n == 0 or d >= 1, (r, idx.size)
        if n:
            a, b = cand[idx[:d]], cand[idx[d // 2:d // 2 + d]]          # the second call: half of them new
            # odd runs: a k-mer's copies side by side (the lanes of one chunk); even ones: the k-mers in turn
            first.append(np.sort(np.resize(a, n)) if i & 1 else np.resize(a, n))
            second.append(np.sort(np.resize(b, n)) if i & 1 else np.resize(b, n))
        made["runs"].append((r, n, d))
    n_reg = p1 * p2
    made["followers"] = []
    for i in FOLLOWED:
        for q, n in (((3 + STEP * i + n_reg // 4) % n_reg, CH + 1), ((3 + STEP * i + 3 * n_reg // 4) % n_reg, 3)):
            idx = pool(q)
            d = min(n, S // 2, idx.size * 2 // 3)
            assert d >= 1, (q, idx.size)
            first.append(np.resize(cand[idx[:d]], n))
            second.append(np.resize(cand[idx[d // 2:d // 2 + d]], n))
            made["followers"].append(q)
    classes = {(3 + STEP * i) % 256 for i in range(len(lengths))}
    taken = set()

    def others():                                             # regions for the special cases: off the chosen regions' strides, one case each
        for r in range(p1 * p2):
            if r % 256 not in classes and r not in taken:
                yield r, pool(r)

    # new k-mers three and six times in a row
    r, idx = next((r, idx) for r, idx in others() if idx.size >= 60)
    taken.add(r)
    first.append(cand[idx[:20]])
    second.append(np.concatenate([np.repeat(cand[idx[20:50]], 3), np.repeat(cand[idx[50:60]], 6), cand[idx[:20]]]))

    # two different new k-mers with one home slot
    for r, idx in others():
        h = home[idx]
        o = np.argsort(h, kind="stable")
        eq = np.flatnonzero(h[o][1:] == h[o][:-1])
        if eq.size:
            x, y = cand[idx[o[eq[0]]]], cand[idx[o[eq[0] + 1]]]
            break
    else:
        raise AssertionError("no two candidates with one home slot")
    taken.add(r)
    made["pair"] = (int(x), int(y), r)
    first.append(cand[idx[o[:eq[0]]]][:10])                    # (others of the region, so that it is not empty in the first call)
    second.append(np.array([x, y, x, y, y], np.uint64))

    # a new k-mer whose home is the region's last slot, which the first call has taken
    for r, idx in others():
        last = idx[home[idx] == S - 1]
        if last.size >= 2:
            break
    else:
        raise AssertionError("no two candidates at home in a region's last slot")
    taken.add(r)
    made["wrap"] = (int(cand[last[0]]), int(cand[last[1]]), r)
    first.append(cand[last[:1]])
    second.append(np.repeat(cand[last[1:2]], 2))

    if S == 256:                                               # a region filled to its last slot by the second call
        for r, idx in others():
            if idx.size >= S:
                break
        else:
            raise AssertionError("no region with as many candidates as slots")
        full = cand[idx[:S]]
        first.append(full[:S - 40])
        second.append(np.concatenate([np.repeat(full[S - 40:], 3), full[:8]]))
        made["full_region"] = r
    used = {int(x) for x in np.unique(region[np.isin(cand, np.concatenate(first + second))])}
    assert len(used) < 48 and set(made["followers"]) <= used, sorted(used)
    for i, (r, n, d) in enumerate(made["runs"]):               # a chosen region holds its run and nothing else; its neighbours in steps of 256 hold nothing,
        assert (r in used) == (n > 0)                          # but for the two followers of some
        on_stride = {q for q in range(r % 256, n_reg, 256) if q != r and q in used}
        assert on_stride == ({(r + n_reg // 4) % n_reg, (r + 3 * n_reg // 4) % n_reg} if i in FOLLOWED else set()), (r, sorted(used))
    return np.concatenate(first), np.concatenate(second), made


def poly_a(k, n_kmers):
    return np.frombuffer(b"A" * (n_kmers + k - 1) + b"N", np.uint8)


def main():
    mode = sys.argv[1]
    assert os.environ["KATGPU_TEST_REGION_SLOTS"] == "1024" and os.environ["KATGPU_TEST_LAZY_MIN_SLOTS"] == "0" and os.environ["KATGPU_TEST_ROUND_ITEMS"] == "8000000"
    assert (os.environ.get("KATGPU_TEST_AP_SEG") == "4096") == (mode == "seg") and (os.environ.get("KATGPU_TEST_SPILL_MOD", "0") == "5") == (mode == "spill")
    eng = kat_amd.Engine(0)
    genome = synth.genome(100_000, seed=21)
    b1 = np.ascontiguousarray(synth.reads(genome, 0, 3000, seed=2))
    buf1 = eng.alloc(b1.size + 32)
    buf1.upload(b1)
    for k, regions, rb, cbits, hb, S, shape in SCENES[:4]:
        tag = "k=%u regions=%u S=%u" % (k, regions, S)
        if mode == "spill":
            shape = "B=1024 KP=5 "
        nw = 16 if shape.startswith("B=1024") else 8
        o1 = ko.Table(k, True).count_bases(b1, threads=8)
        t1 = eng.table(k, True, size_hint=regions * 1024)
        g1 = t1.geometry()
        assert g1.n_regions == regions and g1.region_slots == 1024 and t1.packed_records(), (tag, g1.n_regions, g1.region_slots)
        t1.count_bases_device(buf1.ptr, b1.size)
        same(t1, o1, (tag, "table 1"))
        k1, k2, made = build_streams(k, g1.p1, g1.p2, S, cbits, nw)
        s1, s2 = [records(k, k1)], [records(k, k2)]
        if cbits == 20:                                        # beyond half the count range in each call; the region of AAAA is none of the chosen ones
            _d1, _d2 = place_keys(k, g1.p1, int(g1.p2).bit_length() - 1, np.zeros(1, np.uint64))[:2]
            ra = int(_d1[0]) * g1.p2 + int(_d2[0])
            assert all(ra % 256 != r % 256 for r, _, _ in made["runs"]), ra
            s1.append(poly_a(k, (1 << 19) + 5000))
            s2.append(poly_a(k, (1 << 19) + 100))
        s1, s2 = np.ascontiguousarray(np.concatenate(s1)), np.ascontiguousarray(np.concatenate(s2))
        want1 = ko.Table(k, True).count_bases(s1, threads=8)
        want2 = ko.Table(k, True).count_bases(s1, threads=8).count_bases(s2, threads=8)
        x, y, _ = made["pair"]
        assert (count_of(want1, x), count_of(want1, y), count_of(want2, x), count_of(want2, y)) == (0, 0, 2, 3)
        w0, w1, _ = made["wrap"]
        assert (count_of(want1, w0), count_of(want1, w1), count_of(want2, w1)) == (1, 0, 2)
        if cbits == 20:
            assert count_of(want1, 0) == (1 << 19) + 5000 and count_of(want2, 0) == (1 << 20) + 5100
        t2 = eng.table(k, True, size_hint=regions * S, like=t1)
        g2 = t2.geometry()
        assert (g2.p1, g2.p2, g2.region_slots) == (g1.p1, g1.p2, S) and t2.packed_records(), (tag, g2.p1, g2.p2, g2.region_slots)
        for n_call, (stream, want) in enumerate(((s1, want1), (s2, want2))):
            what = (tag, "call %d" % (n_call + 1))
            buf = eng.alloc(stream.size + 32)
            buf.upload(stream)
            before = len(forms_lines())
            t2.count_bases_device(buf.ptr, stream.size)
            seen = forms_lines()[before:]
            print("%s call %d | %s" % (tag, n_call + 1, " / ".join(seen)))
            assert len(seen) == 1, (what, seen)
            assert " hb=%u " % hb in seen[0] and "apply=packed " + shape in seen[0] and seen[0].endswith(" hooked") == (mode == "spill"), (what, seen)
            fresh = int(seen[0].rsplit("fresh=", 1)[1].split()[0])
            assert fresh == (1 if n_call == 0 and mode != "spill" else 0), (what, seen)          # (the hooked shape has no inline claims)
            assert t2.regrows == 0 and t2.geometry().region_slots == S, what
            same(t2, want, what)
            for gg, ww, name in zip(kat_amd.comp(t1, t2), ko.comp(o1, want), ("main", "counters", "spectra")):
                assert np.array_equal(gg, ww), (what, "comp", name)
        t1.free(); t2.free()
    print("apply period ok:", mode)


if __name__ == "__main__":
    main()
