"""Run in a subprocess by tests/test_gpu_apply_lean.py (the hooks are read when the library loads): the packed apply's walk
(kat_amd/csrc/kg_partition.hpp: ApkWalk; its slot tests and step: kg_apply_lean.hpp) over the slot words, item widths and region sizes it can
meet, with k-mers constructed for the walk's corners.

A scene is (k, regions of the grid, slots per region): table 1 holds reads on a grid of 1024-slot regions, table 2 is made `like=` it with a
hint that gives its regions the scene's size, and k with the grid gives the remainder its length rb (kat_amd.binding.place_keys says it):

  k  regions  rb  count bits  item bytes above 32 bits   slots     kernel shape
  27   2048   43     21              2                     256     B=512 KP=4
  27   1024   44     20              2                    4096     B=512 KP=4     (the last small shape)
  24   2048   37     27              1                    4100     B=512 KP=10    (the first that is not)
  21   2048   31     32              0                    9700     B=1024 KP=5    (no room for a second workgroup's queues)
  13   2048   15     32              0                     256     B=512 KP=4     (remainders short enough to find one that is 0)

Table 2 takes two count calls.  The first (a first round: inline claims) holds a background of k-mers once to three times, a pair of k-mers
with one home slot whose remainders differ only in bits of the slot word's high half, a region's k-mers up to 40 short of all its slots (256-slot
scenes), the neighbours that occupy at least the nine slots from a remainder-0 k-mer's home on and a second remainder-0 k-mer in a region that
holds nothing else (k = 13), and a poly-A run longer than half the count range (count bits 20: segments of the walk, the side table).  The second
(the table is loaded: the steady shape, claims through the queues) is mostly NEW k-mers, each three times in a row -- the same k-mer in several lanes
of a chunk, every one of which saw its slot free --, the 40 k-mers that fill the region to its last slot (chains far beyond the lanes' probes,
wrapping at S - 1: the wave-wide finish), the remainder-0 k-mer behind its neighbours, and the first call's background again.

  apply_lean_case.py one   each call in one round
  apply_lean_case.py two   rounds of 60 000 items (KATGPU_TEST_ROUND_ITEMS: the first call's later rounds load the table) and walks in segments of
                           4096 k-mers (KATGPU_TEST_AP_SEG)

After every call: the trace's "partition forms" lines (item width, kernel shape, inline claims in a table's first round only), the dump and the
statistics against the oracle, and comp(table 1, table 2) -- matrix, counters, spectra -- against the oracle's, exactly."""
import atexit
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import kat_amd  # noqa: E402
from kat_amd import synth  # noqa: E402
from kat_amd.binding import place_keys  # noqa: E402
from oracle import koracle as ko  # noqa: E402

#          k  regions  rb  cbits hb  slots  shape
SCENES = ((27, 2048, 43, 21, 2, 256, "B=512 KP=4 "),
          (27, 1024, 44, 20, 2, 4096, "B=512 KP=4 "),
          (24, 2048, 37, 27, 1, 4100, "B=512 KP=10 "),
          (21, 2048, 31, 32, 0, 9700, "B=1024 KP=5 "),
          (13, 2048, 15, 32, 0, 256, "B=512 KP=4 "))
LANE_PROBES_AND_ROUNDS = 12 + 3          # APK_LANE_PROBES + NR: a chain beyond it is finished by the wave
TRACE = tempfile.NamedTemporaryFile(prefix="apply_lean_trace_", suffix=".txt")
STDERR = os.dup(2)
os.dup2(TRACE.fileno(), 2)                  # the library's trace lines: looked at per count ...


@atexit.register
def _trace_to_parent():                     # ... and handed on
    sys.stderr.flush()
    os.dup2(STDERR, 2)
    with open(TRACE.name) as f:
        sys.stderr.write(f.read()[-20000:])


MARK = "[katgpu] partition forms: "


def forms_lines():
    with open(TRACE.name) as f:
        return [line[len(MARK):].strip() for line in f if line.startswith(MARK)]


def canonical_kmers(k, n, seed):
    """n random canonical k-mers (distinct, sorted)"""
    rng = np.random.default_rng(seed)
    key = rng.integers(0, 1 << (2 * k), n, dtype=np.uint64)
    rc = np.zeros(n, np.uint64)
    x = key.copy()
    for _ in range(k):
        rc = (rc << np.uint64(2)) | (np.uint64(3) - (x & np.uint64(3)))
        x >>= np.uint64(2)
    return np.unique(np.minimum(key, rc))


def records(k, keys):
    """one record per k-mer: its k bases and an N"""
    keys = np.asarray(keys, np.uint64)
    out = np.full((keys.size, k + 1), ord("N"), np.uint8)
    for i in range(k):
        out[:, i] = synth.ACGT[((keys >> np.uint64(2 * (k - 1 - i))) & np.uint64(3)).astype(np.uint8)]
    return out.ravel()


def occupied(homes, S):
    """the slots a linear-probing region of S slots has occupied once k-mers with these home slots are in (any order)"""
    occ = np.zeros(S, bool)
    for h in homes:
        s = int(h)
        while occ[s]:
            s = s + 1 if s + 1 < S else 0
        occ[s] = True
    return occ


def build_streams(k, p1, p2, S, rb, cbits):
    """the two calls' streams and what was constructed, asserted from place_keys"""
    l2 = int(p2).bit_length() - 1
    cand = canonical_kmers(k, 1_000_000, seed=100 + k + S)
    d1, d2, rem, back, rb_seen, home = place_keys(k, p1, l2, cand, region_slots=S)
    assert (back == cand).all() and rb_seen == rb, (rb_seen, rb)
    region = d1.astype(np.int64) * p2 + d2
    made = {}
    taken_regions = set()
    first, second = [], []

    # two k-mers of one region and one home slot whose remainders differ only above bit 32 of the slot word (rem << cbits | count)
    low = rem & np.uint64((1 << (32 - cbits)) - 1)
    order = np.lexsort((low, home, region))
    r_s, h_s, l_s = region[order], home[order], low[order]
    eq = np.flatnonzero((r_s[1:] == r_s[:-1]) & (h_s[1:] == h_s[:-1]) & (l_s[1:] == l_s[:-1]))
    assert eq.size, "no pair of k-mers with one home slot and equal low remainder bits"
    a, b = cand[order[eq[0]]], cand[order[eq[0] + 1]]
    ra, rb_ = int(rem[order[eq[0]]]), int(rem[order[eq[0] + 1]])
    assert ra != rb_ and ((ra ^ rb_) << cbits) & 0xFFFFFFFF == 0
    made["pair"] = (int(a), int(b))
    taken_regions.add(int(r_s[eq[0]]))
    first += [np.repeat(np.array([a, b], np.uint64), [5, 7])]
    second += [np.array([b, a, b], np.uint64)]

    if S == 256:
        # a region filled to its last slot: all but 40 of its k-mers in the first call, the rest in the second
        per = np.bincount(region, minlength=p1 * p2)
        rf = next(int(x) for x in np.flatnonzero(per >= S) if int(x) not in taken_regions)
        full = cand[region == rf][:S]
        taken_regions.add(rf)
        first += [full[:S - 40]]
        second += [full[S - 40:], full[:8]]
        made["full_region"] = rf
    if rb <= 16:
        zeros = np.flatnonzero((rem == 0) & ~np.isin(region, list(taken_regions)))
        assert zeros.size >= 2 and (home[zeros] == 0).all(), "fewer than two remainder-0 k-mers among the candidates"      # (the home slot is a hash of the remainder: slot 0)
        z1 = int(zeros[0])
        # z1: count 1, alone in its region, in the first call (an inline claim of the word 0 << cbits | 1 = 1)
        first += [cand[z1:z1 + 1]]
        taken_regions.add(int(region[z1]))
        # z2: behind neighbours (homes in the region's last slots and slot 0: their chain wraps) that occupy at least the nine slots from its home on
        for z2 in (int(z) for z in zeros[1:]):
            nb = np.flatnonzero((region == region[z2]) & ((home >= S - 14) | (home == 0)) & (rem != 0))
            if occupied(home[nb], S)[:9].all():
                break
        else:
            raise AssertionError("no remainder-0 k-mer with nine occupied slots from its home on")
        first += [cand[nb]]
        second += [cand[z2:z2 + 1]]
        taken_regions.add(int(region[z2]))
        made["rem0"] = (int(cand[z1]), int(cand[z2]))
    free = ~np.isin(region, list(taken_regions))
    pool = cand[free]
    rng = np.random.default_rng(7)
    rng.shuffle(pool)
    bg, new = pool[:12000], pool[12000:42000]
    first += [np.repeat(bg, rng.integers(1, 4, bg.size))]
    second += [np.repeat(new, 3), bg[:3000]]               # mostly new, each three times in a row: not shuffled below

    s1 = np.concatenate(first)
    rng.shuffle(s1)
    parts1 = [records(k, s1)]
    if cbits == 20:                                       # one k-mer beyond half the count range: 2^19 + 5000 times
        n_a = (1 << 19) + 5000 + k - 1
        parts1.append(np.frombuffer(b"A" * n_a + b"N", np.uint8))
        made["poly_a"] = n_a - k + 1
    return np.ascontiguousarray(np.concatenate(parts1)), np.ascontiguousarray(records(k, np.concatenate(second))), made


def same(t, o, what):
    gk, gc = t.dump_sorted()
    wk, wc = o.dump_sorted()
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc), (what, "dump differs", gk.size, wk.size)
    st = t.stats()
    assert st["distinct"] == wk.size and st["total"] == int(wc.sum(dtype=np.uint64)), (what, st)


def count_of(o, key):
    keys, counts = o.dump_sorted()
    i = np.searchsorted(keys, np.uint64(key))
    return int(counts[i]) if i < keys.size and keys[i] == np.uint64(key) else 0


def main():
    mode = sys.argv[1]
    assert os.environ["KATGPU_TEST_REGION_SLOTS"] == "1024" and os.environ["KATGPU_TEST_LAZY_MIN_SLOTS"] == "0"
    assert int(os.environ["KATGPU_TEST_ROUND_ITEMS"]) == (8_000_000 if mode == "one" else 60_000)
    assert (os.environ.get("KATGPU_TEST_AP_SEG") == "4096") == (mode == "two")
    eng = kat_amd.Engine(0)
    genome = synth.genome(100_000, seed=21)
    b1 = np.ascontiguousarray(synth.reads(genome, 0, 3000, seed=2))
    buf1 = eng.alloc(b1.size + 32)
    buf1.upload(b1)
    for k, regions, rb, cbits, hb, S, shape in SCENES:
        tag = "k=%u regions=%u S=%u" % (k, regions, S)
        o1 = ko.Table(k, True).count_bases(b1, threads=8)
        t1 = eng.table(k, True, size_hint=regions * 1024)
        g1 = t1.geometry()
        assert g1.n_regions == regions and g1.region_slots == 1024 and t1.packed_records(), (tag, g1.n_regions, g1.region_slots)
        t1.count_bases_device(buf1.ptr, b1.size)
        same(t1, o1, (tag, "table 1"))
        s1, s2, made = build_streams(k, g1.p1, g1.p2, S, rb, cbits)
        assert ("poly_a" in made) == (cbits == 20) and ("rem0" in made) == (rb <= 16) and ("full_region" in made) == (S == 256), (tag, made)
        want1 = ko.Table(k, True).count_bases(s1, threads=8)
        want2 = ko.Table(k, True).count_bases(s1, threads=8).count_bases(s2, threads=8)
        if "rem0" in made:
            z1, z2 = made["rem0"]
            assert (count_of(want1, z1), count_of(want1, z2), count_of(want2, z2)) == (1, 0, 1)
        if "poly_a" in made:
            assert count_of(want1, 0) == made["poly_a"] > 1 << 19
        t2 = eng.table(k, True, size_hint=regions * S, like=t1)
        g2 = t2.geometry()
        assert (g2.p1, g2.p2, g2.region_slots) == (g1.p1, g1.p2, S) and t2.packed_records(), (tag, g2.p1, g2.p2, g2.region_slots)
        for n_call, (stream, want) in enumerate(((s1, want1), (s2, want2))):
            what = (tag, "call %d" % (n_call + 1))
            buf = eng.alloc(stream.size + 32)
            buf.upload(stream)
            before = len(forms_lines())
            eng.profile_reset()
            t2.count_bases_device(buf.ptr, stream.size)
            prof = eng.profile()
            seen = forms_lines()[before:]
            print("%s call %d | %s" % (tag, n_call + 1, " / ".join(seen)))
            assert len(seen) == 1 if mode == "one" else len(seen) >= 2, (what, seen)
            assert all(" hb=%u " % hb in line and "apply=packed " + shape in line for line in seen), (what, seen)
            fresh = [int(line.rsplit("fresh=", 1)[1].split()[0]) for line in seen]
            assert fresh == [1 if n_call == 0 else 0] + [0] * (len(seen) - 1), (what, seen)
            total = int(want.dump_sorted()[1].sum(dtype=np.uint64))
            assert prof["count"]["units"] <= total // 100, (what, "direct path", prof["count"]["units"], total)
            assert t2.regrows == 0 and t2.geometry().region_slots == S, what
            same(t2, want, what)
            for gg, ww, name in zip(kat_amd.comp(t1, t2), ko.comp(o1, want), ("main", "counters", "spectra")):
                assert np.array_equal(gg, ww), (what, "comp", name)
        t1.free(); t2.free()
    print("apply lean ok:", mode)


if __name__ == "__main__":
    main()
