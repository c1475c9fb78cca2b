"""Run in a subprocess by tests/test_gpu_apply_drain.py (the hooks are read when the library loads): the drains of the packed apply's walk
(kat_amd/csrc/kg_partition.hpp: ApkWalk::drain_pass, whose lanes probe a window of APK_WINDOW consecutive slots per LDS round trip;
kg_apply_lean.hpp: ap_first_event) over probe chains of constructed lengths.

The scenes are tests/apply_lean_case.py's first four (the three kernel shapes: B=512 KP=4 at 256 and 4096 slots, B=512 KP=10 at 4100, B=1024
KP=5 at 9700).  A k-mer's remainder is its low bits and gives its home slot; the bits above choose the region.  So a k-mer with a wanted home
in a wanted region is made from a remainder with that home (Maker below; place_keys checks every one, and only canonical ones are kept).
A CLUSTER of d k-mers with homes h, h + 1, ..., h + d - 1, one each, in an otherwise empty stretch sits in exactly those slots whatever the
order they arrive in.  Each case has a region of its own (regions 5, 42, 79, ...: 37 apart, no two on one workgroup's stride):

  chain d     d = 0 .. 12 (NR = 2 or 3 probe rounds, then none, part, one, two and more than two windows of 2 or 4 slots), 17 and 20 (beyond
              APK_LANE_PROBES + NR: three windows, then the wave-wide finish).  Call 1: the cluster.  Call 2: a new k-mer x with home h, whose first
              free slot lies d slots on, NINE times (a claim at distance d: one copy's compare-and-swap wins, the others find x there).  Call 3: x
              nine times more (a match at distance d).  Nine, because a pass of fewer than 8 entries that nothing follows -- a small run's only
              pass -- skips the lanes' phase and hands everything to the wave-wide finish: with 9 the lanes walk their windows, all on one chain,
              until the event (d - NR slots into the windows: every offset, behind 2 and behind 3 probe rounds).
  wrap j      j = 0 .. 6: the same with h = S - 1 - j and d = j + 3, so that the chain crosses S - 1 -> 0 at every offset of a window, behind 2 and
              behind 3 probe rounds, and the free slot (later x's own) lies behind the wrap.
  race 3/64   x three times (beside nine copies of another new k-mer of the region, which keep the pass in the lanes' phase) and 64 times side by
              side behind clusters of 4 and 5: lanes of one chunk race for the first free slot of a window.
  race pair   x with home h and y with home h + 1 behind a cluster of 4, nine times each in turn: both chains end at slot h + 4; the lanes of the
              k-mer that loses the compare-and-swap find a foreign word there and go on from the slot behind it, in the pass's next iteration.
  mix         four clusters of 3, 5, 7 and 8 in one region, a new k-mer behind each five times: one pass whose lanes stand at different offsets
              and leave it in different iterations.
  segments    the chain d = 6 region receives 4500 copies of its cluster's k-mers in call 3 (two segments under KATGPU_TEST_AP_SEG = 4096).
  full p      256-slot scene, p = 0 .. 3: 255 k-mers fill the region but for one slot f; x's home is f + 1 + p, so its first free slot is the region's
              last-but-p unprobed one (distance S - 1 - p: each position of the walk's last window).  Nothing may spill.  (Chains of this length
              end in the wave-wide finish, as any chain beyond APK_LANE_PROBES + NR: the lanes' windows never come near a budget's end.)  Call 4 brings one k-mer
              more to the p = 0 region, which is full by then: exactly that one takes the direct path, and is counted -- in a table the host has
              made larger for it, which it does past the table's fill limit: the call fills the other regions to just beyond it.

Every chain's length is asserted here, on the CPU, by replaying the calls through a plain linear-probe model of the regions (Model below).
Table A takes the calls 1 to 3 as ONE call, its first sweep (inline claims: every chain is built and probed in the same walk).  Table B takes
them one after another: call 1 is its first sweep, calls 2 to 4 find it loaded (the steady shape: claims through the waves' queues).

  apply_drain_case.py one     as above
  apply_drain_case.py seg     walks in segments of 4096 k-mers (KATGPU_TEST_AP_SEG)
  apply_drain_case.py spill   KATGPU_TEST_SPILL_MOD = 5: a fifth of the k-mers leave the walk for the direct path (the hooked shape, B=1024 KP=5)

After every call: the trace's "partition forms" line, the dump and the statistics against the oracle, the k-mers the direct path took, and
comp(table 1, table 2) -- matrix, counters, spectra -- against the oracle's with a bystander table of reads, exactly."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from apply_lean_case import ROOT, SCENES, canonical_kmers, forms_lines, records, same  # noqa: E402  (its capture of the trace comes with it)

import kat_amd  # noqa: E402
from kat_amd import synth  # noqa: E402
from kat_amd.binding import place_keys  # noqa: E402
from oracle import koracle as ko  # noqa: E402

assert ROOT == os.path.dirname(HERE)
NR_MAX = 3                                 # probe rounds before the queue: 2 in the steady shape, 3 with inline claims and in the hooked shape
WINDOW_MAX = 4                             # the widest window the drain may be built with
LANE_PROBES = 12                           # APK_LANE_PROBES: slots a lane probes before the wave takes over
CHAIN_D = tuple(range(0, NR_MAX + 2 * WINDOW_MAX + 2)) + (LANE_PROBES + NR_MAX + 2, LANE_PROBES + NR_MAX + 5)
WRAP_J = tuple(range(0, 7))
STEP = 37                                  # between the cases' regions
COPIES = 9                                 # of a case's k-mer per call: a drain pass of fewer than 8 entries that nothing follows skips its lanes' phase
U64 = np.uint64


def is_canonical(k, key):
    rc = np.zeros(key.size, U64)
    x = key.copy()
    for _ in range(k):
        rc = (rc << U64(2)) | (U64(3) - (x & U64(3)))
        x >>= U64(2)
    return key <= rc


class Maker:
    """canonical k-mers with a wanted home slot in a wanted region"""

    def __init__(self, k, p1, p2, S, seed):
        self.k, self.p1, self.p2, self.S, self.l2 = k, p1, p2, S, int(p2).bit_length() - 1
        self.rb = place_keys(k, p1, self.l2, np.zeros(1, U64))[4]
        self.n1 = self.rb + self.l2                                # the bits below the level-1 digit's
        assert self.n1 < 2 * k and (1 << (2 * k - self.n1)) <= 2 * p1, (k, p1, p2, self.rb)
        rng = np.random.default_rng(seed)
        rems = np.unique(rng.integers(1, 1 << self.rb, 48 * S, dtype=U64))
        rng.shuffle(rems)
        _, _, rem, _, _, home = place_keys(k, p1, self.l2, rems, region_slots=S)
        assert (rem == rems).all()                                 # the remainder IS the low bits
        order = np.argsort(home, kind="stable")
        self.rems, self.starts, self.at = rems[order], np.searchsorted(home[order], np.arange(S + 1)), np.zeros(S, np.int64)
        self.rng = rng

    def keys_in(self, region, rems):
        """the k-mer of each remainder in `region` and whether it exists, is canonical and lies where it should"""
        k, p1, l2 = self.k, self.p1, self.l2
        d1t, d2t = region >> l2, region & (self.p2 - 1)
        d2_0 = place_keys(k, p1, l2, rems)[1]                      # the level-2 digit xors a hash of the remainder onto the bits above it
        low = ((U64(d2t) ^ d2_0.astype(U64)) << U64(self.rb)) | rems
        d1_0 = place_keys(k, p1, l2, low)[0]                       # the level-1 digit adds a hash of the bits below it, modulo p1
        hi = (np.int64(d1t) + p1 - d1_0.astype(np.int64)) % p1
        ok = hi < (1 << (2 * k - self.n1))
        key = (hi.astype(U64) << U64(self.n1)) | low
        key[~ok] = 0
        d1, d2, rem, back, _, home = place_keys(k, p1, l2, key, region_slots=self.S)
        ok &= (d1 == d1t) & (d2 == d2t) & (rem == rems) & (back == key) & is_canonical(k, key)
        return key, home, ok

    def with_homes(self, region, homes):
        """one k-mer per entry of homes (a home may come several times: different k-mers)"""
        out = np.zeros(len(homes), U64)
        todo = list(range(len(homes)))
        while todo:
            pick = []
            for i in todo:
                h = int(homes[i]) % self.S
                j = self.starts[h] + self.at[h]
                assert j < self.starts[h + 1], ("no remainder left with home", h, "in region", region)
                self.at[h] += 1
                pick.append(j)
            key, home, ok = self.keys_in(region, self.rems[pick])
            assert (home[ok] == np.asarray([int(homes[i]) % self.S for i in todo])[ok]).all()
            for n, i in enumerate(todo):
                if ok[n]:
                    out[i] = key[n]
            todo = [i for n, i in enumerate(todo) if not ok[n]]
        return out

    def anywhere(self, region, n):
        """n k-mers of the region, with their homes"""
        keys, homes = [], []
        while sum(x.size for x in keys) < n:
            key, home, ok = self.keys_in(region, self.rng.choice(self.rems, 4 * n, replace=False))
            keys.append(key[ok]); homes.append(home[ok])
        keys, homes = np.concatenate(keys), np.concatenate(homes)
        keys, first = np.unique(keys, return_index=True)
        assert keys.size >= n
        return keys[:n], homes[first][:n]


class Model:
    """plain linear probing in regions of S slots: where a k-mer lands and how many slots from its home that is"""

    def __init__(self, S):
        self.S, self.occ = S, {}

    def add(self, region, home, key):
        occ, s = self.occ.setdefault(region, {}), int(home)
        for d in range(self.S):
            if s not in occ:
                occ[s] = int(key)
                return d, True
            if occ[s] == int(key):
                return d, False
            s = s + 1 if s + 1 < self.S else 0
        return self.S, None                                        # the region is full

    def first_free(self, region, home):
        occ, s = self.occ.get(region, {}), int(home)
        for d in range(self.S):
            if s not in occ:
                return d
            s = s + 1 if s + 1 < self.S else 0
        return self.S


def build_calls(k, p1, p2, S, seed):
    """the calls' k-mers; every chain asserted against the model"""
    mk, model = Maker(k, p1, p2, S, seed), Model(S)
    n_reg = p1 * p2
    calls = [[], [], [], []]
    regions = iter((5 + STEP * i) % n_reg for i in range(256))
    homes_of = {}

    def cluster(region, h, d):
        keys = mk.with_homes(region, [h + i for i in range(d)])
        for i, key in enumerate(keys):
            homes_of[int(key)] = (h + i) % S
        return keys

    def new_at(region, h):
        key = mk.with_homes(region, [h])[0]
        while int(key) in homes_of:                                 # (a full region's k-mers are drawn from the same remainders)
            key = mk.with_homes(region, [h])[0]
        homes_of[int(key)] = h % S
        return key

    firsts = []                                                     # (region, its k-mers of call 1, a cluster?)

    chains = []                                                     # (region, x, d): x's first free slot lies d slots from its home once call 1 is in
    for n, d in enumerate(CHAIN_D):
        r, h = next(regions), 8 + (S // 3 + 17 * n) % (S - 64)
        c, x = cluster(r, h, d), new_at(r, h)
        firsts.append((r, c, True)); calls[1].append(np.repeat(x, COPIES)); calls[2].append(np.repeat(x, COPIES))
        chains.append((r, x, d))
        if d == 6:                                                  # a run of more than 4096 k-mers: two segments under KATGPU_TEST_AP_SEG
            calls[2].append(np.resize(c, 4500))
    for j in WRAP_J:
        r, h, d = next(regions), S - 1 - j, j + 3
        c, x = cluster(r, h, d), new_at(r, h)
        assert h + d > S                                            # the free slot lies behind the wrap
        firsts.append((r, c, True)); calls[1].append(np.repeat(x, COPIES)); calls[2].append(np.repeat(x, COPIES))
        chains.append((r, x, d))
    races = []
    for copies, d in ((3, NR_MAX + 1), (64, NR_MAX + 2)):
        r, h = next(regions), S // 2 + copies
        c, x = cluster(r, h, d), new_at(r, h)
        firsts.append((r, c, True)); calls[1].append(np.repeat(x, copies)); calls[2].append(np.repeat(x, copies))
        chains.append((r, x, d))
        races.append((int(x), copies))
        if copies < 8:                                              # company that keeps the pass in phase 1: another new k-mer, COPIES times, behind a cluster of its own
            c, w = cluster(r, h + 40, d + 1), new_at(r, h + 40)
            firsts.append((r, c, True)); calls[1].append(np.repeat(w, COPIES)); calls[2].append(np.repeat(w, COPIES))
            chains.append((r, w, d + 1))
    r, h, d = next(regions), S // 2 - 40, NR_MAX + 1
    c, x, y = cluster(r, h, d), new_at(r, h), new_at(r, h + 1)
    firsts.append((r, c, True)); calls[1].append(np.tile(np.array([x, y], U64), COPIES)); calls[2].append(np.tile(np.array([y, x, y], U64), COPIES))
    pair = (r, int(x), int(y), d)
    r = next(regions)                                               # one pass whose lanes stand at different offsets of their windows and leave it in different iterations
    for n, d in enumerate((3, 5, 7, 8)):
        c, x = cluster(r, 20 + 40 * n, d), new_at(r, 20 + 40 * n)
        firsts.append((r, c, True)); calls[1].append(np.repeat(x, 5)); calls[2].append(np.repeat(x, 5))
        chains.append((r, x, d))
    full = []
    if S == 256:
        for p in range(WINDOW_MAX):
            r = next(regions)
            keys, homes = mk.anywhere(r, S - 1)
            for key, hh in zip(keys, homes):
                homes_of[int(key)] = int(hh)
            firsts.append((r, keys, False))
            full.append([r, p])

    # ---- the model: call 1, then every case's chain ----
    for r, keys, is_cluster in firsts:
        calls[0].append(keys)
        got = [model.add(r, homes_of[int(key)], key) for key in keys]
        assert all(new for _, new in got) and (not is_cluster or all(dist == 0 for dist, _ in got)), (r, got)      # a cluster: every k-mer in its home slot
    for r, x, d in chains:
        assert model.first_free(r, homes_of[int(x)]) == d, (r, d)
    r, x, y, d = pair
    assert model.first_free(r, homes_of[x]) == d and model.first_free(r, homes_of[y]) == d - 1 and (homes_of[x] + d + 1) % S not in model.occ[r]
    for f in full:
        r, p = f
        free = [s for s in range(S) if s not in model.occ[r]]
        assert len(free) == 1, (r, free)
        x = new_at(r, free[0] + 1 + p)
        assert model.first_free(r, homes_of[int(x)]) == S - 1 - p
        calls[1].append(np.array([x], U64)); calls[2].append(np.array([x], U64))
        chains.append((r, x, S - 1 - p))
    # calls 2 and 3 through the model: the claims land at the asserted distance, the matches find them there
    for r, x, d in chains:
        assert model.add(r, homes_of[int(x)], x) == (d, True) and model.add(r, homes_of[int(x)], x) == (d, False), (r, d)
    r, x, y, d = pair
    assert model.add(r, homes_of[x], x) == (d, True) and model.add(r, homes_of[y], y) == (d, True)      # (or y first: x then lands one slot on)
    extra = None
    if full:
        r = full[0][0]
        assert len(model.occ[r]) == S
        extra = mk.anywhere(r, S + 8)
        extra = next((key, hh) for key, hh in zip(*extra) if int(key) not in homes_of)
        assert model.add(r, extra[1], extra[0]) == (S, None)       # no slot left for it
        calls[3].append(np.array([extra[0]], U64))
    used = {r for r, _, _ in chains} | {pair[0]}
    assert len({r % 256 for r in used}) == len(used)               # no two cases on one workgroup's stride
    if full:
        # The direct path probes the k-mer's region only, and the host makes room (a larger table) for a spilled k-mer when the TABLE is past its fill
        # limit -- 0.7 - 3 / sqrt(S) of its slots for small regions (kg_table.hip: load_limit), and a round starts without growing up to 0.6.  So
        # the call that brings the k-mer too many also brings the other regions between the two: 272 000 k-mers once each, 0.52 of 2048 x 256
        # slots (a region gets 133 +- 11 of them: none fills up), in one round of KATGPU_TEST_ROUND_ITEMS.
        bg = canonical_kmers(k, 300_000, seed=seed + 1)
        d1, d2 = place_keys(k, p1, mk.l2, bg)[:2]
        bg = bg[~np.isin(d1.astype(np.int64) * p2 + d2, sorted(used))][:272_000]
        n_slots, limit = n_reg * S, (0.7 - 3.0 / np.sqrt(S)) * n_reg * S
        assert bg.size == 272_000 and limit < bg.size < 0.6 * n_slots and (bg.size + 1) * (k + 1) < 8_000_000, (bg.size, limit)
        calls[3].append(bg)
    return [np.concatenate(c) if c else np.zeros(0, U64) for c in calls], {"races": races, "pair": pair, "full": bool(full), "cases": len(used)}


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
        o1 = ko.Table(k, True).count_bases(b1, threads=8)
        t1 = eng.table(k, True, size_hint=regions * 1024)
        g1 = t1.geometry()
        assert g1.n_regions == regions and g1.region_slots == 1024 and t1.packed_records(), (tag, g1.n_regions, g1.region_slots)
        t1.count_bases_device(buf1.ptr, b1.size)
        same(t1, o1, (tag, "table 1"))
        calls, made = build_calls(k, g1.p1, g1.p2, S, seed=500 + k + S)
        assert made["full"] == (S == 256) and made["cases"] == len(CHAIN_D) + len(WRAP_J) + 4 + (WINDOW_MAX if S == 256 else 0), (tag, made)
        streams = [np.ascontiguousarray(records(k, c)) for c in calls]

        def counted(t2, todo, name):
            """todo: (stream, first sweep?, k-mers the direct path must take or None, last call?) per call"""
            want = ko.Table(k, True)
            for n_call, (stream, first_sweep, direct, last) in enumerate(todo):
                what = (tag, name, "call %d" % (n_call + 1))
                want.count_bases(stream, threads=8)
                buf = eng.alloc(stream.size + 32)
                buf.upload(stream)
                before = len(forms_lines())
                eng.profile_reset()
                t2.count_bases_device(buf.ptr, stream.size)
                units = eng.profile()["count"]["units"]
                seen = forms_lines()[before:]
                print("%s %s call %d | %s | direct path: %d" % (tag, name, n_call + 1, " / ".join(seen), units))
                assert len(seen) == 1, (what, seen)
                assert " hb=%u " % hb in seen[0] and "apply=packed " + shape in seen[0] and seen[0].endswith(" hooked") == (mode == "spill"), (what, seen)
                fresh = int(seen[0].rsplit("fresh=", 1)[1].split()[0])
                assert fresh == (1 if first_sweep and mode != "spill" else 0), (what, seen)      # (the hooked shape has no inline claims)
                if mode != "spill":
                    assert units == direct, (what, "direct path", units, direct)
                if not last:
                    assert t2.regrows == 0 and t2.geometry().region_slots == S, what
                same(t2, want, what)
                for gg, ww, nm in zip(kat_amd.comp(t1, t2), ko.comp(o1, want), ("main", "counters", "spectra")):
                    assert np.array_equal(gg, ww), (what, "comp", nm)

        def table2():
            t2 = eng.table(k, True, size_hint=regions * S, like=t1)
            g2 = t2.geometry()
            assert (g2.p1, g2.p2, g2.region_slots) == (g1.p1, g1.p2, S) and t2.packed_records(), (tag, g2.p1, g2.p2, g2.region_slots)
            return t2

        ta = table2()                                              # every chain built and probed in one walk, the table's first sweep
        counted(ta, [(np.ascontiguousarray(np.concatenate(streams[:3])), True, 0, False)], "table A")
        ta.free()
        tb = table2()                                              # call 1: first sweep; calls 2 .. : the steady shape on the loaded table
        todo = [(streams[0], True, 0, False), (streams[1], False, 0, False), (streams[2], False, 0, False)]
        if S == 256:
            todo.append((streams[3], False, 1, True))              # one k-mer more than the region has slots: the direct path's
        counted(tb, todo, "table B")
        t1.free(); tb.free()
    print("apply drain ok:", mode)


if __name__ == "__main__":
    main()
