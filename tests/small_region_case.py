"""Run in a subprocess by tests/test_gpu_small_region_apply.py (the hooks are read when the library loads): the packed apply on small regions
(kat_amd/csrc/kg_partition.hpp: k_p3_apply_pk, the `S <= 4096` shapes of kg_count.hip's apply_pk_shape) and the first shape that is not.

Table 1: about a million bases of reads and a poly-A run of 3000, on a grid of 2048 regions.  Table 2 is made `like=` table 1 with a hint that
gives its regions 256 slots (the floor of a shared grid), 3080 (the bench's second input: no multiple of 1024), 4096 (the last small shape) or
4100 (the first that is not), and counts a stream of single-k-mer records whose runs are constructed with kat_amd.binding.place_keys and
asserted from it: a region with 2048 items (one chunk for each of the eight waves), its neighbour with none, the next with 2049, a region with
one item, the poly-A's region with more than the waves' first chunks hold, and two thousand k-mers elsewhere.  Every table starts uncleared
(KATGPU_TEST_LAZY_MIN_SLOTS=0: the first sweep starts its regions from zeros).

  small_region_case.py one   the stream in one round (a first round from zeros), then a second count call into the same table (the table is loaded)
  small_region_case.py two   the stream in two rounds (KATGPU_TEST_ROUND_ITEMS: the second loads the table)

After every count: the trace's "partition forms" lines (KP = 4 up to 4096 slots, 10 beyond; inline claims in the first round only), the dump
and the statistics against the oracle, and comp(table 1, table 2) -- matrix, 13 counters, spectra -- against the oracle's, exactly."""
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
from tests.comp_sweep_case import canonical_kmers  # noqa: E402

K = 27
SIZES = (256, 3080, 4096, 4100)
TRACE = tempfile.NamedTemporaryFile(prefix="small_region_trace_", suffix=".txt")
STDERR = os.dup(2)
os.dup2(TRACE.fileno(), 2)                  # the library's trace lines: looked at per count ...


@atexit.register
def _trace_to_parent():                     # ... and handed on
    sys.stderr.flush()
    os.dup2(STDERR, 2)
    with open(TRACE.name) as f:
        sys.stderr.write(f.read())


MARK = "[katgpu] partition forms: "


def forms_lines():
    with open(TRACE.name) as f:
        return [line[len(MARK):].strip() for line in f if line.startswith(MARK)]


def records(keys):
    """one record per k-mer: its K bases and an N"""
    keys = np.asarray(keys, np.uint64)
    out = np.full((keys.size, K + 1), ord("N"), np.uint8)
    for i in range(K):
        out[:, i] = synth.ACGT[((keys >> np.uint64(2 * (K - 1 - i))) & np.uint64(3)).astype(np.uint8)]
    return out


def stream_for(p1, p2):
    """the second table's stream and the regions (r, q, a) of its constructed runs: r 2048 items, r + 1 none, r + 2 2049, q one, a the poly-A's"""
    l2 = int(p2).bit_length() - 1
    cand = canonical_kmers(1_000_000, seed=11)
    d1, d2, _, back, _ = place_keys(K, p1, l2, cand)
    assert (back == cand).all()
    region = d1.astype(np.int64) * p2 + d2
    z1, z2 = place_keys(K, p1, l2, np.zeros(1, np.uint64))[:2]
    a = int(z1[0]) * p2 + int(z2[0])                                   # poly-A: the all-zero k-mer
    per = np.bincount(region, minlength=p1 * p2)
    r = next(x for x in range(p1 * p2 - 3) if per[x] >= 64 and per[x + 2] >= 65 and a not in (x, x + 1, x + 2))
    q = next(x for x in range(r + 3, p1 * p2) if per[x] >= 1 and x != a)
    k_r, k_r2, k_q = cand[region == r][:64], cand[region == r + 2][:65], cand[region == q][:1]
    elsewhere = cand[~np.isin(region, (r, r + 1, r + 2, q, a))][:2000]
    keys = np.concatenate([np.repeat(k_r, 32), np.repeat(k_r2[:64], 32), k_r2[64:], k_q, elsewhere])
    np.random.default_rng(5).shuffle(keys)
    half = keys.size // 2
    stream = np.concatenate([records(keys[:half]).ravel(), np.frombuffer(b"A" * 3000 + b"N", np.uint8), records(keys[half:]).ravel()])
    assert stream.size <= 200_000
    return np.ascontiguousarray(stream), (r, q, a)


def runs_are_as_constructed(o, p1, p2, r, q, a):
    keys, counts = o.dump_sorted()
    d1, d2 = place_keys(K, p1, int(p2).bit_length() - 1, keys)[:2]
    items = np.bincount(d1.astype(np.int64) * p2 + d2, weights=counts.astype(np.float64), minlength=p1 * p2).astype(np.int64)
    assert (items[r], items[r + 1], items[r + 2], items[q]) == (2048, 0, 2049, 1), (items[r], items[r + 1], items[r + 2], items[q])
    assert items[a] == 3000 - K + 1 and items[a] > 8 * 256, items[a]      # beyond the eight waves' first chunks: the chunk loop


def same(t, o, what):
    gk, gc = t.dump_sorted()
    wk, wc = o.dump_sorted()
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc), (what, "dump differs", gk.size, wk.size)
    st = t.stats()
    assert st["distinct"] == wk.size and st["total"] == int(wc.sum(dtype=np.uint64)), (what, st)


def main():
    mode = sys.argv[1]
    assert os.environ["KATGPU_TEST_REGION_SLOTS"] == "1024" and os.environ["KATGPU_TEST_LAZY_MIN_SLOTS"] == "0"
    assert int(os.environ["KATGPU_TEST_ROUND_ITEMS"]) == (4_000_000 if mode == "one" else 70_000)
    eng = kat_amd.Engine(0)
    genome = synth.genome(200_000, seed=21)
    b1 = np.ascontiguousarray(np.concatenate([synth.reads(genome, 0, 6600, seed=2), np.frombuffer(b"A" * 3000 + b"N", np.uint8)]))
    o1 = ko.Table(K, True).count_bases(b1, threads=8)
    buf1 = eng.alloc(b1.size + 32)
    buf1.upload(b1)
    b2 = o2 = buf2 = None
    for S in SIZES:
        t1 = eng.table(K, True, size_hint=2 << 20)
        g1 = t1.geometry()
        assert g1.n_regions == 2048 and g1.region_slots == 1024 and t1.packed_records(), (g1.n_regions, g1.region_slots)
        t1.count_bases_device(buf1.ptr, b1.size)
        same(t1, o1, (S, "table 1"))
        if b2 is None:
            b2, (r, q, a) = stream_for(g1.p1, g1.p2)
            o2 = ko.Table(K, True).count_bases(b2)
            runs_are_as_constructed(o2, g1.p1, g1.p2, r, q, a)
            o2_twice = ko.Table(K, True).count_bases(b2).count_bases(b2)
            buf2 = eng.alloc(b2.size + 32)
            buf2.upload(b2)
        t2 = eng.table(K, True, size_hint=2048 * S, like=t1)
        g2 = t2.geometry()
        assert (g2.p1, g2.p2, g2.region_slots) == (g1.p1, g1.p2, S) and t2.packed_records(), (S, g2.p1, g2.p2, g2.region_slots)
        kp = "KP=4 " if S <= 4096 else "KP=10 "
        total = int(o2.dump_sorted()[1].sum(dtype=np.uint64))
        calls = ((o2, "first call"), (o2_twice, "second call")) if mode == "one" else ((o2, "two rounds"),)
        for n_call, (want, what) in enumerate(calls):
            before = len(forms_lines())
            eng.profile_reset()
            t2.count_bases_device(buf2.ptr, b2.size)
            prof = eng.profile()
            seen = forms_lines()[before:]
            print("S=%u %s | %s" % (S, what, " / ".join(seen)))
            assert len(seen) == 1 if mode == "one" else len(seen) >= 2, (S, what, seen)
            assert all("apply=packed B=512 " + kp in line for line in seen), (S, what, seen)
            fresh = [int(line.rsplit("fresh=", 1)[1].split()[0]) for line in seen]
            assert fresh == [1 if n_call == 0 else 0] + [0] * (len(seen) - 1), (S, what, seen)
            assert prof["count"]["units"] <= total // 100, (S, what, "direct path", prof["count"]["units"], total)
            assert t2.regrows == 0 and t2.geometry().region_slots == S
            same(t2, want, (S, what))
            for gg, ww, name in zip(kat_amd.comp(t1, t2), ko.comp(o1, want), ("main", "counters", "spectra")):
                assert np.array_equal(gg, ww), (S, what, "comp", name)
        t1.free(); t2.free()
    print("small regions ok:", mode)


if __name__ == "__main__":
    main()
