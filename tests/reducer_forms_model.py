"""CPU model of the two slot-scan reducers, katgpu_hist and katgpu_gcp (kat_amd/csrc/kg_reduce.hip), and the case lists that run them
through every kernel form at their parameter edges (tests/test_reducer_forms_model.py on the CPU, tests/test_gpu_reducer_forms.py on
the device).

Three parts:
  * hist_model / gcp_model: Histogram::binSlice and Gcp::analyseSlice as oracle/koracle.c restates them (ko_hist, ko_gcp), from a list
    of (key, count) with Python-int keys of up to 126 bits -- plain integers and numpy, nothing of the oracle's code.
  * dispatch / hist_lds_bins / table_geometry: what katgpu_gcp, katgpu_hist and alloc_dev_table decide -- the kernel, the increment
    mode, workgroups per CU, LDS bytes, the slot layout.  The device test compares the library's "reducer form:" trace lines with it.
  * LAYOUTS, HIST_TRIPLES, gcp_args, records: the tables and arguments of the cases."""
import collections
import functools
import math
import random

import numpy as np

from kat_amd import synth

# ---------------------------------------------------------------------------------------------------------------- the reducers


def gc_count(key, k):
    """#G + #C of a 2k-bit k-mer (A=0 C=1 G=2 T=3: the two bits of C and G differ)."""
    mask = int("01" * k, 2)
    return bin((key ^ (key >> 1)) & mask).count("1")


def column(c, scale, bins):
    """Gcp::analyseSlice's column: one IEEE double multiply, ceil, clamp."""
    return min(0 if c == 0 else math.ceil(float(c) * scale), bins)


class Multiset:
    """{k-mer: count} of a list of (key, count) records (a key that comes twice has the sum), as columns: counts (u64) and GC counts."""

    def __init__(self, k, records):
        d = {}
        for key, c in records:
            d[key] = d.get(key, 0) + c
        self.k = k
        self.table = d
        self.keys = list(d)
        self.counts = np.array([d[key] for key in self.keys], np.uint64)
        if k is not None:
            gcs = _gc_memo(k)
            self.gc = np.array([gcs(key) for key in self.keys], np.int64)

    @property
    def distinct(self):
        return len(self.keys)


@functools.lru_cache(maxsize=None)
def _gc_memo(k):
    memo = {}

    def f(key):
        g = memo.get(key)
        if g is None:
            g = memo[key] = gc_count(key, k)
        return g
    return f


def _multiset(records, k):
    return records if isinstance(records, Multiset) else Multiset(k, records)


def hist_model(records, base, ceil, inc, nb):
    """ko_hist: bucket 0 below base, bucket nb - 1 above ceil, (count - base) // inc between."""
    v = records.counts if isinstance(records, Multiset) else Multiset(None, records).counts
    with np.errstate(over="ignore"):
        idx = np.where(v < np.uint64(base), np.uint64(0), np.where(v > np.uint64(ceil), np.uint64(nb - 1), (v - np.uint64(base)) // np.uint64(inc)))
    return np.bincount(idx.astype(np.int64), minlength=nb).astype(np.uint64)


def gcp_model(records, k, scale, bins):
    """ko_gcp: row = GC count (a k-mer of GC == k has no row: dropped), column = min(ceil(double(count) * scale), bins)."""
    m = _multiset(records, k)
    col = np.minimum(np.ceil(m.counts.astype(np.float64) * np.float64(scale)), float(bins)).astype(np.int64)     # (counts are >= 1)
    keep = m.gc < k
    out = np.bincount(m.gc[keep] * (bins + 1) + col[keep], minlength=k * (bins + 1))
    return out.astype(np.uint64).reshape(k, bins + 1)


# ---------------------------------------------------------------------------------------------------------------- the dispatch

HIST_LDS_BINS = 16384                       # k_hist: buckets kept in LDS
LDS_ATTR, LDS_ONE_PER_CU, LDS_LIMIT = 64 * 1024, 75 * 1024, 150 * 1024     # katgpu_gcp's three thresholds
THRESHOLDS = (LDS_ATTR, LDS_ONE_PER_CU, LDS_LIMIT)
SCAN_WAVES = 16                             # waves of a reducer workgroup (SCAN_BLOCK / 64)
KERNEL_OF_SLOT_BYTES = {12: ("flat", "kv12"), 8: ("pk", "pk"), 20: ("wide", "wide")}       # (gcp's name, hist's name)

Form = collections.namedtuple("Form", "kernel use_lds per_cu lds")


def hist_lds_bins(nb):
    return min(nb, HIST_LDS_BINS)


def gcp_lds(k, bins):
    return k * (bins + 1) * 4


def dispatch(k, slot_bytes, bins, plain_inc):
    """katgpu_gcp's choice for a table of this k and layout."""
    lds = gcp_lds(k, bins)
    use_lds = (2 if plain_inc else 1) if lds <= LDS_LIMIT else 0
    per_cu = 1 if use_lds and lds > LDS_ONE_PER_CU else 2
    return Form(KERNEL_OF_SLOT_BYTES[slot_bytes][0], use_lds, per_cu, lds)


def hist_kernel(slot_bytes):
    return KERNEL_OF_SLOT_BYTES[slot_bytes][1]


def table_geometry(k, size_hint, region_slots, packed=True):
    """alloc_dev_table for a one-word table with a test region size: (regions, count bits of a packed slot or 0)."""
    cap = max(size_hint, 1024)
    if cap <= region_slots:
        return 1, 0
    nr = -(-cap // region_slots)
    p2 = 1
    while p2 * p2 < nr:
        p2 += 1
    if k <= 32:
        p2 = 1 << (p2 - 1).bit_length()
    p1 = -(-nr // p2)
    if k > 32:
        return p1 * p2, 0
    l2, hb1 = p2.bit_length() - 1, p1.bit_length() - 1
    n1 = max(2 * k - hb1, 0)
    rb = n1 - min(l2, n1)
    return p1 * p2, (min(64 - rb, 32) if packed and rb + 20 <= 64 else 0)


def reachable_forms(slot_bytes_seen, plain_inc):
    """Every (reducer, kernel, mode, side table in use?) the cases must reach: gcp's three kernels in the LDS mode of the environment and
    with global atomics, k_hist's instantiations and the wide table's with and without global buckets."""
    forms = set()
    for sb in slot_bytes_seen:
        g, h = KERNEL_OF_SLOT_BYTES[sb]
        for ovf in (False, True):
            forms |= {("gcp", g, 2 if plain_inc else 1, ovf), ("gcp", g, 0, ovf), ("hist", h, "lds", ovf), ("hist", h, "global", ovf)}
    return forms


# ---------------------------------------------------------------------------------------------------------------- the cases

Layout = collections.namedtuple("Layout", "name k size_hint region_slots slot_bytes")
REGION_SLOTS = 256
LAYOUTS = (
    Layout("kv12", 32, 1 << 20, 256, 12),                  # k = 32 leaves a slot word no count bits at this size; holds the all-T key
    Layout("pk32", 15, 1 << 20, 256, 8),                   # count bits capped at 32
    Layout("pk22", 27, 1 << 20, 256, 8),                   # 4096 regions: 22 count bits
    Layout("pkmany", 27, 9216 * 256, 256, 8),              # more regions than waves in k_gcp_pk's grid (16 * 2 * 256 CUs): a second region per wave
    Layout("pk512", 27, 1 << 20, 512, 8),                  # 128 quads per region: k_gcp_pk's quad loop repeats
    Layout("wide", 51, 1 << 20, 256, 20),
)
LAYOUT = {la.name: la for la in LAYOUTS}
MANY_REGIONS = 16 * 2 * 256

HIST_TRIPLES = ((1, 16382, 1), (1, 16383, 1), (1, 16384, 1), (1, 100000, 1), (1, 100000, 7), (50, 40000, 3), (3, 3, 1))
SCALES = (1.0, 0.37, 3.0, 0.5)
# the large scale: a count below 2^32 lands beyond 2^32 (the packed kernel's 32-bit path saturates there).  Tables that hold 2^53 + 1
# take 1000.0: the reference casts ceil(count * scale) to 64 bits, which is undefined from 2^63 on, and (2^53 + 1) * 5000 is beyond.
BIG_SCALE = {"a": 5000.0, "b": 1000.0}
HALF_BINS = 1000                             # scale 0.5: counts around 2 * HALF_BINS are exactly integral at the last columns
GLOBAL_BINS = 5000                           # k * 5001 * 4 > 150 KiB for every k of the layouts
ALL_ONES_COUNT = {"a": 1, "b": 50000}        # k = 32: below the bases 49 and 2 / inside every range that starts at 1; above the ceilings up to 40001 / inside (1, 100000, *)


def hist_geometry(low, high):
    base = low - 1 if low > 1 else 1
    return base, high + 1, high + 2 - base


def threshold_bins(k):
    """Per LDS threshold the last bins value at or under it and the first one over: exactly at the threshold where 4k divides it."""
    out = []
    for t in THRESHOLDS:
        b = t // (4 * k) - 1
        out += [b, b + 1]
    return out


def gcp_args(k, twin):
    big = BIG_SCALE[twin]
    tb = threshold_bins(k)
    others = (0.37, 3.0, 0.5, big)
    args = [(1.0, b) for b in tb] + [(others[i % 4], b) for i, b in enumerate(tb)]
    args += [(s, HALF_BINS) for s in (1.0,) + others] + [(0.5, 100)]
    args += [(s, GLOBAL_BINS) for s in (1.0, 0.37, 0.5, big)]
    return args


def limit_in_slot(cbits):
    """The largest count one add leaves in the slot alone: 2^32 - 1 in a 32-bit counter; a packed slot keeps 1 .. 2^(cbits - 1) and hands
    the rest to the side table (kg_device.hpp: table_add_pk)."""
    return (1 << (cbits - 1)) if cbits else (1 << 32) - 1


def edge_counts(k):
    """Counts that land on every edge of the hist and gcp arguments."""
    s = set(range(1, 9))
    for low, high, inc in HIST_TRIPLES:
        base, ceil, nb = hist_geometry(low, high)
        lb = hist_lds_bins(nb)
        s |= {base - 1, base, base + inc - 1, base + inc, ceil - 1, ceil, ceil + 1, ceil + inc}
        s |= {base + inc * (lb - 1), base + inc * lb - 1, base + inc * lb, base + inc * (lb + 1) - 1}
    for b in threshold_bins(k) + [HALF_BINS, 100, GLOBAL_BINS]:
        s |= {b - 1, b, b + 1}
        for scale in (0.37, 3.0, 0.5):
            c = int(b / scale)
            s |= set(range(c - 3, c + 4))
    s |= {(1 << 32) // 5000 - 1, (1 << 32) // 5000, (1 << 32) // 5000 + 1, (1 << 32) // 1000, (1 << 32) // 1000 + 1}     # the large scales cross 2^32 here
    return sorted(c for c in s if c >= 1)


def big_counts(cbits):
    """What only the side table can hold, and the counts on either side of the slot's own limit."""
    s = {(1 << 32) - 1, 1 << 32, (1 << 40) + 3, (1 << 53) + 1}
    if cbits:
        s |= {(1 << (cbits - 1)) + 1, (1 << cbits) - 1, 1 << cbits}
    return sorted(s)


def special_keys(k):
    all_g = int("10" * k, 2)
    keys = {"all_a": 0, "gc1": 1, "gc_k_minus_1": all_g & ~3, "all_g": all_g}
    if k == 32:
        keys["all_ones"] = (1 << 64) - 1
    return keys


@functools.lru_cache(maxsize=None)
def stream():
    """About 240 kilobases: a genome as contigs and reads of it at three-fold coverage."""
    g = synth.genome(60000, seed=29)
    return np.concatenate([synth.stream_of_contigs(g, 20000), synth.reads(g, 0, 1200, seed=3)])


@functools.lru_cache(maxsize=None)
def stream_records(k):
    """The forward k-mers of stream() with their counts, by a rolling Python integer: [(key, count)]."""
    code = {ord(c): v for v, c in enumerate("ACGT")}
    code.update({ord(c): v for v, c in enumerate("acgt")})
    mask = (1 << (2 * k)) - 1
    d, x, run = {}, 0, 0
    for b in stream().tobytes():
        v = code.get(b)
        if v is None:
            run = 0
            continue
        x = ((x << 2) | v) & mask
        run += 1
        if run >= k:
            d[x] = d.get(x, 0) + 1
    return list(d.items())


N_CRAFTED = 3000


@functools.lru_cache(maxsize=None)
def crafted(name):
    """{"a": records, "b": records} of a layout: the same keys in both twins.  Twin a keeps every count in its slot (no side-table entry
    under either layout the table can take); in twin b a handful of keys hold big_counts.  No crafted key but the special ones may be a
    k-mer of the stream, so the stream cannot lift a count of twin a over the slot's limit."""
    la = LAYOUT[name]
    k = la.k
    cbits = table_geometry(k, la.size_hint, la.region_slots)[1]
    limit = limit_in_slot(cbits)
    sp = special_keys(k)
    taken = set(sp.values()) | {key for key, _ in stream_records(k)}
    rng = random.Random(1000 + k + la.region_slots)
    fill = []
    while len(fill) < N_CRAFTED:
        key = rng.getrandbits(2 * k)
        if key not in taken:
            taken.add(key)
            fill.append(key)
    edges = [c for c in edge_counts(k) if c <= limit]
    counts = edges + [limit - 1, limit]
    while len(counts) < N_CRAFTED:                                # the bulk: low counts, a tail up to the widest histogram
        r = rng.random()
        counts.append(rng.randint(1, 40) if r < 0.6 else rng.randint(1, 20000) if r < 0.9 else rng.randint(1, 110000))
    a = list(zip(fill, counts))
    # the special keys: counts that put them on interior columns and buckets
    a += [(sp["all_a"], 7), (sp["gc1"], 600), (sp["gc_k_minus_1"], 16384), (sp["all_g"], 3)]
    b = list(a)
    big = big_counts(cbits)
    for i, c in enumerate(big):                                   # (the first records are the edge counts: a key per big count, from the bulk)
        b[len(edges) + 10 + i] = (fill[len(edges) + 10 + i], c)
    b[-2] = (sp["gc_k_minus_1"], (1 << 40) + 3)                   # the row of a k-mer whose count lies in the side table
    if "all_ones" in sp:
        a.append((sp["all_ones"], ALL_ONES_COUNT["a"]))
        b.append((sp["all_ones"], ALL_ONES_COUNT["b"]))
    return {"a": a, "b": b}


def records(name, twin):
    """Everything a table of the case holds: the crafted records and the stream's k-mers."""
    return crafted(name)[twin] + stream_records(LAYOUT[name].k)


LAZY_KEYS = ((5, 3), (77, 12), (1234567, 1), (999, (1 << 23) + 5), (4242, 1 << 22), (0, 2))      # first merge into an uncleared packed table (k = 21)
LAZY_K, LAZY_HINT = 21, 1 << 16
