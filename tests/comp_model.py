"""CPU model of the comparison reducers, katgpu_comp and katgpu_comp3 (kat_amd/csrc/kg_reduce.hip), and the case lists that drive the
three-input form and the slot-less 32-mer through every branch (tests/test_comp_model.py on the CPU, tests/test_gpu_comp3.py with
tests/comp3_case.py on the device).

Three parts:
  * comp_model / comp3_model: Comp::compareSlice as include/katgpu.h states it for katgpu_comp / katgpu_comp3, from lists of
    (key, count) with Python-int keys of up to 126 bits -- plain integers and numpy, nothing of the oracle's code; the reverse
    complement is written here.
  * comp_forms / geometry: what katgpu_comp and alloc_dev_table decide for the tables of a case -- which kernel form takes each
    pass, the slot layout.  The device test compares the library's "reducer form:" trace lines with it.
  * LAYOUTS, cases(), records(): the tables and arguments of the cases.

The grids.  Every table 1 has a size hint of 2^20: 4096 regions of 256 slots (KATGPU_TEST_REGION_SLOTS=256), 2^20 slots and the
virtual slot `cap` of the all-ones key behind them.  grid_for(items, 256, per_cu) launches min(ceil(items / 256), n_cu * per_cu)
workgroups of 256 threads.  k_comp3_pass1 asks for 3 per CU: on 256 CUs that is min(4097, 768) = 768 workgroups, 196608 threads,
so 2^20 + 1 slots take ceil(1048577 / 196608) = 6 grid-stride rounds, and the virtual slot is the only one of the sixth (thread 65536's
sixth item: block 256, lane 0).  k_comp3_pass3 asks for 8 per CU: min(4097, 2048) = 2048 workgroups, 524288 threads, so a table 3
of 2^20 + 1 slots takes 3 rounds, the third for slot `cap` alone (block 0, thread 0).  Table 3 of the cases has a size hint of its
own, 2^15: 129 workgroups, one round, slot `cap` the first thread of a last block that is otherwise idle.  The case "big3" swaps the
two hints so that pass 3 runs its three rounds as well, and pass 1 a single one."""
import collections
import functools
import itertools
import math
import random

import numpy as np

from tests.reducer_forms_model import big_counts, table_geometry

# ---------------------------------------------------------------------------------------------------------------- the reducers

M64 = (1 << 64) - 1
ALL_ONES = M64                                # the 32-mer of 32 T: the empty-slot mark of a KV12 table, counted outside the slots
(H1_TOTAL, H2_TOTAL, H3_TOTAL, H1_DISTINCT, H2_DISTINCT, H3_DISTINCT, H1_ONLY_TOTAL, H2_ONLY_TOTAL, H1_ONLY_DISTINCT, H2_ONLY_DISTINCT,
 SH_H1_TOTAL, SH_H2_TOTAL, SH_DISTINCT) = range(13)


@functools.lru_cache(maxsize=None)
def revcomp(x, k):
    """Reverse complement of a 2k-bit k-mer (A=0 C=1 G=2 T=3: the complement of a base is 3 - base)."""
    r = 0
    for _ in range(k):
        r = (r << 2) | (3 - (x & 3))
        x >>= 2
    return r


def canonical(x, k):
    return min(x, revcomp(x, k))


def scaled(c, scale, bins):
    """Comp::scaleCounter and the clamp to the matrix: one IEEE double multiply, ceil, at most bins - 1."""
    return min(unclamped(c, scale), bins - 1)


def unclamped(c, scale):
    return 0 if c == 0 else math.ceil(float(c) * scale)


def table_of(records):
    d = {}
    for key, c in records:
        d[key] = d.get(key, 0) + c
    return d


def _dense(cells, shape):
    out = np.zeros(shape, np.uint64)
    for at, n in cells.items():
        out[at] = n
    return out


def comp_model(rec1, rec2, k, canon2, d1_scale=1.0, d2_scale=1.0, d1_bins=1001, d2_bins=1001):
    """katgpu_comp: (main matrix, 13 counters, 4 x min(bins) spectra)."""
    t1, t2 = table_of(rec1), table_of(rec2)
    ss = min(d1_bins, d2_bins)
    main, spec, cc = collections.Counter(), collections.Counter(), [0] * 13
    for key, c1 in t1.items():                                  # pass 1: the probe is canonical iff input 2 is
        c2 = t2.get(canonical(key, k) if canon2 else key, 0)
        cc[H1_TOTAL] += c1
        cc[H1_DISTINCT] += 1
        spec[0, min(c1, ss - 1)] += 1
        if c2 == 0:
            cc[H1_ONLY_TOTAL] += c1
            cc[H1_ONLY_DISTINCT] += 1
        else:
            cc[SH_H1_TOTAL] += c1
            cc[SH_H2_TOTAL] += c2
            cc[SH_DISTINCT] += 1
            spec[2, min(c1, ss - 1)] += 1
            spec[3, min(c2, ss - 1)] += 1
        main[scaled(c1, d1_scale, d1_bins), scaled(c2, d2_scale, d2_bins)] += 1
    for key, c2 in t2.items():                                  # pass 2: the probe is always canonical
        cc[H2_TOTAL] += c2
        cc[H2_DISTINCT] += 1
        spec[1, min(c2, ss - 1)] += 1
        if canonical(key, k) not in t1:
            cc[H2_ONLY_TOTAL] += c2
            cc[H2_ONLY_DISTINCT] += 1
            main[0, scaled(c2, d2_scale, d2_bins)] += 1
    return _dense(main, (d1_bins, d2_bins)), np.array(cc, np.uint64), _dense(spec, (4, ss))


Kmer3 = collections.namedtuple("Kmer3", "key c1 c2 c3 u1 u2 u3 s1 s2 s3 which")      # u: scaled, s: scaled and clamped; which: 0 ends, 1 middle, 2 mixed


def comp3_kmers(rec1, rec2, rec3, k, canon2, canon3, d1_scale, d2_scale, d1_bins, d2_bins):
    """What the third pass over input 1 sees of each of its k-mers."""
    t2, t3 = table_of(rec2), table_of(rec3)
    for key, c1 in table_of(rec1).items():
        can = canonical(key, k)
        c2, c3 = t2.get(can if canon2 else key, 0), t3.get(can if canon3 else key, 0)
        u1, u2, u3 = unclamped(c1, d1_scale), unclamped(c2, d2_scale), unclamped(c3, d2_scale)
        s1, s2, s3 = min(u1, d1_bins - 1), min(u2, d2_bins - 1), min(u3, d2_bins - 1)
        yield Kmer3(key, c1, c2, c3, u1, u2, u3, s1, s2, s3, 0 if s2 == s3 else 2 if s3 > 0 else 1)      # decided on the clamped values


def comp3_model(rec1, rec2, rec3, k, canon2, canon3, d1_scale=1.0, d2_scale=1.0, d1_bins=1001, d2_bins=1001):
    """katgpu_comp3: (main, ends, middle, mixed, 13 counters, spectra); row = scaled count in input 1, column = in input 3."""
    main, cc, sp = comp_model(rec1, rec2, k, canon2, d1_scale, d2_scale, d1_bins, d2_bins)
    mx = [collections.Counter() for _ in range(3)]
    for m in comp3_kmers(rec1, rec2, rec3, k, canon2, canon3, d1_scale, d2_scale, d1_bins, d2_bins):
        mx[m.which][m.s1, m.s3] += 1
    t3 = table_of(rec3)
    cc[H3_TOTAL], cc[H3_DISTINCT] = sum(t3.values()), len(t3)
    return (main,) + tuple(_dense(m, (d1_bins, d2_bins)) for m in mx) + (cc, sp)


# ---------------------------------------------------------------------------------------------------------------- the dispatch

REGION_SLOTS = 256
HINT1, HINT2_OWN, HINT3 = 1 << 20, 1 << 18, 1 << 15
COMP_TILE = 64

Layout = collections.namedtuple("Layout", "name k slot_bytes hooks")
LAYOUTS = (
    Layout("kv12", 32, 12, {}),                               # k = 32 leaves a slot word no count bits at these sizes; holds the all-ones key
    Layout("pk", 27, 8, {}),                                  # 22 count bits at 4096 regions, 20 at 1024, 17 at 128
    Layout("kv12hook", 27, 12, {"KATGPU_NO_PACKED": "1"}),     # pk's records in KV12 slots
    Layout("wide", 51, 20, {}),
)
LAYOUT = {la.name: la for la in LAYOUTS}


def geometry(la, hint, hooks):
    """(regions, count bits) of a table of the layout made with this size hint."""
    return table_geometry(la.k, hint, REGION_SLOTS, packed="KATGPU_NO_PACKED" not in hooks)


def comp_forms(la, strands, like, hooks, cbits1):
    """katgpu_comp's choice: (form of pass 1, form of pass 2).  Tables of these sizes are small either way: a legal join is taken."""
    s1, s2, _ = strands
    same_grid = la.k <= 32 and like and "KATGPU_NO_JOIN" not in hooks
    if same_grid and cbits1 and s1 and s2 and "KATGPU_NO_FUSED" not in hooks:
        return "fused", "fused"
    join1 = same_grid and (s1 or not s2)                        # the probe key of pass 1 is the stored key
    if join1 and s1 and s2 and "KATGPU_NO_SEEN" not in hooks:   # (no case with canonical tables holds the all-ones key in table 2)
        return "join", "seen"
    return "join" if join1 else "probe", "join" if same_grid and s2 else "probe"


def fold(args, hooks):
    d1s, d2s, d1b, d2b = args
    return int("KATGPU_NO_FOLD" not in hooks and d1s == 1.0 and d2s == 1.0 and d1b > COMP_TILE and d2b > COMP_TILE)


# the runs of the device test: (layout, hooks beside the layout's own).  The probes-only run for every layout, the two-pass join
# where the default is the fused one, and pk's tables left uncleared until their first sweep
RUNS = (("kv12", {}), ("kv12", {"KATGPU_NO_JOIN": "1"}),
        ("pk", {}), ("pk", {"KATGPU_NO_JOIN": "1"}), ("pk", {"KATGPU_NO_FUSED": "1"}), ("pk", {"KATGPU_TEST_LAZY_MIN_SLOTS": "1"}),
        ("kv12hook", {}), ("kv12hook", {"KATGPU_NO_JOIN": "1"}),
        ("wide", {}), ("wide", {"KATGPU_NO_JOIN": "1"}))

# the forms of the "reducer form: comp" line that tables of these layouts reach (pass 1 and pass 2 both as a join needs KATGPU_NO_SEEN
# or KATGPU_FORCE_JOIN: tests/test_gpu_comp_forms.py)
REACHABLE_COMP_FORMS = {("fused", "fused"), ("join", "seen"), ("join", "probe"), ("probe", "join"), ("probe", "probe")}

# ---------------------------------------------------------------------------------------------------------------- the cases

C1 = (1, 2, 3, 4, 63, 64, 65, 200, 201, 1000, 5000)
C23 = (0, 1, 3, 4, 63, 64, 65, 100, 101, 900)                  # 0: the table does not hold the key
TRIPLES = tuple(itertools.product(C1, C23, C23))
N_EXTRA = 20                                                   # keys of table 2 only, of table 3 only, of tables 2 and 3 but not 1: each
PALINDROME_COUNTS = ((5, 7, 7), (2, 0, 3), (64, 65, 1), (300, 4, 0))     # even k: k-mers that are their own reverse complement
STRANDS = ((True, True, True), (False, False, False), (False, True, False), (False, False, True), (True, False, True))
ARGS = ((1.0, 1.0, 1001, 1001), (1.0, 1.0, 201, 101), (1.0, 1.0, 64, 65), (1.0, 1.0, 65, 64), (0.3, 4.0, 20, 9), (0.5, 0.5, 300, 130), (1.0, 1.0, 1, 1))
REACH_ARGS, HALF_ARGS = ARGS[1], ARGS[5]
ONES_COUNTS = (1, 50000)

# name; layout; canonical flags of the three tables; side: the table whose counts reach its side table (0: none); likes: table 2 made
# like= table 1 (True), on its own grid (False), or each in turn; ones / polya: the counts of the all-ones key / of poly-A per table;
# empty: the table that holds nothing (0: none); hints: the size hints of the three tables
Case = collections.namedtuple("Case", "name layout strands side likes ones polya empty hints")


def strand_name(strands):
    return "".join("TF"[not s] for s in strands)


def base_strands(la):
    """Where a case is not about strands: canonical tables, but the k = 32 layout non-canonical (it alone keeps the all-ones key)."""
    return STRANDS[1] if la.k == 32 else STRANDS[0]


@functools.lru_cache(maxsize=None)
def cases(name):
    """The cases of a layout.  Pruned from the full product layout x strands x side table x grid of table 2 x all-ones x empty x
    arguments; every case runs every tuple of ARGS.  What runs:
      * every strand set with no side-table count, table 2 like= table 1 and on its own grid;
      * every side-table variant at the layout's base strands: table 1; table 2 like= table 1 and on its own grid (two cases: the
        slot's limit follows the grid); table 3.  Table 2 is on its own grid where the side table is 1's or 3's;
      * the empty tables and big3 at the base strands, table 2 like= table 1 (empty 1, 2) or on its own grid (empty 3, big3);
      * k = 32: the all-ones cases at non-canonical table 1 (the all-ones key is never canonical).
    Left out: side-table counts in more than one table at once and under the four other strand sets; side-table counts together
    with the all-ones key; empty tables under other strand sets; table 3 like= table 1; the all-ones key under canonical table 1."""
    la = LAYOUT[name]
    base, hints = base_strands(la), (HINT1, None, HINT3)        # (table 2's hint follows from like)
    out = [Case("strands-" + strand_name(st), name, st, 0, (True, False), (0, 0, 0), (0, 0, 0), 0, hints) for st in STRANDS]
    out += [Case("side1", name, base, 1, (False,), (0, 0, 0), (0, 0, 0), 0, hints),
            Case("side2-like", name, base, 2, (True,), (0, 0, 0), (0, 0, 0), 0, hints),
            Case("side2-own", name, base, 2, (False,), (0, 0, 0), (0, 0, 0), 0, hints),
            Case("side3", name, base, 3, (False,), (0, 0, 0), (0, 0, 0), 0, hints)]
    out += [Case("empty1", name, base, 0, (True,), (0, 0, 0), (0, 0, 0), 1, hints),
            Case("empty2", name, base, 0, (True,), (0, 0, 0), (0, 0, 0), 2, hints),
            Case("empty3", name, base, 0, (False,), (0, 0, 0), (0, 0, 0), 3, hints),
            Case("big3", name, base, 0, (False,), (0, 0, 0), (0, 0, 0), 0, (HINT3, None, HINT1))]
    if la.k == 32:
        one, many = ONES_COUNTS
        fff, ftf, fft = STRANDS[1], STRANDS[2], STRANDS[3]
        out += [Case("ones-1", name, fff, 0, (True, False), (many, 0, 0), (0, 0, 0), 0, hints),
                Case("ones-2", name, fff, 0, (True, False), (0, one, 0), (0, 0, 0), 0, hints),
                Case("ones-3", name, fff, 0, (False,), (0, 0, many), (0, 0, 0), 0, hints),
                Case("ones-all", name, fff, 0, (True, False), (one, many, one), (0, 0, 0), 0, hints),
                Case("ones-1-fft", name, fft, 0, (True, False), (many, 0, 0), (0, 0, 0), 0, hints),      # join pass 1 with the tail, canonical table 3 without poly-A
                # table 1 holds poly-T as it is; a canonical table holds poly-A: the canonicalised probe turns the all-ones key into 0
                Case("polya-2", name, ftf, 0, (True, False), (many, 0, one), (0, 3, 0), 0, hints),
                Case("polya-3", name, fft, 0, (True, False), (one, many, 0), (0, 0, 100), 0, hints),
                Case("polya-big3", name, fft, 0, (False,), (one, 0, 0), (7, 0, many), 0, (HINT3, None, HINT1))]
    return tuple(out)


def hint2(case, like):
    return case.hints[0] if like else HINT2_OWN


def cbits_of(case, table, like, hooks):
    la = LAYOUT[case.layout]
    hint = hint2(case, like) if table == 2 else case.hints[table - 1]
    return geometry(la, hint, hooks)[1]


@functools.lru_cache(maxsize=None)
def kmer_pool(k):
    """Distinct random k-mers, no two of them a reverse-complement pair, none poly-A or poly-T: [(k-mer, flip in table 2, flip in table 3)].
    A non-canonical table 2 or 3 stores a flipped k-mer only as its reverse complement."""
    rng = random.Random(4000 + k)
    taken = {0}
    pool = []
    while len(pool) < len(TRIPLES) + 3 * N_EXTRA:
        x = rng.getrandbits(2 * k)
        c = canonical(x, k)
        if c not in taken and x != revcomp(x, k):
            taken.add(c)
            pool.append((x, rng.getrandbits(1), rng.getrandbits(1)))
    return pool


def palindromes(k):
    if k % 2:
        return []
    rng = random.Random(77 + k)
    out = []
    for _ in PALINDROME_COUNTS:
        h = rng.getrandbits(k)
        out.append((h << k) | revcomp(h, k // 2))
    return out


def stored(x, k, table_canonical, flip):
    """The key under which a table of this strand mode holds k-mer x (merge_host does not canonicalise: the case does)."""
    if table_canonical:
        return canonical(x, k)
    return revcomp(x, k) if flip else x


@functools.lru_cache(maxsize=None)
def records(case):
    """(records of table 1, of table 2, of table 3), each a tuple of (key, count)."""
    la = LAYOUT[case.layout]
    k = la.k
    pool = kmer_pool(k)
    nt = len(TRIPLES)
    nonzero = [c for c in C23 if c]
    entries = [pool[i] + TRIPLES[i] for i in range(nt)]                                                           # (x, flip2, flip3, c1, c2, c3)
    for j in range(N_EXTRA):
        entries.append(pool[nt + j] + (0, nonzero[j % len(nonzero)], 0))
        entries.append(pool[nt + N_EXTRA + j] + (0, 0, nonzero[(j + 2) % len(nonzero)]))
        entries.append(pool[nt + 2 * N_EXTRA + j] + (0, nonzero[(j + 4) % len(nonzero)], nonzero[j % 3]))
    entries += [(x, 0, 0) + c for x, c in zip(palindromes(k), PALINDROME_COUNTS)]
    flags = case.strands
    keys = [tuple(stored(e[0], k, flags[t], (0, e[1], e[2])[t]) for t in range(3)) for e in entries]
    counts = [list(e[3:]) for e in entries]
    if case.side:
        # a handful of the triple keys that this table holds, and that pass 1 finds there, take the counts only a side table can hold
        t = case.side - 1
        big = big_counts(cbits_of(case, case.side, case.likes[0], la.hooks))       # (around the slot's limit, which follows the layout)
        cand = [i for i in range(nt) if counts[i][t] and (t == 0 or (canonical(keys[i][0], k) if flags[t] else keys[i][0]) == keys[i][t])]
        step = len(cand) // len(big)
        for j, c in enumerate(big):
            counts[cand[j * step + step // 2]][t] = c
    recs = [[(keys[i][t], counts[i][t]) for i in range(len(entries)) if counts[i][t]] for t in range(3)]
    for t in range(3):
        if case.ones[t]:
            recs[t].append((ALL_ONES, case.ones[t]))
        if case.polya[t]:
            recs[t].append((0, case.polya[t]))
    if case.empty:
        recs[case.empty - 1] = []
    return tuple(tuple(r) for r in recs)


def side_tables(case):
    """Which of the three tables must report side-table entries."""
    return tuple(case.side == t + 1 for t in range(3))


# ---------------------------------------------------------------------------------------------------------------- the second witness

def oracle_tables(case, recs):
    """The oracle's tables of a case (oracle/koracle.py: what tests/test_oracle_vs_reference.py pins to the reference's own classes)."""
    from oracle import koracle as ko
    la = LAYOUT[case.layout]
    out = []
    for rec, canon in zip(recs, case.strands):
        o = (ko.WideTable if la.k > 32 else ko.Table)(la.k, canon)
        for key, c in rec:
            o.add(key, c)
        out.append(o)
    return out


def witnesses(case):
    """Per tuple of ARGS: (args, the model's comp3, the oracle's comp3, the model's comp, the oracle's comp)."""
    from oracle import koracle as ko
    la = LAYOUT[case.layout]
    recs = records(case)
    o1, o2, o3 = oracle_tables(case, recs)
    _, canon2, canon3 = case.strands
    for args in ARGS:
        yield (args, comp3_model(recs[0], recs[1], recs[2], la.k, canon2, canon3, *args), ko.comp3(o1, o2, o3, *args),
               comp_model(recs[0], recs[1], la.k, canon2, *args), ko.comp(o1, o2, *args))
