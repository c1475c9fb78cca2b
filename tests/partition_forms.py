"""The partitioned counter's dispatch (kat_amd/csrc/kg_count.hip: count_partitioned), restated on the host, and the table of cases that
reaches every form of it (tests/test_partition_forms_model.py checks the table against the restatement, tests/test_gpu_partition_forms.py
runs it on the device against the oracle).  Plain Python: no GPU, no library.

Which kernels a partition round runs follows from the table's geometry and k:

  geometry   kg_table.hip: alloc_dev_table with a hooked region size rs (KATGPU_TEST_REGION_SLOTS) and a capacity cap (the size hint):
             nr = ceil(cap / rs) regions, p2 = the power of two >= ceil(sqrt(nr)), p1 = ceil(nr / p2);
             n1 = 2k - floor(log2 p1) bits of a level-1 item, rb = n1 - log2 p2 bits of a level-2 item (the remainder);
             packed 8-byte slots iff rb + 20 <= 64 and there is more than one region (never under KATGPU_NO_PACKED), else KV12
  level 1    plan_level1: hb1 = l2_hi_bytes(n1); lean iff 17 <= k <= 31 and 32 <= n1 < 2k; the block edition iff lean, p1 <= 512 and
             hb1 == 2; else a sweep for at most 512 or for 1024 level-1 digits.  The exact editions (KATGPU_L1_FAST=0) are lean or plain.
  items      what level 2 reads: blocks of ten (from the block edition), wide groups (hb1 == 4) or groups
  level 2    launch_l2_hb<hb>: hb = l2_hi_bytes(rb), at most 2 for a packed table; the block edition iff blocks of ten and hb == 1
  apply      launch_apply: packed or KV12, workgroup size and k-mers per lane and pass from the region size, inline claims in a table's first round

A LABEL is "<level 1> <items> hb <hb> <layout>": the level-1 family (Blocks, Lean512, Lean1024, Plain512, Plain1024 -- the segmented
edition the geometry selects), the item form, the level-2 item width and the slot layout."""

MAX_PARTS = 1024
AP2_MAX_SLOTS = 10240
PACK_MIN_CBITS = 20
LDS_BYTES, LDS_GRANULE = 160 * 1024, 1280


def l2_hi_bytes(bits):
    return 0 if bits <= 31 else 1 if bits <= 39 else 2 if bits <= 47 else 4


def lean_applies(k, n1):
    return 17 <= k <= 31 and 32 <= n1 < 2 * k


def load_limit(region_slots, n_regions=2):
    """kg_table.hip: load_limit -- the fill limit of the direct path, which the spilled k-mers of a round take."""
    if region_slots >= 1024 or n_regions == 1:
        return 0.7
    return max(0.25, 0.7 - 3.0 / region_slots ** 0.5)


class Form:
    """What alloc_dev_table and the dispatch make of (k, region slots, capacity)."""

    def __init__(self, k, rs, cap, no_packed=False):
        self.k, self.no_packed = k, no_packed
        cap = max(cap, 1024)
        if cap <= rs:
            self.p1 = self.p2 = 1
            self.region_slots = (cap + 3) & ~3
        else:
            nr = -(-cap // rs)
            p2 = 1
            while p2 * p2 < nr:
                p2 *= 2                       # (the power of two >= ceil(sqrt(nr)): squares of powers of two are squares)
            self.p2, self.p1 = p2, -(-nr // p2)
            self.region_slots = rs
        self.n_regions = self.p1 * self.p2
        self.cap = self.n_regions * self.region_slots
        self.l2 = self.p2.bit_length() - 1
        self.n1 = max(0, 2 * k - (self.p1.bit_length() - 1))
        self.rb = self.n1 - min(self.l2, self.n1)
        self.packed = not no_packed and self.n_regions > 1 and self.rb + PACK_MIN_CBITS <= 64
        self.slot_bytes = 8 if self.packed else 12
        # kg_count.hip: part_geometry
        S = self.region_slots
        self.partitioned = k <= 32 and self.rb <= 63 and self.p1 <= MAX_PARTS and self.p2 <= MAX_PARTS and S % 4 == 0 and 64 <= S <= AP2_MAX_SLOTS
        self.hb1 = l2_hi_bytes(self.n1)
        self.hb = min(l2_hi_bytes(self.rb), 2) if self.packed else l2_hi_bytes(self.rb)
        self.lean = lean_applies(k, self.n1)
        self.pb512 = self.p1 <= 512
        self.blocks = self.lean and self.pb512 and self.hb1 == 2

    # ---- names, as the library's trace line spells them ----
    def family(self):
        return "Blocks" if self.blocks else ("Lean" if self.lean else "Plain") + ("512" if self.pb512 else "1024")

    def edition(self, l1_fast):
        """The L1Edition of a round: a segmented one (KATGPU_L1_FAST=2) or an exact one (0)."""
        if not l1_fast:
            return "ExactLean" if self.lean else "ExactPlain"
        return "Blocks" if self.blocks else "Seg" + self.family()

    def items(self, l1_fast=True):
        return "Blocks" if self.blocks and l1_fast else "WideGroups" if self.hb1 == 4 else "Groups"

    def layout(self):
        return "packed" if self.packed else "KV12"

    def label(self):
        return "%s %s hb %u %s" % (self.family(), self.items(), self.hb, self.layout())

    def level2(self, l1_fast, p2_fast):
        return "exact" if not p2_fast else "blocks" if self.items(l1_fast) == "Blocks" and self.hb == 1 else "one-pass"

    def apply(self, fresh):
        """launch_apply's choice, without the spill hook: (workgroup size, k-mers per lane and pass)."""
        S = self.region_slots
        if self.packed:
            def room(wgs):
                return LDS_BYTES // wgs // LDS_GRANULE * LDS_GRANULE - 64 - S * 8
            per_cu = 4
            while per_cu > 1 and room(per_cu) < 8 * 8 * (72 if per_cu == 2 else 96):
                per_cu -= 1
            blk = 1024 if per_cu == 1 else 512
            kp = 5 if blk == 1024 else 4 if S <= 4096 else 10
        else:
            blk = 512 if S <= 4096 else 1024
            kp = (2 if S <= 2048 else 4) if blk == 512 else 5 if S > 8192 else 4
        return "%s B=%u KP=%u fresh=%u" % (self.layout(), blk, kp, int(bool(fresh)))

    def trace(self, l1_fast, p2_fast, fresh):
        """The text of the library's "partition forms" line (KATGPU_TRACE) for a round of this form."""
        return "l1=%s items=%s hb1=%u hb=%u l2=%s apply=%s" % (self.edition(l1_fast), self.items(l1_fast), self.hb1, self.hb, self.level2(l1_fast, p2_fast), self.apply(fresh))


def label_of_trace(text):
    """The label a "partition forms" line of a segmented round stands for."""
    f = dict(kv.split("=", 1) for kv in text.split() if "=" in kv)
    fam = f["l1"][3:] if f["l1"].startswith("Seg") else f["l1"]
    return "%s %s hb %s %s" % (fam, f["items"], f["hb"], f["apply"])


def grid_caps(rs, max_cap):
    """One capacity per grid (p1, p2) that alloc_dev_table makes of capacities to max_cap at this region size: p2 is the power of two with
    (p2 / 2)^2 < nr <= p2^2, and p1 = ceil(nr / p2) takes every value that leaves the number of regions nr in that range."""
    caps, p2 = [rs], 2
    while (p2 // 2) ** 2 < max_cap // rs:
        lo, hi = (p2 // 2) ** 2 + 1, min(p2 * p2, max_cap // rs)
        caps += [min(p1 * p2, hi) * rs for p1 in range(-(-lo // p2), -(-hi // p2) + 1)]
        p2 *= 2
    return caps


def enumerate_labels(no_packed, ks=range(1, 33), max_cap=1 << 26):
    """Every label the dispatch can reach: k in ks, region sizes 64 .. 8192 (powers of two), capacities to max_cap.  {label: one (k, rs, cap) that reaches it}."""
    found = {}
    rs = 64
    while rs <= 8192:
        for cap in grid_caps(rs, max_cap):
            for k in ks:
                f = Form(k, rs, cap, no_packed)
                if f.partitioned:
                    found.setdefault(f.label(), (k, rs, cap))
        rs *= 2
    return found


# ---- the segmented level 1 at test size ----
SEG_PAD, P1_TILE_STARTS, L1B_TILE_STARTS, L1B_ITEMS = 64, 8160, 16352, 10


def segment_fill(form, starts, density, n_cu=256, p1_wgs=3):
    """plan_level1's segments for a round of `starts` window starts, `density` of them k-mers: (k-mers that a workgroup meets for one bucket, the
    k-mers its segment is meant to take).  A segment is sized for a round whose tiles keep EVERY workgroup busy -- the round's k-mers / (workgroups
    x buckets) + 1/24 + SEG_PAD -- and a round of the test's size has fewer tiles than workgroups: one tile's k-mers of a bucket must fit."""
    wgs, tile = (n_cu, L1B_TILE_STARTS) if form.blocks else (n_cu * min(p1_wgs, 4), P1_TILE_STARTS)
    tiles_per_wg = -(-(-(-starts // tile)) // wgs)
    cap = starts // (wgs * form.p1)                                  # (no probe under KATGPU_TEST_ROUND_ITEMS: every start is taken for a k-mer)
    cap += cap // 24 + SEG_PAD
    if form.blocks:
        cap = -(-cap // L1B_ITEMS) * L1B_ITEMS
    return tiles_per_wg * tile * density / form.p1, cap


# ---- the cases ----
FAST, EXACT, MIXED, EXACT_L1 = (2, 2), (0, 0), (2, 0), (0, 2)    # (KATGPU_L1_FAST, KATGPU_P2_FAST): segmented + one-pass, both exact, segmented + exact level 2, exact level 1 + one-pass
SHORT_BASES = 2500                               # what the rows of one or two regions count: the stream's first bases
# KATGPU_TEST_ROUND_ITEMS: the stream in two rounds -- a table's first round (inline claims) and a later one
ROUND_ITEMS, ROUND_ITEMS_LONG = 600_000, 1_800_000


class Row:
    """seg: the segmented level 1 holds this row's rounds (segment_fill; tests/test_partition_forms_model.py).  Where it does not -- fewer than 128 level-1
    digits, 256 for the block edition -- level 1 falls back to its exact edition whatever KATGPU_L1_FAST says, and a stream that fills the segments does not
    fit the table the row asks for: such a row runs the exact editions, and another row reaches its label.  (The one-pass level 2 behind the exact
    level 1 is for the short rows alone: its runs are sized for a uniform hash of many k-mers, and on grids of a few hundred regions the stream's
    five-fold coverage -- a distinct k-mer is five items of one run -- sends more than the direct path's 1 % beyond them.)
    long: the row counts the long stream (the block edition at 128 level-1 digits: segments that hold a tile need the round's share on top of the pad)."""

    def __init__(self, k, canonical, rs, hint, label, no_packed=False, short=False, seg=True, long=False):
        self.k, self.canonical, self.rs, self.hint, self.label, self.no_packed, self.short, self.seg, self.long = k, canonical, rs, hint, label, no_packed, short, seg and not short, long
        self.form = Form(k, rs, hint, no_packed)

    def settings(self):
        """The kernel editions this row runs with."""
        if self.short:
            return [EXACT_L1, EXACT]
        if not self.seg:
            return [EXACT]
        if self.no_packed:
            return [FAST]
        return [FAST, EXACT] + ([MIXED] if self.form.blocks else [])

    def which(self):
        return "short" if self.short else "long" if self.long else "stream"

    def __repr__(self):
        return "k=%u %s rs=%u hint=%u%s%s" % (self.k, "canonical" if self.canonical else "both strands", self.rs, self.hint, " KV12 forced" if self.no_packed else "",
                                              " " + self.which() if self.which() != "stream" else "")


M = 1 << 20
ROWS = [
    # ---- the layout the table chooses: every label of a table of more than two regions
    Row(24, True, 64, 8 * M, "Blocks Blocks hb 0 packed"),
    Row(22, False, 4096, 2 * M, "Blocks Blocks hb 1 packed", seg=False),            # (a larger region than tests/test_gpu_block_placing.py's)
    Row(25, True, 4096, 2 * M, "Blocks Blocks hb 2 packed", seg=False),
    Row(21, True, 64, 48 * M, "Lean1024 Groups hb 0 packed"),
    Row(26, False, 64, 48 * M, "Lean1024 Groups hb 1 packed"),
    Row(29, True, 64, 48 * M, "Lean1024 WideGroups hb 1 packed"),
    Row(30, False, 64, 48 * M, "Lean1024 WideGroups hb 2 packed"),
    Row(18, False, 4096, 2 * M, "Lean512 Groups hb 0 packed", seg=False),
    Row(20, True, 8192, 2 * M, "Lean512 Groups hb 1 packed", seg=False),
    Row(28, True, 64, 8 * M, "Lean512 WideGroups hb 1 packed"),
    Row(31, False, 64, 16 * M, "Lean512 WideGroups hb 2 packed"),
    Row(27, True, 4096, 2 * M, "Lean512 WideGroups hb 2 KV12", seg=False),
    Row(28, False, 8192, 2 * M, "Lean512 WideGroups hb 4 KV12", seg=False),
    Row(12, True, 64, 48 * M, "Plain1024 Groups hb 0 packed"),
    Row(13, False, 1024, 2 * M, "Plain512 Groups hb 0 packed", seg=False),
    Row(32, False, 64, 64 * M, "Plain1024 WideGroups hb 2 packed"),      # (the size from which a packed table is cleared by its first sweep)
    Row(32, False, 64, 48 * M, "Plain1024 WideGroups hb 2 KV12"),
    Row(32, True, 64, 8 * M, "Plain512 WideGroups hb 2 KV12"),
    Row(32, False, 1024, 2 * M, "Plain512 WideGroups hb 4 KV12", seg=False),
    # ---- the k that the rows above leave out, and the other strand mode of some that they have
    Row(14, False, 64, 48 * M, "Plain1024 Groups hb 0 packed"),
    Row(15, True, 1024, 2 * M, "Plain512 Groups hb 0 packed", seg=False),
    Row(16, False, 4096, 2 * M, "Plain512 Groups hb 0 packed", seg=False),
    Row(17, True, 4096, 2 * M, "Plain512 Groups hb 0 packed", seg=False),  # (30-bit level-1 items: a k of the lean range on the plain sweep)
    Row(19, False, 8192, 2 * M, "Lean512 Groups hb 0 packed", seg=False),
    Row(23, True, 64, 48 * M, "Lean1024 Groups hb 0 packed"),
    Row(21, False, 64, 8 * M, "Lean512 Groups hb 0 packed"),
    Row(32, True, 64, 64 * M, "Plain1024 WideGroups hb 2 packed"),
    # ---- the labels whose rows above cannot have the segmented level 1, on grids of 128 or 256 level-1 digits that can
    Row(25, False, 64, 8 * M, "Blocks Blocks hb 1 packed"),                         # 256 x 512
    Row(27, True, 1024, 16 * M, "Blocks Blocks hb 2 packed", long=True),            # 128 x 128: the largest grid with a 6-byte remainder behind blocks of ten
    Row(23, False, 1024, 16 * M, "Lean512 Groups hb 1 packed"),                     # 128 x 128
    Row(30, True, 1024, 16 * M, "Lean512 WideGroups hb 2 KV12"),
    Row(31, True, 1024, 16 * M, "Lean512 WideGroups hb 4 KV12"),
    Row(16, True, 64, 8 * M, "Plain512 Groups hb 0 packed"),                        # 256 x 512
    Row(32, False, 1024, 16 * M, "Plain512 WideGroups hb 4 KV12"),
    # ---- tables of one level-1 digit (one or two regions; no bits above a level-1 item: never lean) or of a dozen regions: labels that only they reach.
    # They hold a few thousand k-mers, so they count the stream's first SHORT_BASES bases -- a single tile, which no segment holds.
    Row(24, True, 8192, 12 * 8192, "Blocks Blocks hb 2 KV12", short=True),              # 3 x 4
    Row(15, False, 8192, 8192, "Plain512 Groups hb 0 KV12", short=True),                # 1 x 1
    Row(18, True, 8192, 8192, "Plain512 Groups hb 1 KV12", short=True),                 # 1 x 1
    Row(22, False, 8192, 8192, "Plain512 Groups hb 2 KV12", short=True),                # 1 x 1
    Row(19, False, 8192, 2 * 8192, "Plain512 Groups hb 1 packed", short=True),          # 1 x 2
    Row(21, True, 8192, 2 * 8192, "Plain512 Groups hb 2 packed", short=True),           # 1 x 2
    # ---- KATGPU_NO_PACKED=1: the KV12 apply kernels behind every level-1 and level-2 form that otherwise feeds packed slots
    Row(24, True, 64, 8 * M, "Blocks Blocks hb 0 KV12", no_packed=True),
    Row(25, True, 64, 8 * M, "Blocks Blocks hb 1 KV12", no_packed=True),
    Row(23, False, 256, 6 * M, "Blocks Blocks hb 1 KV12", no_packed=True, seg=False),   # 96 x 256
    Row(27, True, 1024, 16 * M, "Blocks Blocks hb 2 KV12", no_packed=True, long=True),
    Row(21, False, 64, 48 * M, "Lean1024 Groups hb 0 KV12", no_packed=True),
    Row(26, True, 64, 48 * M, "Lean1024 Groups hb 1 KV12", no_packed=True),
    Row(29, False, 64, 48 * M, "Lean1024 WideGroups hb 1 KV12", no_packed=True),
    Row(30, True, 64, 48 * M, "Lean1024 WideGroups hb 2 KV12", no_packed=True),
    Row(21, True, 64, 8 * M, "Lean512 Groups hb 0 KV12", no_packed=True),
    Row(23, True, 1024, 16 * M, "Lean512 Groups hb 1 KV12", no_packed=True),
    Row(22, True, 1024, 4 * M, "Lean512 Groups hb 1 KV12", no_packed=True, seg=False),  # 64 x 64
    Row(28, False, 64, 8 * M, "Lean512 WideGroups hb 1 KV12", no_packed=True),
    Row(12, False, 64, 48 * M, "Plain1024 Groups hb 0 KV12", no_packed=True),
    Row(16, False, 64, 8 * M, "Plain512 Groups hb 0 KV12", no_packed=True),
]
# the labels that only a table of one level-1 digit reaches: an exact level 1 is all they ever have in front of their level 2 and apply
LABELS_SHORT_ONLY = {r.label for r in ROWS if r.short} - {r.label for r in ROWS if r.seg}


def groups(per_child=4):
    """The children of tests/test_gpu_partition_forms.py: the hooks are read when the library loads, so rows share a process only when they share the
    region size, the kernel editions and the round size.  [(id, environment, (l1_fast, p2_fast), [row index])], at most per_child rows each."""
    by_env = {}
    for i, r in enumerate(ROWS):
        for st in r.settings():
            by_env.setdefault((r.no_packed, r.which(), st, r.rs, r.hint if r.rs == 64 else 0), []).append(i)
    out = []
    for (no_packed, which, st, rs, _), rows in sorted(by_env.items()):
        for at in range(0, len(rows), per_child):
            env = {"KATGPU_TEST_REGION_SLOTS": str(rs), "KATGPU_L1_FAST": str(st[0]), "KATGPU_P2_FAST": str(st[1]),
                   "KATGPU_TEST_ROUND_ITEMS": str(ROUND_ITEMS_LONG if which == "long" else ROUND_ITEMS)}
            if no_packed:
                env["KATGPU_NO_PACKED"] = "1"
            name = "%s%sl1fast%u-p2fast%u-rs%u-rows%s" % ("kv12-" if no_packed else "", "" if which == "stream" else which + "-", st[0], st[1], rs, "_".join(map(str, rows[at:at + per_child])))
            out.append((name, env, st, rows[at:at + per_child]))
    return out


def stream(long=False):
    """The input of a row: reads of a small genome (about five-fold coverage: counts above one), an N-separated run of 3000 A and 2000 T in their
    middle (one k-mer thousands of times in one bucket, run and region; at k = 32 without canonical k-mers the T are the all-ones key), a stretch
    with lowercase letters and scattered N, and an end that is no multiple of 16 bytes -- about 930 K bases, so that the two runs, which level 1
    and level 2 hand to the direct path, stay under its 1 %; 3.4 M bases for the long rows.  Numpy only."""
    import numpy as np
    from kat_amd import synth
    n_reads = 22_500 if long else 6000
    g = synth.genome(n_reads * 30, seed=77)
    reads = synth.reads(g, 0, n_reads, seed=5)
    noisy = synth.reads(g, n_reads, 100, seed=5).copy()
    rng = np.random.default_rng(12)
    lower = rng.random(noisy.size) < 0.3
    noisy[lower] |= 0x20                                             # (ASCII lowercase)
    noisy[rng.random(noisy.size) < 0.01] = ord("N")
    half = reads.size // 2 + 7                                       # (the run begins inside a read, off every alignment)
    runs = np.frombuffer(b"N" + b"A" * 3000 + b"N" + b"T" * 2000 + b"N", np.uint8)
    s = np.concatenate([reads[:half], runs, reads[half:], noisy, reads[:1000]])
    s = s[:s.size - (s.size - 5) % 16]                               # 5 bytes beyond a multiple of 16
    assert s.size % 16 == 5
    return np.ascontiguousarray(s)
