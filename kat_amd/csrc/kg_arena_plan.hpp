// kg_arena_plan.hpp -- the arithmetic of the partition arena (kg_count.hip: PartArena, plan_level1, level2_and_apply) and of the run layout
// of the one-pass level 2 (kg_partition.hpp: k_p2_fast, kg_l2_blocks.hpp: k_p2x_fast): bytes per k-mer of a round by shape, the level-1
// bucket stride, a run's capacity and base, what a pass of level 2 can write, a round's capacity per level-1 edition, the window starts of a
// round.  Plain integer (and a little double) arithmetic that compiles for the host alone: tests/native/arena_plan_check.cc sweeps it
// without a GPU, kg_count.hip and the kernels include it, so what the host carves and what the kernels address is one text.
//
// What decides the number of table sweeps of a deep read set is how many k-mers the arena holds per round.  Two parts of the former charge
// (11.9 bytes per k-mer at the bench's shape) paid for layouts the bench's kernels do not write:
//   * level 1's block edition (kg_l1_blocks.hpp) writes 64-byte blocks of ten, 6.4 bytes per item, and addresses its segments by blocks;
//     only the host left 8 bytes of room.  Where the shape selects that edition the buffer is carved at 6.4 (`dense`).
//   * the blocked level-2 editions carry a sub-bucket's waiting items across tiles and pad a run ONCE, in its last block of twelve: the
//     allowance of two items per tile and run (12.5 % at 16 K-item tiles and 1024 runs) is for the group editions.
// and two parts are trimmed where that saves a round (`big`: the untrimmed carve does not hold the call's k-mers in one round, and a round has
// at least P2_LONG_RUN k-mers per region; a call that fits one untrimmed round, and a round that fits the trimmed carve's level-2 buffer with the
// untrimmed runs, keep the former slack -- arena_carve, round_trims):
//   (a) a blocked run's slack is 3/64 instead of 1/16.  A run is NOT a Poisson number of k-mers: it holds every copy of its distinct k-mers,
//       so at c copies per distinct k-mer and round its n items have sigma = sqrt(n (c + 1)), not sqrt(n) -- 2.4 % of a run of 23.6 K
//       items at 12.4 copies (a third of the bench's reads) and of a run of 35.3 K at 18.6 copies (half of them).  Runs are sized from level 1's
//       bucket CAPACITY, which contains the segment slack of 1/24, so against the items a run expects the slack is 25/24 x 67/64 - 1 = 9.05 %:
//       3.8 sigma, a k-mer in 3 to 5 million beyond its run (sigma x the normal loss function at 3.8, 1.5e-5) -- tests/test_gpu_bench_geometry.py
//       allows one in a million.  1/32 was built first, on the Poisson figure (sigma 188 of 35.3 K, "5.9 sigma"): 7.4 % is 3.1 of the real
//       sigma and sent 2.5 k-mers in a million (31 220 of 12.4 G) to the direct path at the bench's geometry.  The former 1/16 (10.7 %) is 4.5.
//       At the threshold of 16384 items per run the same 9.05 % is 3.2 sigma at 12 copies (5 k-mers in a million), more at fewer.
//       Sizing the runs from the bucket's EXPECTED k-mers instead (without the 1/24) would leave 4.7 %, 2 sigma: not done.
//       The former allowance of two items per tile served as slack too (12.5 % on top of the 10.7 at the bench's shape): at 62 copies per round
//       (hist's and gcp's configurations: sigma 2.8 % of a run of 81 K) the trimmed 9.05 % sent 35 662 k-mers of 6.2 G to the direct path where
//       tests/test_gpu_bench_geometry.py asks for none.  Those calls fit one untrimmed round and keep what they had.
//   (c) the overflow list holds 1/64 of a round instead of 1/32.  What reaches it: k-mers beyond a level-1 segment (a segment IS a Poisson
//       number -- the copies of a k-mer are spread over the workgroups --: 1/24 of 141 K k-mers is 15 sigma at the bench's shape) or beyond a
//       run (above): a few in a million; it is there for heavy hitters, and 1/64 of a round of 19 G k-mers is 300 M entries.  A list
//       that does not hold falls back to the exact editions.
// 6.4 x 25/24 + 5.33 x 25/24 x 67/64 / 2 + 8/64 = 9.70 bytes per k-mer of a round at the bench's shape with two passes.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KG_PLAN_FN __host__ __device__ __forceinline__
#else
#define KG_PLAN_FN inline
#endif

namespace kg {

// (what kg_device.hpp, kg_partition.hpp and kg_l1_blocks.hpp call MAX_PARTS, P1_TILE_STARTS, L1B_TILE_STARTS, L1B_ITEMS and L1B_BYTES: they
// static_assert the equality)
constexpr uint32_t PLAN_MAX_PARTS = 1024, PLAN_L1_TILE_STARTS = 8160, PLAN_L1B_TILE_STARTS = 16352, PLAN_L1B_ITEMS = 10, PLAN_L1B_BYTES = 64;

// ---- the level-2 buffer's formats (kg_partition.hpp "the level-2 buffer") ----
KG_PLAN_FN uint32_t l2_tile_items(uint32_t hb) { return hb == 4 ? 12 * 1024 : 16 * 1024; }
KG_PLAN_FN constexpr bool l2_blocked(uint32_t hb) { return hb == 1; }
constexpr uint32_t L2_BLOCK_ITEMS = 12, L2_BLOCK_BYTES = 64;
// bytes the level-2 buffer takes for `items` items (a multiple of 4) + the granule runs are aligned to, in items
KG_PLAN_FN uint64_t l2_buffer_bytes(uint32_t hb, uint64_t items) { return l2_blocked(hb) ? (items / L2_BLOCK_ITEMS + 2) * L2_BLOCK_BYTES : items / 4 * (16 + 4 * hb); }
KG_PLAN_FN double l2_bytes_per_item(uint32_t hb) { return l2_blocked(hb) ? (double)L2_BLOCK_BYTES / L2_BLOCK_ITEMS : 4.0 + hb; }
KG_PLAN_FN uint32_t l2_run_align(uint32_t hb) { return l2_blocked(hb) ? L2_BLOCK_ITEMS : 4u; }

// ---- the exact layouts ----
// l1_bucket_base(first item of b, b): byte of bucket b's first group in the exact level 1's layout, 8 bytes of room per item
KG_PLAN_FN uint64_t l1_bucket_base(uint64_t first_item, uint32_t b) { return 8 * first_item + 32ULL * b; }   // (+ 32 b: a bucket's last group may hold up to three items more than the bucket)
// first item of bucket b1's runs in the exact level 2: every run may end on up to three padding items
KG_PLAN_FN uint64_t p2_exact_base(uint64_t beg, uint32_t b1, uint32_t P2) { return (beg + 4 * ((uint64_t)P2 + 1) * b1 + 3) & ~3ULL; }

// ---- runs of the one-pass level 2 ----
// Both in ITEMS, both multiples of `al`.  p2_out_base(beg + n, b1 + 1) - p2_out_base(beg, b1) >= P2 * p2_region_cap(n): buckets do not overlap.
// (`al`: l2_run_align -- 4, or 12 where the items are blocked: runs start and end on block boundaries there; the 48 items of slack per run
// in p2_out_base cover the rounding of either.)
// trim = false: mean + 1/16 + what the group padding can add (two items per tile, on average 1.5) + 16.
// trim = true (l2_trims: blocked items, a round of long runs): mean + 3/64 + 16 -- (a) above; no per-tile term: a blocked run is padded once.
//   With s(n) = (n >> 5) + (n >> 6): P2 * cap(n) <= n + s(n) + 27 P2 (16 + the rounding to 12), base(beg + n, b1 + 1) - base(beg, b1) >= n + s(n) - 2 + 48 P2 - 11.
constexpr uint32_t P2_RUN_SLACK = 48;
constexpr uint64_t P2_LONG_RUN = 16384;
KG_PLAN_FN bool l2_trims(uint32_t hb, uint64_t round_items, uint64_t regions) { return l2_blocked(hb) && regions && round_items / regions >= P2_LONG_RUN; }
KG_PLAN_FN uint64_t p2_region_cap(uint64_t n_b, uint32_t P2, uint32_t tile, uint32_t al = 4, bool trim = false) {
    const uint32_t sh = 31 - __builtin_clz(P2);      // (P2 is a power of two: a 64-bit division here kept its reciprocal in two spilled registers)
    const uint64_t c = trim ? ((n_b + (n_b >> 5) + (n_b >> 6)) >> sh) + 16 : ((n_b + (n_b >> 4)) >> sh) + 2 * (n_b / tile + 1) + 16;
    return (c + al - 1) / al * al;
}
KG_PLAN_FN uint64_t p2_out_base(uint64_t beg, uint32_t b1, uint32_t P2, uint32_t tile, uint32_t al = 4, bool trim = false) {
    const uint64_t o = beg + (trim ? (beg >> 5) + (beg >> 6) : (beg >> 4) + 2 * (uint64_t)P2 * (beg / tile)) + (uint64_t)b1 * P2 * P2_RUN_SLACK;
    return (o + al - 1) / al * al;
}
// Bound of what level 2 writes for nb buckets of nn k-mers together, in items, WHICHEVER edition runs: the one-pass editions' runs end at
// p2_out_base(beg + nn, b_lo + nb) - p2_out_base(beg, b_lo) at the latest, the exact k_p2 (all its instantiations: obeg = p2_exact_base's
// difference, runs padded to whole groups) at nn + 4 (P2 + 1) nb + 3 -- below the former at either setting, since 4 (P2 + 1) < 48 P2; the
// maximum is taken so that this stays true whatever becomes of the formulas.
KG_PLAN_FN uint64_t p2_pass_extent(uint64_t nn, uint32_t nb, uint32_t P2, uint32_t tile, bool trim) {
    const uint64_t fast = nn + (trim ? nn / 32 + nn / 64 : nn / 16 + 2ULL * P2 * (nn / tile + 1)) + (uint64_t)nb * P2 * P2_RUN_SLACK + 64;
    const uint64_t exact = nn + 4 * ((uint64_t)P2 + 1) * nb + 8;
    return fast > exact ? fast : exact;
}

// ---- level 1's segments (kg_partition.hpp: k_p1v2_scatter<true>; kg_l1_blocks.hpp: k_p1b_scatter) ----
// A segment per workgroup and bucket: its share of the round's k-mers + 1/24 + SEG_PAD (tests/partition_forms.py models this), in whole
// blocks of ten (block edition) or whole groups of four with the group padding's allowance (group editions).
// stride: bytes from one bucket's first segment to the next's.  Block edition: the segments' blocks -- wgs * segb * 64 -- and 32 bytes that
// keep the former tail pad, rounded to whole blocks (k_p1b_scatter takes the stride in blocks; level 2's 12-byte pair loads of a bucket's
// last tile run on into the next bucket, or into the level-2 buffer behind the last one: mapped, never decoded).  Group editions: 8 bytes
// per k-mer a bucket can hold (its part of the buffer is the pass's spill list later) or the groups' bytes, whichever is more, + 32.
constexpr uint64_t SEG_PAD = 64;
struct L1Segments {
    uint64_t seg_cap, cap_plain, stride;   // slots of a segment; k-mers it takes at most; bytes of a bucket
    bool fits;                             // P1 strides lie inside the level-1 buffer and the kernels' 24- and 32-bit arithmetic holds
};
KG_PLAN_FN L1Segments l1_segments(bool blocks, uint32_t P1, uint32_t hb1, uint32_t wgs, uint64_t est_items, uint64_t tiles_per_wg, uint32_t test_cpb, uint64_t l1_bytes) {
    L1Segments s;
    uint64_t seg_cap = est_items / ((uint64_t)wgs * P1);
    seg_cap += seg_cap / 24 + SEG_PAD;
    if (test_cpb && seg_cap > test_cpb) seg_cap = test_cpb;
    if (blocks) seg_cap = (seg_cap + PLAN_L1B_ITEMS - 1) / PLAN_L1B_ITEMS * PLAN_L1B_ITEMS;       // whole blocks: every slot may hold a k-mer
    s.cap_plain = seg_cap;
    // groups: a bucket's k-mers of a tile are padded to whole groups, 1.5 items per tile and bucket on average
    if (!blocks && hb1 != 4 && !test_cpb) { const uint64_t pad = 2 * tiles_per_wg; seg_cap += pad < 3 * seg_cap ? pad : 3 * seg_cap; }
    if (!blocks) seg_cap = (seg_cap + 3) & ~3ULL;                                  // whole groups
    s.seg_cap = seg_cap;
    if (blocks) s.stride = ((uint64_t)wgs * (seg_cap / PLAN_L1B_ITEMS) * PLAN_L1B_BYTES + 32 + 63) & ~63ULL;
    else { const uint64_t a = 8 * (uint64_t)wgs * s.cap_plain, b = (uint64_t)(4 + hb1) * wgs * seg_cap; s.stride = (a > b ? a : b) + 32; }
    s.fits = s.stride * P1 <= l1_bytes && seg_cap < (1u << 24) && s.stride <= 0xFFFFFFFFULL;
    return s;
}

// ---- the carve ----
// [small arrays | level-1 buffer | guard | level-2 buffer | guard | overflow list | guard]
// L1 buffer: a round's k-mers + 1/24 + SEG_PAD per workgroup and bucket (the segment slack), at 8 bytes per item -- or 6.4 (`dense`) where
// the table's shape selects level 1's block edition and a round is large enough to run it.
// L2 buffer: one PASS of level 2 + apply (a CU-full of buckets): the L1 count / passes x the run slack + 48 per run.
// A round's capacity depends on the edition that runs it: the exact level 1 (l1_bucket_base: 8 bytes per item) places fewer k-mers in a
// dense buffer than the block edition does -- `exact_items`.
constexpr size_t ARENA_GUARD = 4096;           // bytes behind each of the three buffers (KATGPU_TESTING: a byte pattern that count_partitioned checks after each round)
constexpr uint64_t L1_FAST_MIN_ITEMS = (uint64_t)64 << 20;   // rounds of fewer k-mers run the exact level 1 (kg_count.hip: KATGPU_L1_FAST = 1)
KG_PLAN_FN double l1_bytes_per_item(bool dense) { return dense ? (double)PLAN_L1B_BYTES / PLAN_L1B_ITEMS : 8.0; }
KG_PLAN_FN double l2_items_per_l1_item(uint32_t hb, bool big) { return big && l2_blocked(hb) ? 1 + 3.0 / 64 : 1 + 1.0 / 16 + 2.0 * PLAN_MAX_PARTS / l2_tile_items(hb); }
KG_PLAN_FN uint64_t ovf_share(bool big) { return big ? 64 : 32; }
// bytes of arena per k-mer of a round (0.002: the divisions' roundings; what is fixed is arena_fixed_bytes)
KG_PLAN_FN double arena_bytes_per_item(uint32_t hb, uint32_t passes, bool dense, bool big) {
    return l1_bytes_per_item(dense) * (1 + 1.0 / 24) + l2_bytes_per_item(hb) * (1 + 1.0 / 24) * l2_items_per_l1_item(hb, big) / passes + 8.0 / ovf_share(big) + 0.002;
}
struct ArenaCarve {
    bool dense, big;
    double per_item;
    uint64_t round_items;      // k-mers of a round of a segmented edition (and of the exact one where the buffer is not dense)
    uint64_t exact_items;      // ... of a round of the exact level 1
    uint64_t l1_count, l1_bytes, l2_items, l2_bytes, ovf_cap;
    uint64_t total_bytes;      // the three buffers and their guards
};
// room for the segments' fixed part: SEG_PAD per workgroup and bucket -- W workgroups and 1024 buckets; the block edition (dense: nothing else is
// segmented in such a buffer) runs one workgroup per CU on at most 512 buckets, and rounds a segment up to a block of ten
KG_PLAN_FN uint64_t arena_fixed_l1(uint32_t W, uint32_t n_cu, bool dense) { return dense ? (uint64_t)n_cu * 512 * (SEG_PAD + 2 * PLAN_L1B_ITEMS) : (uint64_t)W * PLAN_MAX_PARTS * SEG_PAD; }
KG_PLAN_FN uint64_t arena_l2_items(uint64_t l1_count, uint32_t hb, uint32_t passes, bool big) {
    return ((uint64_t)((double)l1_count * l2_items_per_l1_item(hb, big) / passes) + (uint64_t)PLAN_MAX_PARTS * PLAN_MAX_PARTS * P2_RUN_SLACK + 4096 + 11) / 12 * 12;
}
// what the buffers take beyond per_item x round_items: the fixed parts of both buffers, the guards, the roundings
KG_PLAN_FN uint64_t arena_fixed_bytes(uint32_t hb, uint32_t passes, uint32_t W, uint32_t n_cu, bool dense, bool big) {
    const uint64_t f1 = arena_fixed_l1(W, n_cu, dense) + 16;
    return (uint64_t)((double)f1 * l1_bytes_per_item(dense)) + 256 + l2_buffer_bytes(hb, arena_l2_items(f1, hb, passes, big) + 12) + 16 + 1024 * 8 + 3 * ARENA_GUARD + 4096;
}
KG_PLAN_FN ArenaCarve arena_carve_as(uint64_t buf_bytes, uint64_t want_items, uint32_t hb, uint32_t passes, uint32_t W, uint32_t n_cu, bool dense, bool big, uint64_t test_ovf_cap) {
    ArenaCarve c;
    c.dense = dense; c.big = big;
    c.per_item = arena_bytes_per_item(hb, passes, dense, big);
    const uint64_t fixed = arena_fixed_bytes(hb, passes, W, n_cu, dense, big);
    const uint64_t by_bytes = buf_bytes > fixed ? (uint64_t)((double)(buf_bytes - fixed) / c.per_item) : 0;
    c.round_items = want_items < by_bytes ? want_items : by_bytes;
    c.l1_count = (c.round_items + c.round_items / 24 + arena_fixed_l1(W, n_cu, dense) + 15) & ~(uint64_t)15;      // (a multiple of 16)
    c.l1_bytes = dense ? (((c.l1_count / PLAN_L1B_ITEMS + 1) * PLAN_L1B_BYTES + 127) & ~(uint64_t)127) : c.l1_count * 8;   // (the level-2 buffer starts on a 128-byte boundary)
    c.l2_items = arena_l2_items(c.l1_count, hb, passes, big);
    c.l2_bytes = (l2_buffer_bytes(hb, c.l2_items) + 15) & ~(uint64_t)15;
    c.ovf_cap = test_ovf_cap ? test_ovf_cap : c.round_items / ovf_share(big) + 1024;
    const uint64_t exact = (c.l1_bytes - 32 * ((uint64_t)PLAN_MAX_PARTS + 1)) / 8;
    c.exact_items = exact < c.round_items ? exact : c.round_items;
    c.total_bytes = c.l1_bytes + ARENA_GUARD + c.l2_bytes + ARENA_GUARD + c.ovf_cap * 8 + ARENA_GUARD;
    return c;
}
// The carve of buf_bytes (the arena behind its small arrays) for rounds of at most want_items k-mers.  blocks_shape: the table's shape selects
// level 1's block edition (plan_level1); l1_fast: KATGPU_L1_FAST (0: never segmented, 1: rounds of at least L1_FAST_MIN_ITEMS, 2: always).
// dense only where a round of the block edition can run at all.  big (the trimmed run slack and list) only where the untrimmed carve does not
// hold want_items in ONE round and the round the trimmed carve makes has long runs: the slack is spent where the arena has room for all of the
// call, and nothing shrinks there.  NOT decided by whether the trimmed carve makes FEWER rounds than the untrimmed one: the carve is made before the
// prefix probe, from window starts, and how many k-mers they hold (0.82 per start at the bench's reads) is what tells two rounds from three.  A call
// of several rounds either way therefore runs its full rounds with 3/64 runs and the 1/64 list as well: more k-mers per round, never more rounds.
KG_PLAN_FN ArenaCarve arena_carve(uint64_t buf_bytes, uint64_t want_items, uint32_t hb, uint32_t passes, uint32_t W, uint32_t n_cu, uint64_t regions, bool blocks_shape, uint32_t l1_fast, uint64_t test_ovf_cap) {
    bool dense = blocks_shape && l1_fast != 0;
    for (;;) {
        ArenaCarve c = arena_carve_as(buf_bytes, want_items, hb, passes, W, n_cu, dense, false, test_ovf_cap);
        if (c.round_items < want_items) {
            const ArenaCarve t = arena_carve_as(buf_bytes, want_items, hb, passes, W, n_cu, dense, true, test_ovf_cap);
            if (regions && t.round_items / regions >= P2_LONG_RUN) c = t;
        }
        if (!dense || l1_fast == 2 || c.round_items >= L1_FAST_MIN_ITEMS) return c;
        dense = false;
    }
}
// A round's one-pass level 2 sizes its runs by the trimmed form only in a big carve, for long blocked runs, and only where a pass of nb buckets
// of nn k-mers does not fit the level-2 buffer with the untrimmed one (a round smaller than the carve's, the last of a call for instance).
// nn is the segmented level 1's bound (buckets x capacity).  Behind an EXACT level 1 the caller has only an estimate when it decides (the round's
// k-mers shared out evenly + 1/64); level2_and_apply decides again from the buckets' own counts before it shapes the passes.
KG_PLAN_FN bool round_trims(const ArenaCarve& c, uint32_t hb, uint64_t est_items, uint64_t regions, uint64_t nn, uint32_t nb, uint32_t P2) {
    return c.big && l2_trims(hb, est_items, regions) && p2_pass_extent(nn, nb, P2, l2_tile_items(hb), false) > c.l2_items;
}

// A round's capacity by the edition that runs it, over the rounds of a call: the block edition's where the buffer is dense and that edition can run,
// the exact level 1's (8 bytes per item in the same bytes) for the round that is repeated after a fall back and for EVERY later one.
struct RoundCaps {
    bool dense_ok = true;
    KG_PLAN_FN uint64_t cap(const ArenaCarve& c, bool blocks_can_run) const { return dense_ok && blocks_can_run && c.dense ? c.round_items : c.exact_items; }
    KG_PLAN_FN void exact_from_here() { dense_ok = false; }
};

// window starts of the next round, of `left`: what fills the buffers, the remaining rounds balanced
KG_PLAN_FN size_t round_starts(size_t left, size_t round_items, double items_per_start) {
    size_t m = left;                                                           // items <= starts: this always fits
    if (m > round_items) { const size_t by = (size_t)((double)round_items / items_per_start * 0.98); if (by < m) m = by; }
    if (m < left) {
        if (!m) m = 1;
        const size_t rounds_left = (left + m - 1) / m;
        m = (left + rounds_left - 1) / rounds_left;
        m += PLAN_L1_TILE_STARTS - m % PLAN_L1_TILE_STARTS;                    // whole tiles, keeps the next round 16-byte aligned
        if (m > left) m = left;
    }
    return m;
}

}  // namespace kg
