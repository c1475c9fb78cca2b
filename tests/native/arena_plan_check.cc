// arena_plan_check.cc -- kg_arena_plan.hpp on the host, without a GPU (tests/test_arena_plan.py builds this plain and with
// -fsanitize=address,undefined and runs both): the carve, level 1's stride, the runs' capacity and base, a pass's extent and the rounds of the
// bench's default configuration, over P1 x P2 x level-1 workgroups x round sizes from 1e5 to 2e10 k-mers in quarter-octave steps.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../kat_amd/csrc/kg_arena_plan.hpp"

using namespace kg;

static unsigned long long n_checks = 0, n_failed = 0;
#define CHECK(cond, ...)                                                       \
    do {                                                                       \
        ++n_checks;                                                            \
        if (!(cond)) {                                                         \
            if (++n_failed <= 20) { printf("FAILED %s:%d %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                      \
    } while (0)

// the formulas as they stood before the arena was sized by the blocked items: what "no capacity below today's" compares with
static uint64_t old_region_cap(uint64_t n_b, uint32_t P2, uint32_t tile, uint32_t al) {
    uint32_t sh = 0;
    while ((1u << sh) < P2) ++sh;
    const uint64_t c = ((n_b + (n_b >> 4)) >> sh) + 2 * (n_b / tile + 1) + 16;
    return (c + al - 1) / al * al;
}
static uint64_t old_l2_items(uint64_t l1_items, uint32_t hb, uint32_t passes) {
    return ((uint64_t)((double)l1_items * (1 + 1.0 / 16 + 2.0 * 1024 / l2_tile_items(hb)) / passes) + (uint64_t)1024 * 1024 * 48 + 4096 + 11) / 12 * 12;
}
static uint32_t passes_of(uint32_t P1, uint32_t n_cu) { return n_cu && P1 > n_cu && P1 % n_cu == 0 ? P1 / n_cu : 1; }      // (kg_count.hip: pass_buckets)

static void check_runs() {
    // the run-base invariant for both alignments and both forms; blocked capacities are whole blocks
    const uint64_t ns[] = {0, 1, 5, 11, 12, 100, 4095, 4096, 16383, 16384, 16385, 100000, 1234567, 36090000, 40000000, 3000000000ULL};
    const uint64_t begs[] = {0, 1, 31, 32, 16383, 16384, 999999, 123456789, 9000000000ULL, 19999999999ULL};
    for (uint32_t P2 = 2; P2 <= 1024; P2 *= 2)
        for (uint32_t hb : {0u, 1u, 2u, 4u})
            for (uint32_t al : {4u, 12u})
                for (int trim = 0; trim < 2; ++trim)
                    for (uint64_t n : ns) {
                        const uint32_t tile = l2_tile_items(hb);
                        const uint64_t cap = p2_region_cap(n, P2, tile, al, trim != 0);
                        CHECK(cap % al == 0, "cap %llu al %u", (unsigned long long)cap, al);
                        CHECK(cap >= (n + P2 - 1) / P2, "cap %llu below the mean of n %llu P2 %u", (unsigned long long)cap, (unsigned long long)n, P2);
                        if (!trim) CHECK(cap == old_region_cap(n, P2, tile, al), "untrimmed cap changed: n %llu P2 %u", (unsigned long long)n, P2);
                        for (uint64_t beg : begs)
                            for (uint32_t b1 : {0u, 1u, 255u, 511u}) {
                                const uint64_t lo = p2_out_base(beg, b1, P2, tile, al, trim != 0), hi = p2_out_base(beg + n, b1 + 1, P2, tile, al, trim != 0);
                                CHECK(lo % al == 0 && hi - lo >= (uint64_t)P2 * cap, "bases %llu %llu cap %llu P2 %u al %u trim %d n %llu beg %llu", (unsigned long long)lo, (unsigned long long)hi,
                                      (unsigned long long)cap, P2, al, trim, (unsigned long long)n, (unsigned long long)beg);
                                // a pass of one bucket: its extent bounds the bucket's runs and the exact edition's
                                const uint64_t ext = p2_pass_extent(n, 1, P2, tile, trim != 0);
                                CHECK(ext >= hi - lo - (lo ? al : 0) && ext >= p2_exact_base(beg + n, b1 + 1, P2) - p2_exact_base(beg, b1, P2),
                                      "extent %llu of n %llu P2 %u al %u trim %d beg %llu", (unsigned long long)ext, (unsigned long long)n, P2, al, trim, (unsigned long long)beg);
                            }
                    }
}

static void check_shape(uint32_t P1, uint32_t P2, uint32_t n_cu, uint32_t hb, bool blocks_shape, uint32_t hb1, double size, bool by_bytes) {
    const uint32_t W = 3 * n_cu, passes = passes_of(P1, n_cu), tile = l2_tile_items(hb);
    const uint64_t R = (uint64_t)P1 * P2, items = (uint64_t)size;
    const uint64_t fixed = arena_fixed_bytes(hb, passes, W, n_cu, false, false);
    const uint64_t buf_bytes = by_bytes ? fixed + (uint64_t)(size * 10.0) : fixed + (uint64_t)(size * 20.0);
    const ArenaCarve c = arena_carve(buf_bytes, by_bytes ? ~0ULL >> 2 : items, hb, passes, W, n_cu, R, blocks_shape, 2, 0);
    CHECK(c.total_bytes <= buf_bytes, "carve of %llu bytes in %llu", (unsigned long long)c.total_bytes, (unsigned long long)buf_bytes);
    CHECK(!c.dense || blocks_shape, "dense without the block edition");
    CHECK(c.exact_items <= c.round_items && l1_bucket_base(c.exact_items, PLAN_MAX_PARTS) + 32 <= c.l1_bytes, "exact capacity %llu in %llu bytes", (unsigned long long)c.exact_items, (unsigned long long)c.l1_bytes);
    CHECK(c.l2_items % 12 == 0 && l2_buffer_bytes(hb, c.l2_items) <= c.l2_bytes, "level-2 buffer");
    if (!by_bytes) CHECK(!c.big, "a call that fits one round was trimmed");
    if (!by_bytes) CHECK(c.round_items == items, "round items %llu of %llu wanted", (unsigned long long)c.round_items, (unsigned long long)items);
    // short runs: nothing is below what it was
    if (c.round_items / R < 2048) {
        const uint64_t l1_old = (c.round_items + c.round_items / 24 + (uint64_t)W * 1024 * 64 + 15) & ~15ULL;
        // (a dense buffer keeps SEG_PAD per workgroup and bucket for the block edition's workgroups and buckets alone: the round's capacity, the runs and the list are what they were)
        CHECK(!c.big && (c.dense || c.l1_count == l1_old) && c.l1_count >= c.round_items + c.round_items / 24 && c.l2_items >= old_l2_items(c.l1_count, hb, passes) && c.ovf_cap >= c.round_items / 32 + 1024, "short runs: a capacity shrank");
        CHECK(!l2_trims(hb, c.round_items, R), "short runs trimmed");
    }
    for (int exact = 0; exact < 2; ++exact) {
        // the round as count_partitioned plans it: at most the capacity of the edition that runs
        const bool blocks = blocks_shape && !exact;
        const uint64_t est = blocks && c.dense ? c.round_items : c.exact_items;
        const uint32_t nb = P1 / passes;
        uint64_t nn;
        if (!exact) {
            const uint32_t wgs = blocks ? n_cu : W;
            const uint64_t starts = (uint64_t)((double)est / 0.8212), n_tiles = (starts + (blocks ? PLAN_L1B_TILE_STARTS : PLAN_L1_TILE_STARTS) - 1) / (blocks ? PLAN_L1B_TILE_STARTS : PLAN_L1_TILE_STARTS);
            const L1Segments s = l1_segments(blocks, P1, hb1, wgs, est, (n_tiles + wgs - 1) / wgs, 0, c.l1_bytes);
            if (blocks) CHECK(s.stride % 64 == 0 && s.stride >= (uint64_t)wgs * (s.seg_cap / PLAN_L1B_ITEMS) * PLAN_L1B_BYTES + 32 && s.seg_cap % PLAN_L1B_ITEMS == 0, "stride %llu", (unsigned long long)s.stride);
            else CHECK(s.stride >= (uint64_t)wgs * s.seg_cap * (4 + hb1) && s.stride >= 8 * (uint64_t)wgs * s.cap_plain && s.seg_cap % 4 == 0, "stride %llu", (unsigned long long)s.stride);
            CHECK(!s.fits || (uint64_t)P1 * s.stride <= c.l1_bytes, "P1 strides beyond the buffer");          // (else the plan says "not segmented")
            CHECK(s.cap_plain >= est / ((uint64_t)wgs * P1) * 25 / 24 + SEG_PAD - 1, "segment capacity below share + 1/24 + pad");
            // a round that fills the buffer is segmented where segments are of any size (the fixed part covers SEG_PAD per workgroup and bucket)
            if (est >= L1_FAST_MIN_ITEMS && s.seg_cap < (1u << 24) && s.stride <= 0xFFFFFFFFULL) CHECK(s.fits, "a full round of %llu items is not segmented (P1 %u wgs %u dense %d)", (unsigned long long)est, P1, wgs, (int)c.dense);
            if (!s.fits) continue;
            nn = (uint64_t)nb * wgs * s.cap_plain;
        } else nn = (uint64_t)((double)est * nb / P1 * (1 + 1.0 / 64)) + 1024;      // (exact level 1: the buckets' own counts; 1/64 is 6 sigma of a bucket of 150 K)
        const bool trim = round_trims(c, hb, est, R, nn, nb, P2);          // (as count_partitioned decides it)
        CHECK(!trim || (c.big && l2_trims(hb, est, R)), "a round trims in a carve that does not");
        const uint64_t ext = p2_pass_extent(nn, nb, P2, tile, trim);
        CHECK(ext <= c.l2_items, "pass extent %llu beyond the level-2 buffer of %llu items (P1 %u P2 %u cus %u hb %u est %llu exact %d dense %d big %d trim %d)", (unsigned long long)ext,
              (unsigned long long)c.l2_items, P1, P2, n_cu, hb, (unsigned long long)est, exact, (int)c.dense, (int)c.big, (int)trim);
        if (l2_blocked(hb)) CHECK(p2_region_cap(nn / nb, P2, tile, 12, trim) % 12 == 0, "blocked capacity");
        if (nn / nb / P2 < 2048) CHECK(p2_region_cap(nn / nb, P2, tile, l2_run_align(hb), trim) >= old_region_cap(nn / nb, P2, tile, l2_run_align(hb)), "a short run's capacity shrank");
    }
}

// the rounds count_partitioned makes of `starts` window starts (the block edition throughout)
static int rounds_of(uint64_t starts, double ips, const ArenaCarve& c, double* spare) {
    uint64_t left = starts;
    int rounds = 0;
    *spare = 1;
    while (left) {
        const size_t m = round_starts(left, c.round_items, ips);
        const double s = 1.0 - (double)m * ips / (double)c.round_items;
        if (s < *spare) *spare = s;
        left -= m;
        ++rounds;
    }
    return rounds;
}
static void check_config4() {
    // bench.py's default: arena 189.3e9 bytes, 256 CUs, hb 1, hb1 2, P1 512, P2 1024, 45.0e9 window starts at 0.8212 k-mers per start
    const uint32_t P1 = 512, P2 = 1024, n_cu = 256, W = 3 * n_cu, passes = passes_of(P1, n_cu);
    const uint64_t starts = 45000000000ULL;
    const double ips = 0.8212;
    for (double share : {1.0, 0.97}) {
        const uint64_t arena = (uint64_t)(189.3e9 * share);
        const uint64_t small = (uint64_t)W * 1024 * 12 + 1025 * 8 + (1024 * 1024 + 1) * 8 + 1024 * 1024 * 4 + 1024 * 12 + 8 * 256;      // (PartArena's small arrays)
        const ArenaCarve c = arena_carve(arena - small, starts, 1, passes, W, n_cu, (uint64_t)P1 * P2, true, 1, 0);
        double spare;
        const int rounds = rounds_of(starts, ips, c, &spare);
        printf("config 4 at %.1f GB: %.3f bytes per item, %.3f G items per round (exact level 1: %.3f G), dense %d big %d, %d rounds, %.1f %% to spare\n", arena / 1e9, c.per_item, c.round_items / 1e9,
               c.exact_items / 1e9, (int)c.dense, (int)c.big, rounds, 100 * spare);
        CHECK(passes == 2 && c.dense && c.big, "config 4's shape");
        CHECK(rounds == 2, "config 4 makes %d rounds at %.1f GB", rounds, arena / 1e9);
        if (share == 1.0) CHECK(spare >= 0.03, "config 4 has %.2f %% to spare", 100 * spare);
        // the round as it is planned: segmented at the dense stride, each of two passes inside the level-2 buffer, the trimmed runs
        const uint64_t est = (uint64_t)((double)round_starts(starts, c.round_items, ips) * ips);
        const L1Segments s = l1_segments(true, P1, 2, n_cu, est, 0, 0, c.l1_bytes);
        CHECK(s.fits && s.stride == (uint64_t)n_cu * (s.seg_cap / 10) * 64 + 64, "config 4's level 1 is not segmented at the dense stride");
        CHECK(round_trims(c, 1, est, (uint64_t)P1 * P2, (uint64_t)256 * n_cu * s.cap_plain, 256, P2), "config 4's rounds do not trim their runs");
        CHECK(p2_pass_extent((uint64_t)256 * n_cu * s.cap_plain, 256, P2, l2_tile_items(1), true) <= c.l2_items, "config 4: a half pass beyond the level-2 buffer");
        // a third of the reads in a call of its own (tests/test_gpu_bench_geometry.py's slices), and hist's whole input: one untrimmed round
        for (uint64_t part : {15100000000ULL, 7550000000ULL}) {
            const ArenaCarve c1 = arena_carve(arena - small, part, 1, passes, W, n_cu, (uint64_t)P1 * P2, true, 1, 0);
            CHECK(!c1.big && c1.round_items == part && c1.dense, "a call of %llu window starts is trimmed or split", (unsigned long long)part);
        }
        // ... and what the exact level 1 would make of it: more rounds, never more than 8 bytes per item fit
        ArenaCarve e = c;
        e.round_items = c.exact_items;
        const int exact_rounds = rounds_of(starts, ips, e, &spare);
        CHECK(exact_rounds >= 3 && 8 * c.exact_items <= c.l1_bytes, "config 4 with the exact level 1: %d rounds", exact_rounds);
        // the call's rounds as count_partitioned plans them when the FIRST block round is abandoned (RoundEnd::RedoExactL1): that round again and every
        // later one at the exact capacity, each inside what 8 bytes per item fit
        {
            RoundCaps caps;
            uint64_t left = starts;
            int n = 0;
            bool abandoned = false;
            while (left) {
                const uint64_t cap = caps.cap(c, !abandoned);
                const size_t m = round_starts(left, cap, ips);
                const uint64_t items = (uint64_t)((double)m * ips);
                if (!abandoned) {
                    CHECK(cap == c.round_items && items > c.exact_items, "the first round is not sized for the block edition");
                    abandoned = true; caps.exact_from_here();
                    continue;
                }
                CHECK(cap == c.exact_items && items <= cap && l1_bucket_base(items, P1) + 32 <= c.l1_bytes, "round %d after the fall back: %llu items, capacity %llu", n, (unsigned long long)items, (unsigned long long)cap);
                CHECK(caps.cap(c, true) == c.exact_items, "a later round is sized for the block edition again");
                left -= m; ++n;
            }
            CHECK(n == exact_rounds, "%d rounds after the fall back, %d expected", n, exact_rounds);
        }
    }
}

int main() {
    check_runs();
    for (uint32_t P1 : {128u, 256u, 384u, 512u})
        for (uint32_t P2 = 64; P2 <= 1024; P2 *= 2)
            for (uint32_t n_cu : {1u, 104u, 256u, 304u})
                for (uint32_t hb : {0u, 1u, 2u, 4u})
                    for (double size = 1e5; size <= 2e10 * 1.0001; size *= pow(2.0, 0.25)) {
                        check_shape(P1, P2, n_cu, hb, true, 2, size, false);      // the block edition's shape
                        check_shape(P1, P2, n_cu, hb, true, 2, size, true);
                        check_shape(P1, P2, n_cu, hb, false, 2, size, false);     // the group editions
                        check_shape(P1, P2, n_cu, hb, false, 4, size, true);
                    }
    check_config4();
    printf("%llu checks, %llu failed\n", n_checks, n_failed);
    if (n_failed) return 1;
    printf("arena plan ok\n");
    return 0;
}
