// Host check of kg_exchange_layout.hpp: the buffer of the multi-GPU exchange (the send list and the receive sets of kg_comm.hip's
// struct Exchange) for every send list and set size from 0 to 4096, a few large ones, both shapes (pipelined: two sets of one size;
// split: one set per chunk, of different sizes, empty ones included) and both wire forms (keys u64 + counts u32; rem_lo u32 + rem_hi
// u8 + counts u32).  Per layout and form: the arrays in use are pairwise disjoint over the records they hold, each is aligned for its
// element, each ends inside the bytes the layout reports, and each group has room for its records.
// Built with hipcc -x hip (as the library's units are) and run on the CPU; prints "exchange layout ok".
#include "../../kat_amd/csrc/kg_exchange_layout.hpp"

#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

using namespace kg;

struct Arr { uint64_t o, len, align; const char* name; size_t group; };

static uint64_t g_checked = 0;

static bool check(const XLayout& l, uint64_t total_send, const std::vector<uint64_t>& sets, const char* shape) {
    if (l.sets.size() != sets.size()) { printf("%s: %zu sets for %zu\n", shape, l.sets.size(), sets.size()); return false; }
    std::vector<const XGroup*> gs{&l.send};
    std::vector<uint64_t> want{total_send};
    for (size_t i = 0; i < sets.size(); ++i) { gs.push_back(&l.sets[i]); want.push_back(sets[i]); }
    std::vector<Arr> arrs;
    for (int packed = 0; packed < 2; ++packed) {
        arrs.clear();
        for (size_t i = 0; i < gs.size(); ++i) {
            const XGroup& g = *gs[i];
            const uint64_t n = std::max<uint64_t>(want[i], 1);
            if (g.n < n) { printf("%s: group %zu has room for %llu records, needs %llu\n", shape, i, (unsigned long long)g.n, (unsigned long long)n); return false; }
            if (packed) { arrs.push_back({g.rem_lo, 4 * n, 4, "rem_lo", i}); arrs.push_back({g.rem_hi, n, 1, "rem_hi", i}); }
            else arrs.push_back({g.keys, 8 * n, 8, "keys", i});
            arrs.push_back({g.counts, 4 * n, 4, "counts", i});
        }
        for (const Arr& a : arrs) {
            if (a.o % a.align) { printf("%s: %s of group %zu at %llu is not aligned to %llu\n", shape, a.name, a.group, (unsigned long long)a.o, (unsigned long long)a.align); return false; }
            if (a.o + a.len > l.bytes) { printf("%s: %s of group %zu ends at %llu, past the %llu bytes\n", shape, a.name, a.group, (unsigned long long)(a.o + a.len), (unsigned long long)l.bytes); return false; }
        }
        std::sort(arrs.begin(), arrs.end(), [](const Arr& x, const Arr& y) { return x.o < y.o; });
        for (size_t i = 1; i < arrs.size(); ++i)
            if (arrs[i - 1].o + arrs[i - 1].len > arrs[i].o) {
                printf("%s (%s records, send list %llu, %zu sets): %s of group %zu [%llu, %llu) overlaps %s of group %zu at %llu\n", shape,
                       packed ? "9-byte" : "12-byte", (unsigned long long)total_send, sets.size(), arrs[i - 1].name, arrs[i - 1].group,
                       (unsigned long long)arrs[i - 1].o, (unsigned long long)(arrs[i - 1].o + arrs[i - 1].len), arrs[i].name, arrs[i].group, (unsigned long long)arrs[i].o);
                return false;
            }
        ++g_checked;
    }
    return true;
}

static bool pipelined(uint64_t total_send, uint64_t set_records) {
    return check(exchange_layout_pipelined(total_send, set_records), total_send, {set_records, set_records}, "pipelined");
}

static bool split(uint64_t total_send, const std::vector<uint64_t>& sets) {
    return check(exchange_layout(total_send, sets.data(), sets.size()), total_send, sets, "split");
}

int main() {
    const uint64_t large[] = {1ull << 20, 1ull << 28, (1ull << 31) + 5};
    // pipelined: every send list size up to 4096 against every set size up to 96, every 7th beyond and its own; the same the other way round
    for (uint64_t s = 0; s <= 4096; ++s) {
        for (uint64_t r = 0; r <= 4096; r += r < 96 ? 1 : 7)
            if (!pipelined(s, r) || !pipelined(r, s)) return 1;
        if (!pipelined(s, s)) return 1;
    }
    for (uint64_t s : large) {
        for (uint64_t r = 0; r <= 4096; ++r) if (!pipelined(s, r) || !pipelined(r, s)) return 1;
        for (uint64_t r : large) if (!pipelined(s, r)) return 1;
    }
    // split: C sets of different sizes, empty ones included
    for (uint64_t n = 0; n <= 4096; ++n) {
        if (!split(n, {n}) || !split(n, {0, n, 1, n + 1, 0}) || !split(0, {n, 32, 33, 0}) || !split(33, {0, 0, n})) return 1;
    }
    std::mt19937_64 rng(20261016);
    for (int rep = 0; rep < 200000; ++rep) {
        auto size = [&]() -> uint64_t {
            switch (rng() % 5) {
                case 0: return 0;
                case 1: return rng() % 40;
                case 2: return rng() % 4097;
                case 3: return 28 + rng() % 10;
                default: return rep % 97 == 0 ? large[rng() % 3] : rng() % 300;
            }
        };
        std::vector<uint64_t> sets(1 + rng() % 64);
        for (uint64_t& x : sets) x = size();
        if (!split(size(), sets)) return 1;
    }
    for (uint64_t s : large) if (!split(s, {0, large[0], 1, large[2], 32, 0, large[1]})) return 1;
    printf("exchange layout ok: %llu layouts\n", (unsigned long long)g_checked);
    return 0;
}
