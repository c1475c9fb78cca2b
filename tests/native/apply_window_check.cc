// Host check of kg_apply_lean.hpp's window selection (ap_first_event: the first slot of a drain window that is free or holds the remainder)
// against a plain loop over ap_holds / ap_taken, slot by slot: W = 2 and 4, every budget from 1 to W + 1, count fields of 20 to 32 bits, and
// in every position of the window a word that is free, another k-mer's, this k-mer's -- also where this k-mer's remainder is 0, whose word
// has nothing above the count --, so every event position, the event beyond the budget and no event come up; and ap_slot_at against
// repeated next_slot.  Built with hipcc -x hip (so that the headers are the real ones) and run on the CPU; prints "apply window ok".
#include "../../kat_amd/csrc/kg_device.hpp"
#include "../../kat_amd/csrc/kg_apply_lean.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>

using namespace kg;

static uint64_t checked = 0, seen_kind[3] = {0, 0, 0}, seen_at[5] = {0, 0, 0, 0, 0};
static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

template <int W>
static ApEvent plain(const unsigned long long (&w)[W], uint64_t rem, uint32_t cb, uint32_t budget) {
    const uint32_t n = budget < (uint32_t)W ? budget : (uint32_t)W;
    for (uint32_t j = 0; j < n; ++j) {
        if (ap_holds(w[j], rem, cb)) return ApEvent{AP_EV_HOLDS, j};
        if (!ap_taken((uint32_t)w[j])) return ApEvent{AP_EV_FREE, j};
    }
    return ApEvent{AP_EV_NONE, n};
}

enum Kind { FREE = 0, FOREIGN = 1, OWN = 2 };

template <int W>
static void windows(std::mt19937_64& rng) {
    int n_kinds = 1;
    for (int j = 0; j < W; ++j) n_kinds *= 3;
    for (uint32_t cb = 20; cb <= 32; ++cb) {
        const uint32_t rb = 64 - cb;
        const uint64_t rmask = (1ULL << rb) - 1, cmax = pk_cmask(cb), half = pk_half(cb);
        const uint64_t counts[4] = {1, 2, half, cmax};
        for (int r = 0; r < 40; ++r) {
            // remainder 0 (its own word is the count alone), 1, all ones, and random ones
            const uint64_t rem = r < 10 ? 0 : r == 10 ? 1 : r == 11 ? rmask : (rng() & rmask);
            for (int code = 0; code < n_kinds; ++code) {
                unsigned long long w[W];
                int c = code;
                for (int j = 0; j < W; ++j, c /= 3) {
                    const uint64_t cnt = counts[rng() & 3];
                    uint64_t other = rng() & rmask;                 // another k-mer's remainder: differs in one bit, or at random
                    if (rng() & 1) other = rem ^ (1ULL << (rng() % rb));
                    if (other == rem) other = rem ^ 1;
                    w[j] = c % 3 == FREE ? 0ULL : (((c % 3 == OWN ? rem : other) << cb) | cnt);
                }
                for (uint32_t budget = 1; budget <= (uint32_t)W + 1; ++budget) {
                    const ApEvent got = ap_first_event<W>(w, rem, cb, budget), want = plain<W>(w, rem, cb, budget);
                    CHECK(got.kind == want.kind && got.at == want.at, "W %d code %d rem %llx cb %u budget %u: kind %u at %u, want %u at %u", W, code,
                          (unsigned long long)rem, cb, budget, got.kind, got.at, want.kind, want.at);
                    ++checked; ++seen_kind[want.kind]; ++seen_at[want.at];
                }
            }
        }
    }
}

int main() {
    std::mt19937_64 rng(20261021);
    windows<2>(rng);
    windows<4>(rng);
    for (int k = 0; k < 3; ++k) CHECK(seen_kind[k] > 1000, "kind %d came up %llu times", k, (unsigned long long)seen_kind[k]);
    for (int a = 0; a < 5; ++a) CHECK(seen_at[a] > 1000, "offset %d came up %llu times", a, (unsigned long long)seen_at[a]);
    // the window's indices: slot + d with the wrap at S, d up to a window and up to the whole region
    for (uint32_t S : {64u, 256u, 4096u, 4100u, 9344u, 9700u})
        for (uint32_t s : {0u, 1u, S / 2, S - 5, S - 4, S - 3, S - 2, S - 1}) {
            uint32_t t = s;
            for (uint32_t d = 0; d <= 5; ++d) {
                CHECK(ap_slot_at(s, d, S) == t, "s %u d %u S %u", s, d, S);
                t = t + 1 == S ? 0 : t + 1;
                ++checked;
            }
            CHECK(ap_slot_at(s, S, S) == s, "s %u d S = %u", s, S);
        }
    if (failures) { printf("apply window FAILED: %d of %llu\n", failures, (unsigned long long)checked); return 1; }
    if (checked < 100000) { printf("apply window: only %llu checks\n", (unsigned long long)checked); return 1; }
    printf("apply window ok: %llu windows\n", (unsigned long long)checked);
    return 0;
}
