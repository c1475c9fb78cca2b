// Host check of kg_apply_lean.hpp: the packed apply's slot tests and step against the statements they replace -- pk_holds of kg_device.hpp
// (`w != 0 && (w >> cbits) == rem`: a __device__ function, restated here word for word), `w == 0` and the walk's next_slot
// (`s + 1 == S ? 0 : s + 1`) -- over every count-field width, remainders of 0, 1 and all ones, stored remainders that differ in one bit of
// either half of the word, and counts at the ends and the middle of their range.
// Built with hipcc -x hip (so that kg_device.hpp is the real one) and run on the CPU; prints "apply lean ok".
#include "../../kat_amd/csrc/kg_device.hpp"
#include "../../kat_amd/csrc/kg_apply_lean.hpp"

#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

using namespace kg;

static uint64_t checked = 0;
static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static bool holds64(uint64_t w, uint64_t rem, uint32_t cb) { return w != 0 && (w >> cb) == rem; }          // pk_holds
static uint32_t next_slot64(uint32_t s, uint32_t S) { return s + 1 == S ? 0 : s + 1; }

static void one_word(uint64_t w, uint64_t rem, uint32_t cb) {
    CHECK(ap_holds(w, rem, cb) == holds64(w, rem, cb), "w %016llx rem %llx cb %u", (unsigned long long)w, (unsigned long long)rem, cb);
    CHECK(ap_taken((uint32_t)w) == (w != 0), "w %016llx cb %u", (unsigned long long)w, cb);
    ++checked;
}

int main() {
    std::mt19937_64 rng(20261020);
    struct Shape { uint32_t cb, rb; };
    std::vector<Shape> shapes;
    for (uint32_t cb = 20; cb <= 32; ++cb) shapes.push_back({cb, 64 - cb});
    for (uint32_t rb : {31u, 24u, 16u, 9u}) shapes.push_back({32u, rb});          // cbits = min(64 - rb, 32)
    for (const Shape& sh : shapes) {
        const uint32_t cb = sh.cb, rb = sh.rb;
        const uint64_t rmask = rb == 64 ? ~0ULL : (1ULL << rb) - 1, half = pk_half(cb), cmax = pk_cmask(cb);
        const uint64_t seg_len = (half - 1) & ~3ULL;                                  // a walk covers fewer k-mers than half the range, a multiple of 4
        const uint64_t counts[5] = {1, 2, half, half + seg_len - 1, cmax};
        std::vector<uint64_t> rems = {0, 1, rmask};
        for (int i = 0; i < 3000; ++i) rems.push_back(rng() & rmask);
        for (uint64_t rem : rems) {
            const uint64_t key = rem << cb;
            // stored remainders: equal; differing in bit 0, in bit rb - 1, in a bit that lands in the word's low half and in one that lands in its
            // high half (where the remainder has such bits), and at random
            std::vector<uint64_t> stored = {rem, rem ^ 1, rem ^ (1ULL << (rb - 1)), rng() & rmask};
            if (cb < 32) stored.push_back(rem ^ (1ULL << (rng() % (32 - cb))));                                   // bits cb .. 31 of the word
            if (rb + cb > 32) { const uint32_t lo_bit = 32 - cb; stored.push_back(rem ^ (1ULL << (lo_bit + rng() % (rb - lo_bit)))); }   // bits 32 .. of the word
            for (uint64_t sr : stored)
                for (uint64_t c : counts) one_word((sr << cb) | c, rem, cb);
            one_word(0, rem, cb);                                // the free slot: never a hit, remainder 0 included
            // a claim's word is the key with a count of 1
            CHECK(holds64(key | 1, rem, cb), "rem %llx cb %u", (unsigned long long)rem, cb);
        }
    }
    // the step: next_slot where `go`, the slot itself where not
    for (uint32_t S : {64u, 256u, 3080u, 4096u, 9344u, 10240u})
        for (uint32_t s : {0u, 1u, S / 2, S - 2, S - 1}) {
            CHECK(ap_advance(s, true, S) == next_slot64(s, S), "s %u S %u", s, S);
            CHECK(ap_advance(s, false, S) == s, "s %u S %u", s, S);
            ++checked;
        }
    if (failures) { printf("apply lean FAILED: %d of %llu\n", failures, (unsigned long long)checked); return 1; }
    if (checked < 1000000) { printf("apply lean: only %llu checks\n", (unsigned long long)checked); return 1; }
    printf("apply lean ok: %llu words\n", (unsigned long long)checked);
    return 0;
}
