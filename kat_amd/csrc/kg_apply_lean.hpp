// kg_apply_lean.hpp -- the slot tests and the step of the packed apply's walk (kg_partition.hpp: ApkWalk), written for their instruction count.
//
// A packed slot is one 64-bit word, remainder << cbits | count, 0 = free (kg_device.hpp "P8").  The walk is bound by the VECTOR instructions it
// issues, and per k-mer and probe round the compiler's plain form spent ten: `word != 0` and `word == 0` as two 64-bit
// compares, the shift, the compare with the remainder, the select of the add's operand, four for next_slot under its condition, and the LDS
// address.  Here "taken" is ONE 32-bit compare of the word's low half, "free" its complement (a scalar and-not), and the step is an add of
// the condition, a subtract and a minimum: nine per k-mer and round with the shift, the compare and the address.  The shift by cbits and the 64-bit compare with the
// remainder stay: the same test on 32-bit halves (the key = remainder << cbits made once per k-mer, two xors, an and-or and a compare per
// round) is one instruction MORE -- built, measured 4.6 ms per step slower than the plain form and taken out
// (profiles/apply_lean_parent_vs_branch.txt); that a 64-bit shift or compare issues like a 32-bit instruction on gfx950 is read from that
// A/B, not from a microbenchmark.
// Every function is plain integer arithmetic and compiles for the host too: tests/native/apply_lean_check.cc compares each with pk_holds of
// kg_device.hpp, `word == 0` and next_slot, word by word.
#pragma once
#include <stdint.h>
#include "kg_device.hpp"
#include "kg_l1_lean.hpp"         // KG_LEAN_FN

namespace kg {

// An occupied slot counts 1 .. 2^cbits - 1 in the low cbits <= 32 bits of its word throughout a walk (the 1 .. half invariant of table_add_pk,
// a walk covers fewer k-mers than half the range, and add1 never carries: add1 relies on the same three), so the low word alone says whether
// the slot is taken -- also when the remainder stored there is 0.
KG_LEAN_FN bool ap_taken(uint32_t word_lo) { return word_lo != 0; }
// pk_holds: the slot is taken, by this remainder (a free slot holds nothing, a remainder of 0 included)
KG_LEAN_FN bool ap_holds(unsigned long long word, uint64_t rem, uint32_t cbits) { return ap_taken((uint32_t)word) && (word >> cbits) == rem; }
// the next slot of a region of S slots, taken only where `go`: s + go, S -> 0 (unsigned: s + go - S wraps to a number above s + go unless that is S)
KG_LEAN_FN uint32_t ap_advance(uint32_t s, bool go, uint32_t S) {
    const uint32_t t = s + (go ? 1u : 0u), w = t - S;
    return w < t ? w : t;
}

// The drain's window (ApkWalk::drain_pass): W consecutive slots read in one round trip, of which a k-mer with `budget` slots left to probe may
// use the first min(W, budget).  Its first EVENT is the lowest of them that is free or holds the remainder; the slots in front of it hold other
// k-mers.  `at` is the event's offset -- and with no event the number of slots the window has covered, min(W, budget): what the k-mer advances by.
// A free slot is free whatever its high bits compare to (a remainder of 0 equals a free word's): the low half decides first, as in ap_holds.
// Per slot: the shift and compare of ap_holds, the 32-bit compare of ap_taken, the scalar or / and with the constant `j < budget`, and two selects;
// taken from the last slot to the first, so that the lowest event is the one that stays -- no chain of "found already" conditions.
enum ApEventKind : uint32_t { AP_EV_NONE = 0, AP_EV_HOLDS = 1, AP_EV_FREE = 2 };
struct ApEvent { uint32_t kind, at; };
template <int W>
KG_LEAN_FN ApEvent ap_first_event(const unsigned long long (&word)[W], uint64_t rem, uint32_t cbits, uint32_t budget) {
    ApEvent e{AP_EV_NONE, budget < (uint32_t)W ? budget : (uint32_t)W};
#pragma unroll
    for (int j = W - 1; j >= 0; --j) {
        const bool fr = !ap_taken((uint32_t)word[j]);
        const bool ev = (fr || (word[j] >> cbits) == rem) && (uint32_t)j < budget;
        e.kind = ev ? (fr ? AP_EV_FREE : AP_EV_HOLDS) : e.kind;
        e.at = ev ? (uint32_t)j : e.at;
    }
    return e;
}
// slot s + d of a region of S slots, for d <= S (the window's indices: each from s, none from its neighbour)
KG_LEAN_FN uint32_t ap_slot_at(uint32_t s, uint32_t d, uint32_t S) {
    const uint32_t t = s + d, w = t - S;
    return w < t ? w : t;
}

}  // namespace kg
