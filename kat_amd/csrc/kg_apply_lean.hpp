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

}  // namespace kg
