// kg_exchange_layout.hpp -- where the arrays of the multi-GPU exchange (kg_comm_exchange.hip, struct Exchange) lie in its buffer: the send list
// and the receive sets, each a group of record arrays.  Host arithmetic only (no device code): exchange_bytes, the split buffer's size
// and Exchange::plan's carve-up all come from here, and tests/native/exchange_layout_check.cc checks it on the CPU.
//
// A group of n records (room for at least one) in either wire form:
//   key + count (12 bytes):     keys   u64[n] at +0,                 counts u32[n] at +xkey_room(n)
//   packed (4 + 1 + 4 bytes):   rem_lo u32[n] at +0, rem_hi u8[n] at +xalign(4n), counts u32[n] at +xkey_room(n)
// The key room holds either the keys or rem_lo then rem_hi: it is the larger of the two (for n <= 32, 8n bytes round up to the same
// 256 as 4n, and rem_hi has to lie past rem_lo's room).  One layout serves both forms because the buffer is sized before the ranks
// agree on the form.  Every array starts on 256 bytes.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace kg {

inline uint64_t xalign(uint64_t n, uint64_t a = 256) { return (n + a - 1) / a * a; }

struct XGroup { uint64_t keys, rem_lo, rem_hi, counts, n; };     // byte offsets from the buffer's start; n: records it has room for (>= 1)
struct XLayout { XGroup send; std::vector<XGroup> sets; uint64_t bytes; };

inline uint64_t xkey_room(uint64_t n) { return std::max(xalign(8 * n), xalign(4 * n) + xalign(n)); }

inline XGroup xgroup_at(uint64_t& at, uint64_t n_records) {
    const uint64_t n = std::max<uint64_t>(n_records, 1);
    const XGroup g{at, at, at + xalign(4 * n), at + xkey_room(n), n};
    at += xkey_room(n) + xalign(4 * n);
    return g;
}

// the send list of `total_send` records, then a receive set per entry of `set_records` (pipelined: two of the largest chunk; split:
// one per chunk, empty ones included), then 256 bytes of slack
inline XLayout exchange_layout(uint64_t total_send, const uint64_t* set_records, size_t n_sets) {
    XLayout l;
    uint64_t at = 0;
    l.send = xgroup_at(at, total_send);
    l.sets.reserve(n_sets);
    for (size_t i = 0; i < n_sets; ++i) l.sets.push_back(xgroup_at(at, set_records[i]));
    l.bytes = at + 256;
    return l;
}

inline XLayout exchange_layout_pipelined(uint64_t total_send, uint64_t set_records) {
    const uint64_t two[2] = {set_records, set_records};
    return exchange_layout(total_send, two, 2);
}

}  // namespace kg
