// kg_record_kernels.hpp -- a table out to (k-mer, count) records and records back into a table, written for gfx950 (CDNA4, wave64):
// what kg_records.hip launches beside k_filter (kg_filter.hpp).
//
//  K6 k_partition      every record of a table, counted or scattered by owner    (dump / export; the owner partition of the multi-GPU merge)
//     k_export         every record of a wide table, in slot order
//  K7 k_merge          add (key,count) records into a table
// k_partition and k_merge are one body each for one-word and wide k-mers (k <= 32, 33 <= k <= 63: the template parameter W;
// kg_device.hpp "one body for both key widths"); k_export is the wide tables' own export.  Streaming reads of the slots and
// random 8-16 B slot accesses for the adds, bound by HBM; no MFMA.
#pragma once
#include "kg_device.hpp"

namespace kg {

// K7: add (key,count) records of a record list into a table (what k_regrow, kg_table.hip, does with another table's slots).
template <bool W>
__global__ void __launch_bounds__(256)
k_merge(DevTable dst, RecCols<W, const uint64_t> rec, uint64_t n) {
    uint32_t new_distinct = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t c = rec.count[i];
        if (c) table_add(dst, rec.load(i), c, new_distinct);
    }
    flush_distinct(dst, new_distinct);
}

// ---- export / owner partition ----
// mode 0: count records per part into sizes[]; mode 1: scatter records to cursors[part]++.  A one-word table is walked over cap + 1
// slots (slot_rec_or_ones).
template <int MODE, bool W>
__global__ void __launch_bounds__(256)
k_partition(DevTable t, uint32_t n_ovf, uint32_t n_parts, unsigned long long* __restrict__ sizes_or_cursors, RecCols<W> out) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t end = W ? t.cap : t.cap + 1;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < end; i += stride) {
        const SlotRec<W> s = slot_rec_or_ones<W>(t, i, n_ovf);
        if (!s.occ) continue;
        const uint32_t part = n_parts > 1 ? owner_of(s.key, t.k, n_parts) : 0;
        const unsigned long long at = atomicAdd(&sizes_or_cursors[part], 1ULL);
        if (MODE == 1) out.store(at, s.key, s.total);
    }
}

// every (k-mer, count) of a wide table, in slot order: a wave compacts its occupied lanes with one ballot and one cursor add
static __global__ void __launch_bounds__(256)
k_export(DevTable t, uint32_t n_ovf, RecCols<true> out, unsigned long long* cursor) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t rounds = (t.cap + stride - 1) / stride;
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t r = 0; r < rounds; ++r) {
        const uint64_t i = first + r * stride;
        SlotRec<true> s{};
        if (i < t.cap) s = slot_rec<true>(t, i, n_ovf);
        const unsigned long long live = __ballot(s.occ);
        if (!live) continue;
        unsigned long long base = 0;
        if (lane == (uint32_t)(__ffsll((long long)live) - 1)) base = atomicAdd(cursor, (unsigned long long)__popcll(live));
        base = __shfl(base, __ffsll((long long)live) - 1, 64);
        if (s.occ) out.store(base + __popcll(live & ((1ULL << lane) - 1)), s.key, s.total);
    }
}

}  // namespace kg
