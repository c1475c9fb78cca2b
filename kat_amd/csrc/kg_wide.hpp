// kg_wide.hpp -- the kernels that exist only for wide tables (33 <= k <= 63; kg_device.hpp "wide keys"): regrow, record merge,
// export, owner partition, lookup.  The direct counter and the per-position profile are k_count<ALIGNED, true> and
// k_profile<ALIGNED, true> (kg_kernels.hpp: one body for both key widths); the reducers (k_hist, k_total, k_gcp<true>,
// k_comp<PASS, true>, k_comp3_pass1<true>, k_comp3_pass3) are the narrow ones with the second key word read where the k-mer itself
// matters.
//
// Replaces the same reference code as the narrow kernels -- multi-word mer_dna (mer_dna.hpp:235-258,330-378) and hash_counter --
// for k-mers that take two machine words.  Inputs of size are counted through kg_partition_wide.hpp (16-byte items through two radix
// levels, regions applied in LDS).
#pragma once
#include "kg_kernels.hpp"

namespace kg {

// K2 for wide tables: hash_counter::double_size (hash_counter.hpp:204-244)
static __global__ void __launch_bounds__(256)
k_regrow_w(DevTable dst, DevTable src, uint32_t src_n_ovf) {
    uint32_t new_distinct = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < src.cap; i += stride) {
        const uint64_t a = src.keys[i];
        if (a != EMPTY) table_add_w(dst, KeyW{a, src.keys_b[i]}, slot_count(src, i, i, src_n_ovf), new_distinct);
    }
    flush_distinct(dst, new_distinct);
}

// K7 for wide tables: (hi, lo, count) records into a table
static __global__ void __launch_bounds__(256)
k_merge_w(DevTable dst, const uint64_t* __restrict__ hi, const uint64_t* __restrict__ lo, const uint64_t* __restrict__ counts, uint64_t n) {
    uint32_t new_distinct = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (counts[i]) table_add_w(dst, keyw_from_words(hi[i], lo[i]), counts[i], new_distinct);
    flush_distinct(dst, new_distinct);
}

// every (k-mer, count) of the table, in slot order: a wave compacts its occupied lanes with one ballot and one cursor add
static __global__ void __launch_bounds__(256)
k_export_w(DevTable t, uint32_t n_ovf, uint64_t* __restrict__ hi, uint64_t* __restrict__ lo, uint64_t* __restrict__ counts, unsigned long long* cursor) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t rounds = (t.cap + stride - 1) / stride;
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t r = 0; r < rounds; ++r) {
        const uint64_t i = first + r * stride;
        const uint64_t a = i < t.cap ? t.keys[i] : EMPTY;
        const bool occ = a != EMPTY;
        const unsigned long long live = __ballot(occ);
        if (!live) continue;
        unsigned long long base = 0;
        if (lane == (uint32_t)(__ffsll((long long)live) - 1)) base = atomicAdd(cursor, (unsigned long long)__popcll(live));
        base = __shfl(base, __ffsll((long long)live) - 1, 64);
        if (occ) {
            const uint64_t at = base + __popcll(live & ((1ULL << lane) - 1));
            const KeyW kw{a, t.keys_b[i]};
            hi[at] = keyw_hi(kw); lo[at] = keyw_lo(kw); counts[at] = slot_count(t, i, i, n_ovf);
        }
    }
}

// owner-partitioned export for the multi-GPU merge (k_partition for wide tables).  MODE 0: records per part; MODE 1: scatter
// (hi, lo, count) records to cursors[part]++.
template <int MODE>
__global__ void __launch_bounds__(256)
k_partition_w(DevTable t, uint32_t n_ovf, uint32_t n_parts, unsigned long long* __restrict__ sizes_or_cursors,
              uint64_t* __restrict__ out_hi, uint64_t* __restrict__ out_lo, uint64_t* __restrict__ out_counts) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < t.cap; i += stride) {
        const uint64_t a = t.keys[i];
        if (a == EMPTY) continue;
        const KeyW kw{a, t.keys_b[i]};
        const uint32_t part = n_parts > 1 ? owner_of_w(kw, t.k, n_parts) : 0;
        const unsigned long long at = atomicAdd(&sizes_or_cursors[part], 1ULL);
        if (MODE == 1) { out_hi[at] = keyw_hi(kw); out_lo[at] = keyw_lo(kw); out_counts[at] = slot_count(t, i, i, n_ovf); }
    }
}

// batch lookup (JellyfishHelper::getCount, lib/src/jellyfish_helper.cc:189-194)
static __global__ void __launch_bounds__(256)
k_get_w(DevTable t, uint32_t n_ovf, const uint64_t* __restrict__ hi, const uint64_t* __restrict__ lo, uint64_t n, int canonicalise, uint64_t* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    KeyW kw = keyw_from_words(hi[i], lo[i]);
    if (canonicalise) kw = keyw_canonical(kw, t.k);
    out[i] = table_get_w(t, kw, n_ovf);
}

}  // namespace kg
