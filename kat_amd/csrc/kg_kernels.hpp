// kg_kernels.hpp -- what the kernels that walk a base stream share, written for gfx950 (CDNA4, wave64): the geometry of a staged
// chunk (the constants, Chunk<W>) and the direct counter.
//
//  K1 k_count          extract + canonicalise + 2-bit pack + hash + insert      (replaces mer_iterator + hash_counter::add)
// K1 is one body for one-word and wide k-mers (k <= 32, 33 <= k <= 63: the template parameter W; kg_device.hpp "one body for both
// key widths").  kg_count.hip launches it, kg_context.hip asks for its occupancy, tools/ubench_count.hip measures against it.
// The chunk geometry is also what the partitioned counter (kg_partition.hpp, kg_partition_wide.hpp, kg_l1_blocks.hpp), the profile
// kernels (kg_query_kernels.hpp) and the per-record kernels (kg_filter.hpp, kg_record_stats.hpp, kg_record_regions.hpp) cut their
// input by.
//
// Every other kernel lives with the one unit that launches it, so that no unit compiles a kernel it cannot launch:
//   kg_count.hip             k_sweep                               kg_table.hip             k_regrow, k_total
//   kg_reduce_kernels.hpp    k_hist, k_gcp*, k_comp*               kg_query_kernels.hpp     k_get, k_profile*, k_hits_sum
//   kg_record_kernels.hpp    k_partition, k_export, k_merge        kg_exchange_kernels.hpp  k_extract_*, k_merge_apply / _deferred / 32, k_occupied
//   kg_synth_kernels.hpp     k_synth_*                             kg_rows_scan.hpp         k_rows_scan (two launchers)
//
// Integer / byte work bound by HBM (random 8-16 B slot accesses); not a contraction, so no MFMA.
#pragma once
#include "kg_device.hpp"
#include "kg_windows.hpp"
#include <type_traits>

namespace kg {

constexpr int COUNT_BLOCK = 256;                 // 4 waves
constexpr int CHUNK_BYTES = COUNT_BLOCK * BASES_PER_LANE;        // 4096 bytes staged per block iteration
constexpr int CHUNK_OVERLAP = 32;                // >= k-1 for k <= 32, keeps chunk starts 16-byte aligned
constexpr int CHUNK_STARTS = CHUNK_BYTES - CHUNK_OVERLAP;        // 4064 window start positions per chunk
constexpr int LANES_WITH_STARTS = CHUNK_STARTS / BASES_PER_LANE; // 254
constexpr int WIDE_OVERLAP = 64;                                   // >= k-1 for k <= 63, keeps chunk starts 16-byte aligned
constexpr int WIDE_CHUNK_STARTS = CHUNK_BYTES - WIDE_OVERLAP;      // 4032 window starts per staged chunk
constexpr int WIDE_LANES_WITH_STARTS = WIDE_CHUNK_STARTS / BASES_PER_LANE;   // 252

// a staged chunk of the direct kernels (K1, K8, K10) at either key width.  W: wide k-mers (33 <= k <= 63; kg_device.hpp "wide keys")
template <bool W>
struct Chunk {
    static constexpr int STARTS = W ? WIDE_CHUNK_STARTS : CHUNK_STARTS;
    static constexpr int LANES = STARTS / BASES_PER_LANE;               // lanes that own window starts
    typedef StagedTile<COUNT_BLOCK, W ? 4 : 2> Tile;
    typedef typename std::conditional<W, LaneWindowW, LaneWindow>::type Window;
};

// K1.  One block iteration stages 4096 consecutive bytes of the base stream: each lane issues one coalesced 16-byte
// load (1 KiB per wave instruction), packs it to 32 code bits + 16 validity bits and parks both in LDS.  After the
// barrier lane t owns the 16 window starts [16t, 16t+16) and slides its register window over them (kg_windows.hpp).
// The direct counter (global atomics): small inputs and whatever the partitioned counters leave.
template <bool ALIGNED, bool W = false>
__global__ void __launch_bounds__(COUNT_BLOCK)
k_count(DevTable t, const uint8_t* __restrict__ bases, uint64_t n, uint64_t n_chunks) {
    __shared__ typename Chunk<W>::Tile s;
    const uint32_t tid = threadIdx.x;
    const bool canonical = t.canonical != 0;
    uint32_t new_distinct = 0;
    s.pad();

    for (uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint64_t off = chunk * Chunk<W>::STARTS + (uint64_t)tid * BASES_PER_LANE;
        uint32_t w[4];
        load16<ALIGNED>(bases, n, off, w);
        uint32_t code, bad;
        encode16(w, code, bad);
        s.stage(code, bad);
        __syncthreads();

        if (tid < Chunk<W>::LANES) {
            typename Chunk<W>::Window lw;
            lw.init(s.code, s.bad, tid, t.k);
            constexpr int UNROLL = W ? 2 : 4;
#pragma unroll UNROLL
            for (int j = 0; j < BASES_PER_LANE; ++j, lw.step())
                if (lw.valid()) table_inc(t, lw.counted(t.k, canonical), new_distinct);
        }
        __syncthreads();
    }
    flush_distinct(t, new_distinct);
}

}  // namespace kg
