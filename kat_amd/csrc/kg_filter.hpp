// kg_filter.hpp -- the two hot loops of `kat filter`, written for gfx950 (CDNA4, wave64).
//
//  K9  k_filter<SEP, W>        one pass over every slot of a table: count x GC box -> keep / drop tables  (replaces FilterKmer::filterSlice)
//  K10 k_seq_hits              per-record number of windows found in a table                              (replaces FilterSeq::getProfile + the
//                                                                                                          nbFound loop of processSeq)
//      k_seq_hits_owned        the same over the windows whose k-mer this rank owns; k_hits_sum (kg_query_kernels.hpp) adds the ranks' arrays on rank 0
// Both units that launch these include this header (kg_records.hip: K9; kg_query.hip: K10), and kg_per_record.hip's record headers take
// the record search from it (hits_lower_bound), so it holds templates only: a kernel that is no template would be compiled into the
// units that do not launch it.  From kg_kernels.hpp it takes Chunk and COUNT_BLOCK.
// K9 rebuilds rather than clears: probing is linear inside a region (kg_device.hpp: Probe), so clearing a slot in place would cut the
// probe chain of every k-mer placed after it.  The keep / drop tables are made with the source's region grid, so a k-mer lands in the
// region of the same index it came from (a subset of a region's k-mers never probes further than the full set did) and the blocks that
// walk consecutive source slots write the same few destination regions: K2's re-insert (k_regrow), with a predicate in front.
#pragma once
#include "kg_kernels.hpp"

namespace kg {

// counters[] of katgpu_table_filter: distinct / total of the input, of the kept and of the dropped k-mers
constexpr int FC_ALL_D = 0, FC_ALL_T = 1, FC_KEEP_D = 2, FC_KEEP_T = 3, FC_DROP_D = 4, FC_DROP_T = 5, FC_N = 6;

struct FilterBox { uint64_t low_count, high_count; uint32_t low_gc, high_gc; };

// FilterKmer::inBounds (src/filter_kmer.cc:290-307): GC by popcount on the packed key, as k_gcp_pk
__device__ __forceinline__ bool filter_in_bounds(const FilterBox& b, uint64_t count, uint32_t gc) {
    return b.low_gc <= gc && gc <= b.high_gc && b.low_count <= count && count <= b.high_count;
}

// a lane's share of the six counters (FilterTally::c is only ever indexed by constants: it stays in registers); one atomic each per wave
struct FilterTally {
    uint64_t c[FC_N];
    __device__ __forceinline__ void add(bool keep, bool drop, uint64_t cnt) {
        c[FC_ALL_D] += 1; c[FC_ALL_T] += cnt;
        c[FC_KEEP_D] += keep ? 1 : 0; c[FC_KEEP_T] += keep ? cnt : 0;
        c[FC_DROP_D] += drop ? 1 : 0; c[FC_DROP_T] += drop ? cnt : 0;
    }
    __device__ __forceinline__ void flush(unsigned long long* __restrict__ out) {
#pragma unroll
        for (int i = 0; i < FC_N; ++i) {
            uint64_t s = c[i];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
            if ((threadIdx.x & 63) == 0 && s) atomicAdd(&out[i], (unsigned long long)s);
        }
    }
};

// Routing of FilterKmer::filterSlice (src/filter_kmer.cc:251-288): without `separate` a k-mer is kept when in_bounds != invert;
// with it, in-bounds k-mers are kept and the rest dropped -- `invert` plays no part there, whatever the help text says.
template <bool SEP>
__device__ __forceinline__ bool filter_keeps(bool in_b, bool invert) { return SEP ? in_b : in_b != invert; }

// K9, one body for one-word tables (P8 and KV12) and wide ones (W: k = 33 .. 63).  slot_rec gives the full count of a slot -- the
// in-slot count plus its side-table entry -- and table_add splits it again for the destination slot, so side-table entries follow
// their k-mer.  The all-ones k-mer a one-word table keeps in its counter block (k = 32, non-canonical) is routed by lane 0 of block 0.
template <bool SEP, bool W>
__global__ void __launch_bounds__(256)
k_filter(DevTable keep, DevTable drop, DevTable src, uint32_t src_n_ovf, FilterBox box, int invert, unsigned long long* __restrict__ counters) {
    uint32_t nd_keep = 0, nd_drop = 0;
    FilterTally v{{0, 0, 0, 0, 0, 0}};
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < src.cap; i += stride) {
        const SlotRec<W> s = slot_rec<W>(src, i, src_n_ovf);
        if (!s.occ) continue;
        const bool to_keep = filter_keeps<SEP>(filter_in_bounds(box, s.total, kmer_gc(s.key, src.k)), invert != 0);
        if (to_keep) table_add(keep, s.key, s.total, nd_keep);
        else if (SEP) table_add(drop, s.key, s.total, nd_drop);
        v.add(to_keep, SEP && !to_keep, s.total);
    }
    if constexpr (!W) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            const uint64_t ones = src.ctrs[CTR_ONES];
            if (ones) {
                const bool to_keep = filter_keeps<SEP>(filter_in_bounds(box, ones, kmer_gc(EMPTY, src.k)), invert != 0);
                if (to_keep) atomicAdd((unsigned long long*)&keep.ctrs[CTR_ONES], (unsigned long long)ones);
                else if (SEP) atomicAdd((unsigned long long*)&drop.ctrs[CTR_ONES], (unsigned long long)ones);
                v.add(to_keep, SEP && !to_keep, ones);
            }
        }
    }
    flush_distinct(keep, nd_keep);
    if (SEP) flush_distinct(drop, nd_drop);
    v.flush(counters);
}

// K10.  hits[r] = windows of record r that hold only ACGTacgt and whose k-mer the table counts (FilterSeq::getProfile,
// src/filter_sequence.cc:398-430, summed as processSeq does).  k_profile's front end (16-byte loads, packed codes through LDS, a register
// window slid 16 times per lane); its back end keeps no per-position count: a lane runs along its 16 window starts, knows the record they
// lie in (records are given by start and length, in increasing order and disjoint), and adds its run of hits for that record to an LDS
// bin once the record changes.  A block's bins go to HBM once per chunk, one atomic per record it saw: 8 bytes per record where
// k_profile writes 8 per position.  A window is looked up only when it lies inside one record.
constexpr int HITS_LDS_RECS = 2048;   // records of a chunk with an LDS bin (a chunk with more -- empty records -- adds the rest to HBM directly)

__device__ __forceinline__ uint64_t hits_lower_bound(const uint64_t* __restrict__ a, const uint64_t* __restrict__ len, uint64_t lo, uint64_t hi,
                                                     uint64_t x, bool by_end) {
    while (lo < hi) {                                              // first r in [lo, hi) with (start, or end) >= x (resp. > x for ends)
        const uint64_t mid = lo + (hi - lo) / 2;
        const bool before = by_end ? a[mid] + len[mid] <= x : a[mid] < x;
        if (before) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One body for K10 and its owned form (OWNED: `rank` and `n_ranks` are read, and a window whose k-mer another rank owns is passed over).
template <bool ALIGNED, bool W, bool OWNED>
__device__ __forceinline__ void seq_hits_body(const DevTable& t, uint32_t n_ovf, int canonicalise, const uint8_t* __restrict__ bases, uint64_t n, uint64_t n_chunks,
                                              const uint64_t* __restrict__ rec_start, const uint64_t* __restrict__ rec_len, uint64_t n_rec,
                                              unsigned long long* __restrict__ hits, uint32_t rank, uint32_t n_ranks) {
    constexpr int CS = Chunk<W>::STARTS;
    __shared__ typename Chunk<W>::Tile s;
    __shared__ uint32_t s_hits[HITS_LDS_RECS];
    __shared__ uint64_t s_r[2];
    const uint32_t tid = threadIdx.x;
    const uint32_t k = t.k;
    const uint64_t n_out = n - k + 1;
    s.pad();
    for (uint32_t i = tid; i < HITS_LDS_RECS; i += COUNT_BLOCK) s_hits[i] = 0;

    for (uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint64_t c0 = chunk * CS;
        const uint64_t c1 = c0 + CS < n_out ? c0 + CS : n_out;
        if (tid == 0) {                                            // the records that meet [c0, c1): ends beyond c0, starts before c1
            const uint64_t lo = hits_lower_bound(rec_start, rec_len, 0, n_rec, c0, true);
            s_r[0] = lo;
            s_r[1] = hits_lower_bound(rec_start, rec_len, lo, n_rec, c1, false);
        }
        const uint64_t off = c0 + (uint64_t)tid * BASES_PER_LANE;
        uint32_t w[4];
        load16<ALIGNED>(bases, n, off, w);
        uint32_t code, bad;
        encode16(w, code, bad);
        s.stage(code, bad);
        __syncthreads();
        const uint64_t r_lo = s_r[0], r_hi = s_r[1];

        if (tid < Chunk<W>::LANES && off < n_out && r_lo < r_hi) {
            // the record of the first window start: the last one of [r_lo, r_hi) that starts at or before it (none: r = r_lo - 1)
            int64_t r = (int64_t)hits_lower_bound(rec_start, rec_len, r_lo, r_hi, off + 1, false) - 1;
            uint64_t rs = 0, re = 0;
            if (r >= (int64_t)r_lo) { rs = rec_start[r]; re = rs + rec_len[r]; }
            uint64_t ns = (uint64_t)(r + 1) < r_hi ? rec_start[r + 1] : ~0ULL;
            int64_t cur = -1;
            uint32_t run = 0;
            auto flush = [&]() {
                if (!run) return;
                const uint64_t idx = (uint64_t)cur - r_lo;
                if (idx < HITS_LDS_RECS) atomicAdd(&s_hits[idx], run);
                else atomicAdd(&hits[cur], (unsigned long long)run);
            };
            typename Chunk<W>::Window lw;
            lw.init(s.code, s.bad, tid, k);
            for (int j = 0; j < BASES_PER_LANE; ++j, lw.step()) {
                const uint64_t pos = off + j;
                while (pos >= ns) { ++r; rs = ns; re = rs + rec_len[r]; ns = (uint64_t)(r + 1) < r_hi ? rec_start[r + 1] : ~0ULL; }
                if (r >= (int64_t)r_lo && pos >= rs && pos + k <= re && lw.valid()) {
                    auto key = lw.fwd();
                    bool mine = true;
                    if constexpr (OWNED) mine = n_ranks == 1 || owner_of(key, k, n_ranks) == rank;
                    if (mine) {
                        if (canonicalise) key = kmer_canonical(key, k);
                        if (table_get(t, key, n_ovf)) { if (r != cur) { flush(); cur = r; run = 0; } ++run; }
                    }
                }
            }
            flush();
        }
        __syncthreads();
        const uint64_t nb = r_hi - r_lo < (uint64_t)HITS_LDS_RECS ? r_hi - r_lo : (uint64_t)HITS_LDS_RECS;
        for (uint32_t i = tid; i < nb; i += COUNT_BLOCK) {
            const uint32_t h = s_hits[i];
            if (h) { atomicAdd(&hits[r_lo + i], (unsigned long long)h); s_hits[i] = 0; }
        }
        __syncthreads();
    }
}

template <bool ALIGNED, bool W>
__global__ void __launch_bounds__(COUNT_BLOCK)
k_seq_hits(DevTable t, uint32_t n_ovf, int canonicalise, const uint8_t* __restrict__ bases, uint64_t n, uint64_t n_chunks,
           const uint64_t* __restrict__ rec_start, const uint64_t* __restrict__ rec_len, uint64_t n_rec, unsigned long long* __restrict__ hits) {
    seq_hits_body<ALIGNED, W, false>(t, n_ovf, canonicalise, bases, n, n_chunks, rec_start, rec_len, n_rec, hits, 0, 1);
}

// K10 across ranks (katgpu_table_seq_hits_gathered_host): after the exchange a k-mer lives on one rank, so every rank walks the same
// records and looks up the windows whose k-mer it OWNS -- owner_of mixes the canonical form whatever the table's strand mode; the lookup
// follows `canonicalise` as in K10.  Hits add across owners: a record's hit count is the sum of the ranks' (k_hits_sum, on rank 0).
// n_ranks == 1: every window is this rank's.
template <bool ALIGNED, bool W>
__global__ void __launch_bounds__(COUNT_BLOCK)
k_seq_hits_owned(DevTable t, uint32_t n_ovf, int canonicalise, const uint8_t* __restrict__ bases, uint64_t n, uint64_t n_chunks,
                 const uint64_t* __restrict__ rec_start, const uint64_t* __restrict__ rec_len, uint64_t n_rec, unsigned long long* __restrict__ hits,
                 uint32_t rank, uint32_t n_ranks) {
    seq_hits_body<ALIGNED, W, true>(t, n_ovf, canonicalise, bases, n, n_chunks, rec_start, rec_len, n_rec, hits, rank, n_ranks);
}

}  // namespace kg
