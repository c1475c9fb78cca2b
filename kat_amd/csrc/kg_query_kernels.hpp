// kg_query_kernels.hpp -- lookups that leave the table as it is, written for gfx950 (CDNA4, wave64): what kg_query.hip launches
// beside the kernels of kg_filter.hpp, kg_record_stats.hpp, kg_record_regions.hpp, kg_cvg_text.hpp and kg_gc_text.hpp.
//
//     k_get            batch lookup of keys                                      (replaces JellyfishHelper::getCount)
//  K8 k_profile        per-position lookup of a sequence's windows               (replaces the lookups of Sect::processSeq)
//     k_profile_owned, k_profile_scatter                                        the same across ranks: runs of (window, count) by owner, made dense on rank 0
//     k_hits_sum       rank 0 of k_seq_hits_owned (kg_filter.hpp): the ranks' per-record hit counts added up
// k_get and K8 are one body each for one-word and wide k-mers (k <= 32, 33 <= k <= 63: the template parameter W; kg_device.hpp
// "one body for both key widths").  Read-only probes of random 8-16 B slots, bound by HBM; no MFMA.
#pragma once
#include "kg_kernels.hpp"

namespace kg {

// ---- batch lookup (JellyfishHelper::getCount, lib/src/jellyfish_helper.cc:189-194): rec.count[i] = the table's count of key i ----
template <bool W>
__global__ void __launch_bounds__(256)
k_get(DevTable t, uint32_t n_ovf, RecCols<W> rec, uint64_t n, int canonicalise) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Key<W> key = rec.load(i);
    rec.count[i] = table_get(t, canonicalise ? kmer_canonical(key, t.k) : key, n_ovf);
}

// K8.  Per-position coverage of a sequence (kat sect / kat cold; src/sect.cc:516-535): out[i] = count of the k-window
// starting at base i, 0 when the window holds anything but ACGTacgt.  Same front end as k_count (16-byte loads, packed
// codes through LDS, a register window slid 16 times); the back end is a read-only probe, so the table's
// cache lines are shared between waves and nothing is atomic.  Each lane produces 16 consecutive counts = one 128-byte
// line of `out`, written as 8 dwordx4 stores.
template <bool ALIGNED, bool W>
__global__ void __launch_bounds__(COUNT_BLOCK)
k_profile(DevTable t, uint32_t n_ovf, int canonicalise, const uint8_t* __restrict__ bases, uint64_t n, uint64_t n_chunks,
          uint64_t* __restrict__ out) {
    __shared__ typename Chunk<W>::Tile s;
    const uint32_t tid = threadIdx.x;
    const uint32_t k = t.k;
    const uint64_t n_out = n - k + 1;
    s.pad();

    for (uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint64_t off = chunk * Chunk<W>::STARTS + (uint64_t)tid * BASES_PER_LANE;
        uint32_t w[4];
        load16<ALIGNED>(bases, n, off, w);
        uint32_t code, bad;
        encode16(w, code, bad);
        s.stage(code, bad);
        __syncthreads();

        if (tid < Chunk<W>::LANES && off < n_out) {
            typename Chunk<W>::Window lw;
            lw.init(s.code, s.bad, tid, k);
            uint64_t c[BASES_PER_LANE];
#pragma unroll
            for (int j = 0; j < BASES_PER_LANE; ++j, lw.step()) {           // (unrolled: c[j] stays in registers)
                c[j] = 0;
                if (lw.valid()) {
                    auto key = lw.fwd();
                    if (canonicalise) key = kmer_canonical(key, k);
                    c[j] = table_get(t, key, n_ovf);
                }
            }
            if (off + BASES_PER_LANE <= n_out) {
                ulonglong2* o = reinterpret_cast<ulonglong2*>(out + off);           // off is a multiple of 16: 128-byte aligned
#pragma unroll
                for (int j = 0; j < BASES_PER_LANE / 2; ++j) o[j] = make_ulonglong2(c[2 * j], c[2 * j + 1]);
            } else {
#pragma unroll
                for (int j = 0; j < BASES_PER_LANE; ++j) if (off + j < n_out) out[off + j] = c[j];
            }
        }
        __syncthreads();
    }
}

// K8 across ranks (katgpu_table_profile_gathered_host): after the exchange a k-mer lives on one rank, so every rank walks the same
// windows and looks up the ones whose k-mer it OWNS -- owner_of mixes the canonical form whatever the table's strand mode; the lookup
// follows `canonicalise` as in K8 -- and appends (window index, count) to its run wherever the count is not 0: two arrays, so that both
// stay naturally aligned.  A wave reserves its slots with one add: the ballot of its hits, their number, added by the first of them;
// the order within a run is free.  Every lane of a wave goes through the window loop (the ballots want them all; the pad words of the
// tile cover the last lanes' reads), and those that own no window start never hit.  n_ranks == 1: every window is this rank's.
// The run arrays hold a record per window start of the batch: there is no more room to check.
template <bool ALIGNED, bool W>
__global__ void __launch_bounds__(COUNT_BLOCK)
k_profile_owned(DevTable t, uint32_t n_ovf, int canonicalise, const uint8_t* __restrict__ bases, uint64_t n, uint64_t n_chunks,
                uint32_t rank, uint32_t n_ranks, uint32_t* __restrict__ run_idx, uint64_t* __restrict__ run_cnt,
                unsigned long long* __restrict__ run_len) {
    __shared__ typename Chunk<W>::Tile s;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t k = t.k;
    const uint64_t n_out = n - k + 1;
    s.pad();

    for (uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint64_t off = chunk * Chunk<W>::STARTS + (uint64_t)tid * BASES_PER_LANE;
        uint32_t w[4];
        load16<ALIGNED>(bases, n, off, w);
        uint32_t code, bad;
        encode16(w, code, bad);
        s.stage(code, bad);
        __syncthreads();

        const bool has_starts = tid < Chunk<W>::LANES;
        typename Chunk<W>::Window lw;
        lw.init(s.code, s.bad, tid, k);
        for (int j = 0; j < BASES_PER_LANE; ++j, lw.step()) {
            uint64_t c = 0;
            if (has_starts && off + j < n_out && lw.valid()) {
                auto key = lw.fwd();
                if (n_ranks == 1 || owner_of(key, k, n_ranks) == rank) {
                    if (canonicalise) key = kmer_canonical(key, k);
                    c = table_get(t, key, n_ovf);
                }
            }
            const unsigned long long hits = __ballot(c != 0);
            if (!hits) continue;
            const int first = __ffsll((long long)hits) - 1;
            unsigned long long base = 0;
            if (lane == (uint32_t)first) base = atomicAdd(run_len, (unsigned long long)__popcll(hits));
            base = __shfl(base, first, 64);
            if (c) {
                const unsigned long long at = base + __popcll(hits & ((1ULL << lane) - 1));
                run_idx[at] = (uint32_t)(off + j);
                run_cnt[at] = c;
            }
        }
        __syncthreads();
    }
}

// Rank 0 of the same: the batch's dense array from the runs.  CLEAR: out[0, n_out) = 0, a launch of its own -- a record's store must
// not be overtaken by another workgroup's zeros.  Otherwise out[run_idx[i]] = run_cnt[i] for the n_rec records of the runs laid behind
// one another: the ranks own disjoint k-mers, so no two records name one window, and plain stores do.  An index that names no window
// of the batch (the runs came over the wire) is dropped.
template <bool CLEAR>
static __global__ void __launch_bounds__(256)
k_profile_scatter(uint64_t* __restrict__ out, uint64_t n_out, const uint32_t* __restrict__ run_idx, const uint64_t* __restrict__ run_cnt, uint64_t n_rec) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (CLEAR ? n_out : n_rec); i += stride) {
        if (CLEAR) out[i] = 0;
        else { const uint32_t at = run_idx[i]; if (at < n_out) out[at] = run_cnt[i]; }
    }
}

// Rank 0 of k_seq_hits_owned (kg_filter.hpp): hits[r] += the n_parts arrays of m words that came from the other ranks, laid behind
// one another in `part`.
static __global__ void __launch_bounds__(256)
k_hits_sum(uint64_t* __restrict__ hits, const uint64_t* __restrict__ part, uint64_t m, uint32_t n_parts) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < m; r += stride) {
        uint64_t s = hits[r];
        for (uint32_t p = 0; p < n_parts; ++p) s += part[(uint64_t)p * m + r];
        hits[r] = s;
    }
}

}  // namespace kg
