// kg_record_regions.hpp -- count-range regions of records on the device, written for gfx950 (CDNA4, wave64): what Sect::printRegions
// (src/sect.cc:373-424) keeps of a record's per-position counts -- the maximal runs of window starts whose count lies in a range --
// without the counts leaving the device.  One or two ranges share the lookups (`sect -E -F`).
//
//  K14 k_regions_mask    every window of every record looked up once; one bit per base position and range says "in range", one more
//                        says "a record's first window": (1 + ranges) / 8 bytes per base where k_profile writes 8
//  K15 k_regions_count   run starts and run ends in every RG_BLOCK words of the masks
//  K16 k_regions_scan    those counts to offsets, range 1's regions behind range 0's
//  K17 k_regions_emit    the masks again, no table access: the i-th run start writes (record, start) of region i, the i-th run end its
//                        stop -- starts and ends alternate in position order, so they meet in the same region
//
// K14 uses the front end of kg_windows.hpp (load16 / encode16 / Chunk<W>::Tile / Window), k_rstats_long's walk along the records and
// its two sources of counts (kg_record_stats.hpp: CountsTable / CountsDense), so one body serves both key widths and both sources.  Records are given by start and length, increasing and disjoint (the convention of k_seq_hits); a
// window belongs to a record when it lies wholly inside it; an invalid window (a byte outside ACGTacgt) counts 0.  A position's bit in a
// mask is bit (position & 63) of word (position >> 6): a lane's 16 starts are one 16-bit store, and nobody else writes them.
// Whether a run opens at a position depends on the position before it, which another lane, chunk or block owns: K15 and K17 take
// both from the masks (rg_edges), the same way, so the offsets K16 makes are the ones K17 fills -- whatever the masks hold.  A run
// never continues into another record: records that touch have their last and first windows side by side only at k = 1, and there
// the "first window" bit cuts the run.
#pragma once
#include "kg_record_stats.hpp"

namespace kg {

constexpr int RG_MAX_RANGES = 2;
constexpr int RG_BLOCK = 256;                                        // K15 / K17: mask words (of 64 positions) per block iteration
constexpr int RG_SCAN_BLOCK = 1024;                                  // K16: one block
constexpr int RG_FIELDS = 3;                                         // katgpu_region (include/katgpu.h) as three 64-bit words
constexpr int RG_RECORD = 0, RG_START = 1, RG_STOP = 2;

struct RgRanges { uint64_t min[RG_MAX_RANGES], max[RG_MAX_RANGES]; uint32_t n; };   // max == 0: no upper bound

__device__ __forceinline__ bool rg_in(const RgRanges& rg, int q, uint64_t c) { return c >= rg.min[q] && (rg.max[q] == 0 || c <= rg.max[q]); }

// K14.  Chunks are cut by bytes, as in k_rstats_long: a chunk owns Chunk<W>::STARTS positions and the windows that start on them.  A lane
// runs along its 16 positions, knows the record they lie in, looks up the windows that lie inside it (0 for an invalid one) and keeps
// three 16-bit words: first window of a record | in range 0 | in range 1.  Every position below 64 * n_words gets its bits, zeros where
// no window starts: the masks need no clearing.  mask: 1 + rg.n arrays of 4 * n_words 16-bit words.
template <bool ALIGNED, bool W, typename Src>
__global__ void __launch_bounds__(COUNT_BLOCK)
k_regions_mask(Src src, const uint8_t* __restrict__ bases, uint64_t n, uint64_t n_chunks,
               const uint64_t* __restrict__ rec_start, const uint64_t* __restrict__ rec_len, uint64_t n_rec, RgRanges rg, uint64_t n_words,
               uint16_t* __restrict__ mask) {
    constexpr int CS = Chunk<W>::STARTS;
    __shared__ typename Chunk<W>::Tile s;
    __shared__ uint64_t s_r[2];
    const uint32_t tid = threadIdx.x;
    const uint32_t k = src.k();
    s.pad();

    for (uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint64_t c0 = chunk * CS;
        const uint64_t c1 = c0 + CS < n ? c0 + CS : n;
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

        uint32_t first = 0, in0 = 0, in1 = 0;
        if (tid < Chunk<W>::LANES && off < n && r_lo < r_hi) {
            // the record of the first position: the last one of [r_lo, r_hi) that starts at or before it (none: r = r_lo - 1)
            int64_t r = (int64_t)hits_lower_bound(rec_start, rec_len, r_lo, r_hi, off + 1, false) - 1;
            uint64_t rs = 0, re = 0;
            if (r >= (int64_t)r_lo) { rs = rec_start[r]; re = rs + rec_len[r]; }
            uint64_t ns = (uint64_t)(r + 1) < r_hi ? rec_start[r + 1] : ~0ULL;
            typename Chunk<W>::Window lw;
            lw.init(s.code, s.bad, tid, k);
            for (int j = 0; j < BASES_PER_LANE; ++j, lw.step()) {
                const uint64_t pos = off + j;
                while (pos >= ns) { ++r; rs = ns; re = rs + rec_len[r]; ns = (uint64_t)(r + 1) < r_hi ? rec_start[r + 1] : ~0ULL; }
                if (r < (int64_t)r_lo || pos < rs || pos + k > re || pos + k > n) continue;
                uint64_t c = 0;
                if (lw.valid()) c = src.get(lw, pos);
                first |= (uint32_t)(pos == rs) << j;
                in0 |= (uint32_t)rg_in(rg, 0, c) << j;
                in1 |= (uint32_t)(rg.n > 1 && rg_in(rg, 1, c)) << j;
            }
        }
        if (tid < Chunk<W>::LANES && off < n_words * 64) {
            const uint64_t i = off / BASES_PER_LANE;
            mask[i] = (uint16_t)first;
            mask[4 * n_words + i] = (uint16_t)in0;
            if (rg.n > 1) mask[8 * n_words + i] = (uint16_t)in1;
        }
        __syncthreads();
    }
}

// the positions of word w where a run opens, and where one closes (its last position): between two neighbouring positions a run breaks
// unless both are in range and the second is no record's first window
struct RgEdges { uint64_t open, close; };
__device__ __forceinline__ RgEdges rg_edges(const uint64_t* __restrict__ first, const uint64_t* __restrict__ in, uint64_t w, uint64_t n_words) {
    RgEdges e{0, 0};
    if (w >= n_words) return e;
    const uint64_t m = in[w];
    if (!m) return e;
    const uint64_t f = first[w];
    const uint64_t prev = w ? in[w - 1] >> 63 : 0;
    uint64_t next = 0, fnext = 0;
    if (w + 1 < n_words) { next = in[w + 1] & 1; fnext = first[w + 1] & 1; }
    e.open = m & (~((m << 1) | prev) | f);
    e.close = m & (~((m >> 1) | (next << 63)) | (f >> 1) | (fnext << 63));
    return e;
}
// a thread's opens and closes (at most 64 each) in one word, and a block's (at most 16384 each): 16 bits a piece
__device__ __forceinline__ uint32_t rg_pack(const RgEdges& e) { return (uint32_t)__popcll(e.open) | ((uint32_t)__popcll(e.close) << 16); }
// sums of v over the threads before this one in a block of RG_BLOCK, and over all of them; s_w: RG_BLOCK / 64 words, free to write
__device__ __forceinline__ uint32_t rg_block_before(uint32_t v, uint32_t* s_w, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if ((int)lane >= d) inc += o; }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint32_t before = inc - v;
    total = 0;
#pragma unroll
    for (uint32_t i = 0; i < RG_BLOCK / 64; ++i) { const uint32_t x = s_w[i]; if (i < wave) before += x; total += x; }
    __syncthreads();
    return before;
}

// K15.  cnt[(q * n_blk + b) * 2 + {0, 1}] = run starts, run ends of range q in words [b * RG_BLOCK, (b + 1) * RG_BLOCK)
static __global__ void __launch_bounds__(RG_BLOCK)
k_regions_count(const uint64_t* __restrict__ masks, uint64_t n_words, uint64_t n_blk, uint32_t n_ranges, unsigned long long* __restrict__ cnt) {
    __shared__ uint32_t s_w[RG_BLOCK / 64];
    for (uint64_t b = blockIdx.x; b < n_blk; b += gridDim.x)
        for (uint32_t q = 0; q < n_ranges; ++q) {
            uint32_t total;
            rg_block_before(rg_pack(rg_edges(masks, masks + (q + 1) * n_words, b * RG_BLOCK + threadIdx.x, n_words)), s_w, total);
            if (threadIdx.x == 0) { cnt[(q * n_blk + b) * 2] = total & 0xFFFF; cnt[(q * n_blk + b) * 2 + 1] = total >> 16; }
        }
}

// K16.  In place: the counts of K15 become the index of a block's first run start and first run end among the regions of the call,
// range q + 1's regions following range q's; totals[q] = regions of range q.  One block, RG_SCAN_BLOCK mask blocks a round.
static __global__ void __launch_bounds__(RG_SCAN_BLOCK)
k_regions_scan(unsigned long long* __restrict__ cnt, uint64_t n_blk, uint32_t n_ranges, unsigned long long* __restrict__ totals) {
    __shared__ uint64_t s_o[RG_SCAN_BLOCK / 64], s_c[RG_SCAN_BLOCK / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t base = 0;                                             // regions of the ranges before q
    for (uint32_t q = 0; q < n_ranges; ++q) {
        uint64_t base_o = base, base_c = base;
        for (uint64_t b0 = 0; b0 < n_blk; b0 += RG_SCAN_BLOCK) {
            const uint64_t b = b0 + tid;
            unsigned long long* p = cnt + (q * n_blk + b) * 2;
            const uint64_t o = b < n_blk ? p[0] : 0, c = b < n_blk ? p[1] : 0;
            uint64_t io = o, ic = c;                               // inclusive sums along the wave
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint64_t to = __shfl_up(io, d, 64), tc = __shfl_up(ic, d, 64);
                if ((int)lane >= d) { io += to; ic += tc; }
            }
            if (lane == 63) { s_o[wave] = io; s_c[wave] = ic; }
            __syncthreads();
            uint64_t po = 0, pc = 0, to = 0, tc = 0;
            for (uint32_t i = 0; i < RG_SCAN_BLOCK / 64; ++i) {
                if (i < wave) { po += s_o[i]; pc += s_c[i]; }
                to += s_o[i]; tc += s_c[i];
            }
            if (b < n_blk) { p[0] = base_o + po + io - o; p[1] = base_c + pc + ic - c; }
            base_o += to; base_c += tc;
            __syncthreads();
        }
        if (tid == 0) totals[q] = base_o - base;
        base = base_o;                                             // (== base_c: every run that opens closes)
    }
}

// K17.  off = K16's offsets.  A thread takes one word of a range's mask; its run starts and run ends are numbered by a block-wide sum in
// front of the block's offsets.  The record of a position: the last one that starts at or before it (a position with a bit lies in
// a window of a record, and of the records that start where it starts only the last has bases).  Regions from index cap on are not
// written.  rec_base: the index of the call's first record in the caller's numbering.
static __global__ void __launch_bounds__(RG_BLOCK)
k_regions_emit(const uint64_t* __restrict__ masks, uint64_t n_words, uint64_t n_blk, uint32_t n_ranges, const unsigned long long* __restrict__ off,
               const uint64_t* __restrict__ rec_start, const uint64_t* __restrict__ rec_len, uint64_t n_rec, uint64_t rec_base,
               unsigned long long* __restrict__ out, uint64_t cap) {
    __shared__ uint32_t s_w[RG_BLOCK / 64];
    auto record_of = [&](uint64_t pos) {
        const uint64_t lb = hits_lower_bound(rec_start, rec_len, 0, n_rec, pos + 1, false);
        return lb ? lb - 1 : 0;
    };
    for (uint64_t b = blockIdx.x; b < n_blk; b += gridDim.x)
        for (uint32_t q = 0; q < n_ranges; ++q) {
            const uint64_t w = b * RG_BLOCK + threadIdx.x;
            RgEdges e = rg_edges(masks, masks + (q + 1) * n_words, w, n_words);
            uint32_t total;
            const uint32_t before = rg_block_before(rg_pack(e), s_w, total);
            if (!total) continue;                                  // (the same for every thread of the block)
            uint64_t io = off[(q * n_blk + b) * 2] + (before & 0xFFFF), ic = off[(q * n_blk + b) * 2 + 1] + (before >> 16);
            for (; e.open; e.open &= e.open - 1, ++io) {
                if (io >= cap) break;
                const uint64_t pos = w * 64 + (__ffsll((unsigned long long)e.open) - 1), r = record_of(pos);
                out[io * RG_FIELDS + RG_RECORD] = rec_base + r;
                out[io * RG_FIELDS + RG_START] = pos - rec_start[r];
            }
            for (; e.close; e.close &= e.close - 1, ++ic) {
                if (ic >= cap) break;
                const uint64_t pos = w * 64 + (__ffsll((unsigned long long)e.close) - 1);
                out[ic * RG_FIELDS + RG_STOP] = pos + 1 - rec_start[record_of(pos)];
            }
        }
}

}  // namespace kg
