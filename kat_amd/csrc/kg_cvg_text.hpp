// kg_cvg_text.hpp -- the text of `kat sect`'s -counts.cvg on the device, written for gfx950 (CDNA4, wave64): what Sect::printCounts
// (src/sect.cc:328-346) makes of a record's per-position counts, without its ">name" line -- the counts in decimal, a space between
// them, a newline behind the last; "0\n" for a record without a window -- so that 2-3 bytes per position come back where k_profile's
// counts are 8.
//
//      k_profile         (K8, as it stands) the count of every window of the batch into device memory
//  K18 k_cvg_tiles<0>    the bytes every tile of CT_TILE positions adds to the text: digits + 1 of each window that lies in a record
//  K19 k_cvg_scan        those sums to offsets; beside them the bytes of the records that have no window ("0\n": 2 each) to offsets
//  K18 k_cvg_tiles<1>    the tiles again: the widths summed along the block, then every lane writes its windows' digits and separators
//
// Records are given by start and length, increasing and disjoint (the convention of k_seq_hits); a window belongs to a record when it
// lies wholly inside it.  The byte a window's text starts at is the sum of two offsets, because a record without a window has no
// position that could carry its two bytes: P(pos), the widths of the windows that start before pos, and E(r), the bytes of the
// window-less records before record r.  Window-less records are written by the lane that owns the position they start at, on its way
// along the records (cvg_walk) -- so the positions run from 0 to n inclusive: a record may start where the bases end.
#pragma once
#include "kg_record_regions.hpp"

namespace kg {

constexpr int CT_BLOCK = RG_BLOCK;                                   // (rg_block_before sums along a block of this size)
constexpr int CT_LANE = 16;                                          // consecutive positions of a lane: one 128-byte line of counts
constexpr int CT_TILE = CT_BLOCK * CT_LANE;
constexpr int CT_SCAN_BLOCK = 1024, CT_SCAN_ITEMS = 8;               // K19: one block per array, CT_SCAN_ITEMS consecutive entries a thread and round

// decimal digits of a count: compared against the powers of ten, 32 bits wide below 2^32 (nearly every count)
__device__ __forceinline__ uint32_t cvg_digits(uint64_t c) {
    constexpr uint32_t P32[9] = {10u, 100u, 1000u, 10000u, 100000u, 1000000u, 10000000u, 100000000u, 1000000000u};
    constexpr uint64_t P64[10] = {10000000000ULL, 100000000000ULL, 1000000000000ULL, 10000000000000ULL, 100000000000000ULL, 1000000000000000ULL,
                                  10000000000000000ULL, 100000000000000000ULL, 1000000000000000000ULL, 10000000000000000000ULL};
    uint32_t d;
    if (c >> 32 == 0) {
        const uint32_t v = (uint32_t)c;
        d = 1;
#pragma unroll
        for (int i = 0; i < 9; ++i) d += v >= P32[i];
    } else {                                                         // >= 2^32: ten digits at least
        d = 10;
#pragma unroll
        for (int i = 0; i < 10; ++i) d += c >= P64[i];
    }
    return d;
}

// A lane's way along positions [off, off + CT_LANE) and the records that start there.  [r_lo, r_hi): where the first record that
// starts at or after `off` may be found.  on_record(r, len) for every record that starts at one of the lane's positions, in order
// and before the windows of that position; on_window(r, pos, last) for every position that starts a window of a record, `last`
// when it is the record's last one.  The record a position lies in is the last one that starts at or before it (of the records that
// start at one position only the last can have bases).
template <typename OnRecord, typename OnWindow>
__device__ __forceinline__ void cvg_walk(const uint64_t* __restrict__ rec_start, const uint64_t* __restrict__ rec_len, uint64_t n_rec, uint64_t r_lo,
                                         uint64_t r_hi, uint64_t off, uint64_t n, uint32_t k, OnRecord&& on_record, OnWindow&& on_window) {
    uint64_t nr = hits_lower_bound(rec_start, rec_len, r_lo, r_hi, off, false);
    uint64_t cur = nr - 1, re = 0;                                   // (re == 0: no record yet -- nothing is inside it)
    if (nr) re = rec_start[cur] + rec_len[cur];
    uint64_t ns = nr < n_rec ? rec_start[nr] : ~0ULL;
    for (int j = 0; j < CT_LANE; ++j) {
        const uint64_t pos = off + j;
        if (pos > n) break;
        while (pos >= ns) {
            cur = nr++;
            const uint64_t len = rec_len[cur];
            re = ns + len;
            ns = nr < n_rec ? rec_start[nr] : ~0ULL;
            on_record(cur, len);
        }
        if (pos + k <= re && pos + k <= n) on_window(cur, pos, pos + k == re);
    }
}

// The frame of the text kernels (K18, and K20 of kg_gc_text.hpp).  A tile is CT_TILE positions, a lane's share CT_LANE consecutive ones;
// n_tiles covers positions 0 .. n.  s_w, s_r: CT_BLOCK / 64 and 2 words of the kernel's LDS.
// WRITE == false: tile_sum[tile] = bytes of the windows that start in the tile.
// WRITE == true:  tile_sum holds K19's offsets.  Byte o of the text goes to text[o] when o < cap; text_off[r] = text_base + the byte
//                 record r's text starts at, text_off[n_rec] = text_base + the total.
// Src says what a window's string is: stage(c0, tid) before the tile's first barrier and lane(off) behind it make ready what the lane's
// windows are read from; width(pos) is the length of the string of the window at pos; emit(pos, o, put) writes it from byte o on and
// returns that length (the frame puts the separator behind it); Src::EMPTY is the text of a record without a window.
template <typename Src> constexpr uint32_t text_empty_bytes() { return sizeof(Src::EMPTY) - 1; }     // K19's empty_bytes

template <bool WRITE, typename Src>
__device__ __forceinline__ void text_tiles(Src& src, uint32_t* s_w, uint64_t* s_r, uint64_t n, uint32_t k, const uint64_t* __restrict__ rec_start,
                                           const uint64_t* __restrict__ rec_len, uint64_t n_rec, uint64_t n_tiles, unsigned long long* __restrict__ tile_sum,
                                           const uint64_t* __restrict__ extra, const unsigned long long* __restrict__ totals, uint64_t text_base,
                                           uint8_t* __restrict__ text, uint64_t cap, uint64_t* __restrict__ text_off) {
    const uint32_t tid = threadIdx.x;
    if (WRITE && blockIdx.x == 0 && tid == 0) text_off[n_rec] = text_base + totals[0] + totals[1];

    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t c0 = tile * CT_TILE;
        if (tid == 0) {                                            // the records that start in the tile
            const uint64_t lo = hits_lower_bound(rec_start, rec_len, 0, n_rec, c0, false);
            s_r[0] = lo;
            s_r[1] = hits_lower_bound(rec_start, rec_len, lo, n_rec, c0 + CT_TILE, false);
        }
        const uint64_t off = c0 + (uint64_t)tid * CT_LANE;
        src.stage(c0, tid);
        __syncthreads();
        const uint64_t r_lo = s_r[0], r_hi = s_r[1];
        src.lane(off);

        uint32_t sum = 0;
        cvg_walk(rec_start, rec_len, n_rec, r_lo, r_hi, off, n, k, [](uint64_t, uint64_t) {},
                 [&](uint64_t, uint64_t pos, bool) { sum += src.width(pos) + 1; });
        uint32_t total;
        const uint32_t before = rg_block_before(sum, s_w, total);    // (its barriers also keep s_r and what Src staged for the slowest thread)
        if constexpr (!WRITE) {
            if (tid == 0) tile_sum[tile] = total;
        } else {
            uint64_t at = tile_sum[tile] + before;                   // P(pos) along the lane
            auto put = [&](uint64_t o, char ch) { if (o < cap) text[o] = (uint8_t)ch; };
            cvg_walk(rec_start, rec_len, n_rec, r_lo, r_hi, off, n, k,
                     [&](uint64_t r, uint64_t len) {
                         const uint64_t o = at + extra[r];
                         text_off[r] = text_base + o;
                         if (len < k) {
#pragma unroll
                             for (uint32_t i = 0; i < text_empty_bytes<Src>(); ++i) put(o + i, Src::EMPTY[i]);
                         }
                     },
                     [&](uint64_t r, uint64_t pos, bool last) {
                         const uint64_t o = at + extra[r];
                         const uint32_t d = src.emit(pos, o, put);
                         put(o + d, last ? '\n' : ' ');
                         at += d + 1;
                     });
        }
    }
}

// the windows of the .cvg text: a count in decimal, read from k_profile's array
struct CvgWindows {
    static constexpr char EMPTY[] = "0\n";
    const uint64_t* __restrict__ counts;
    __device__ __forceinline__ void stage(uint64_t, uint32_t) const {}
    __device__ __forceinline__ void lane(uint64_t) const {}
    __device__ __forceinline__ uint32_t width(uint64_t pos) const { return cvg_digits(counts[pos]); }
    template <typename Put>
    __device__ __forceinline__ uint32_t emit(uint64_t pos, uint64_t o, Put&& put) const {
        const uint64_t c = counts[pos];
        const uint32_t d = cvg_digits(c);
        uint64_t p = o + d;                                          // the separator's place; the digits from the last one down
        if (c >> 32 == 0) {
            uint32_t v = (uint32_t)c;
            do { put(--p, (char)('0' + v % 10)); v /= 10; } while (v);
        } else {
            uint64_t v = c;
            do { put(--p, (char)('0' + v % 10)); v /= 10; } while (v);
        }
        return d;
    }
};

// K18
template <bool WRITE>
__global__ void __launch_bounds__(CT_BLOCK)
k_cvg_tiles(const uint64_t* __restrict__ counts, uint64_t n, uint32_t k, const uint64_t* __restrict__ rec_start, const uint64_t* __restrict__ rec_len,
            uint64_t n_rec, uint64_t n_tiles, unsigned long long* __restrict__ tile_sum, const uint64_t* __restrict__ extra,
            const unsigned long long* __restrict__ totals, uint64_t text_base, uint8_t* __restrict__ text, uint64_t cap, uint64_t* __restrict__ text_off) {
    __shared__ uint32_t s_w[CT_BLOCK / 64];
    __shared__ uint64_t s_r[2];
    CvgWindows src{counts};
    text_tiles<WRITE>(src, s_w, s_r, n, k, rec_start, rec_len, n_rec, n_tiles, tile_sum, extra, totals, text_base, text, cap, text_off);
}

// K19.  Block 0: the tile sums become, in place, the offset of each tile's first byte among the windows' bytes.  Block 1: extra[r] =
// empty_bytes x the records before r that have no window (2 for the "0\n" of the .cvg text, 4 for the "0.0\n" of kg_gc_text.hpp's).
// totals[b] = the sum of block b's array.
static __global__ void __launch_bounds__(CT_SCAN_BLOCK)
k_cvg_scan(unsigned long long* __restrict__ tile_sum, uint64_t n_tiles, const uint64_t* __restrict__ rec_len, uint64_t n_rec, uint32_t k,
           uint32_t empty_bytes, uint64_t* __restrict__ extra, unsigned long long* __restrict__ totals) {
    __shared__ uint64_t s_w[CT_SCAN_BLOCK / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool recs = blockIdx.x == 1;
    const uint64_t cnt = recs ? n_rec : n_tiles;
    uint64_t base = 0;
    for (uint64_t i0 = 0; i0 < cnt; i0 += (uint64_t)CT_SCAN_BLOCK * CT_SCAN_ITEMS) {
        const uint64_t i = i0 + (uint64_t)tid * CT_SCAN_ITEMS;
        uint64_t v[CT_SCAN_ITEMS], sum = 0;
#pragma unroll
        for (int j = 0; j < CT_SCAN_ITEMS; ++j) {
            v[j] = i + j >= cnt ? 0 : recs ? (rec_len[i + j] < k ? empty_bytes : 0) : tile_sum[i + j];
            sum += v[j];
        }
        uint64_t inc = sum;                                        // inclusive sums along the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint64_t o = __shfl_up(inc, d, 64); if ((int)lane >= d) inc += o; }
        if (lane == 63) s_w[wave] = inc;
        __syncthreads();
        uint64_t run = base + inc - sum, total = 0;
        for (uint32_t w = 0; w < CT_SCAN_BLOCK / 64; ++w) { const uint64_t x = s_w[w]; if (w < wave) run += x; total += x; }
#pragma unroll
        for (int j = 0; j < CT_SCAN_ITEMS; ++j) {
            if (i + j < cnt) { if (recs) extra[i + j] = run; else tile_sum[i + j] = run; }
            run += v[j];
        }
        base += total;
        __syncthreads();
    }
    if (tid == 0) totals[blockIdx.x] = base;
}

}  // namespace kg
