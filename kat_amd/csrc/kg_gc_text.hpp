// kg_gc_text.hpp -- the text of `kat sect -g`'s -counts.gc on the device, written for gfx950 (CDNA4, wave64): what Sect::printGCCounts
// (src/sect.cc:348-370) makes of a record's windows, without its ">name" line -- "%.1f" of the G+C percentage of every window, "-0.1"
// for a window that holds a byte outside ACGTacgt (validKmer / gcCount, lib/include/kat/str_utils.hpp:151-201), a space between them, a
// newline behind the last; "0.0\n" for a record without a window.
//
//  K20 k_gc_tiles<0>     the bytes every tile of CT_TILE positions adds to the text: string + 1 of each window that lies in a record
//  K19 k_cvg_scan        (kg_cvg_text.hpp) those sums to offsets; beside them the bytes of the window-less records ("0.0\n": 4 each)
//  K20 k_gc_tiles<1>     the tiles again: the widths summed along the block, then every lane writes its windows' strings and separators
//
// The text needs no table and no lookup, and a window has only k + 2 possible strings: the k + 1 percentages, formatted on the host by
// snprintf and handed over as a table of characters and a length (GcStrings), and "-0.1".  The kernel copies characters and never
// formats a number.  A window's string follows from its G+C tally and its validity alone, and both are bits: per tile the bytes
// [c0, c0 + CT_TILE + k - 1) become two masks in LDS, 16 positions to a halfword -- "is G g C c" and "is not one of ACGTacgt", bytes
// at or beyond n being no base -- from the unit's loader and classifier (load16 / encode16, kg_windows.hpp); a lane takes the 80 bits
// of each that its CT_LANE positions and their k - 1 followers need, and window j is a shift, a mask of k bits, a popcount and a test.
// So, unlike the .cvg text, nothing per position is written to device memory between the sizing pass and the writing pass: each pass
// reads the bases again, 2 bytes per position between them, against the 4.5-5 bytes per position of text that are written.
// The walk along the records, the sums along the block, the offsets and the tile geometry are those of kg_cvg_text.hpp: its text_tiles
// is the whole frame of K20, and what is written here is the window's string (GcWindows).
#pragma once
#include "kg_cvg_text.hpp"

namespace kg {

constexpr int GC_MAX_STRINGS = 65;                                   // g = 0 .. k for k <= 63, and "-0.1"
constexpr int GC_HALO = 4;                                           // halfwords of 16 positions behind a tile: k - 1 <= 62 followers
static_assert(CT_LANE == BASES_PER_LANE && CT_LANE == 16, "a lane's positions are one 16-byte load and one halfword of each mask");

// e[g]: the string of a valid window with g of G/C, e[k + 1]: "-0.1".  Characters in bytes 0 .. 4, the length in byte 7.
struct GcStrings { uint64_t e[GC_MAX_STRINGS]; };

// 16 bytes to 16 "is G g C c" bits, the first byte in bit 0.  Among ACGTacgt bit 1 of the byte tells C and G from A and T; the bit of
// any other byte means nothing and is never looked at: that byte is flagged in the other mask, and its windows are "-0.1".
__device__ __forceinline__ uint32_t gc_bits16(const uint32_t w[4]) {
    uint32_t m = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t x = (w[q] >> 1) & 0x01010101u;               // A, C, T, G -> 0, 1, 0, 1 (encode16's x, its low bit)
        m |= ((x * 0x01020408u) >> 24) << (4 * q);                   // the four flags side by side (distinct partial products: no carries)
    }
    return m;
}

// the windows of the .gc text (text_tiles' Src, kg_cvg_text.hpp): one of k + 2 strings, told from the two masks of the tile in LDS
template <bool ALIGNED>
struct GcWindows {
    static constexpr char EMPTY[] = "0.0\n";
    const uint8_t* __restrict__ bases;
    uint64_t n;
    uint32_t k;
    uint64_t k_mask;                                                 // k ones
    const uint64_t* s_str;                                          // GC_MAX_STRINGS entries
    uint16_t *s_gc, *s_bad;                                          // CT_BLOCK + GC_HALO halfwords each
    uint64_t off, gc_lo, bad_lo, gc_hi, bad_hi;                      // lane(): its first position and its 80 bits of each mask

    __device__ __forceinline__ void stage16(uint32_t h, uint64_t at) const {     // 16 bytes from `at` to halfword h of both masks
        uint32_t w[4], code, bad;
        load16<ALIGNED>(bases, n, at, w);                            // (past n: 'N')
        encode16(w, code, bad);
        s_gc[h] = (uint16_t)gc_bits16(w);
        s_bad[h] = (uint16_t)(__brev(bad) >> 16);                    // encode16 has the first byte on top
    }
    __device__ __forceinline__ void stage(uint64_t c0, uint32_t tid) const {
        for (uint32_t h = tid; h < CT_BLOCK + GC_HALO; h += CT_BLOCK) stage16(h, c0 + (uint64_t)h * CT_LANE);   // (the first GC_HALO lanes: the halo too)
    }
    // positions off .. off + 15 and the k - 1 <= 62 behind them: 78 bits of 80
    __device__ __forceinline__ void lane(uint64_t off_) {
        const uint32_t tid = threadIdx.x;
        off = off_;
        gc_lo = (uint64_t)s_gc[tid] | (uint64_t)s_gc[tid + 1] << 16 | (uint64_t)s_gc[tid + 2] << 32 | (uint64_t)s_gc[tid + 3] << 48;
        bad_lo = (uint64_t)s_bad[tid] | (uint64_t)s_bad[tid + 1] << 16 | (uint64_t)s_bad[tid + 2] << 32 | (uint64_t)s_bad[tid + 3] << 48;
        gc_hi = s_gc[tid + 4]; bad_hi = s_bad[tid + 4];
    }
    __device__ __forceinline__ uint64_t string_of(uint64_t pos) const {          // the table entry of the window that starts at pos
        const uint32_t j = (uint32_t)(pos - off);
        const uint64_t b = ((bad_lo >> j) | (j ? bad_hi << (64 - j) : 0)) & k_mask;
        const uint64_t g = ((gc_lo >> j) | (j ? gc_hi << (64 - j) : 0)) & k_mask;
        return s_str[b ? k + 1 : (uint32_t)__popcll(g)];
    }
    __device__ __forceinline__ uint32_t width(uint64_t pos) const { return (uint32_t)(string_of(pos) >> 56); }
    template <typename Put>
    __device__ __forceinline__ uint32_t emit(uint64_t pos, uint64_t o, Put&& put) const {
        const uint64_t s = string_of(pos);
        const uint32_t d = (uint32_t)(s >> 56);
        put(o, (char)s); put(o + 1, (char)(s >> 8)); put(o + 2, (char)(s >> 16));
        if (d > 3) put(o + 3, (char)(s >> 24));
        if (d > 4) put(o + 4, (char)(s >> 32));
        return d;
    }
};

// K20
template <bool WRITE, bool ALIGNED>
__global__ void __launch_bounds__(CT_BLOCK)
k_gc_tiles(const uint8_t* __restrict__ bases, uint64_t n, uint32_t k, const GcStrings strs, const uint64_t* __restrict__ rec_start,
           const uint64_t* __restrict__ rec_len, uint64_t n_rec, uint64_t n_tiles, unsigned long long* __restrict__ tile_sum,
           const uint64_t* __restrict__ extra, const unsigned long long* __restrict__ totals, uint64_t text_base, uint8_t* __restrict__ text,
           uint64_t cap, uint64_t* __restrict__ text_off) {
    __shared__ uint32_t s_w[CT_BLOCK / 64];
    __shared__ uint64_t s_r[2];
    __shared__ uint64_t s_str[GC_MAX_STRINGS];
    __shared__ uint16_t s_gc[CT_BLOCK + GC_HALO], s_bad[CT_BLOCK + GC_HALO];
    if (threadIdx.x < k + 2) s_str[threadIdx.x] = strs.e[threadIdx.x];   // (k + 2 <= GC_MAX_STRINGS; the tile loop's first barrier is behind it)
    GcWindows<ALIGNED> src{bases, n, k, (1ULL << k) - 1, s_str, s_gc, s_bad};
    text_tiles<WRITE>(src, s_w, s_r, n, k, rec_start, rec_len, n_rec, n_tiles, tile_sum, extra, totals, text_base, text, cap, text_off);
}

}  // namespace kg
