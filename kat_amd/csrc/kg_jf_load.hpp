// kg_jf_load.hpp -- the records of a Jellyfish "binary/sorted" hash file, unpacked and added to a table on the device.
//
// Replaces binary_reader (JF/include/jellyfish/binary_dumper.hpp:114-119: key_.template read<1>(is), then counter_len bytes of
// count) and the loop HashLoader::loadHash runs over it, hash->add(reader.key(), reader.val()) per record
// (lib/src/jellyfish_helper.cc:172-174).  kg_jf.cpp describes the file around the records.
//
//  L1 k_jf_add<W>  a workgroup takes JL_TILE consecutive records: the aligned 16-byte words that cover the tile's bytes go to LDS
//                  with one 16-byte load per lane (a wave reads 1 KB in a row), each lane then puts its records' key and count
//                  together from LDS dwords with shifts and adds them with table_add (W = false: k <= 32, both slot layouts;
//                  W = true: two key words).  The semantics are k_merge's: exact 64-bit sums, a zero count skipped, equal keys
//                  summed, amounts beyond the slot's field to the side table.
//
// A record is R = ceil(key_len / 8) + counter_len bytes (2 .. 24, 11 at k = 27), both fields little endian, back to back; the
// records start at any byte address.  Bits of the key above key_len are masked off: Jellyfish writes zeros there, and a key
// with more than 2k bits would probe outside the region its placement belongs to.
//
// Memory: the caller's n * R bytes of records and 24 KB of LDS per workgroup; nothing is allocated.  The kernel reads every record
// byte once from HBM; its time is the table's random slot traffic, as k_merge's is.  Integer and byte work; no MFMA.
#pragma once
#include "kg_device.hpp"

namespace kg {

constexpr int JL_BLOCK = 256;
constexpr uint32_t JL_TILE = 1024;            // records per workgroup pass: at most 24 KB of LDS
constexpr uint32_t JL_MAX_REC_BYTES = 24;     // k = 63: 16 key bytes + 8 count bytes
constexpr uint32_t JL_IMG_WORDS = JL_TILE * JL_MAX_REC_BYTES / 16 + 2;   // + the tile's misalignment (< 16 bytes) and the slack lds_u64 reads into

// the 8 bytes at byte offset `at` of the LDS image, little endian: three dwords and a funnel shift (bytes past the field are the caller's to mask)
__device__ __forceinline__ uint64_t lds_u64(const uint32_t* img, uint32_t at) {
    const uint32_t d = at >> 2, sh = (at & 3) * 8;
    const uint64_t lo = ((uint64_t)img[d + 1] << 32) | img[d];
    return sh ? (lo >> sh) | ((uint64_t)img[d + 2] << (64 - sh)) : lo;
}

__device__ __forceinline__ uint64_t low_bits(uint32_t n) { return n >= 64 ? ~0ULL : (1ULL << n) - 1; }     // n = 0: none

// The n_words aligned 16-byte words from `base` on, which cover a tile of the packed records in [first, last), to LDS: one 16-byte load
// per lane (a wave reads 1 KB in a row).  Words inside the buffer, the ones a tile shares with its neighbours included, are loaded
// whole; the at most two words that hang over the buffer's ends are put together from the bytes that belong to it.
__device__ __forceinline__ void jf_tile_image(uint4* s_img, uintptr_t first, uintptr_t last, uintptr_t base, uint32_t n_words, uint32_t tid, uint32_t block) {
    for (uint32_t w = tid; w < n_words; w += block) {
        const uintptr_t a = base + (uintptr_t)w * 16;
        uint4 v;
        if (a >= first && a + 16 <= last) v = *reinterpret_cast<const uint4*>(a);
        else {
            uint32_t d[4] = {0, 0, 0, 0};
            for (uint32_t x = 0; x < 16; ++x)
                if (a + x >= first && a + x < last) d[x >> 2] |= (uint32_t)*reinterpret_cast<const uint8_t*>(a + x) << (8 * (x & 3));
            v = make_uint4(d[0], d[1], d[2], d[3]);
        }
        s_img[w] = v;
    }
}

// L1.  recs .. recs + n * (key_bytes + counter_len) is device memory; nothing outside it is read.
template <bool W>
__global__ void __launch_bounds__(JL_BLOCK)
k_jf_add(DevTable dst, const uint8_t* __restrict__ recs, uint64_t n, uint32_t key_len, uint32_t counter_len) {
    __shared__ uint4 s_img[JL_IMG_WORDS];
    const uint32_t* img = reinterpret_cast<const uint32_t*>(s_img);
    const uint32_t tid = threadIdx.x;
    const uint32_t key_bytes = (key_len + 7) / 8, rb = key_bytes + counter_len;
    const uint64_t lo_mask = low_bits(key_len), hi_mask = key_len > 64 ? low_bits(key_len - 64) : 0, cnt_mask = low_bits(8 * counter_len);
    const uintptr_t first = reinterpret_cast<uintptr_t>(recs), last = first + n * rb;        // the buffer is [first, last)
    uint32_t new_distinct = 0;
    const uint64_t n_tiles = (n + JL_TILE - 1) / JL_TILE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t r0 = tile * JL_TILE;
        const uint32_t n_tile = n - r0 < JL_TILE ? (uint32_t)(n - r0) : JL_TILE;
        const uintptr_t from = first + r0 * rb, base = from & ~(uintptr_t)15;
        const uint32_t mis = (uint32_t)(from - base);
        const uint32_t n_words = (mis + n_tile * rb + 15) / 16;                               // <= JL_IMG_WORDS - 1
        jf_tile_image(s_img, first, last, base, n_words, tid, JL_BLOCK);
        __syncthreads();
        for (uint32_t i = tid; i < n_tile; i += JL_BLOCK) {
            const uint32_t at = mis + i * rb;
            const uint64_t cnt = lds_u64(img, at + key_bytes) & cnt_mask;
            if (!cnt) continue;
            const uint64_t lo = lds_u64(img, at) & lo_mask;
            Key<W> key;
            if constexpr (W) key = keyw_from_words(lds_u64(img, at + 8) & hi_mask, lo);     // (bits above 2k masked off, as lo's are)
            else key = lo;
            table_add(dst, key, cnt, new_distinct);
        }
        __syncthreads();
    }
    flush_distinct(dst, new_distinct);
}

}  // namespace kg
