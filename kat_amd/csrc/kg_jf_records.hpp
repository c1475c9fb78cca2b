// kg_jf_records.hpp -- the records of a Jellyfish "binary/sorted" hash file, ordered and packed on the device.
// One body per kernel for both key widths: <W> is a two-word ("wide", 33 <= k <= 63) table, whose key is (hi, lo).
//
// Replaces the order sorted_dumper emits (JF/include/jellyfish/sorted_dumper.hpp:80-112) and the bytes
// binary_writer writes per record (binary_dumper.hpp:47-51): records ascending by ((M * kmer) & (size - 1), kmer) -- a two-word k-mer
// compares as multi-word mer_dna::operator< does, hi first, unsigned -- each ceil(2k/8) key bytes + 4 count bytes, little endian, the
// count saturated.  kg_jf.cpp describes the file around them.
//
//  J1 k_jf_select     slot walk: rebuild the key, position = parity(key & row) per matrix row, keep [pos_lo, pos_hi);
//                     <2> counts the range, <0> histograms it over buckets of 2^shift positions, <1> scatters (pos, [hi,] key, count)
//                     records to their bucket's stretch of the scratch segment
//     k_jf_select_runs  the same three modes over packed records in device memory (sorted runs gathered from several tables)
//  J2 k_jf_scan       exclusive scan of the bucket histogram (one workgroup), the total and the largest bucket
//  J3 k_jf_rank       buckets beyond one LDS tile only: a record's rank among its bucket, by comparison with all of it (global memory)
//  J4 k_jf_sort_pack  one workgroup per bucket: bitonic sort of the bucket on (pos, [hi,] key) in LDS (or, for a ranked bucket, a gather
//                     by rank, tile after tile), then the tile's bytes assembled in LDS and stored as whole dwords
//
// Positions of distinct keys under a random matrix are close to uniform, so the host picks `shift` for a mean of at most
// JF_BUCKET_MEAN records per bucket: a bucket beyond JF_TILE is then some 16 standard deviations out, and only a matrix that
// maps many keys to few positions sends work through J3.  Integer and byte work bound by the table walk; no MFMA.
#pragma once
#include "kg_device.hpp"
#include "kg_jf_load.hpp"

namespace kg {

constexpr int JF_BLOCK = 256;
constexpr uint32_t JF_TILE = 512;            // records sorted and packed per workgroup pass: 10 KB of records + 6 KB of bytes in LDS (wide: 14 + 10)
constexpr uint32_t JF_BUCKET_MEAN = 256;     // the host sizes buckets for at most this many expected records
constexpr uint32_t JF_RANK_MAX = 1u << 16;      // the largest bucket the ranking path takes: 2^32 comparisons, a fraction of a second
template <bool W> constexpr uint32_t JF_MAX_REC_BYTES = W ? 20 : 12;    // k = 32: 8 key bytes + 4 count bytes; k = 63: 16 + 4
constexpr int JF_SCAN_BLOCK = 1024;

// the r rows of M over the 2k key bits (row j, bit i = column 2k-1-i, bit j).  Passed by value: the rows sit in the kernel
// argument segment and a wave reads them with scalar loads.  A wide key's bits 64..125 meet row_hi.
template <bool W> struct JfRows { uint64_t row[63]; };
template <> struct JfRows<true> { uint64_t row[63], row_hi[63]; };

template <bool W>
__device__ __forceinline__ uint64_t jf_pos(const JfRows<W>& m, uint32_t r, uint64_t hi, uint64_t key) {
    uint64_t pos = 0;
    for (uint32_t j = 0; j < r; ++j) {
        uint32_t ones = __popcll(key & m.row[j]);
        if constexpr (W) ones += __popcll(hi & m.row_hi[j]);
        pos |= (uint64_t)(ones & 1) << j;
    }
    return pos;
}

// (one-word keys come with hi = 0 on both sides)
__device__ __forceinline__ bool jf_less(uint64_t pa, uint64_t ha, uint64_t ka, uint64_t pb, uint64_t hb, uint64_t kb) {
    return pa != pb ? pa < pb : ha != hb ? ha < hb : ka < kb;
}

// J1, what either source does with one record at position `pos`.  MODE 2: count it.  MODE 0: ++hist[bucket].  MODE 1: record ->
// scratch[cursor[bucket]++]; count32() is the record's count, saturated to 32 bits, asked for only here.
struct JfSink {
    uint32_t* __restrict__ hist_or_cursor; unsigned long long* __restrict__ total;
    uint64_t* __restrict__ out_pos; uint64_t* __restrict__ out_hi; uint64_t* __restrict__ out_key; uint32_t* __restrict__ out_cnt;
};
template <int MODE, bool W, typename Count32>
__device__ __forceinline__ void jf_put(const JfSink& o, uint64_t pos, uint64_t hi, uint64_t key, uint64_t pos_lo, uint64_t pos_hi, uint32_t shift, uint64_t& mine, Count32&& count32) {
    if (pos < pos_lo || pos >= pos_hi) return;
    if (MODE == 2) { ++mine; return; }
    const uint64_t b = (pos - pos_lo) >> shift;
    const uint32_t at = atomicAdd(&o.hist_or_cursor[b], 1u);
    if (MODE == 1) {
        if constexpr (W) o.out_hi[at] = hi;
        o.out_pos[at] = pos; o.out_key[at] = key;
        o.out_cnt[at] = count32();
    }
}
template <int MODE>
__device__ __forceinline__ void jf_put_total(const JfSink& o, uint64_t mine) {
    if (MODE == 2) {
        for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
        if ((threadIdx.x & 63) == 0 && mine) atomicAdd(o.total, (unsigned long long)mine);
    }
}

// J1 over a table.  A wide table is walked as k_export walks it, and every k-mer of it is in a slot (the all-T 63-mer's first word is
// 2^63 - 1, not EMPTY).
template <int MODE, bool W>
__global__ void __launch_bounds__(JF_BLOCK)
k_jf_select(DevTable t, uint32_t n_ovf, JfRows<W> m, uint32_t r, uint64_t pos_lo, uint64_t pos_hi, uint32_t shift,
            uint32_t* __restrict__ hist_or_cursor, unsigned long long* __restrict__ total,
            uint64_t* __restrict__ out_pos, uint64_t* __restrict__ out_hi, uint64_t* __restrict__ out_key, uint32_t* __restrict__ out_cnt) {
    const JfSink o{hist_or_cursor, total, out_pos, out_hi, out_key, out_cnt};
    uint64_t mine = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t end = W ? t.cap : t.cap + 1;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < end; i += stride) {
        uint64_t key = EMPTY, hi = 0, in_slot = 0;
        if constexpr (W) {
            const uint64_t a = t.keys[i];
            if (a == EMPTY) continue;
            const KeyW kw{a, t.keys_b[i]};
            hi = keyw_hi(kw); key = keyw_lo(kw);
        }
        else if (i < t.cap) { const SlotView v = slot_view(t, i); if (!v.occ) continue; key = v.key; in_slot = v.cnt; }
        else if (!t.ctrs[CTR_ONES]) continue;                                  // the all-ones k-mer lives beside the slots
        jf_put<MODE, W>(o, jf_pos<W>(m, r, hi, key), hi, key, pos_lo, pos_hi, shift, mine, [&]() {
            uint64_t c;
            if constexpr (W) c = slot_count(t, i, n_ovf);
            else c = i < t.cap ? slot_total(t, i, key, in_slot, n_ovf) : t.ctrs[CTR_ONES];
            return c > 0xFFFFFFFFULL ? 0xFFFFFFFFu : (uint32_t)c;              // binary_writer::write saturates
        });
    }
    jf_put_total<MODE>(o, mine);
}

// J1 over packed records: the same three modes for n records of key_bytes + 4 bytes that start at any byte address -- sorted runs of
// several tables laid behind one another (katgpu_jf_dump_gathered).  A workgroup takes JR_TILE consecutive records through LDS as
// k_jf_add does (kg_jf_load.hpp: 16-byte loads of the aligned words around the tile, a record put together from LDS dwords with
// shifts); its count is carried as it stands, a packed count is saturated already.  Bound by those reads and by the scatter.
constexpr uint32_t JR_TILE = 1024;            // records per workgroup pass: 12 KB of LDS (wide: 20 KB)
template <bool W> constexpr uint32_t JR_IMG_WORDS = JR_TILE * JF_MAX_REC_BYTES<W> / 16 + 2;   // + the tile's misalignment and the slack lds_u64 reads into
template <int MODE, bool W>
__global__ void __launch_bounds__(JF_BLOCK)
k_jf_select_runs(const uint8_t* __restrict__ recs, uint64_t n, uint32_t key_len, JfRows<W> m, uint32_t r, uint64_t pos_lo, uint64_t pos_hi, uint32_t shift,
                 uint32_t* __restrict__ hist_or_cursor, unsigned long long* __restrict__ total,
                 uint64_t* __restrict__ out_pos, uint64_t* __restrict__ out_hi, uint64_t* __restrict__ out_key, uint32_t* __restrict__ out_cnt) {
    __shared__ uint4 s_img[JR_IMG_WORDS<W>];
    const JfSink o{hist_or_cursor, total, out_pos, out_hi, out_key, out_cnt};
    const uint32_t* img = reinterpret_cast<const uint32_t*>(s_img);
    const uint32_t tid = threadIdx.x;
    const uint32_t key_bytes = (key_len + 7) / 8, rb = key_bytes + 4;          // (the host sends W = false for key_len <= 64 only: rb <= JF_MAX_REC_BYTES<W>)
    const uint64_t lo_mask = low_bits(key_len), hi_mask = key_len > 64 ? low_bits(key_len - 64) : 0;
    const uintptr_t first = reinterpret_cast<uintptr_t>(recs), last = first + n * rb;
    uint64_t mine = 0;
    const uint64_t n_tiles = (n + JR_TILE - 1) / JR_TILE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t r0 = tile * JR_TILE;
        const uint32_t n_tile = n - r0 < JR_TILE ? (uint32_t)(n - r0) : JR_TILE;
        const uintptr_t from = first + r0 * rb, base = from & ~(uintptr_t)15;
        const uint32_t mis = (uint32_t)(from - base);
        jf_tile_image(s_img, first, last, base, (mis + n_tile * rb + 15) / 16, tid, JF_BLOCK);   // <= JR_IMG_WORDS - 1 words
        __syncthreads();
        for (uint32_t i = tid; i < n_tile; i += JF_BLOCK) {
            const uint32_t at = mis + i * rb;
            const uint64_t key = lds_u64(img, at) & lo_mask;
            uint64_t hi = 0;
            if constexpr (W) hi = lds_u64(img, at + 8) & hi_mask;
            jf_put<MODE, W>(o, jf_pos<W>(m, r, hi, key), hi, key, pos_lo, pos_hi, shift, mine, [&]() { return (uint32_t)lds_u64(img, at + key_bytes); });
        }
        __syncthreads();
    }
    jf_put_total<MODE>(o, mine);
}

// J2.  off[i] = cursor[i] = sum of hist[0..i), off[nb] = the total; res[0] = total (64 bits), res[1] = largest bucket.
static __global__ void __launch_bounds__(JF_SCAN_BLOCK)
k_jf_scan(const uint32_t* __restrict__ hist, uint32_t nb, uint32_t* __restrict__ off, uint32_t* __restrict__ cursor, unsigned long long* __restrict__ res) {
    __shared__ uint32_t s_wave[JF_SCAN_BLOCK / 64];
    __shared__ uint32_t s_max;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_max = 0;
    uint64_t carry = 0;
    uint32_t mx = 0;
    for (uint32_t base = 0; base < nb; base += JF_SCAN_BLOCK) {
        const uint32_t i = base + tid;
        const uint32_t v = i < nb ? hist[i] : 0;
        mx = v > mx ? v : mx;
        uint32_t x = v;
        for (int d = 1; d < 64; d <<= 1) { const uint32_t y = __shfl_up(x, d, 64); if ((int)lane >= d) x += y; }
        if (lane == 63) s_wave[wave] = x;
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < JF_SCAN_BLOCK / 64; ++w) { const uint32_t s = s_wave[w]; all += s; if (w < wave) before += s; }
        if (i < nb) { const uint32_t e = (uint32_t)carry + before + x - v; off[i] = e; cursor[i] = e; }
        carry += all;
        __syncthreads();
    }
    for (int o = 32; o > 0; o >>= 1) { const uint32_t y = __shfl_down(mx, o, 64); mx = y > mx ? y : mx; }
    if (lane == 0) atomicMax(&s_max, mx);
    __syncthreads();
    if (tid == 0) { off[nb] = (uint32_t)carry; res[0] = carry; res[1] = s_max; }
}

// J3.  rank[i] = how many records of i's bucket sort before record i, for the buckets one LDS tile cannot hold.  Quadratic in the
// bucket: the host refuses a range whose largest bucket exceeds JF_RANK_MAX before it launches this.
template <bool W>
__global__ void __launch_bounds__(JF_BLOCK)
k_jf_rank(const uint64_t* __restrict__ pos, const uint64_t* __restrict__ khi, const uint64_t* __restrict__ key, uint32_t n, uint64_t pos_lo, uint32_t shift,
          const uint32_t* __restrict__ off, uint32_t* __restrict__ rank) {
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t p = pos[i], kk = key[i], hh = W ? khi[i] : 0;
        const uint64_t b = (p - pos_lo) >> shift;
        const uint32_t lo = off[b], hi = off[b + 1];
        if (hi - lo <= JF_TILE) continue;
        uint32_t before = 0;
        for (uint32_t j = lo; j < hi; ++j) before += jf_less(pos[j], W ? khi[j] : 0, key[j], p, hh, kk) ? 1u : 0u;
        rank[i] = before;
    }
}

// J4.  Bucket b holds the records [off[b], off[b+1]) of the scratch segment and of the output.  The packed bytes of a tile start at
// any byte address, so the tile is laid out in LDS with the same misalignment as its place in `out`: every dword of the image that
// lies wholly inside the tile goes out as one dword store (a wave's stores are 256 contiguous bytes), and the at most two dwords a
// tile shares with its neighbours go out byte by byte.
// A wide record's key bytes are the 8 of lo, then the low key_bytes - 8 of hi.
template <bool W>
__global__ void __launch_bounds__(JF_BLOCK)
k_jf_sort_pack(const uint64_t* __restrict__ pos, const uint64_t* __restrict__ khi, const uint64_t* __restrict__ key, const uint32_t* __restrict__ cnt,
               const uint32_t* __restrict__ off, const uint32_t* __restrict__ rank, uint32_t nb, uint32_t key_bytes, uint8_t* __restrict__ out) {
    __shared__ uint64_t s_pos[JF_TILE];
    __shared__ uint64_t s_hi[W ? JF_TILE : 1];
    __shared__ uint64_t s_key[JF_TILE];
    __shared__ uint32_t s_cnt[JF_TILE];
    __shared__ uint32_t s_img[JF_TILE * JF_MAX_REC_BYTES<W> / 4 + 2];
    const uint32_t tid = threadIdx.x;
    const uint32_t rb = key_bytes + 4;
    for (uint32_t b = blockIdx.x; b < nb; b += gridDim.x) {
        const uint32_t lo = off[b], m = off[b + 1] - lo;
        for (uint32_t t0 = 0; t0 < m; t0 += JF_TILE) {
            const uint32_t n_tile = m - t0 < JF_TILE ? m - t0 : JF_TILE;
            if (m <= JF_TILE) {
                uint32_t p2 = 1;
                while (p2 < m) p2 <<= 1;
                for (uint32_t i = tid; i < p2; i += JF_BLOCK) {
                    const bool real = i < m;                                  // padding sorts last: a position is below 2^63
                    s_pos[i] = real ? pos[lo + i] : ~0ULL; s_key[i] = real ? key[lo + i] : ~0ULL; s_cnt[i] = real ? cnt[lo + i] : 0;
                    if constexpr (W) s_hi[i] = real ? khi[lo + i] : ~0ULL;
                }
                __syncthreads();
                for (uint32_t k2 = 2; k2 <= p2; k2 <<= 1)
                    for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
                        for (uint32_t t = tid; t < p2 / 2; t += JF_BLOCK) {
                            const uint32_t i = 2 * t - (t & (j - 1)), l = i + j;
                            const bool up = (i & k2) == 0;
                            const uint64_t pa = s_pos[i], ka = s_key[i], pb = s_pos[l], kb = s_key[l];
                            const uint64_t ha = W ? s_hi[i] : 0, hb = W ? s_hi[l] : 0;
                            if (jf_less(pb, hb, kb, pa, ha, ka) == up) {
                                s_pos[i] = pb; s_key[i] = kb; s_pos[l] = pa; s_key[l] = ka;
                                if constexpr (W) { s_hi[i] = hb; s_hi[l] = ha; }
                                const uint32_t ca = s_cnt[i]; s_cnt[i] = s_cnt[l]; s_cnt[l] = ca;
                            }
                        }
                        __syncthreads();
                    }
            } else {
                for (uint32_t i = tid; i < m; i += JF_BLOCK) {
                    const uint32_t at = rank[lo + i] - t0;                   // (wraps below t0: not this tile's)
                    if (at < n_tile) { s_key[at] = key[lo + i]; s_cnt[at] = cnt[lo + i]; if constexpr (W) s_hi[at] = khi[lo + i]; }
                }
                __syncthreads();
            }
            uint8_t* dst = out + (uint64_t)(lo + t0) * rb;
            const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3);
            uint8_t* img = reinterpret_cast<uint8_t*>(s_img);
            for (uint32_t i = tid; i < n_tile; i += JF_BLOCK) {
                uint8_t* p = img + mis + i * rb;
                const uint64_t kk = s_key[i];
                const uint32_t c = s_cnt[i];
                const uint32_t lo_bytes = W ? 8 : key_bytes;
                for (uint32_t x = 0; x < lo_bytes; ++x) p[x] = (uint8_t)(kk >> (8 * x));
                if constexpr (W) { const uint64_t hh = s_hi[i]; for (uint32_t x = 8; x < key_bytes; ++x) p[x] = (uint8_t)(hh >> (8 * (x - 8))); }
                for (uint32_t x = 0; x < 4; ++x) p[key_bytes + x] = (uint8_t)(c >> (8 * x));
            }
            __syncthreads();
            const uint32_t end = mis + n_tile * rb;                           // the image is bytes [mis, end) of s_img
            uint32_t* dst32 = reinterpret_cast<uint32_t*>(dst - mis);
            for (uint32_t d = tid; d < (end + 3) / 4; d += JF_BLOCK) {
                if (4 * d >= mis && 4 * d + 4 <= end) dst32[d] = s_img[d];
                else for (uint32_t x = 4 * d; x < 4 * d + 4; ++x) if (x >= mis && x < end) dst[x - mis] = img[x];
            }
            __syncthreads();
        }
    }
}

}  // namespace kg
