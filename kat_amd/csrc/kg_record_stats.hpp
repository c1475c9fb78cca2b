// kg_record_stats.hpp -- per-record coverage statistics on the device, written for gfx950 (CDNA4, wave64): what Sect::processSeq
// (src/sect.cc:490-589) and Cold::processSeq (src/cold.cc:303-406) compute from a record's per-position counts -- their sum, the
// non-zero and the invalid windows, the G/C and N bases, and sorted(counts)[nb / 2] -- without the counts leaving the device.
//
//  K11 k_rstats_short   records of at most RS_SHORT_WINDOWS windows: counts looked up (or read from a dense array: CountsTable / CountsDense) into LDS, reduced and radix-selected there
//  K12 k_rstats_long    the other records: counts to a device scratch array that holds the long records' windows and no others,
//                       sums by k_seq_hits' pattern
//  K13 k_rstats_hist / k_rstats_pick   exact multi-pass radix select over that array, 8 bits a pass, per record
//
// Both lookup kernels use the front end of kg_windows.hpp (load16 / encode16 / Chunk<W>::Tile / Window), so one body serves both
// key widths.  Records are given by start and length, increasing and disjoint (the convention of k_seq_hits); a window belongs to a
// record when it lies wholly inside it; an invalid window (a byte outside ACGTacgt) counts 0 in the median, as in the reference's
// sorted copy, and enters neither the sum nor the non-zero count.
#pragma once
#include "kg_filter.hpp"

namespace kg {

// one record of the result: katgpu_record_stats (include/katgpu.h) as six 64-bit words
constexpr int RS_SUM = 0, RS_MEDIAN = 1, RS_NON_ZERO = 2, RS_INVALID = 3, RS_GC = 4, RS_N = 5, RS_FIELDS = 6;

// K11 stages RS_TILE_BYTES consecutive bytes and owns the records that START in the first RS_TILE_STRIDE of them; a short record is
// at most RS_SHORT_MAX_LEN bases long, so it ends inside the tile.  With k <= 63, a record of RS_SHORT_WINDOWS windows has at most
// 960 + 62 bases.  Tile starts stay 16-byte aligned.  LDS: 32 KiB of counts + 6 KiB of codes and masks = 38 KiB, four blocks a CU.
constexpr int RS_TILE_BYTES = COUNT_BLOCK * BASES_PER_LANE;          // 4096
constexpr int RS_SHORT_MAX_LEN = 1024;
constexpr int RS_TILE_STRIDE = RS_TILE_BYTES - RS_SHORT_MAX_LEN;     // 3072
constexpr uint32_t RS_SHORT_WINDOWS = 960;                           // the short / long limit, in windows
static_assert(RS_SHORT_WINDOWS + 62 <= RS_SHORT_MAX_LEN && RS_TILE_STRIDE % 16 == 0, "a short record must end inside its tile");
constexpr uint32_t RS_NO_SLOT = 0xFFFFFFFFu;                         // rec_slot[] of a record that is not long
constexpr int RS_LDS_RECS = 32;                                      // K12: records of a chunk with LDS bins (long records: a chunk meets a handful)
constexpr int RS_SEL_CHUNK = 4096;                                   // K13: positions of the scratch array per block iteration
constexpr int RS_DIGITS = 256;                                       // K13: 8 bits a pass

// the selection state of one long record (K13)
struct RsSel { unsigned long long orv, prefix, rank, rec, off; };     // OR of its counts | digits fixed so far | rank among those that match them | its index | its first count in cnt[]

__device__ __forceinline__ uint64_t rs_windows(uint64_t len, uint32_t k) { return len >= k ? len - k + 1 : 0; }
__device__ __forceinline__ uint64_t rs_uniform(uint64_t v) {          // a value every lane holds, in scalar registers
    return ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)v);
}
__device__ __forceinline__ uint64_t rs_wave_sum(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ uint32_t rs_wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ uint64_t rs_wave_or(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off, 64);
    return v;
}
// bits [lo, hi) of a 16-bit mask word whose bit j stands for position 16 * word + j, for the range [a, b) of positions
__device__ __forceinline__ uint32_t rs_range_mask(uint32_t word, uint32_t a, uint32_t b) {
    const uint32_t w0 = word * BASES_PER_LANE;
    const uint32_t lo = a > w0 ? a - w0 : 0, hi = b < w0 + BASES_PER_LANE ? b - w0 : BASES_PER_LANE;
    return ((1u << hi) - 1) & ~((1u << lo) - 1);
}
// Where a window's count comes from, a compile-time choice of K11, K12 and K14 (kg_record_regions.hpp); the rest of their bodies is one.
// get(lw, p): the count of the valid window lw, which starts at base p of the buffer -- asked for the windows of records only.
//  CountsTable  looked up in a table of this rank (katgpu_table_record_*)
//  CountsDense  counts[p], a dense array of n_counts = n - k + 1 words made elsewhere (katgpu_record_*_from_counts_device: the gathered
//               profile of a table that lies on several ranks); 8-byte aligned, no more
struct CountsTable {
    DevTable t; uint32_t n_ovf; int canonicalise;
    __device__ __forceinline__ uint32_t k() const { return t.k; }
    template <typename Win> __device__ __forceinline__ uint64_t get(const Win& lw, uint64_t) const {
        auto key = lw.fwd();
        if (canonicalise) key = kmer_canonical(key, t.k);
        return table_get(t, key, n_ovf);
    }
};
struct CountsDense {
    const uint64_t* __restrict__ counts; uint64_t n_counts; uint32_t k_;
    __device__ __forceinline__ uint32_t k() const { return k_; }
    template <typename Win> __device__ __forceinline__ uint64_t get(const Win&, uint64_t p) const { return p < n_counts ? counts[p] : 0; }
};

// a lane's 16 bytes: which are G g C c, which are N n (bit j = byte j)
__device__ __forceinline__ void rs_base_masks(const uint32_t (&w)[4], uint32_t& gc, uint32_t& nn) {
    gc = 0; nn = 0;
#pragma unroll
    for (int j = 0; j < BASES_PER_LANE; ++j) {
        const uint32_t c = ((w[j >> 2] >> (8 * (j & 3))) & 0xFF) | 0x20;
        gc |= (uint32_t)(c == 'g' || c == 'c') << j;
        nn |= (uint32_t)(c == 'n') << j;
    }
}

// K11.  A block stages a tile (one 16-byte load per lane, codes and flags to LDS, the G/C and N masks of the bytes beside them), marks
// the windows of the short records it owns, looks those up into LDS -- lane t its 16 window starts, as in k_profile, 0 for an invalid
// window -- and then gives every owned record to one wave: sum / non-zero / invalid / base classes by wave reductions over the LDS
// counts and masks, the nb/2-th smallest by a bit-wise radix select from the highest bit set in any count of the record down (genomic
// counts: a dozen rounds of one LDS read per 64 windows and a ballot).  A wave loads the records 64 at a time and walks those a ballot
// names, so runs of empty records cost one load.  `out` was cleared by the caller: an empty record is never written.
template <bool ALIGNED, bool W, typename Src>
__global__ void __launch_bounds__(COUNT_BLOCK)
k_rstats_short(Src src, const uint8_t* __restrict__ bases, uint64_t n, uint64_t n_tiles,
               const uint64_t* __restrict__ rec_start, const uint64_t* __restrict__ rec_len, uint64_t n_rec, uint32_t limit,
               unsigned long long* __restrict__ out) {
    __shared__ typename Chunk<W>::Tile s;
    __shared__ uint64_t s_cnt[RS_TILE_BYTES];
    __shared__ uint32_t s_own[COUNT_BLOCK], s_inv[COUNT_BLOCK], s_gc[COUNT_BLOCK], s_nn[COUNT_BLOCK];
    __shared__ uint64_t s_r[2];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t k = src.k();
    s.pad();

    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t c0 = tile * RS_TILE_STRIDE;
        if (tid == 0) {                                            // the records that start in [c0, c0 + RS_TILE_STRIDE)
            const uint64_t lo = hits_lower_bound(rec_start, rec_len, 0, n_rec, c0, false);
            s_r[0] = lo;
            s_r[1] = hits_lower_bound(rec_start, rec_len, lo, n_rec, c0 + RS_TILE_STRIDE, false);
        }
        __syncthreads();
        const uint64_t r_lo = s_r[0], r_hi = s_r[1];
        if (r_lo == r_hi) { __syncthreads(); continue; }

        // f(record, its first base in the tile, its length) for every owned short record that has bases, one wave per record
        auto for_owned = [&](auto f) {
            for (uint64_t g = r_lo + wave * 64; g < r_hi; g += COUNT_BLOCK) {
                const uint64_t r = g + lane;
                uint64_t rs = 0, len = 0;
                if (r < r_hi) { rs = rec_start[r]; len = rec_len[r]; }
                uint64_t todo = __ballot(len != 0 && rs_windows(len, k) <= limit && rs >= c0 && rs - c0 < RS_TILE_STRIDE);
                while (todo) {
                    const int src = __ffsll((unsigned long long)todo) - 1;
                    todo &= todo - 1;
                    f(g + src, (uint32_t)(rs_uniform(__shfl(rs, src, 64)) - c0), (uint32_t)rs_uniform(__shfl(len, src, 64)));
                }
            }
        };

        const uint64_t off = c0 + (uint64_t)tid * BASES_PER_LANE;
        uint32_t w[4];
        load16<ALIGNED>(bases, n, off, w);
        uint32_t code, bad, gcm, nnm;
        encode16(w, code, bad);
        rs_base_masks(w, gcm, nnm);
        s.stage(code, bad);
        s_gc[tid] = gcm; s_nn[tid] = nnm; s_own[tid] = 0;
        __syncthreads();

        for_owned([&](uint64_t, uint32_t a, uint32_t len) {
            const uint32_t nb = (uint32_t)rs_windows(len, k);
            if (nb) for (uint32_t wd = (a >> 4) + lane; wd <= ((a + nb - 1) >> 4); wd += 64) atomicOr(&s_own[wd], rs_range_mask(wd, a, a + nb));
        });
        __syncthreads();

        {
            const uint32_t own = s_own[tid];
            uint32_t inv = 0;
            if (own) {
                typename Chunk<W>::Window lw;
                lw.init(s.code, s.bad, tid, k);
                for (int j = 0; j < BASES_PER_LANE; ++j, lw.step()) {
                    if (!((own >> j) & 1)) continue;
                    uint64_t c = 0;
                    if (lw.valid()) c = src.get(lw, off + j);
                    else inv |= 1u << j;
                    s_cnt[tid * BASES_PER_LANE + j] = c;
                }
            }
            s_inv[tid] = inv;
        }
        __syncthreads();

        for_owned([&](uint64_t r, uint32_t a, uint32_t len) {
            const uint32_t nb = (uint32_t)rs_windows(len, k);
            uint64_t sum = 0, orv = 0;
            uint32_t nz = 0, ninv = 0, gc = 0, nn = 0;
            for (uint32_t i = lane; i < nb; i += 64) {
                const uint32_t p = a + i;
                const uint64_t v = s_cnt[p];
                sum += v; orv |= v; nz += v != 0;
                ninv += (s_inv[p >> 4] >> (p & 15)) & 1;
            }
            for (uint32_t wd = (a >> 4) + lane; wd <= ((a + len - 1) >> 4); wd += 64) {
                const uint32_t m = rs_range_mask(wd, a, a + len);
                gc += __popc(s_gc[wd] & m); nn += __popc(s_nn[wd] & m);
            }
            sum = rs_wave_sum(sum); nz = rs_wave_sum(nz); ninv = rs_wave_sum(ninv); gc = rs_wave_sum(gc); nn = rs_wave_sum(nn);
            orv = rs_uniform(rs_wave_or(orv));
            // the element of rank nb / 2: fix the bits from the top; `rank` counts within the elements that match the bits fixed so far
            uint64_t prefix = 0;
            uint32_t rank = nb / 2;
            if (orv) for (int b = 63 - __clzll((long long)orv); b >= 0; --b) {
                uint32_t zeros = 0;                                // of those elements, the ones whose bit b is 0
                for (uint32_t i0 = 0; i0 < nb; i0 += 64) {
                    const uint32_t i = i0 + lane;
                    zeros += __popcll(__ballot(i < nb && ((s_cnt[a + (i < nb ? i : 0)] ^ prefix) >> b) == 0));
                }
                if (rank >= zeros) { rank -= zeros; prefix |= 1ULL << b; }
            }
            if (lane == 0) {
                unsigned long long* o = out + r * RS_FIELDS;
                o[RS_SUM] = sum; o[RS_MEDIAN] = prefix; o[RS_NON_ZERO] = nz; o[RS_INVALID] = ninv; o[RS_GC] = gc; o[RS_N] = nn;
            }
        });
        __syncthreads();
    }
}

// how many records are long, and how many windows they have (the device form of the entry point: the host form counts them itself)
static __global__ void __launch_bounds__(256)
k_rstats_count_long(const uint64_t* __restrict__ rec_len, uint64_t n_rec, uint32_t k, uint32_t limit, unsigned long long* __restrict__ n_long) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rec) return;
    const uint64_t nb = rs_windows(rec_len[r], k);
    if (nb > limit) { atomicAdd(&n_long[0], 1ULL); atomicAdd(&n_long[1], (unsigned long long)nb); }
}

// A slot of selection state for every long record and a stretch of cnt[] for its windows, both in record order: slot s + 1 follows
// slot s, its counts follow s's counts, so K13 finds the records of a stretch of cnt[] by a binary search on RsSel::off.  One block
// runs a prefix sum over the records, 1024 at a time (the records of a batch: at most 2^20).  rec_slot[] was set to RS_NO_SLOT.
constexpr int RS_CLASSIFY_BLOCK = 1024;
static __global__ void __launch_bounds__(RS_CLASSIFY_BLOCK)
k_rstats_classify(const uint64_t* __restrict__ rec_len, uint64_t n_rec, uint32_t k, uint32_t limit, uint64_t n_slots, uint64_t n_cnt,
                  uint32_t* __restrict__ rec_slot, RsSel* __restrict__ sel) {
    __shared__ uint32_t s_c[RS_CLASSIFY_BLOCK / 64];
    __shared__ uint64_t s_w[RS_CLASSIFY_BLOCK / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t slot0 = 0, off0 = 0;                                  // long records / their windows before this round's records
    for (uint64_t r0 = 0; r0 < n_rec; r0 += RS_CLASSIFY_BLOCK) {
        const uint64_t r = r0 + tid;
        const uint64_t nb = r < n_rec ? rs_windows(rec_len[r], k) : 0;
        const bool is_long = nb > limit;
        uint32_t ic = is_long;                                     // inclusive sums along the wave
        uint64_t iw = is_long ? nb : 0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t tc = __shfl_up(ic, d, 64);
            const uint64_t tw = __shfl_up(iw, d, 64);
            if ((int)lane >= d) { ic += tc; iw += tw; }
        }
        if (lane == 63) { s_c[wave] = ic; s_w[wave] = iw; }
        __syncthreads();
        uint64_t pc = 0, pw = 0, tc = 0, tw = 0;
        for (uint32_t i = 0; i < RS_CLASSIFY_BLOCK / 64; ++i) {
            if (i < wave) { pc += s_c[i]; pw += s_w[i]; }
            tc += s_c[i]; tw += s_w[i];
        }
        if (is_long) {
            const uint64_t slot = slot0 + pc + ic - 1, off = off0 + pw + iw - nb;
            if (slot < n_slots && off + nb <= n_cnt) {             // (the record lengths changed under the call: write nothing out of bounds)
                rec_slot[r] = (uint32_t)slot;
                sel[slot] = RsSel{0, 0, nb / 2, r, off};
            }
        }
        slot0 += tc; off0 += tw;
        __syncthreads();
    }
}

// K12.  k_seq_hits over the long records: a lane runs along its 16 bytes and window starts (chunks are cut by bytes here: a chunk owns
// Chunk<W>::STARTS bytes and the windows that start on them), knows the record they lie in, writes every window's count to the record's stretch of cnt[] (0
// for an invalid one; the radix select reads them there) and keeps its run of sum / non-zero / invalid / G+C / N / OR-of-counts for that
// record, which goes to LDS bins when the record changes and from there to HBM once per chunk, one atomic per record and field.
template <bool ALIGNED, bool W, typename Src>
__global__ void __launch_bounds__(COUNT_BLOCK)
k_rstats_long(Src src, const uint8_t* __restrict__ bases, uint64_t n, uint64_t n_chunks,
              const uint64_t* __restrict__ rec_start, const uint64_t* __restrict__ rec_len, uint64_t n_rec,
              const uint32_t* __restrict__ rec_slot, uint64_t* __restrict__ cnt, uint64_t n_cnt, RsSel* __restrict__ sel,
              unsigned long long* __restrict__ out) {
    constexpr int CS = Chunk<W>::STARTS;
    __shared__ typename Chunk<W>::Tile s;
    __shared__ unsigned long long s_sum[RS_LDS_RECS], s_or[RS_LDS_RECS];
    __shared__ uint32_t s_u[4][RS_LDS_RECS];                       // non-zero, invalid, G+C, N
    __shared__ uint64_t s_r[2];
    const uint32_t tid = threadIdx.x;
    const uint32_t k = src.k();
    s.pad();
    if (tid < RS_LDS_RECS) { s_sum[tid] = 0; s_or[tid] = 0; s_u[0][tid] = 0; s_u[1][tid] = 0; s_u[2][tid] = 0; s_u[3][tid] = 0; }

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
        uint32_t code, bad, gcm, nnm;
        encode16(w, code, bad);
        rs_base_masks(w, gcm, nnm);
        s.stage(code, bad);
        __syncthreads();
        const uint64_t r_lo = s_r[0], r_hi = s_r[1];

        if (tid < Chunk<W>::LANES && off < n && r_lo < r_hi) {
            // the record of the first byte: the last one of [r_lo, r_hi) that starts at or before it (none: r = r_lo - 1)
            int64_t r = (int64_t)hits_lower_bound(rec_start, rec_len, r_lo, r_hi, off + 1, false) - 1;
            uint64_t rs = 0, re = 0;
            bool is_long = false;
            uint64_t coff = 0;                                     // where the record's counts start in cnt[]
            auto enter = [&]() { const uint32_t sl = rec_slot[r]; is_long = sl != RS_NO_SLOT; if (is_long) coff = sel[sl].off; };
            if (r >= (int64_t)r_lo) { rs = rec_start[r]; re = rs + rec_len[r]; enter(); }
            uint64_t ns = (uint64_t)(r + 1) < r_hi ? rec_start[r + 1] : ~0ULL;
            int64_t cur = -1;
            uint64_t sum = 0, orv = 0;
            uint32_t nz = 0, ninv = 0, gc = 0, nn = 0;
            auto flush = [&]() {
                if (cur < 0) return;
                const uint64_t idx = (uint64_t)cur - r_lo;
                if (idx < RS_LDS_RECS) {
                    if (sum) atomicAdd(&s_sum[idx], (unsigned long long)sum);
                    if (orv) atomicOr(&s_or[idx], (unsigned long long)orv);
                    if (nz) atomicAdd(&s_u[0][idx], nz);
                    if (ninv) atomicAdd(&s_u[1][idx], ninv);
                    if (gc) atomicAdd(&s_u[2][idx], gc);
                    if (nn) atomicAdd(&s_u[3][idx], nn);
                } else {
                    unsigned long long* o = out + (uint64_t)cur * RS_FIELDS;
                    if (sum) atomicAdd(&o[RS_SUM], (unsigned long long)sum);
                    if (orv) atomicOr(&sel[rec_slot[cur]].orv, (unsigned long long)orv);
                    if (nz) atomicAdd(&o[RS_NON_ZERO], (unsigned long long)nz);
                    if (ninv) atomicAdd(&o[RS_INVALID], (unsigned long long)ninv);
                    if (gc) atomicAdd(&o[RS_GC], (unsigned long long)gc);
                    if (nn) atomicAdd(&o[RS_N], (unsigned long long)nn);
                }
            };
            typename Chunk<W>::Window lw;
            lw.init(s.code, s.bad, tid, k);
            for (int j = 0; j < BASES_PER_LANE; ++j, lw.step()) {
                const uint64_t pos = off + j;
                while (pos >= ns) {
                    ++r; rs = ns; re = rs + rec_len[r]; enter();
                    ns = (uint64_t)(r + 1) < r_hi ? rec_start[r + 1] : ~0ULL;
                }
                if (!is_long || pos < rs || pos >= re) continue;   // (r >= r_lo here: is_long is false before the first record)
                if (r != cur) { flush(); cur = r; sum = 0; orv = 0; nz = 0; ninv = 0; gc = 0; nn = 0; }
                gc += (gcm >> j) & 1; nn += (nnm >> j) & 1;
                if (pos + k <= re && pos + k <= n) {
                    uint64_t c = 0;
                    if (lw.valid()) {
                        c = src.get(lw, pos);
                        sum += c; orv |= c; nz += c != 0;
                    } else ++ninv;
                    const uint64_t ci = coff + (pos - rs);
                    if (ci < n_cnt) cnt[ci] = c;
                }
            }
            flush();
        }
        __syncthreads();
        const uint64_t nbin = r_hi - r_lo < (uint64_t)RS_LDS_RECS ? r_hi - r_lo : (uint64_t)RS_LDS_RECS;
        if (tid < nbin) {
            const uint64_t r = r_lo + tid;
            unsigned long long* o = out + r * RS_FIELDS;
            if (s_sum[tid]) { atomicAdd(&o[RS_SUM], s_sum[tid]); s_sum[tid] = 0; }
            if (s_or[tid]) { atomicOr(&sel[rec_slot[r]].orv, s_or[tid]); s_or[tid] = 0; }
            if (s_u[0][tid]) { atomicAdd(&o[RS_NON_ZERO], (unsigned long long)s_u[0][tid]); s_u[0][tid] = 0; }
            if (s_u[1][tid]) { atomicAdd(&o[RS_INVALID], (unsigned long long)s_u[1][tid]); s_u[1][tid] = 0; }
            if (s_u[2][tid]) { atomicAdd(&o[RS_GC], (unsigned long long)s_u[2][tid]); s_u[2][tid] = 0; }
            if (s_u[3][tid]) { atomicAdd(&o[RS_N], (unsigned long long)s_u[3][tid]); s_u[3][tid] = 0; }
        }
        __syncthreads();
    }
}

// K13, one pass of the select for the digit at `shift` (56, 48, ... 0).  A record whose counts have no bit at or above `shift` keeps
// its prefix and rank and its counts are not read in that pass: genomic counts take the last two.  k_rstats_hist: a block walks
// RS_SEL_CHUNK positions of cnt[] -- the long records' windows only -- finds the records they belong to by RsSel::off, and for each
// histograms the digit of the counts that match the record's prefix above it -- in LDS, flushed once per record and block.  A wave
// whose counts all carry one digit (the upper digits of most records) adds once.  k_rstats_pick: a wave per long record, four bins a
// lane, scans the 256 bins to the one that holds the rank, fixes the digit, clears the bins, and after the last pass writes the median.
static __global__ void __launch_bounds__(256)
k_rstats_hist(const uint64_t* __restrict__ cnt, uint64_t n_cnt, uint64_t n_chunks, uint32_t k, const uint64_t* __restrict__ rec_len,
              const RsSel* __restrict__ sel, uint64_t n_long, uint32_t shift, unsigned long long* __restrict__ hist) {
    __shared__ uint32_t s_h[RS_DIGITS];
    __shared__ uint64_t s_r[2];
    const uint32_t tid = threadIdx.x;
    s_h[tid] = 0;
    auto last_at_or_before = [&](uint64_t lo, uint64_t x) {        // the last slot of [lo, n_long) whose counts start at or before x
        uint64_t hi = n_long;
        while (hi - lo > 1) { const uint64_t mid = lo + (hi - lo) / 2; if (sel[mid].off <= x) lo = mid; else hi = mid; }
        return lo;
    };
    for (uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const uint64_t c0 = chunk * RS_SEL_CHUNK;
        const uint64_t c1 = c0 + RS_SEL_CHUNK < n_cnt ? c0 + RS_SEL_CHUNK : n_cnt;
        if (tid == 0) { s_r[0] = last_at_or_before(0, c0); s_r[1] = last_at_or_before(s_r[0], c1 - 1) + 1; }
        __syncthreads();
        const uint64_t s_lo = s_r[0], s_hi = s_r[1];
        for (uint64_t slot = s_lo; slot < s_hi; ++slot) {          // (every thread takes the same turns: the barriers below are met by all)
            const uint64_t orv = sel[slot].orv;
            if ((orv >> shift) == 0) continue;
            const uint64_t prefix = sel[slot].prefix;
            const uint64_t ws = sel[slot].off, we = ws + rs_windows(rec_len[sel[slot].rec], k);
            const uint64_t a = ws > c0 ? ws : c0, b = we < c1 ? we : c1;
            if (a >= b) continue;
            for (uint64_t p0 = a; p0 < b; p0 += 256) {
                const uint64_t p = p0 + tid;
                bool in = false;
                uint32_t d = 0;
                if (p < b) { const uint64_t v = cnt[p]; in = (((v ^ prefix) >> shift) >> 8) == 0; d = (uint32_t)(v >> shift) & (RS_DIGITS - 1); }
                const uint64_t m = __ballot(in);
                if (!m) continue;
                const int first = __ffsll((unsigned long long)m) - 1;
                const uint32_t d0 = __shfl(d, first, 64);
                if (__all(!in || d == d0)) { if ((int)(tid & 63) == first) atomicAdd(&s_h[d0], (uint32_t)__popcll(m)); }
                else if (in) atomicAdd(&s_h[d], 1u);
            }
            __syncthreads();
            const uint32_t h = s_h[tid];
            if (h) { atomicAdd(&hist[slot * RS_DIGITS + tid], (unsigned long long)h); s_h[tid] = 0; }
            __syncthreads();
        }
        __syncthreads();
    }
}

static __global__ void __launch_bounds__(256)
k_rstats_pick(RsSel* __restrict__ sel, uint64_t n_long, uint32_t shift, unsigned long long* __restrict__ hist, unsigned long long* __restrict__ out) {
    const uint64_t slot = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    if (slot >= n_long) return;
    const RsSel v = sel[slot];
    if ((v.orv >> shift) == 0) return;                             // (orv == 0: the median stays the 0 the caller cleared it to)
    ulonglong2* h = reinterpret_cast<ulonglong2*>(hist + slot * RS_DIGITS + lane * 4);
    const ulonglong2 lo = h[0], hi = h[1];
    h[0] = make_ulonglong2(0, 0); h[1] = make_ulonglong2(0, 0);
    const unsigned long long mine = lo.x + lo.y + hi.x + hi.y;
    unsigned long long upto = mine;                                // counts in this lane's bins and the lanes' before it
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const unsigned long long o = __shfl_up(upto, d, 64); if ((int)lane >= d) upto += o; }
    if (v.rank >= upto - mine && v.rank < upto) {                  // the one lane whose four bins hold the rank
        unsigned long long rank = v.rank - (upto - mine), digit = lane * 4;
        if (rank >= lo.x) { rank -= lo.x; ++digit; if (rank >= lo.y) { rank -= lo.y; ++digit; if (rank >= hi.x) { rank -= hi.x; ++digit; } } }
        const unsigned long long prefix = v.prefix | (digit << shift);
        sel[slot].prefix = prefix; sel[slot].rank = rank;
        if (shift == 0) out[v.rec * RS_FIELDS + RS_MEDIAN] = prefix;
    }
}

}  // namespace kg
