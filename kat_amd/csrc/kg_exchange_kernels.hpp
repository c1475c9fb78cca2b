// kg_exchange_kernels.hpp -- region-ordered extraction and merge: the device side of the multi-GPU exchange (kat_amd/dist.py), written
// for gfx950 (CDNA4, wave64).  What kg_exchange.hip launches beside k_rows_scan (kg_rows_scan.hpp).
//
//  K6 k_extract_count, k_extract_write                                           a table's records by owner, in region order
//  K7 k_merge_apply, k_merge_deferred, k_merge32                                 add (key,count) records into a table: per region in LDS, or directly
//     k_occupied                                                                 occupied slots of a share of a table
// One-word k-mers only (k <= 32: the exchange is not available for wide tables).
//
// Every rank counts into a table of the same region grid, so the records of one region of one rank belong to the same
// region of the owner's table.  Extraction walks the table region by region and writes each owner's records in region
// order; the owner then applies, per region, the runs it received from every rank to that region in LDS -- no
// global atomic per record and no re-partitioning on the receiving side.
// Integer / byte work bound by HBM and by LDS round trips; no MFMA.
#pragma once
#include "kg_device.hpp"

namespace kg {

constexpr int EXTRACT_BLOCK = 256;
constexpr int EXTRACT_UNROLL = 4;            // 16-byte loads a lane of the extraction kernels has in flight (packed tables)
constexpr uint32_t MAX_EXCHANGE_PARTS = 256;
constexpr int MAX_MERGE_SRC = 16;
constexpr int MERGE_BATCH = 8;               // records a thread of k_merge_apply fetches before it applies the first
constexpr int MERGE_BLOCK = 512;             // threads of a k_merge_apply workgroup

// occupied slots of [pos_lo, pos_hi): what a share of the table holds, when the table's load as a whole does not say (merge_regions_impl)
static __global__ void __launch_bounds__(256)
k_occupied(DevTable t, uint64_t pos_lo, uint64_t pos_hi, unsigned long long* out) {
    uint32_t s = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = pos_lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < pos_hi; i += stride) {
        const uint64_t w = t.keys[i];
        s += (t.cbits ? w != 0 : w != EMPTY) ? 1u : 0u;
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(out, (unsigned long long)s);
}

// pass 1: rcnt[p * R + g] = number of records of region g owned by part p.  One workgroup per region.
static __global__ void __launch_bounds__(EXTRACT_BLOCK)
k_extract_count(DevTable t, uint32_t n_parts, uint32_t* __restrict__ rcnt) {
    __shared__ uint32_t s_cnt[MAX_EXCHANGE_PARTS];
    const uint32_t tid = threadIdx.x, S = t.region_slots;
    for (uint32_t g = blockIdx.x; g < t.n_regions; g += gridDim.x) {
        for (uint32_t p = tid; p < n_parts; p += EXTRACT_BLOCK) s_cnt[p] = 0;
        __syncthreads();
        const uint64_t base = (uint64_t)g * S;
        const RegionPlace rp = region_place(t, g);
        if (t.cbits) {
            // packed slots: four 16-byte loads per lane in flight before the first is looked at (the kernel waits for memory 0.63 of its
            // wave cycles with one 8-byte load per lane: profiles/r06_exchange_components.txt) -- regions are multiples of four slots
            const ulonglong2* w2 = reinterpret_cast<const ulonglong2*>(t.keys + base);
            const uint32_t n2 = S >> 1;
            for (uint32_t i0 = 0; i0 < n2; i0 += EXTRACT_BLOCK * EXTRACT_UNROLL) {
                ulonglong2 w[EXTRACT_UNROLL];
#pragma unroll
                for (int u = 0; u < EXTRACT_UNROLL; ++u) { const uint32_t i = i0 + u * EXTRACT_BLOCK + tid; w[u] = i < n2 ? w2[i] : make_ulonglong2(0, 0); }
#pragma unroll
                for (int u = 0; u < EXTRACT_UNROLL; ++u)
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const uint64_t x = h ? w[u].y : w[u].x;
                        if (x) atomicAdd(&s_cnt[n_parts > 1 ? owner_of(key_in(pk_rem(x, t.cbits), rp), t.k, n_parts) : 0], 1u);
                    }
            }
        } else {
            for (uint32_t i = tid; i < S; i += EXTRACT_BLOCK) {
                const SlotView v = slot_view_in(t, rp, base + i);
                if (v.occ) atomicAdd(&s_cnt[n_parts > 1 ? owner_of(v.key, t.k, n_parts) : 0], 1u);
            }
        }
        __syncthreads();
        for (uint32_t p = tid; p < n_parts; p += EXTRACT_BLOCK) rcnt[(uint64_t)p * t.n_regions + g] = s_cnt[p];
        __syncthreads();
    }
}

// pass 2: write the records.  off[p * R + g] = global index of the first record of (part p, region g).  Counts that do
// not fit 32 bits travel in the `big` list (their record carries count 0, which a merge skips).
// PACKED: a record is what a packed slot holds of the k-mer -- the remainder (rb <= 44 bits) -- below its count, 72 bits cut into a u32, a u8
// and a u32: 9 bytes where key + count take 12.  The third word's low rb - 40 bits (none for rb <= 40) are the
// remainder's top ones; the count has the 32 - (rb - 40) >= 28 above them, and what does not fit travels in the `big` list like a count
// beyond 32 bits does.  The region the record lies in says the rest of the k-mer: the form for owners that share the sender's region grid.
__device__ __host__ __forceinline__ uint32_t rec_xs(uint32_t rb) { return rb > 40 ? rb - 40 : 0; }
struct PackedRec { uint64_t rem; uint32_t c; };
__device__ __forceinline__ PackedRec packed_rec(const uint32_t* __restrict__ lo, const uint8_t* __restrict__ hi, const uint32_t* __restrict__ cw, uint64_t i, uint32_t xs) {
    const uint32_t w = cw[i];
    PackedRec r;
    r.c = w >> xs;
    r.rem = r.c ? (((uint64_t)(w & ((1u << xs) - 1)) << 40) | ((uint64_t)hi[i] << 32) | lo[i]) : 0;     // (count 0: a record whose count travels out of band, skipped)
    return r;
}
template <bool PACKED>
static __global__ void __launch_bounds__(EXTRACT_BLOCK)
k_extract_write(DevTable t, uint32_t n_ovf, uint32_t n_parts, const uint64_t* __restrict__ off, uint64_t* __restrict__ out_keys,
                uint32_t* __restrict__ out_rem_lo, uint8_t* __restrict__ out_rem_hi,
                uint32_t* __restrict__ out_counts, uint64_t* __restrict__ big_keys, uint64_t* __restrict__ big_counts,
                unsigned long long* __restrict__ big_n, uint32_t big_cap) {
    __shared__ uint32_t s_cur[MAX_EXCHANGE_PARTS];
    const uint32_t tid = threadIdx.x, S = t.region_slots;
    for (uint32_t g = blockIdx.x; g < t.n_regions; g += gridDim.x) {
        for (uint32_t p = tid; p < n_parts; p += EXTRACT_BLOCK) s_cur[p] = 0;
        __syncthreads();
        const uint64_t base = (uint64_t)g * S;
        const RegionPlace rp = region_place(t, g);
        auto emit = [&](uint64_t pos, uint64_t key, uint64_t in_slot) {
            const uint32_t p = n_parts > 1 ? owner_of(key, t.k, n_parts) : 0;
            const uint64_t at = off[(uint64_t)p * t.n_regions + g] + atomicAdd(&s_cur[p], 1u);
            uint64_t c = slot_total(t, pos, key, in_slot, n_ovf);
            const uint32_t xs = PACKED ? rec_xs(rp.pl.rb) : 0;
            if (c > (0xFFFFFFFFULL >> xs)) {
                const unsigned long long b = atomicAdd(big_n, 1ULL);
                if (b < big_cap) { big_keys[b] = key; big_counts[b] = c; }
                c = 0;
            }
            if constexpr (PACKED) {
                const uint64_t rem = rem_in(key, rp);
                out_rem_lo[at] = (uint32_t)rem; out_rem_hi[at] = (uint8_t)(rem >> 32);
                out_counts[at] = c ? ((uint32_t)c << xs) | (uint32_t)(rem >> 40) : 0u;
            } else { out_keys[at] = key; out_counts[at] = (uint32_t)c; }
        };
        if (t.cbits) {                                             // (packed slots: as k_extract_count, four 16-byte loads per lane in flight)
            const ulonglong2* w2 = reinterpret_cast<const ulonglong2*>(t.keys + base);
            const uint32_t n2 = S >> 1;
            for (uint32_t i0 = 0; i0 < n2; i0 += EXTRACT_BLOCK * EXTRACT_UNROLL) {
                ulonglong2 w[EXTRACT_UNROLL];
#pragma unroll
                for (int u = 0; u < EXTRACT_UNROLL; ++u) { const uint32_t i = i0 + u * EXTRACT_BLOCK + tid; w[u] = i < n2 ? w2[i] : make_ulonglong2(0, 0); }
#pragma unroll
                for (int u = 0; u < EXTRACT_UNROLL; ++u)
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const uint64_t x = h ? w[u].y : w[u].x;
                        if (x) emit(base + 2 * (uint64_t)(i0 + u * EXTRACT_BLOCK + tid) + h, key_in(pk_rem(x, t.cbits), rp), pk_count(x, t.cbits));
                    }
            }
        } else {
            for (uint32_t i = tid; i < S; i += EXTRACT_BLOCK) {
                const SlotView v = slot_view_in(t, rp, base + i);
                if (v.occ) emit(base + i, v.key, v.cnt);
            }
        }
        __syncthreads();
    }
}

struct MergeSrc { const uint64_t* keys; const uint32_t* counts; const uint64_t* off; const uint32_t* rem_lo; const uint8_t* rem_hi; };   // off: u64[regions + 1], relative to the record arrays; keys == null: packed records (rem_lo / rem_hi)
struct MergeSrcs { MergeSrc s[MAX_MERGE_SRC]; uint32_t n; uint32_t src_p1, src_n1, src_l2; };      // src_*: the grid packed records were cut from (the table's, unless it has grown since)
// the k-mer of record i of region g of a source (packed records: from the SENDER's grid)
__device__ __forceinline__ uint64_t merge_src_key(const DevTable& t, const MergeSrcs& srcs, const MergeSrc& s, uint32_t g, uint64_t i, uint32_t& c) {
    if (s.keys) { c = s.counts[i]; return s.keys[i]; }
    const Place pl = place_make(t.k, srcs.src_p1, srcs.src_n1, srcs.src_l2);
    const PackedRec r = packed_rec(s.rem_lo, s.rem_hi, s.counts, i, rec_xs(pl.rb));
    c = r.c;
    return place_key_d(g >> srcs.src_l2, g & ((1u << srcs.src_l2) - 1), r.rem, pl);
}

// Owner side: regions [g_lo, g_hi).  LDS: keys[S] (u64) | counts[S] (u32) (KV12) or the S packed words (PK); the protocol of the
// apply kernels with arbitrary 32-bit amounts.  A region that could overflow (occupied + incoming > S) is not touched: its index
// goes to `deferred` and the host sends its runs through the direct path after making room.
template <int BLOCK, bool PK>
__global__ void __launch_bounds__(BLOCK, 4)     // 512 threads, four waves per SIMD (<= 128 VGPRs: a batch of records in registers): two workgroups per CU, a region of <= 77 KB each
k_merge_apply(DevTable t, uint32_t g_lo, uint32_t g_hi, MergeSrcs srcs, uint32_t* __restrict__ deferred, unsigned long long* __restrict__ n_deferred,
              uint32_t zero_fill /* PK: the regions hold whatever the memory held (katgpu_table::zero_from): each starts from zeros in LDS instead of being loaded,
                                    and EVERY region of [g_lo, g_hi) is written -- one that nothing arrives for, or that is deferred, as zeros */) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    __shared__ uint32_t s_occ;
    unsigned long long* rk = reinterpret_cast<unsigned long long*>(lds_raw);
    uint32_t* rc = reinterpret_cast<uint32_t*>(lds_raw + (size_t)t.region_slots * 8);      // (KV12 only)
    const uint32_t tid = threadIdx.x, S = t.region_slots, cb = t.cbits;
    const uint64_t cmask = PK ? pk_cmask(cb) : 0, half = PK ? pk_half(cb) : 0;
    uint32_t new_distinct = 0;
    for (uint32_t g = g_lo + blockIdx.x; g < g_hi; g += gridDim.x) {
        const uint32_t j = g - g_lo;
        uint64_t incoming = 0;
        for (uint32_t s = 0; s < srcs.n; ++s) incoming += srcs.s[s].off[j + 1] - srcs.s[s].off[j];
        const uint64_t base = (uint64_t)g * S;
        if (incoming == 0 || (zero_fill && incoming > S)) {                      // uniform over the workgroup
            if (zero_fill) {                                                     // (S % 4 == 0: regions are 32-byte aligned)
                ulonglong2* z = reinterpret_cast<ulonglong2*>(t.keys + base);
                for (uint32_t i = tid; i < (S >> 1); i += BLOCK) z[i] = make_ulonglong2(0, 0);
            }
            if (incoming && tid == 0) deferred[atomicAdd(n_deferred, 1ULL)] = g;
            continue;
        }
        if (tid == 0) s_occ = 0;
        __syncthreads();
        const RegionPlace rp = region_place(t, g);
        uint32_t occ = 0;
        if (PK && zero_fill) {
            for (uint32_t i = tid; i < S; i += BLOCK) rk[i] = 0;
        } else {
            for (uint32_t i = tid; i < S; i += BLOCK) {
                const uint64_t key = t.keys[base + i];
                rk[i] = key;
                if constexpr (PK) occ += key != 0; else { rc[i] = t.counts[base + i]; occ += key != EMPTY; }
            }
        }
        for (int d = 32; d > 0; d >>= 1) occ += __shfl_down(occ, d, 64);
        if ((tid & 63) == 0 && occ) atomicAdd(&s_occ, occ);
        __syncthreads();
        if ((uint64_t)s_occ + incoming > S) {                                    // uniform
            if (tid == 0) deferred[atomicAdd(n_deferred, 1ULL)] = g;
            __syncthreads();
            continue;
        }
        for (uint32_t s = 0; s < srcs.n; ++s) {
            const uint64_t beg = srcs.s[s].off[j], end = srcs.s[s].off[j + 1];
            // A thread has a handful of records per region and source, and applying one is a chain of LDS round trips behind three loads: the
            // loads of MERGE_BATCH records are issued before the first is applied (the kernel waited for memory 0.71 of its wave cycles
            // fetching them one at a time).
            // A source's run of a region is in slot order (the extraction walks the region): lanes that took CONSECUTIVE records would all claim
            // slots of one neighbourhood at once and a wave would wait for the longest chain of claims among them, step after step (24 of the
            // kernel's 28 ms).  A thread takes a BLOCK of consecutive records instead: a wave's lanes work a dozen slots apart.
            const uint64_t per_thread = (end - beg + BLOCK - 1) / BLOCK;
            const uint64_t t_beg = beg + (uint64_t)tid * per_thread, t_end = t_beg + per_thread < end ? t_beg + per_thread : end;
            for (uint64_t i0 = t_beg; i0 < t_end; i0 += MERGE_BATCH) {
              uint32_t bc[MERGE_BATCH]; uint64_t brem[MERGE_BATCH];
#pragma unroll
              for (int u = 0; u < MERGE_BATCH; ++u) {
                const uint64_t i = i0 + (uint64_t)u;
                bc[u] = 0; brem[u] = 0;
                if (i < t_end) {
                    if (PK && !srcs.s[s].keys) { const PackedRec r = packed_rec(srcs.s[s].rem_lo, srcs.s[s].rem_hi, srcs.s[s].counts, i, rec_xs(rp.pl.rb)); bc[u] = r.c; brem[u] = r.rem; }   // (packed records: this table's grid is the sender's -- the host checked)
                    else { bc[u] = srcs.s[s].counts[i]; brem[u] = PK ? rem_in(srcs.s[s].keys[i], rp) : srcs.s[s].keys[i]; }
                }
              }
#pragma unroll
              for (int u = 0; u < MERGE_BATCH; ++u) {
                const uint32_t c = bc[u];
                uint64_t rem = brem[u];
                if (!c) continue;
                if constexpr (PK) {
                    uint32_t slot = place_offset(rem, rp.pl, S);
                    uint64_t q, r;
                    pk_split((uint64_t)c, cb, q, r);
                    const uint64_t in = r ? r : half, qq0 = r ? q : q - 1;
                    const unsigned long long claim = (unsigned long long)((rem << cb) | in);
                    for (uint32_t probe = 0; probe < S; ++probe) {               // cannot fail: occupied + incoming <= S
                        // the claim is tried outright: what it returns is what a read would have (one LDS round trip per step, not two)
                        unsigned long long w = atomicCAS(&rk[slot], 0ULL, claim);
                        if (w == 0) { ++new_distinct; if (qq0) ovf_add(t, base + slot, qq0 * half); break; }
                        if ((w >> cb) == rem) {
                            if (r) {
                                for (;;) {
                                    uint64_t cc = (w & cmask) + r, qq = q;
                                    if (cc > half) { cc -= half; ++qq; }                  // (the invariant of packed slots: 1 .. half)
                                    const unsigned long long got = atomicCAS(&rk[slot], w, (unsigned long long)((w & ~cmask) | cc));
                                    if (got == w) { q = qq; break; }
                                    w = got;
                                }
                            }
                            if (q) ovf_add(t, base + slot, q * half);
                            break;
                        }
                        slot = slot + 1 == S ? 0 : slot + 1;
                    }
                } else {
                    const unsigned long long key = rem;                          // (KV12 tables: never packed records; brem holds the key)
                    uint32_t slot = home_offset_in(key, rp);
                    for (uint32_t probe = 0; probe < S; ++probe) {               // cannot fail: occupied + incoming <= S
                        unsigned long long cur = rk[slot];
                        if (cur == EMPTY) {
                            cur = atomicCAS(&rk[slot], (unsigned long long)EMPTY, key);
                            if (cur == EMPTY) { ++new_distinct; cur = key; }
                        }
                        if (cur == key) {
                            const uint32_t old = atomicAdd(&rc[slot], c);
                            if ((uint32_t)(old + c) < old) ovf_add(t, key, 1ULL << 32);
                            break;
                        }
                        slot = slot + 1 == S ? 0 : slot + 1;
                    }
                }
              }
            }
        }
        __syncthreads();
        if constexpr (PK) {                                        // (16-byte stores: S % 4 == 0)
            ulonglong2* o2 = reinterpret_cast<ulonglong2*>(t.keys + base);
            const ulonglong2* r2 = reinterpret_cast<const ulonglong2*>(rk);
            for (uint32_t i = tid; i < (S >> 1); i += BLOCK) o2[i] = r2[i];
        } else
        for (uint32_t i = tid; i < S; i += BLOCK) { t.keys[base + i] = rk[i]; if constexpr (!PK) t.counts[base + i] = rc[i]; }
        __syncthreads();
    }
    flush_distinct(t, new_distinct);
}

// The runs of the regions k_merge_apply deferred, through the direct path: one workgroup per deferred region, every source's
// run of that region.  (One launch for all of them: when a whole table is too small, every region is on the list.)
static __global__ void __launch_bounds__(256)
k_merge_deferred(DevTable t, uint32_t g_lo, MergeSrcs srcs, const uint32_t* __restrict__ deferred, uint32_t n_deferred) {
    uint32_t new_distinct = 0;
    for (uint32_t d = blockIdx.x; d < n_deferred; d += gridDim.x) {
        const uint32_t j = deferred[d] - g_lo;
        for (uint32_t s = 0; s < srcs.n; ++s) {
            const uint64_t beg = srcs.s[s].off[j], end = srcs.s[s].off[j + 1];
            for (uint64_t i = beg + threadIdx.x; i < end; i += blockDim.x) {
                uint32_t c;
                const uint64_t key = merge_src_key(t, srcs, srcs.s[s], deferred[d], i, c);
                if (c) table_add(t, key, (uint64_t)c, new_distinct);
            }
        }
    }
    flush_distinct(t, new_distinct);
}

// records with 32-bit counts through the direct path (sources of another grid, deferred regions)
static __global__ void __launch_bounds__(256)
k_merge32(DevTable dst, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ counts, uint64_t n) {
    uint32_t new_distinct = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (counts[i]) table_add(dst, keys[i], (uint64_t)counts[i], new_distinct);
    flush_distinct(dst, new_distinct);
}

}  // namespace kg
