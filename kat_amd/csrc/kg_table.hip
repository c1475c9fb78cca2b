// kg_table.hip -- the HBM-resident count table behind katgpu_table and its life cycle: geometry and layout choice, allocation, regrow
// (hash_counter::double_size), the counters and statistics, and the room made for records that are added in bulk (add_in_rooms).
#include "kg_host.hpp"

static const uint32_t g_region_slots = (uint32_t)hook_u64("KATGPU_TEST_REGION_SLOTS", REGION_SLOTS);
static const bool g_no_packed = hook("KATGPU_NO_PACKED") != nullptr;   // tests / A-B: every table in the KV12 layout

// like_p1/like_p2 != 0: adopt that region grid (so that comp can join region against region) and take up the capacity in the
// region size, if a region of the resulting size still fits LDS.
static const bool g_no_lazy_zero = hook("KATGPU_NO_LAZY_ZERO") != nullptr;   // A/B: every table cleared when it is made
static const uint64_t g_lazy_min_slots = hook_u64("KATGPU_TEST_LAZY_MIN_SLOTS", 1ULL << 26);   // tests: packed tables from this size on leave their clearing to the first sweep
int alloc_dev_table(katgpu_ctx* c, uint32_t k, int canonical, uint64_t cap, DevTable* out, uint32_t like_p1, uint32_t like_p2, bool* lazy_zero) {
    DevTable d{};
    const uint64_t like_r = (uint64_t)like_p1 * like_p2;
    // slots per region: a wide slot is 20 bytes (two key words + the count), and the wide apply kernel holds a region in LDS like the
    // narrow ones do (kg_partition_wide.hpp): 6144 slots = 120 KB
    const uint32_t rs = k > 32 ? std::min<uint32_t>(g_region_slots, REGION_SLOTS_WIDE) : g_region_slots;
    // capacity is a whole number of regions (kg_device.hpp: Probe); a table smaller than one region is a single short region
    // (regions of fewer than 256 slots are not worth a common grid: the spread of the region loads would eat the table's fill limit)
    if (like_r > 1 && (cap + like_r - 1) / like_r <= AP2_MAX_SLOTS - 4 && (cap + like_r - 1) / like_r >= 256) {
        d.p1 = like_p1; d.p2 = like_p2; d.n_regions = (uint32_t)like_r;
        d.region_slots = (uint32_t)((std::max<uint64_t>((cap + like_r - 1) / like_r, 16) + 3) & ~3ULL);   // whole 16-byte lines of keys and counts per region
    } else if (cap <= rs) { d.n_regions = d.p1 = d.p2 = 1; d.region_slots = (uint32_t)((cap + 3) & ~3ULL); }
    else {
        const uint64_t nr = (cap + rs - 1) / rs;
        if (nr > 0x3FFFFFFFULL) return fail(c, KATGPU_ERR_NOMEM, "table of %llu slots exceeds the region index", (unsigned long long)cap);
        uint32_t p2 = 1;
        while ((uint64_t)p2 * p2 < nr) ++p2;                   // two radix digits of about the same size
        if (k <= 32) { uint32_t q = 1; while (q < p2) q <<= 1; p2 = q; }   // one-word tables: the level-2 digit is a bit field of the placement hash
        d.p2 = p2; d.p1 = (uint32_t)((nr + p2 - 1) / p2);
        d.region_slots = rs;
        // Level 2 of the partitioned counter works one bucket per workgroup and CU at a time: 584 buckets on 256 CUs are three
        // passes of which the last keeps 72 CUs busy.  With more buckets than CUs, make them a whole number of passes -- fewer,
        // larger regions if the apply kernel's LDS holds them (AP2_MAX_SLOTS), else more, smaller ones.
        const uint32_t ncu = (uint32_t)c->n_cu;
        if (k <= 32 && g_region_slots == REGION_SLOTS && ncu && d.p1 > ncu && d.p1 % ncu) {
            auto slots_for = [&](uint32_t p1) { return (uint32_t)(((cap + (uint64_t)p1 * p2 - 1) / ((uint64_t)p1 * p2) + 3) & ~3ULL); };
            const uint32_t lo = d.p1 / ncu * ncu, hi = lo + ncu;
            if (slots_for(lo) <= AP2_MAX_SLOTS) { d.p1 = lo; d.region_slots = slots_for(lo); }
            else if (hi <= MAX_PARTS) { d.p1 = hi; d.region_slots = slots_for(hi); }
        }
        d.n_regions = d.p1 * d.p2;
    }
    cap = (uint64_t)d.n_regions * d.region_slots;
    d.cap = cap; d.k = k; d.canonical = canonical ? 1 : 0;
    if (k <= 32) {                                             // the placement hash's bit budget (kg_device.hpp "placement")
        if (d.p2 & (d.p2 - 1)) return fail(c, KATGPU_ERR_INVALID_ARG, "a one-word table needs a power-of-two level-2 digit (got p2 = %u)", d.p2);
        while ((1u << d.l2) < d.p2) ++d.l2;
        d.n1 = place_n1(k, d.p1);
        // Packed slots (kg_device.hpp "P8") whenever the placement hash leaves the slot word at least PACK_MIN_CBITS count bits: the
        // remainder has n1 - l2 bits, so this is every table of >= 2^(2k - 44) regions -- 8 M slots at k = 27, 2 G at k = 31.
        const Place pl = place_make(k, d.p1, d.n1, d.l2);
        if (!g_no_packed && d.n_regions > 1 && pl.rb + PACK_MIN_CBITS <= 64) d.cbits = std::min<uint32_t>(64 - pl.rb, 32);
        d.inv_slots = 1.0 / (double)d.region_slots;
    }
    const double t0 = now_ms();
    const bool wide = k > 32;                                  // two key words per slot (kg_device.hpp "wide keys"), one block
    const size_t key_bytes = cap * sizeof(uint64_t) * (wide ? 2 : 1);
    HIPCHK(c, pool_alloc(c, (void**)&d.keys, key_bytes, /* take_reservation: a table made "like" another -- kat comp's later inputs */ like_p1 != 0 || like_p2 != 0));
    if (wide) d.keys_b = d.keys + cap;
    if (g_trace) fprintf(stderr, "[katgpu] alloc %s %.1f GB: %.1f ms\n", d.cbits ? "packed slots" : "keys", cap * 8 / 1e9, now_ms() - t0);
    hipError_t e = d.cbits ? hipSuccess : pool_alloc(c, (void**)&d.counts, cap * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&d.ovf_keys, OVF_CAP * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMalloc(&d.ovf_hi, OVF_CAP * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMalloc(&d.ctrs, CTR_WORDS * sizeof(uint64_t));
    if (e != hipSuccess) {
        pool_release(c, d.keys); pool_release(c, d.counts); hipFree(d.ovf_keys); hipFree(d.ovf_hi); hipFree(d.ctrs);
        return fail(c, KATGPU_ERR_NOMEM, "device allocation of a %llu-slot table failed: %s", (unsigned long long)cap, hipGetErrorString(e));
    }
    // a packed table the partitioned counter will take (>= 64 M slots): cleared by its first round's apply, region by region (katgpu_table::zero_from)
    const bool lazy = lazy_zero && !g_no_lazy_zero && d.cbits && !wide && cap >= g_lazy_min_slots;
    if (lazy_zero) *lazy_zero = lazy;
    if (!lazy) HIPCHK(c, hipMemsetAsync(d.keys, d.cbits ? 0 : 0xFF, key_bytes, c->stream));
    if (d.counts) HIPCHK(c, hipMemsetAsync(d.counts, 0, cap * sizeof(uint32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(d.ovf_keys, 0xFF, OVF_CAP * sizeof(uint64_t), c->stream));
    HIPCHK(c, hipMemsetAsync(d.ovf_hi, 0, OVF_CAP * sizeof(uint64_t), c->stream));
    HIPCHK(c, hipMemsetAsync(d.ctrs, 0, CTR_WORDS * sizeof(uint64_t), c->stream));
    if (g_trace) { const double t1 = now_ms(); hipStreamSynchronize(c->stream); fprintf(stderr, "[katgpu +%.0f ms] table alloc: mallocs+enqueue %.1f ms, memsets done after %.1f ms more\n", since_load(), t1 - t0, now_ms() - t1); }
    *out = d;
    return KATGPU_OK;
}

void free_dev_table(katgpu_ctx* c, DevTable& d) {
    pool_release(c, d.keys); pool_release(c, d.counts);
    hipFree(d.ovf_keys); hipFree(d.ovf_hi); hipFree(d.ctrs);
    d = DevTable{};
}

// like != nullptr: on its region grid.  (No common grid across key widths; none for wide tables either: nothing joins or merges them region by
// region, and a grid handed down could make regions the wide apply kernel cannot hold.)
static int create_table(katgpu_ctx* c, const katgpu_table* like, uint32_t k, int canonical, uint64_t size_hint, int disable_grow, katgpu_table** out) {
    *out = nullptr;
    if (k < 1 || k > KATGPU_MAX_K) return fail(c, KATGPU_ERR_K, "k = %u unsupported: this build keeps a k-mer in at most two 63-bit words (1 <= k <= %d)", k, KATGPU_MAX_K);
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t cap = std::max<uint64_t>(size_hint ? size_hint : (1u << 20), 1024);
    katgpu_table* t = new katgpu_table();
    t->ctx = c; t->disable_grow = disable_grow;
    bool lazy = false;
    const bool grid = like && k <= 32 && like->dv.k <= 32;
    int rc = alloc_dev_table(c, k, canonical, cap, &t->dv, grid ? like->dv.p1 : 0, grid ? like->dv.p2 : 0, &lazy);
    if (rc) { delete t; return rc; }
    if (lazy) t->zero_from = 0;
    *out = t;
    return KATGPU_OK;
}

extern "C" int katgpu_table_create(katgpu_ctx* c, uint32_t k, int canonical, uint64_t size_hint, int disable_grow, katgpu_table** out) {
    return c && out ? create_table(c, nullptr, k, canonical, size_hint, disable_grow, out) : KATGPU_ERR_INVALID_ARG;
}
extern "C" int katgpu_table_create_like(katgpu_ctx* c, const katgpu_table* like, uint32_t k, int canonical, uint64_t size_hint,
                                        int disable_grow, katgpu_table** out) {
    return c && out && like ? create_table(c, like, k, canonical, size_hint, disable_grow, out) : KATGPU_ERR_INVALID_ARG;
}

int table_wait(katgpu_table* t) {
    std::lock_guard<std::mutex> lk(t->alloc_mu);
    if (t->alloc_thread.joinable()) t->alloc_thread.join();
    if (t->alloc_rc) return fail(t->ctx, t->alloc_rc, "%s", t->alloc_err.c_str());
    return KATGPU_OK;
}

extern "C" void katgpu_table_free(katgpu_table* t) {
    if (!t) return;
    (void)table_wait(t);
    hipSetDevice(t->ctx->device);
    hipStreamSynchronize(t->ctx->stream);
    t->zero_from = ~0ULL;                                  // (what was never cleared need not be now)
    free_dev_table(t->ctx, t->dv);
    delete t;
}

extern "C" uint32_t katgpu_table_k(const katgpu_table* t) { return t ? t->dv.k : 0; }
extern "C" uint32_t katgpu_table_regrows(const katgpu_table* t) { return t ? t->n_regrows : 0; }
extern "C" uint32_t katgpu_table_slot_bytes(const katgpu_table* t) { return !t ? 0 : t->dv.keys_b ? 20 : t->dv.cbits ? 8 : 12; }
extern "C" int katgpu_table_canonical(const katgpu_table* t) { return t ? (int)t->dv.canonical : 0; }

// read the counter block back (one small D2H; synchronises the compute stream)
// may this table's slots be left uncleared for a first sweep to clear (katgpu_table::zero_from)?  What alloc_dev_table asks of a new table.
bool table_may_stay_uncleared(const DevTable& d) { return !g_no_lazy_zero && d.cbits && !d.keys_b && d.n_regions > 1 && d.cap >= g_lazy_min_slots; }

int refresh_counters(katgpu_table* t) {
    katgpu_ctx* c = t->ctx;
    if (t->zero_failed) return fail(c, KATGPU_ERR_DEVICE, "the table's unswept slots could not be cleared (hipMemsetAsync failed): its contents are not to be trusted");
    uint64_t h[CTR_WORDS];
    HIPCHK(c, hipMemcpyAsync(h, t->dv.ctrs, sizeof h, hipMemcpyDeviceToHost, c->stream));      // (the counters only: a table whose slots wait for their first sweep stays that way)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint64_t d = 0;
    for (int i = 0; i < CTR_NSTRIPES; ++i) d += h[CTR_DISTINCT0 + i];
    t->ones = h[CTR_ONES];
    t->distinct = d + (t->ones ? 1 : 0);
    t->n_ovf = (uint32_t)h[CTR_OVF_USED];
    if (h[CTR_FULL]) return fail(c, KATGPU_ERR_TABLE_FULL, "Hash full");
    return KATGPU_OK;
}

namespace kg {
// K2: re-insert a table's (key,count) records into a larger one (hash_counter::double_size, hash_counter.hpp:204-244; k_merge,
// kg_record_kernels.hpp, does the same with a record list).  One body for one-word and wide k-mers (W).
template <bool W>
__global__ void __launch_bounds__(256)
k_regrow(DevTable dst, DevTable src, uint32_t src_n_ovf) {
    uint32_t new_distinct = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < src.cap; i += stride) {
        const SlotRec<W> s = slot_rec<W>(src, i, src_n_ovf);
        if (s.occ) table_add(dst, s.key, s.total, new_distinct);
    }
    flush_distinct(dst, new_distinct);
}
}  // namespace kg

// hash_counter::double_size (deps/jellyfish-2.2.0/include/jellyfish/hash_counter.hpp:204-244): allocate a larger array,
// re-insert every (key,count), swap.  Here one grid-stride kernel instead of a barrier-synchronised thread team.
int regrow(katgpu_table* t, uint64_t new_cap) {
    katgpu_ctx* c = t->ctx;
    DevTable nd{};
    int rc = alloc_dev_table(c, t->dev().k, t->dev().canonical, new_cap, &nd, t->dev().n_regions > 1 ? t->dev().p1 : 0, t->dev().n_regions > 1 ? t->dev().p2 : 0);
    if (rc) return rc;
    {
        ScopedTimer tm(c, KATGPU_K_REGROW, t->dev().cap);
        launch_wide(t->dev().keys_b != nullptr, [&](auto W) {
            hipLaunchKernelGGL(k_regrow<decltype(W)::value>, dim3(grid_for(c, t->dev().cap, 256, 8)), dim3(256), 0, c->stream, nd, t->dev(), t->n_ovf);
        });
    }
    HIPCHK(c, hipMemcpyAsync(&nd.ctrs[CTR_ONES], &t->dev().ctrs[CTR_ONES], sizeof(uint64_t), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    free_dev_table(c, t->dev());
    t->dev() = nd;
    ++t->n_regrows;
    t->count_bound = 0xFFFFFFFFULL;           // full counts were folded back into the slots: the next unchecked launch sweeps first
    t->unchecked_adds = 0;
    return refresh_counters(t);
}

// The fill limit of the direct path.  A k-mer probes inside its region only, so it is the fullest REGION that must not run out
// of slots: regions get Binomial(n, 1/R) k-mers, and small regions (a table created "like" a much bigger one) need more slack
// than the 0.7 that suits regions of thousands of slots.
double load_limit(const DevTable& d) {
    if (d.region_slots >= 1024 || d.n_regions == 1) return 0.7;
    return std::max(0.25, 0.7 - 3.0 / std::sqrt((double)d.region_slots));
}

// Make room for up to `incoming` new distinct k-mers (an upper bound: one per window start) at load <= the fill limit.
int ensure_room(katgpu_table* t, uint64_t incoming) {
    int rc = refresh_counters(t);
    if (rc) return rc;
    const uint64_t need = t->distinct + incoming;
    if ((double)need <= load_limit(t->dev()) * (double)t->dev().cap) return KATGPU_OK;
    if (t->disable_grow) return fail(t->ctx, KATGPU_ERR_TABLE_FULL, "Hash full");
    uint64_t new_cap = t->dev().cap;
    while ((double)need > 0.5 * (double)new_cap) new_cap *= 2;
    return regrow(t, new_cap);
}

int add_in_rooms(katgpu_table* t, size_t n, uint64_t* unseen, const std::function<int(size_t pos, uint64_t take)>& launch) {
    auto limit = [&]() { return (uint64_t)(load_limit(t->dev()) * (double)t->dev().cap); };
    size_t pos = 0;
    while (pos < n) {
        const uint64_t want = n - pos;
        uint64_t take = want;
        if (!unseen || t->distinct + *unseen + want > limit()) {
            int rc = refresh_counters(t); if (rc) return rc;
            if (unseen) *unseen = 0;
            const uint64_t room = limit() > t->distinct ? limit() - t->distinct : 0;
            if (room < std::min<uint64_t>(want, std::max<uint64_t>(t->dev().cap / 8, 1024))) {
                rc = ensure_room(t, std::min<uint64_t>(want, std::max<uint64_t>(t->dev().cap / 2, 1024)));
                if (rc) return rc;
                continue;
            }
            take = std::min(want, room);
        }
        // The amounts are arbitrary: the next k_count launch sweeps first.  (Inert for wide tables: launch_count returns before
        // maybe_sweep for them.)
        t->count_bound = 0xFFFFFFFFULL;
        const int rc = launch(pos, take);
        if (rc) return rc;
        if (unseen) *unseen += take;
        pos += take;
    }
    return KATGPU_OK;
}

namespace kg {
// Σ counts (table_stats "total")
static __global__ void __launch_bounds__(256)
k_total(DevTable t, uint32_t n_ovf, uint64_t* out) {
    uint64_t s = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < t.cap; i += stride) {
        const uint64_t w = t.keys[i];
        if (t.cbits ? w != 0 : w != EMPTY) s += slot_total(t, i, w, t.cbits ? pk_count(w, t.cbits) : (uint64_t)t.counts[i], n_ovf);
    }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd((unsigned long long*)out, (unsigned long long)s);
}
}  // namespace kg

extern "C" int katgpu_table_stats(katgpu_table* t, uint64_t* distinct, uint64_t* total, uint64_t* capacity) {
    if (!t) return KATGPU_ERR_INVALID_ARG;
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    if (distinct) *distinct = t->distinct;
    if (capacity) *capacity = t->dev().cap;
    if (total) {
        uint64_t* scratch = &t->dev().ctrs[CTR_SCRATCH];
        HIPCHK(c, hipMemsetAsync(scratch, 0, sizeof(uint64_t), c->stream));
        hipLaunchKernelGGL(k_total, dim3(grid_for(c, t->dev().cap, 256, 8)), dim3(256), 0, c->stream, t->dev(), t->n_ovf, scratch);
        uint64_t s = 0;
        HIPCHK(c, hipMemcpyAsync(&s, scratch, sizeof s, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        *total = s + t->ones;
    }
    return KATGPU_OK;
}
