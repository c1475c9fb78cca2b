// kg_table.hip -- the HBM-resident count table behind katgpu_table: geometry and layout choice, allocation, regrow
// (hash_counter::double_size), statistics, batch lookups and per-position profiles, record export / merge, .jf records out and in, the k-mer filter and the
// per-record hit counts of `kat filter`, the per-record coverage statistics of `kat sect -n` and `kat cold`.
#include "kg_host.hpp"
#include "kg_kernels.hpp"
#include "kg_wide.hpp"
#include "kg_filter.hpp"
#include "kg_record_stats.hpp"
#include "kg_jf_records.hpp"
#include "kg_jf_load.hpp"
#include "kg_jf.hpp"

static const uint32_t g_region_slots = (uint32_t)hook_u64("KATGPU_TEST_REGION_SLOTS", REGION_SLOTS);
static const bool g_no_packed = hook("KATGPU_NO_PACKED") != nullptr;   // tests / A-B: every table in the KV12 layout
static const bool g_forbid_profile_host = hook_u64("KATGPU_TEST_FORBID_PROFILE_HOST", 0) != 0;   // tests: a driver that should not need per-position counts asks for none

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

extern "C" int katgpu_table_create(katgpu_ctx* c, uint32_t k, int canonical, uint64_t size_hint, int disable_grow, katgpu_table** out) {
    if (!c || !out) return KATGPU_ERR_INVALID_ARG;
    *out = nullptr;
    if (k < 1 || k > KATGPU_MAX_K) return fail(c, KATGPU_ERR_K, "k = %u unsupported: this build keeps a k-mer in at most two 63-bit words (1 <= k <= %d)", k, KATGPU_MAX_K);
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t cap = std::max<uint64_t>(size_hint ? size_hint : (1u << 20), 1024);
    katgpu_table* t = new katgpu_table();
    t->ctx = c; t->disable_grow = disable_grow;
    bool lazy = false;
    int rc = alloc_dev_table(c, k, canonical, cap, &t->dv, 0, 0, &lazy);
    if (rc) { delete t; return rc; }
    if (lazy) t->zero_from = 0;
    *out = t;
    return KATGPU_OK;
}

extern "C" int katgpu_table_create_like(katgpu_ctx* c, const katgpu_table* like, uint32_t k, int canonical, uint64_t size_hint,
                                        int disable_grow, katgpu_table** out) {
    if (!c || !out || !like) return KATGPU_ERR_INVALID_ARG;
    *out = nullptr;
    if (k < 1 || k > KATGPU_MAX_K) return fail(c, KATGPU_ERR_K, "k = %u unsupported: this build keeps a k-mer in at most two 63-bit words (1 <= k <= %d)", k, KATGPU_MAX_K);
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t cap = std::max<uint64_t>(size_hint ? size_hint : (1u << 20), 1024);
    katgpu_table* t = new katgpu_table();
    t->ctx = c; t->disable_grow = disable_grow;
    // (no common grid across key widths; none for wide tables either: nothing joins or merges them region by region, and a grid
    // handed down could make regions the wide apply kernel cannot hold)
    bool lazy = false;
    int rc = k > 32 || like->dv.k > 32 ? alloc_dev_table(c, k, canonical, cap, &t->dv, 0, 0, &lazy)
                                       : alloc_dev_table(c, k, canonical, cap, &t->dv, like->dv.p1, like->dv.p2, &lazy);
    if (rc) { delete t; return rc; }
    if (lazy) t->zero_from = 0;
    *out = t;
    return KATGPU_OK;
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

// hash_counter::double_size (deps/jellyfish-2.2.0/include/jellyfish/hash_counter.hpp:204-244): allocate a larger array,
// re-insert every (key,count), swap.  Here one grid-stride kernel instead of a barrier-synchronised thread team.
int regrow(katgpu_table* t, uint64_t new_cap) {
    katgpu_ctx* c = t->ctx;
    DevTable nd{};
    int rc = alloc_dev_table(c, t->dev().k, t->dev().canonical, new_cap, &nd, t->dev().n_regions > 1 ? t->dev().p1 : 0, t->dev().n_regions > 1 ? t->dev().p2 : 0);
    if (rc) return rc;
    {
        ScopedTimer tm(c, KATGPU_K_REGROW, t->dev().cap);
        if (t->dev().keys_b) hipLaunchKernelGGL(k_regrow_w, dim3(grid_for(c, t->dev().cap, 256, 8)), dim3(256), 0, c->stream, nd, t->dev(), t->n_ovf);
        else hipLaunchKernelGGL(k_regrow, dim3(grid_for(c, t->dev().cap, 256, 8)), dim3(256), 0, c->stream, nd, t->dev(), t->n_ovf);
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

extern "C" int katgpu_table_get(katgpu_table* t, const uint64_t* keys, size_t n, int canonicalise, uint64_t* counts) {
    if (!t || (n && (!keys || !counts))) return KATGPU_ERR_INVALID_ARG;
    NARROW_ONLY(t, "katgpu_table_get: use katgpu_table_get_wide;");
    if (!n) return KATGPU_OK;
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    uint64_t *dk = nullptr, *dc = nullptr;
    HIPCHK(c, hipMalloc(&dk, n * 8));
    if (hipMalloc(&dc, n * 8) != hipSuccess) { hipFree(dk); return fail(c, KATGPU_ERR_NOMEM, "lookup buffers"); }
    hipMemcpyAsync(dk, keys, n * 8, hipMemcpyHostToDevice, c->stream);
    hipLaunchKernelGGL(k_get, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, t->dev(), t->n_ovf, dk, (uint64_t)n, canonicalise, dc);
    hipMemcpyAsync(counts, dc, n * 8, hipMemcpyDeviceToHost, c->stream);
    hipError_t e = hipStreamSynchronize(c->stream);
    hipFree(dk); hipFree(dc);
    if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "%s", hipGetErrorString(e));
    return KATGPU_OK;
}

static int launch_profile(katgpu_table* t, const uint8_t* dev_bases, size_t n, int canonicalise, uint64_t* dev_counts) {
    katgpu_ctx* c = t->ctx;
    const bool wide = t->dev().keys_b != nullptr;
    const uint64_t n_out = n - t->dev().k + 1;
    const uint64_t per_chunk = wide ? WIDE_CHUNK_STARTS : CHUNK_STARTS;
    const uint64_t n_chunks = (n_out + per_chunk - 1) / per_chunk;
    const int grid = (int)std::min<uint64_t>(n_chunks, (uint64_t)c->n_cu * 8);
    const bool aligned = (reinterpret_cast<uintptr_t>(dev_bases) & 15) == 0 && (reinterpret_cast<uintptr_t>(dev_counts) & 15) == 0;
    ScopedTimer tm(c, KATGPU_K_PROFILE, n_out);
    if (wide && aligned) hipLaunchKernelGGL((k_profile<true, true>), dim3(grid), dim3(COUNT_BLOCK), 0, c->stream, t->dev(), t->n_ovf, canonicalise, dev_bases, (uint64_t)n, n_chunks, dev_counts);
    else if (wide) hipLaunchKernelGGL((k_profile<false, true>), dim3(grid), dim3(COUNT_BLOCK), 0, c->stream, t->dev(), t->n_ovf, canonicalise, dev_bases, (uint64_t)n, n_chunks, dev_counts);
    else if (aligned) hipLaunchKernelGGL((k_profile<true, false>), dim3(grid), dim3(COUNT_BLOCK), 0, c->stream, t->dev(), t->n_ovf, canonicalise, dev_bases, (uint64_t)n, n_chunks, dev_counts);
    else hipLaunchKernelGGL((k_profile<false, false>), dim3(grid), dim3(COUNT_BLOCK), 0, c->stream, t->dev(), t->n_ovf, canonicalise, dev_bases, (uint64_t)n, n_chunks, dev_counts);
    HIPCHK(c, hipGetLastError());
    return KATGPU_OK;
}

extern "C" int katgpu_table_profile_device(katgpu_table* t, const uint8_t* dev_bases, size_t n, int canonicalise, uint64_t* dev_counts) {
    if (!t || (n && (!dev_bases || !dev_counts))) return KATGPU_ERR_INVALID_ARG;
    if (n < t->dev().k) return KATGPU_OK;
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    return launch_profile(t, dev_bases, n, canonicalise, dev_counts);
}

// Host form: the sequence goes through the device in batches of PROFILE_BATCH window starts (each batch re-sends the
// k-1 bases it shares with the next one), so any length fits next to the table.
extern "C" int katgpu_table_profile_host(katgpu_table* t, const char* bases, size_t n, int canonicalise, uint64_t* counts) {
    if (!t || (n && (!bases || !counts))) return KATGPU_ERR_INVALID_ARG;
    if (g_forbid_profile_host) return fail(t->ctx, KATGPU_ERR_INVALID_ARG, "katgpu_table_profile_host is forbidden (KATGPU_TEST_FORBID_PROFILE_HOST)");
    const uint32_t k = t->dev().k;
    if (n < k) return KATGPU_OK;
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    const size_t n_out = n - k + 1;
    const size_t PROFILE_BATCH = (size_t)32 << 20;
    const size_t batch = std::min(n_out, PROFILE_BATCH);
    uint8_t* db = nullptr; uint64_t* dc = nullptr;
    HIPCHK(c, pool_alloc(c, (void**)&db, batch + 64));
    if (pool_alloc(c, (void**)&dc, batch * 8) != hipSuccess) { pool_release(c, db); return fail(c, KATGPU_ERR_NOMEM, "profile buffers"); }
    hipError_t e = hipSuccess;
    for (size_t pos = 0; pos < n_out && rc == KATGPU_OK && e == hipSuccess; pos += batch) {
        const size_t starts = std::min(batch, n_out - pos);
        const size_t nb = starts + k - 1;
        e = hipMemcpyAsync(db, bases + pos, nb, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) break;
        rc = launch_profile(t, db, nb, canonicalise, dc);
        if (rc) break;
        e = hipMemcpyAsync(counts + pos, dc, starts * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    hipStreamSynchronize(c->stream);
    pool_release(c, db); pool_release(c, dc);
    if (rc) return rc;
    if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "%s", hipGetErrorString(e));
    return KATGPU_OK;
}

// ------------------------------------------------------------------ partition / export / merge -------

extern "C" int katgpu_table_partition_sizes(katgpu_table* t, uint32_t n_parts, uint64_t* sizes) {
    if (!t || !sizes || n_parts == 0 || n_parts > 4096) return KATGPU_ERR_INVALID_ARG;
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    unsigned long long* d = nullptr;
    HIPCHK(c, hipMalloc(&d, n_parts * 8));
    hipMemsetAsync(d, 0, n_parts * 8, c->stream);
    {
        ScopedTimer tm(c, KATGPU_K_PARTITION, t->dev().cap);
        if (t->dev().keys_b)
            hipLaunchKernelGGL(k_partition_w<0>, dim3(grid_for(c, t->dev().cap, 256, 8)), dim3(256), 0, c->stream, t->dev(), t->n_ovf, n_parts, d, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr);
        else
            hipLaunchKernelGGL(k_partition<0>, dim3(grid_for(c, t->dev().cap + 1, 256, 8)), dim3(256), 0, c->stream, t->dev(), t->n_ovf, n_parts, d, (uint64_t*)nullptr, (uint64_t*)nullptr);
    }
    hipMemcpyAsync(sizes, d, n_parts * 8, hipMemcpyDeviceToHost, c->stream);
    hipError_t e = hipStreamSynchronize(c->stream);
    hipFree(d);
    if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "%s", hipGetErrorString(e));
    return KATGPU_OK;
}

extern "C" int katgpu_table_partition(katgpu_table* t, uint32_t n_parts, const uint64_t* offsets, uint64_t* dev_keys, uint64_t* dev_counts) {
    if (!t || !offsets || n_parts == 0 || n_parts > 4096) return KATGPU_ERR_INVALID_ARG;
    NARROW_ONLY(t, "katgpu_table_partition");
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    unsigned long long* d = nullptr;
    HIPCHK(c, hipMalloc(&d, n_parts * 8));
    hipMemcpyAsync(d, offsets, n_parts * 8, hipMemcpyHostToDevice, c->stream);
    {
        ScopedTimer tm(c, KATGPU_K_PARTITION, t->dev().cap);
        hipLaunchKernelGGL(k_partition<1>, dim3(grid_for(c, t->dev().cap + 1, 256, 8)), dim3(256), 0, c->stream, t->dev(), t->n_ovf, n_parts, d, dev_keys, dev_counts);
    }
    hipError_t e = hipStreamSynchronize(c->stream);
    hipFree(d);
    if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "%s", hipGetErrorString(e));
    return KATGPU_OK;
}

extern "C" int katgpu_table_export(katgpu_table* t, uint64_t* keys, uint64_t* counts, size_t cap, size_t* n_out) {
    if (!t || !n_out) return KATGPU_ERR_INVALID_ARG;
    NARROW_ONLY(t, "katgpu_table_export: use katgpu_table_export_wide;");
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    *n_out = (size_t)t->distinct;
    if (cap == 0) return KATGPU_OK;
    if (cap < t->distinct || !keys || !counts) return fail(c, KATGPU_ERR_INVALID_ARG, "export buffer too small: %zu < %llu", cap, (unsigned long long)t->distinct);
    if (!t->distinct) return KATGPU_OK;
    uint64_t *dk = nullptr, *dc = nullptr;
    HIPCHK(c, hipMalloc(&dk, t->distinct * 8));
    if (hipMalloc(&dc, t->distinct * 8) != hipSuccess) { hipFree(dk); return fail(c, KATGPU_ERR_NOMEM, "export buffers"); }
    uint64_t zero = 0;
    rc = katgpu_table_partition(t, 1, &zero, dk, dc);
    if (!rc) {
        hipError_t e = hipMemcpy(keys, dk, t->distinct * 8, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(counts, dc, t->distinct * 8, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(c, KATGPU_ERR_DEVICE, "export: %s", hipGetErrorString(e));
    }
    hipFree(dk); hipFree(dc);
    return rc;
}

extern "C" int katgpu_table_merge_device(katgpu_table* t, const uint64_t* dev_keys, const uint64_t* dev_counts, size_t n) {
    if (!t || (n && (!dev_keys || !dev_counts))) return KATGPU_ERR_INVALID_ARG;
    NARROW_ONLY(t, "katgpu_table_merge_device");
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    size_t pos = 0;
    while (pos < n) {
        int rc = refresh_counters(t); if (rc) return rc;
        uint64_t room = (uint64_t)(load_limit(t->dev()) * (double)t->dev().cap) > t->distinct ? (uint64_t)(load_limit(t->dev()) * (double)t->dev().cap) - t->distinct : 0;
        uint64_t want = n - pos;
        if (room < std::min<uint64_t>(want, std::max<uint64_t>(t->dev().cap / 8, 1024))) {
            rc = ensure_room(t, std::min<uint64_t>(want, std::max<uint64_t>(t->dev().cap / 2, 1024)));
            if (rc) return rc;
            continue;
        }
        uint64_t take = std::min(want, room);
        t->count_bound = 0xFFFFFFFFULL;          // merged amounts are arbitrary: the next k_count launch sweeps first
        {
            ScopedTimer tm(c, KATGPU_K_MERGE, take);
            hipLaunchKernelGGL(k_merge, dim3(grid_for(c, take, 256, 8)), dim3(256), 0, c->stream, t->dev(), dev_keys + pos, dev_counts + pos, take);
        }
        pos += take;
    }
    return refresh_counters(t);
}

extern "C" int katgpu_table_merge_host(katgpu_table* t, const uint64_t* keys, const uint64_t* counts, size_t n) {
    if (!t || (n && (!keys || !counts))) return KATGPU_ERR_INVALID_ARG;
    NARROW_ONLY(t, "katgpu_table_merge_host: use katgpu_table_merge_host_wide;");
    if (!n) return KATGPU_OK;
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    uint64_t *dk = nullptr, *dc = nullptr;
    HIPCHK(c, hipMalloc(&dk, n * 8));
    if (hipMalloc(&dc, n * 8) != hipSuccess) { hipFree(dk); return fail(c, KATGPU_ERR_NOMEM, "merge buffers"); }
    hipError_t e = hipMemcpy(dk, keys, n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dc, counts, n * 8, hipMemcpyHostToDevice);
    int rc = e == hipSuccess ? katgpu_table_merge_device(t, dk, dc, n) : fail(c, KATGPU_ERR_DEVICE, "merge: %s", hipGetErrorString(e));
    hipFree(dk); hipFree(dc);
    return rc;
}

// ------------------------------------------------------------------ .jf records in file order ----

namespace {
// device scratch of the record producer, kept across the ranges of one dump
struct JfScratch {
    uint32_t* hist = nullptr; size_t nb_cap = 0;         // hist[nb_cap], cursor[nb_cap], off[nb_cap + 1]
    uint64_t* recs = nullptr; size_t rec_cap = 0;        // pos[rec_cap], key[rec_cap], then 32-bit counts: 20 bytes per record
    uint32_t* rank = nullptr; size_t rank_cap = 0;       // buckets beyond one LDS tile only
    ~JfScratch() { hipFree(hist); hipFree(recs); hipFree(rank); }
};
struct JfRange { uint64_t lo, hi, n; };
}

// (the pool may be sitting on freed table arrays: give them back before giving up)
static hipError_t jf_malloc(katgpu_ctx* c, void** p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); pool_trim(c); e = hipMalloc(p, bytes); if (e != hipSuccess) (void)hipGetLastError(); }
    return e;
}
template <typename T>
static bool jf_ensure(katgpu_ctx* c, T*& p, size_t& have, size_t want, size_t bytes_for_want) {
    if (have >= want) return true;
    hipFree(p); p = nullptr; have = 0;
    if (jf_malloc(c, (void**)&p, bytes_for_want) != hipSuccess) return false;
    have = want;
    return true;
}

// the columns of M ("matrix1": bit i of the k-mer selects column 2k-1-i) as rows over the key bits
static JfRows jf_rows(uint32_t k, uint32_t r, const uint64_t* cols) {
    JfRows m{};
    const uint32_t c = 2 * k;
    for (uint32_t j = 0; j < r; ++j)
        for (uint32_t i = 0; i < c; ++i) m.row[j] |= ((cols[c - 1 - i] >> j) & 1ULL) << i;
    return m;
}

// buckets of 2^shift positions: at most JF_BUCKET_MEAN expected records each when `distinct` records spread evenly over 2^r positions
static uint32_t jf_bucket_shift(uint64_t distinct, uint32_t r) {
    uint32_t s = 0;
    while (s < r && std::ldexp((double)std::max<uint64_t>(distinct, 1), (int)s + 1) <= std::ldexp((double)JF_BUCKET_MEAN, (int)r)) ++s;
    return s;
}

static void jf_launch_select_hist(katgpu_table* t, const JfRows& m, uint32_t r, uint64_t pos_lo, uint64_t pos_hi, uint32_t shift, uint32_t* hist) {
    katgpu_ctx* c = t->ctx;
    hipLaunchKernelGGL(k_jf_select<0>, dim3(grid_for(c, t->dev().cap + 1, JF_BLOCK, 8)), dim3(JF_BLOCK), 0, c->stream, t->dev(), t->n_ovf, m, r, pos_lo, pos_hi, shift,
                       hist, (unsigned long long*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr);
}

// Select, order and pack the records of [pos_lo, pos_hi) into dev_out (room for `cap` records).  Synchronises once, to learn how many
// the range holds (*n_out); the scatter, the sort and the pack are left running on the compute stream.
static int jf_range(katgpu_table* t, const JfRows& m, uint32_t r, uint32_t shift, uint64_t pos_lo, uint64_t pos_hi, uint8_t* dev_out, size_t cap,
                    size_t* n_out, JfScratch& s) {
    katgpu_ctx* c = t->ctx;
    *n_out = 0;
    if (pos_lo == pos_hi) return KATGPU_OK;
    const uint64_t nb64 = ((pos_hi - pos_lo - 1) >> shift) + 1;
    if (nb64 >= (1ULL << 31)) return fail(c, KATGPU_ERR_INVALID_ARG, "jf records: a range of %llu buckets: ask for a narrower one", (unsigned long long)nb64);
    const uint32_t nb = (uint32_t)nb64;
    if (!jf_ensure(c, s.hist, s.nb_cap, (size_t)nb, ((size_t)nb * 3 + 1) * sizeof(uint32_t))) return fail(c, KATGPU_ERR_NOMEM, "jf records: no device memory for %u bucket counters", nb);
    uint32_t *hist = s.hist, *cursor = s.hist + s.nb_cap, *off = s.hist + 2 * s.nb_cap;
    unsigned long long* res = (unsigned long long*)&t->dev().ctrs[CTR_SCRATCH];
    const DevTable dv = t->dev();
    HIPCHK(c, hipMemsetAsync(hist, 0, (size_t)nb * sizeof(uint32_t), c->stream));
    jf_launch_select_hist(t, m, r, pos_lo, pos_hi, shift, hist);
    hipLaunchKernelGGL(k_jf_scan, dim3(1), dim3(JF_SCAN_BLOCK), 0, c->stream, hist, nb, off, cursor, res);
    unsigned long long h[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(h, res, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_out = (size_t)h[0];
    if (!h[0]) return KATGPU_OK;
    if (h[0] > cap) return fail(c, KATGPU_ERR_INVALID_ARG, "jf records: the range holds %llu records, the buffer %zu", h[0], cap);
    if (h[0] >= (1ULL << 31)) return fail(c, KATGPU_ERR_INVALID_ARG, "jf records: %llu records in one range: ask for a narrower one", h[0]);
    const size_t n = (size_t)h[0];
    if (!jf_ensure(c, s.recs, s.rec_cap, n, n * 20)) return fail(c, KATGPU_ERR_NOMEM, "jf records: no device memory to order %zu records", n);
    uint64_t *d_pos = s.recs, *d_key = s.recs + s.rec_cap;
    uint32_t* d_cnt = (uint32_t*)(s.recs + 2 * s.rec_cap);
    const uint32_t key_bytes = (2 * dv.k + 7) / 8;
    // (none of these launches is booked under a kernel class of katgpu_profile_get: the dump reports its own phases, katgpu_timing "jf_dump")
    hipLaunchKernelGGL(k_jf_select<1>, dim3(grid_for(c, dv.cap + 1, JF_BLOCK, 8)), dim3(JF_BLOCK), 0, c->stream, dv, t->n_ovf, m, r, pos_lo, pos_hi, shift,
                       cursor, (unsigned long long*)nullptr, d_pos, d_key, d_cnt);
    // The ranking path compares every record of an oversized bucket with the whole bucket.  That is for the odd run of equal positions,
    // not for a matrix that piles a table onto a few of them: beyond JF_RANK_MAX records in one bucket the range is refused.
    if (h[1] > JF_RANK_MAX)
        return fail(c, KATGPU_ERR_INVALID_ARG, "jf records: %llu records share one stretch of 2^%u positions (at most %u are ordered there): the matrix does not spread this table",
                    h[1], shift, JF_RANK_MAX);
    if (h[1] > JF_TILE) {
        if (!jf_ensure(c, s.rank, s.rank_cap, n, n * sizeof(uint32_t))) return fail(c, KATGPU_ERR_NOMEM, "jf records: no device memory to rank %zu records", n);
        hipLaunchKernelGGL(k_jf_rank, dim3(grid_for(c, n, JF_BLOCK, 8)), dim3(JF_BLOCK), 0, c->stream, d_pos, d_key, (uint32_t)n, pos_lo, shift, off, s.rank);
    }
    hipLaunchKernelGGL(k_jf_sort_pack, dim3(std::min<uint32_t>(nb, (uint32_t)c->n_cu * 5)), dim3(JF_BLOCK), 0, c->stream, d_pos, d_key, d_cnt, off, s.rank, nb, key_bytes, dev_out);
    HIPCHK(c, hipGetLastError());
    return KATGPU_OK;
}

extern "C" int katgpu_table_jf_records_device(katgpu_table* t, uint32_t r, const uint64_t* cols, uint64_t pos_lo, uint64_t pos_hi,
                                              uint8_t* dev_out, size_t cap_records, size_t* n_out) {
    if (!t || !cols || !n_out) return KATGPU_ERR_INVALID_ARG;
    NARROW_ONLY(t, "katgpu_table_jf_records_device");
    katgpu_ctx* c = t->ctx;
    const uint32_t k = t->dv.k;
    if (r < 1 || r > std::min<uint32_t>(2 * k, 63) || pos_lo > pos_hi || pos_hi > (1ULL << r))
        return fail(c, KATGPU_ERR_INVALID_ARG, "jf records: need 1 <= r <= min(2k, 63) and pos_lo <= pos_hi <= 2^r (r = %u, [%llu, %llu))", r, (unsigned long long)pos_lo, (unsigned long long)pos_hi);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    *n_out = 0;
    const JfRows m = jf_rows(k, r, cols);
    if (!dev_out || !cap_records) {
        unsigned long long* total = (unsigned long long*)&t->dev().ctrs[CTR_SCRATCH];
        HIPCHK(c, hipMemsetAsync(total, 0, sizeof(uint64_t), c->stream));
        hipLaunchKernelGGL(k_jf_select<2>, dim3(grid_for(c, t->dev().cap + 1, JF_BLOCK, 8)), dim3(JF_BLOCK), 0, c->stream, t->dev(), t->n_ovf, m, r, pos_lo, pos_hi, 0u,
                           (uint32_t*)nullptr, total, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr);
        unsigned long long h = 0;
        HIPCHK(c, hipMemcpyAsync(&h, total, sizeof h, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        *n_out = (size_t)h;
        return KATGPU_OK;
    }
    JfScratch s;
    rc = jf_range(t, m, r, jf_bucket_shift(t->distinct, r), pos_lo, pos_hi, dev_out, cap_records, n_out, s);
    const hipError_t e = hipStreamSynchronize(c->stream);            // (before the scratch goes)
    if (!rc && e != hipSuccess) rc = fail(c, KATGPU_ERR_DEVICE, "jf records: %s", hipGetErrorString(e));
    return rc;
}

static const uint64_t g_jf_range_records = hook_u64("KATGPU_JF_RANGE_RECORDS", 0);   // tests: many ranges at tiny sizes

int jf_stream_records(katgpu_table* t, uint32_t r, const uint64_t* cols, FILE* f, JfDumpTiming* tm) {
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    const uint64_t distinct = t->distinct;
    if (!distinct) return KATGPU_OK;
    const uint32_t k = t->dev().k, rb = (2 * k + 7) / 8 + 4;
    const JfRows m = jf_rows(k, r, cols);
    const uint32_t shift = jf_bucket_shift(distinct, r);
    JfScratch s;

    // Where to cut: the records per stretch of 2^(r - cb) positions, once; ranges are whole stretches, so what each holds is known.
    const uint32_t cb = std::min<uint32_t>(r, 16), cshift = r - cb;
    const size_t nbins = (size_t)1 << cb;
    if (!jf_ensure(c, s.hist, s.nb_cap, nbins, (nbins * 3 + 1) * sizeof(uint32_t))) return KG_JF_NO_SCRATCH;
    std::vector<uint32_t> bins(nbins);
    HIPCHK(c, hipMemsetAsync(s.hist, 0, nbins * sizeof(uint32_t), c->stream));
    jf_launch_select_hist(t, m, r, 0, 1ULL << r, cshift, s.hist);
    HIPCHK(c, hipMemcpyAsync(bins.data(), s.hist, nbins * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));

    // a range's records: 20 bytes to order them, 4 should they need ranking, its bytes in each of the two output buffers.  Half of what
    // is free, and at most 2^25 records: the pinned buffers are what the host pays (and pinning is not free: kg_host.hpp, ScanCache).
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    uint64_t want = std::min<uint64_t>(std::max<uint64_t>(free_b / 2 / (24 + 2 * rb), 1 << 16), 1 << 25);
    if (g_jf_range_records) want = g_jf_range_records;
    std::vector<JfRange> ranges;
    uint64_t acc = 0, start = 0, max_n = 0, sum = 0;
    for (size_t b = 0; b < nbins; ++b) {
        if (acc && acc + bins[b] > want) { ranges.push_back({start << cshift, (uint64_t)b << cshift, acc}); max_n = std::max(max_n, acc); start = b; acc = 0; }
        acc += bins[b]; sum += bins[b];
    }
    ranges.push_back({start << cshift, 1ULL << r, acc}); max_n = std::max(max_n, acc);
    if (sum != distinct) return fail(c, KATGPU_ERR_DEVICE, "jf dump: the position histogram holds %llu records, the table %llu", (unsigned long long)sum, (unsigned long long)distinct);
    if (max_n >= (1ULL << 31)) return KG_JF_NO_SCRATCH;           // (a matrix that piles the table onto one stretch of positions)

    // everything a range can need is allocated before a byte of records is written: the bucket counters of the widest range here, the
    // record scratch and the buffers below; what could still fail (the rank array of a skewed range, a refused bucket) leads to the
    // host writer as well, which starts the file afresh
    uint64_t max_nb = 1;
    for (const JfRange& g : ranges) max_nb = std::max(max_nb, ((g.hi - g.lo - 1) >> shift) + 1);
    if (max_nb >= (1ULL << 31) || !jf_ensure(c, s.hist, s.nb_cap, (size_t)max_nb, ((size_t)max_nb * 3 + 1) * sizeof(uint32_t))) return KG_JF_NO_SCRATCH;
    const int nbuf = ranges.size() > 1 ? 2 : 1;
    const size_t buf_bytes = (size_t)max_n * rb;
    uint8_t *d_out[2] = {nullptr, nullptr}, *pinned[2] = {nullptr, nullptr};
    hipEvent_t ev[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};      // range started, produced, copied
    hipStream_t copy = nullptr;
    auto release = [&]() {
        hipStreamSynchronize(c->stream);
        if (copy) { hipStreamSynchronize(copy); hipStreamDestroy(copy); }
        for (int i = 0; i < 2; ++i) { hipFree(d_out[i]); if (pinned[i]) hipHostFree(pinned[i]); for (hipEvent_t e : ev[i]) if (e) hipEventDestroy(e); }
    };
    bool have = jf_ensure(c, s.recs, s.rec_cap, (size_t)max_n, (size_t)max_n * 20) && hipStreamCreateWithFlags(&copy, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; have && i < nbuf; ++i) {
        have = jf_malloc(c, (void**)&d_out[i], buf_bytes) == hipSuccess && hipHostMalloc((void**)&pinned[i], buf_bytes, hipHostMallocDefault) == hipSuccess;
        for (int j = 0; have && j < 3; ++j) have = hipEventCreate(&ev[i][j]) == hipSuccess;
    }
    if (!have) { (void)hipGetLastError(); release(); return KG_JF_NO_SCRATCH; }

    int pend = -1, slot = 0;
    size_t pend_n = 0;
    uint64_t written = 0;
    auto drain = [&]() -> int {                                   // the copy of the range before this one has landed: write it
        if (pend < 0) return KATGPU_OK;
        HIPCHK(c, hipEventSynchronize(ev[pend][2]));
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev[pend][0], ev[pend][1]) == hipSuccess) tm->device_s += ms * 1e-3;
        if (hipEventElapsedTime(&ms, ev[pend][1], ev[pend][2]) == hipSuccess) tm->copy_s += ms * 1e-3;
        const double t0 = now_ms();
        const bool ok = fwrite(pinned[pend], rb, pend_n, f) == pend_n;
        tm->write_s += (now_ms() - t0) * 1e-3;
        written += pend_n; pend = -1;
        return ok ? KATGPU_OK : KATGPU_ERR_IO;
    };
    for (const JfRange& g : ranges) {
        size_t n = 0;
        hipEventRecord(ev[slot][0], c->stream);
        rc = jf_range(t, m, r, shift, g.lo, g.hi, d_out[slot], (size_t)max_n, &n, s);
        if (!rc && n != g.n) rc = fail(c, KATGPU_ERR_DEVICE, "jf dump: positions [%llu, %llu) hold %zu records, their histogram said %llu", (unsigned long long)g.lo, (unsigned long long)g.hi, n, (unsigned long long)g.n);
        if (rc == KATGPU_ERR_NOMEM || rc == KATGPU_ERR_INVALID_ARG) rc = KG_JF_NO_SCRATCH;
        if (rc) break;
        if (n) {
            hipEventRecord(ev[slot][1], c->stream);
            hipStreamWaitEvent(copy, ev[slot][1], 0);
            const hipError_t e = hipMemcpyAsync(pinned[slot], d_out[slot], n * rb, hipMemcpyDeviceToHost, copy);
            hipEventRecord(ev[slot][2], copy);
            if (e != hipSuccess) { rc = fail(c, KATGPU_ERR_DEVICE, "jf dump: %s", hipGetErrorString(e)); break; }
        }
        rc = drain();                                             // (while this range is ordered and copied)
        if (rc) break;
        if (n) { pend = slot; pend_n = n; slot = (slot + 1) % nbuf; }
        ++tm->ranges;
    }
    if (!rc) rc = drain();
    release();
    if (!rc && written != distinct) rc = fail(c, KATGPU_ERR_DEVICE, "jf dump: wrote %llu of %llu records", (unsigned long long)written, (unsigned long long)distinct);
    return rc;
}

// ------------------------------------------------------------------ .jf records into a table ----

// n packed records at dev_recs added to t, with room made the way katgpu_table_merge_device makes it.  *unseen: records launched since
// t->distinct was read -- every one may be a new k-mer; while the table holds that bound below its fill limit nothing is read back, so
// a caller that feeds chunk after chunk synchronises only where the table may have to grow.
static int jf_add_records(katgpu_table* t, const uint8_t* dev_recs, size_t n, uint32_t key_len, uint32_t counter_len, uint64_t* unseen) {
    katgpu_ctx* c = t->ctx;
    const uint32_t rb = (key_len + 7) / 8 + counter_len;
    size_t pos = 0;
    while (pos < n) {
        const uint64_t limit = (uint64_t)(load_limit(t->dev()) * (double)t->dev().cap);
        const uint64_t want = n - pos;
        uint64_t take = want;
        if (t->distinct + *unseen + want > limit) {
            int rc = refresh_counters(t); if (rc) return rc;
            *unseen = 0;
            const uint64_t room = limit > t->distinct ? limit - t->distinct : 0;
            if (room < std::min<uint64_t>(want, std::max<uint64_t>(t->dev().cap / 8, 1024))) {
                rc = ensure_room(t, std::min<uint64_t>(want, std::max<uint64_t>(t->dev().cap / 2, 1024)));
                if (rc) return rc;
                continue;
            }
            take = std::min(want, room);
        }
        t->count_bound = 0xFFFFFFFFULL;          // the amounts are arbitrary: the next k_count launch sweeps first
        {
            ScopedTimer tm(c, KATGPU_K_MERGE, take);
            const dim3 grid((unsigned)std::min<uint64_t>((take + JL_TILE - 1) / JL_TILE, (uint64_t)c->n_cu * 8));
            if (t->dev().keys_b) hipLaunchKernelGGL(k_jf_add<true>, grid, dim3(JL_BLOCK), 0, c->stream, t->dev(), dev_recs + pos * rb, (uint64_t)take, key_len, counter_len);
            else hipLaunchKernelGGL(k_jf_add<false>, grid, dim3(JL_BLOCK), 0, c->stream, t->dev(), dev_recs + pos * rb, (uint64_t)take, key_len, counter_len);
        }
        HIPCHK(c, hipGetLastError());
        *unseen += take;
        pos += take;
    }
    return KATGPU_OK;
}

extern "C" int katgpu_table_add_jf_records_device(katgpu_table* t, const uint8_t* dev_records, size_t n_records, uint32_t key_len, uint32_t counter_len) {
    if (!t || (n_records && !dev_records)) return KATGPU_ERR_INVALID_ARG;
    katgpu_ctx* c = t->ctx;
    if (key_len != 2 * t->dv.k) return fail(c, KATGPU_ERR_MISMATCH, "jf records of %u key bits into a table of k = %u", key_len, t->dv.k);
    if (counter_len < 1 || counter_len > 8) return fail(c, KATGPU_ERR_INVALID_ARG, "jf records: a count of %u bytes (1 to 8 are possible)", counter_len);
    if (!n_records) return KATGPU_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    uint64_t unseen = 0;
    rc = jf_add_records(t, dev_records, n_records, key_len, counter_len, &unseen);
    if (rc) return rc;
    return refresh_counters(t);
}

static const uint64_t g_jf_load_records = hook_u64("KATGPU_JF_LOAD_RECORDS", 0);   // tests: many chunks at tiny sizes

int jf_stream_load(katgpu_table* t, FILE* f, size_t n, uint32_t key_len, uint32_t counter_len, JfLoadTiming* tm) {
    katgpu_ctx* c = t->ctx;
    if (!n) return KATGPU_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const uint32_t rb = (key_len + 7) / 8 + counter_len;
    const size_t chunk = (size_t)std::min<uint64_t>(g_jf_load_records ? g_jf_load_records : (uint64_t)1 << 24, n);
    const size_t buf_bytes = chunk * rb;
    const int nbuf = n > chunk ? 2 : 1;
    uint8_t *d_buf[2] = {nullptr, nullptr}, *pinned[2] = {nullptr, nullptr};
    hipEvent_t ev[2][4] = {{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}};      // copy started, copied, add started, added
    bool used[2] = {false, false};
    hipStream_t copy = nullptr;
    auto release = [&]() {
        hipStreamSynchronize(c->stream);
        if (copy) { hipStreamSynchronize(copy); hipStreamDestroy(copy); }
        for (int i = 0; i < 2; ++i) { pool_release(c, d_buf[i]); if (pinned[i]) hipHostFree(pinned[i]); for (hipEvent_t e : ev[i]) if (e) hipEventDestroy(e); }
    };
    bool have = hipStreamCreateWithFlags(&copy, hipStreamNonBlocking) == hipSuccess;
    for (int i = 0; have && i < nbuf; ++i) {
        have = pool_alloc(c, (void**)&d_buf[i], buf_bytes) == hipSuccess && hipHostMalloc((void**)&pinned[i], buf_bytes, hipHostMallocDefault) == hipSuccess;
        for (int j = 0; have && j < 4; ++j) have = hipEventCreate(&ev[i][j]) == hipSuccess;
    }
    if (!have) { (void)hipGetLastError(); release(); return KG_JF_NO_SCRATCH; }

    auto collect = [&](int slot) -> int {                         // the chunk that went through this slot has been added: its buffers are free
        if (!used[slot]) return KATGPU_OK;
        HIPCHK(c, hipEventSynchronize(ev[slot][3]));
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev[slot][0], ev[slot][1]) == hipSuccess) tm->copy_s += ms * 1e-3;
        if (hipEventElapsedTime(&ms, ev[slot][2], ev[slot][3]) == hipSuccess) tm->device_s += ms * 1e-3;
        used[slot] = false;
        return KATGPU_OK;
    };
    int rc = refresh_counters(t);
    uint64_t unseen = 0;
    int slot = 0;
    for (size_t pos = 0; !rc && pos < n; slot = (slot + 1) % nbuf) {
        const size_t take = std::min(chunk, n - pos);
        rc = collect(slot);                                       // (the chunk before this one is being copied or added meanwhile)
        if (rc) break;
        const double t0 = now_ms();
        const bool ok = fread(pinned[slot], rb, take, f) == take;
        tm->read_s += (now_ms() - t0) * 1e-3;
        if (!ok) { rc = KATGPU_ERR_IO; break; }
        hipEventRecord(ev[slot][0], copy);
        const hipError_t e = hipMemcpyAsync(d_buf[slot], pinned[slot], take * rb, hipMemcpyHostToDevice, copy);
        hipEventRecord(ev[slot][1], copy);
        if (e != hipSuccess) { rc = fail(c, KATGPU_ERR_DEVICE, "jf load: %s", hipGetErrorString(e)); break; }
        hipStreamWaitEvent(c->stream, ev[slot][1], 0);
        hipEventRecord(ev[slot][2], c->stream);
        rc = jf_add_records(t, d_buf[slot], take, key_len, counter_len, &unseen);
        hipEventRecord(ev[slot][3], c->stream);
        used[slot] = true;
        pos += take;
        ++tm->chunks;
    }
    for (int i = 0; i < nbuf; ++i) { const int x = collect((slot + i) % nbuf); if (!rc) rc = x; }
    release();
    return rc ? rc : refresh_counters(t);
}

// ------------------------------------------------------------------ wide tables (33 <= k <= 63): records in and out ----

extern "C" int katgpu_table_export_wide(katgpu_table* t, uint64_t* keys_hi, uint64_t* keys_lo, uint64_t* counts, size_t cap, size_t* n_out) {
    if (!t || !n_out) return KATGPU_ERR_INVALID_ARG;
    katgpu_ctx* c = t->ctx;
    if (!t->dev().keys_b) return fail(c, KATGPU_ERR_K, "katgpu_table_export_wide is for k > 32 tables (k = %u): use katgpu_table_export", t->dev().k);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    *n_out = (size_t)t->distinct;
    if (cap == 0) return KATGPU_OK;
    if (cap < t->distinct || !keys_hi || !keys_lo || !counts) return fail(c, KATGPU_ERR_INVALID_ARG, "export buffer too small: %zu < %llu", cap, (unsigned long long)t->distinct);
    if (!t->distinct) return KATGPU_OK;
    const size_t n = (size_t)t->distinct;
    uint64_t* d = nullptr;
    HIPCHK(c, hipMalloc(&d, (3 * n + 1) * 8));
    unsigned long long* cursor = (unsigned long long*)(d + 3 * n);
    hipMemsetAsync(cursor, 0, 8, c->stream);
    hipLaunchKernelGGL(k_export_w, dim3(grid_for(c, t->dev().cap, 256, 8)), dim3(256), 0, c->stream, t->dev(), t->n_ovf, d, d + n, d + 2 * n, cursor);
    hipMemcpyAsync(keys_hi, d, n * 8, hipMemcpyDeviceToHost, c->stream);
    hipMemcpyAsync(keys_lo, d + n, n * 8, hipMemcpyDeviceToHost, c->stream);
    hipMemcpyAsync(counts, d + 2 * n, n * 8, hipMemcpyDeviceToHost, c->stream);
    hipError_t e = hipStreamSynchronize(c->stream);
    hipFree(d);
    if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "%s", hipGetErrorString(e));
    return KATGPU_OK;
}

extern "C" int katgpu_table_partition_wide(katgpu_table* t, uint32_t n_parts, const uint64_t* offsets, uint64_t* dev_hi, uint64_t* dev_lo, uint64_t* dev_counts) {
    if (!t || !offsets || n_parts == 0 || n_parts > 4096) return KATGPU_ERR_INVALID_ARG;
    katgpu_ctx* c = t->ctx;
    if (!t->dev().keys_b) return fail(c, KATGPU_ERR_K, "katgpu_table_partition_wide is for k > 32 tables (k = %u): use katgpu_table_partition", t->dev().k);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    if (t->distinct && (!dev_hi || !dev_lo || !dev_counts)) return KATGPU_ERR_INVALID_ARG;
    unsigned long long* d = nullptr;
    HIPCHK(c, hipMalloc(&d, n_parts * 8));
    hipMemcpyAsync(d, offsets, n_parts * 8, hipMemcpyHostToDevice, c->stream);
    {
        ScopedTimer tm(c, KATGPU_K_PARTITION, t->dev().cap);
        hipLaunchKernelGGL(k_partition_w<1>, dim3(grid_for(c, t->dev().cap, 256, 8)), dim3(256), 0, c->stream, t->dev(), t->n_ovf, n_parts, d, dev_hi, dev_lo, dev_counts);
    }
    hipError_t e = hipStreamSynchronize(c->stream);
    hipFree(d);
    if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "%s", hipGetErrorString(e));
    return KATGPU_OK;
}

extern "C" int katgpu_table_merge_device_wide(katgpu_table* t, const uint64_t* dev_hi, const uint64_t* dev_lo, const uint64_t* dev_counts, size_t n) {
    if (!t || (n && (!dev_hi || !dev_lo || !dev_counts))) return KATGPU_ERR_INVALID_ARG;
    katgpu_ctx* c = t->ctx;
    if (!t->dev().keys_b) return fail(c, KATGPU_ERR_K, "katgpu_table_merge_device_wide is for k > 32 tables (k = %u): use katgpu_table_merge_device", t->dev().k);
    HIPCHK(c, hipSetDevice(c->device));
    size_t pos = 0;
    while (pos < n) {
        int rc = refresh_counters(t); if (rc) return rc;
        const uint64_t room = (uint64_t)(load_limit(t->dev()) * (double)t->dev().cap) > t->distinct ? (uint64_t)(load_limit(t->dev()) * (double)t->dev().cap) - t->distinct : 0;
        const uint64_t want = n - pos;
        if (room < std::min<uint64_t>(want, std::max<uint64_t>(t->dev().cap / 8, 1024))) {
            rc = ensure_room(t, std::min<uint64_t>(want, std::max<uint64_t>(t->dev().cap / 2, 1024)));
            if (rc) return rc;
            continue;
        }
        const uint64_t take = std::min(want, room);
        ScopedTimer tm(c, KATGPU_K_MERGE, take);
        hipLaunchKernelGGL(k_merge_w, dim3(grid_for(c, take, 256, 8)), dim3(256), 0, c->stream, t->dev(), dev_hi + pos, dev_lo + pos, dev_counts + pos, (uint64_t)take);
        pos += take;
    }
    return refresh_counters(t);
}

extern "C" int katgpu_table_merge_host_wide(katgpu_table* t, const uint64_t* keys_hi, const uint64_t* keys_lo, const uint64_t* counts, size_t n) {
    if (!t || (n && (!keys_hi || !keys_lo || !counts))) return KATGPU_ERR_INVALID_ARG;
    katgpu_ctx* c = t->ctx;
    if (!t->dev().keys_b) return fail(c, KATGPU_ERR_K, "katgpu_table_merge_host_wide is for k > 32 tables (k = %u): use katgpu_table_merge_host", t->dev().k);
    if (!n) return KATGPU_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const uint32_t k = t->dev().k;
    const uint64_t hi_mask = (1ULL << (2 * k - 64)) - 1;           // 2 <= 2k - 64 <= 62
    for (size_t i = 0; i < n; ++i)
        if (keys_hi[i] & ~hi_mask) return fail(c, KATGPU_ERR_INVALID_ARG, "record %zu: key wider than 2k = %u bits", i, 2 * k);
    uint64_t* d = nullptr;
    HIPCHK(c, hipMalloc(&d, 3 * n * 8));
    hipError_t e = hipMemcpy(d, keys_hi, n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + n, keys_lo, n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + 2 * n, counts, n * 8, hipMemcpyHostToDevice);
    int rc = e == hipSuccess ? katgpu_table_merge_device_wide(t, d, d + n, d + 2 * n, n) : fail(c, KATGPU_ERR_DEVICE, "merge: %s", hipGetErrorString(e));
    hipStreamSynchronize(c->stream);
    hipFree(d);
    return rc;
}

extern "C" int katgpu_table_get_wide(katgpu_table* t, const uint64_t* keys_hi, const uint64_t* keys_lo, size_t n, int canonicalise, uint64_t* counts) {
    if (!t || (n && (!keys_hi || !keys_lo || !counts))) return KATGPU_ERR_INVALID_ARG;
    katgpu_ctx* c = t->ctx;
    if (!t->dev().keys_b) return fail(c, KATGPU_ERR_K, "katgpu_table_get_wide is for k > 32 tables (k = %u): use katgpu_table_get", t->dev().k);
    if (!n) return KATGPU_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    uint64_t* d = nullptr;
    HIPCHK(c, hipMalloc(&d, 3 * n * 8));
    hipMemcpyAsync(d, keys_hi, n * 8, hipMemcpyHostToDevice, c->stream);
    hipMemcpyAsync(d + n, keys_lo, n * 8, hipMemcpyHostToDevice, c->stream);
    hipLaunchKernelGGL(k_get_w, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, t->dev(), t->n_ovf, d, d + n, (uint64_t)n, canonicalise, d + 2 * n);
    hipMemcpyAsync(counts, d + 2 * n, n * 8, hipMemcpyDeviceToHost, c->stream);
    hipError_t e = hipStreamSynchronize(c->stream);
    hipFree(d);
    if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "%s", hipGetErrorString(e));
    return KATGPU_OK;
}


// ------------------------------------------------------------------ kat filter ----

// FilterKmer::execute + filterSlice (src/filter_kmer.cc:136-288): the reference adds the chosen k-mers of the input hash into one or two
// new hashes of the input's size.  Here the new tables take the input's capacity and region grid (as regrow does), so one pass of K9 over
// the input's slots fills them region by region, and the six counters come back from the same pass.
extern "C" int katgpu_table_filter(katgpu_table* t, uint64_t low_count, uint64_t high_count, uint32_t low_gc, uint32_t high_gc,
                                   int invert, int separate, katgpu_table** keep, katgpu_table** drop, uint64_t counters[6]) {
    if (!t || !keep || (separate && !drop) || !counters) return KATGPU_ERR_INVALID_ARG;
    *keep = nullptr;
    if (drop) *drop = nullptr;
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    const DevTable src = t->dev();
    const bool grid = src.n_regions > 1;
    katgpu_table* out[2] = {nullptr, nullptr};
    for (int i = 0; i < (separate ? 2 : 1); ++i) {
        out[i] = new katgpu_table();
        out[i]->ctx = c; out[i]->disable_grow = t->disable_grow;
        rc = alloc_dev_table(c, src.k, (int)src.canonical, src.cap, &out[i]->dv, grid ? src.p1 : 0, grid ? src.p2 : 0);
        if (rc) { delete out[i]; out[i] = nullptr; break; }
    }
    if (!rc) {
        unsigned long long* ctr = (unsigned long long*)&src.ctrs[CTR_SCRATCH];
        const FilterBox box{low_count, high_count, low_gc, high_gc};
        const DevTable& dk = out[0]->dv;
        const DevTable& dd = separate ? out[1]->dv : out[0]->dv;   // (not written without `separate`)
        const dim3 g(grid_for(c, src.cap, 256, 8));
        hipError_t e = hipMemsetAsync(ctr, 0, FC_N * sizeof(uint64_t), c->stream);
        if (e == hipSuccess) {
            if (src.keys_b && separate) hipLaunchKernelGGL(k_filter_w<true>, g, dim3(256), 0, c->stream, dk, dd, src, t->n_ovf, box, invert, ctr);
            else if (src.keys_b) hipLaunchKernelGGL(k_filter_w<false>, g, dim3(256), 0, c->stream, dk, dd, src, t->n_ovf, box, invert, ctr);
            else if (separate) hipLaunchKernelGGL(k_filter<true>, g, dim3(256), 0, c->stream, dk, dd, src, t->n_ovf, box, invert, ctr);
            else hipLaunchKernelGGL(k_filter<false>, g, dim3(256), 0, c->stream, dk, dd, src, t->n_ovf, box, invert, ctr);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(counters, ctr, FC_N * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = fail(c, KATGPU_ERR_DEVICE, "filter: %s", hipGetErrorString(e));
        for (int i = 0; i < 2 && !rc; ++i) if (out[i]) rc = refresh_counters(out[i]);
        if (!rc && (out[0]->distinct != counters[FC_KEEP_D] || (separate && out[1]->distinct != counters[FC_DROP_D])))
            rc = fail(c, KATGPU_ERR_DEVICE, "filter: the new tables hold %llu / %llu distinct k-mers, the pass routed %llu / %llu",
                      (unsigned long long)out[0]->distinct, (unsigned long long)(separate ? out[1]->distinct : 0),
                      (unsigned long long)counters[FC_KEEP_D], (unsigned long long)counters[FC_DROP_D]);
    }
    if (rc) { katgpu_table_free(out[0]); katgpu_table_free(out[1]); return rc; }
    *keep = out[0];
    if (separate) *drop = out[1];
    return KATGPU_OK;
}

static int launch_seq_hits(katgpu_table* t, const uint8_t* dev_bases, size_t n, const uint64_t* dev_start, const uint64_t* dev_len, size_t n_rec,
                           int canonicalise, uint64_t* dev_hits) {
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipMemsetAsync(dev_hits, 0, n_rec * sizeof(uint64_t), c->stream));
    const uint32_t k = t->dev().k;
    if (n < k || !n_rec) return KATGPU_OK;
    const bool wide = t->dev().keys_b != nullptr;
    const uint64_t n_out = n - k + 1;
    const uint64_t per_chunk = wide ? WIDE_CHUNK_STARTS : CHUNK_STARTS;
    const uint64_t n_chunks = (n_out + per_chunk - 1) / per_chunk;
    const int grid = (int)std::min<uint64_t>(n_chunks, (uint64_t)c->n_cu * 8);
    const bool aligned = (reinterpret_cast<uintptr_t>(dev_bases) & 15) == 0;
    unsigned long long* h = (unsigned long long*)dev_hits;
    ScopedTimer tm(c, KATGPU_K_PROFILE, n_out);
    if (wide && aligned) hipLaunchKernelGGL((k_seq_hits<true, true>), dim3(grid), dim3(COUNT_BLOCK), 0, c->stream, t->dev(), t->n_ovf, canonicalise, dev_bases, (uint64_t)n, n_chunks, dev_start, dev_len, (uint64_t)n_rec, h);
    else if (wide) hipLaunchKernelGGL((k_seq_hits<false, true>), dim3(grid), dim3(COUNT_BLOCK), 0, c->stream, t->dev(), t->n_ovf, canonicalise, dev_bases, (uint64_t)n, n_chunks, dev_start, dev_len, (uint64_t)n_rec, h);
    else if (aligned) hipLaunchKernelGGL((k_seq_hits<true, false>), dim3(grid), dim3(COUNT_BLOCK), 0, c->stream, t->dev(), t->n_ovf, canonicalise, dev_bases, (uint64_t)n, n_chunks, dev_start, dev_len, (uint64_t)n_rec, h);
    else hipLaunchKernelGGL((k_seq_hits<false, false>), dim3(grid), dim3(COUNT_BLOCK), 0, c->stream, t->dev(), t->n_ovf, canonicalise, dev_bases, (uint64_t)n, n_chunks, dev_start, dev_len, (uint64_t)n_rec, h);
    HIPCHK(c, hipGetLastError());
    return KATGPU_OK;
}

extern "C" int katgpu_table_seq_hits_device(katgpu_table* t, const uint8_t* dev_bases, size_t n, const uint64_t* dev_rec_start,
                                            const uint64_t* dev_rec_len, size_t n_rec, int canonicalise, uint64_t* dev_hits) {
    if (!t || (n_rec && (!dev_rec_start || !dev_rec_len || !dev_hits)) || (n && !dev_bases)) return KATGPU_ERR_INVALID_ARG;
    if (!n_rec) return KATGPU_OK;
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    return launch_seq_hits(t, dev_bases, n, dev_rec_start, dev_rec_len, n_rec, canonicalise, dev_hits);
}

// Host form: the records go through the device in batches of at most SEQ_HITS_BATCH bases and SEQ_HITS_RECS records (a record longer
// than that is a batch of its own), so any input fits next to the table.
extern "C" int katgpu_table_seq_hits_host(katgpu_table* t, const char* bases, size_t n, const uint64_t* rec_start, const uint64_t* rec_len,
                                          size_t n_rec, int canonicalise, uint64_t* hits) {
    if (!t || (n_rec && (!rec_start || !rec_len || !hits)) || (n && !bases)) return KATGPU_ERR_INVALID_ARG;
    if (!n_rec) return KATGPU_OK;
    katgpu_ctx* c = t->ctx;
    for (size_t r = 0; r < n_rec; ++r) {
        if (rec_start[r] > n || rec_len[r] > n - rec_start[r]) return fail(c, KATGPU_ERR_INVALID_ARG, "record %zu lies beyond the %zu bases", r, n);
        if (r && rec_start[r] < rec_start[r - 1] + rec_len[r - 1]) return fail(c, KATGPU_ERR_INVALID_ARG, "record %zu starts before record %zu ends: records must be in order and disjoint", r, r - 1);
    }
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    const size_t SEQ_HITS_BATCH = (size_t)64 << 20, SEQ_HITS_RECS = (size_t)1 << 20;
    uint8_t* db = nullptr; uint64_t* dr = nullptr;
    size_t db_bytes = 0;
    HIPCHK(c, pool_alloc(c, (void**)&dr, SEQ_HITS_RECS * 3 * sizeof(uint64_t)));
    std::vector<uint64_t> st(SEQ_HITS_RECS), ln(SEQ_HITS_RECS);
    hipError_t e = hipSuccess;
    for (size_t r0 = 0; r0 < n_rec && !rc && e == hipSuccess;) {
        const uint64_t base = rec_start[r0];
        size_t r1 = r0 + 1;
        while (r1 < n_rec && r1 - r0 < SEQ_HITS_RECS && rec_start[r1] + rec_len[r1] - base <= SEQ_HITS_BATCH) ++r1;
        const size_t nb = rec_start[r1 - 1] + rec_len[r1 - 1] - base;
        if (nb + 64 > db_bytes) {
            pool_release(c, db); db = nullptr;
            db_bytes = std::max(nb + 64, std::min(SEQ_HITS_BATCH, n) + 64);
            e = pool_alloc(c, (void**)&db, db_bytes);
            if (e != hipSuccess) { db_bytes = 0; break; }
        }
        for (size_t r = r0; r < r1; ++r) { st[r - r0] = rec_start[r] - base; ln[r - r0] = rec_len[r]; }
        const size_t m = r1 - r0;
        if (nb) e = hipMemcpyAsync(db, bases + base, nb, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(dr, st.data(), m * 8, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(dr + SEQ_HITS_RECS, ln.data(), m * 8, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) break;
        rc = launch_seq_hits(t, db, nb, dr, dr + SEQ_HITS_RECS, m, canonicalise, dr + 2 * SEQ_HITS_RECS);
        if (rc) break;
        e = hipMemcpyAsync(hits + r0, dr + 2 * SEQ_HITS_RECS, m * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        r0 = r1;
    }
    hipStreamSynchronize(c->stream);
    pool_release(c, db); pool_release(c, dr);
    if (rc) return rc;
    if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "seq hits: %s", hipGetErrorString(e));
    return KATGPU_OK;
}

// ------------------------------------------------------------------ per-record coverage statistics (kat sect -n, kat cold) ----

static const uint32_t g_stats_short = (uint32_t)std::min<uint64_t>(hook_u64("KATGPU_TEST_STATS_SHORT", RS_SHORT_WINDOWS), RS_SHORT_WINDOWS);   // tests: the short / long limit, in windows
static const size_t g_stats_batch = (size_t)std::max<uint64_t>(hook_u64("KATGPU_TEST_STATS_BATCH", (uint64_t)32 << 20), 1);                    // tests: bases per batch of the host form
static_assert(sizeof(katgpu_record_stats) == RS_FIELDS * sizeof(uint64_t), "the kernels write a record's statistics as six words");

// Everything on the stream: the result cleared, K11 over the tiles, and, when n_long records are long (long_windows windows in all),
// their slots, K12 and the eight passes of K13 over those windows.  *ws is the workspace of the long records (null: none), to be
// pool_release'd once the stream has run.  Two timed sections: the second only when there are long records.
static int launch_record_stats(katgpu_table* t, const uint8_t* dev_bases, size_t n, const uint64_t* dev_start, const uint64_t* dev_len, size_t n_rec,
                               int canonicalise, katgpu_record_stats* dev_out, uint64_t n_long, uint64_t long_windows, void** ws) {
    katgpu_ctx* c = t->ctx;
    *ws = nullptr;
    HIPCHK(c, hipMemsetAsync(dev_out, 0, n_rec * sizeof(katgpu_record_stats), c->stream));
    if (!n || !n_rec) return KATGPU_OK;
    const DevTable& d = t->dev();
    const uint32_t k = d.k;
    const bool wide = d.keys_b != nullptr;
    const bool aligned = (reinterpret_cast<uintptr_t>(dev_bases) & 15) == 0;
    const uint64_t n_out = n >= k ? n - k + 1 : 0;
    unsigned long long* o = (unsigned long long*)dev_out;
    {
        ScopedTimer tm(c, KATGPU_K_PROFILE, n_out);
        const uint64_t n_tiles = (n + RS_TILE_STRIDE - 1) / RS_TILE_STRIDE;
        const dim3 g((unsigned)std::min<uint64_t>(n_tiles, (uint64_t)c->n_cu * 8)), b(COUNT_BLOCK);
#define RS_SHORT(A, W) hipLaunchKernelGGL((k_rstats_short<A, W>), g, b, 0, c->stream, d, t->n_ovf, canonicalise, dev_bases, (uint64_t)n, n_tiles, dev_start, dev_len, (uint64_t)n_rec, g_stats_short, o)
        if (wide && aligned) RS_SHORT(true, true); else if (wide) RS_SHORT(false, true); else if (aligned) RS_SHORT(true, false); else RS_SHORT(false, false);
#undef RS_SHORT
        HIPCHK(c, hipGetLastError());
    }
    if (!n_long || !long_windows) return KATGPU_OK;
    // the long records' workspace: selection state | digit histograms | slot of every record | a count per window of a long record
    const size_t hist_off = align_up(n_long * sizeof(RsSel), 16), slot_off = hist_off + n_long * RS_DIGITS * sizeof(uint64_t);
    const size_t cnt_off = align_up(slot_off + n_rec * sizeof(uint32_t), 16), bytes = cnt_off + long_windows * sizeof(uint64_t);
    uint8_t* w = nullptr;
    if (pool_alloc(c, (void**)&w, bytes) != hipSuccess)
        return fail(c, KATGPU_ERR_NOMEM, "record statistics: no %zu bytes of device memory for the counts of %llu long records (%llu windows)", bytes,
                    (unsigned long long)n_long, (unsigned long long)long_windows);
    *ws = w;
    RsSel* sel = (RsSel*)w;
    unsigned long long* hist = (unsigned long long*)(w + hist_off);
    uint32_t* rec_slot = (uint32_t*)(w + slot_off);
    uint64_t* cnt = (uint64_t*)(w + cnt_off);
    ScopedTimer tm(c, KATGPU_K_PROFILE, 0);
    HIPCHK(c, hipMemsetAsync(w, 0, slot_off, c->stream));
    HIPCHK(c, hipMemsetAsync(rec_slot, 0xFF, n_rec * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_rstats_classify, dim3(1), dim3(RS_CLASSIFY_BLOCK), 0, c->stream, dev_len, (uint64_t)n_rec, k, g_stats_short, n_long, long_windows, rec_slot, sel);
    {
        const uint64_t per_chunk = wide ? WIDE_CHUNK_STARTS : CHUNK_STARTS;
        const uint64_t n_chunks = (n + per_chunk - 1) / per_chunk;
        const dim3 g((unsigned)std::min<uint64_t>(n_chunks, (uint64_t)c->n_cu * 8)), b(COUNT_BLOCK);
#define RS_LONG(A, W) hipLaunchKernelGGL((k_rstats_long<A, W>), g, b, 0, c->stream, d, t->n_ovf, canonicalise, dev_bases, (uint64_t)n, n_chunks, dev_start, dev_len, (uint64_t)n_rec, rec_slot, cnt, long_windows, sel, o)
        if (wide && aligned) RS_LONG(true, true); else if (wide) RS_LONG(false, true); else if (aligned) RS_LONG(true, false); else RS_LONG(false, false);
#undef RS_LONG
    }
    const uint64_t sel_chunks = (long_windows + RS_SEL_CHUNK - 1) / RS_SEL_CHUNK;
    const dim3 hg((unsigned)std::min<uint64_t>(sel_chunks, (uint64_t)c->n_cu * 8)), pg((unsigned)((n_long + 3) / 4));
    for (int shift = 56; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(k_rstats_hist, hg, dim3(256), 0, c->stream, cnt, long_windows, sel_chunks, k, dev_len, sel, n_long, (uint32_t)shift, hist);
        hipLaunchKernelGGL(k_rstats_pick, pg, dim3(256), 0, c->stream, sel, n_long, (uint32_t)shift, hist, o);
    }
    HIPCHK(c, hipGetLastError());
    return KATGPU_OK;
}

// Device form.  The number of long records and of their windows comes back from the device first (two words; refresh_counters has synchronised already);
// with none, the rest is asynchronous on the stream, otherwise the call returns when the selection's workspace has been released.
extern "C" int katgpu_table_record_stats_device(katgpu_table* t, const uint8_t* dev_bases, size_t n, const uint64_t* dev_rec_start,
                                                const uint64_t* dev_rec_len, size_t n_rec, int canonicalise, katgpu_record_stats* dev_out) {
    if (!t || (n_rec && (!dev_rec_start || !dev_rec_len || !dev_out)) || (n && !dev_bases)) return KATGPU_ERR_INVALID_ARG;
    if (!n_rec) return KATGPU_OK;
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    unsigned long long* scratch = (unsigned long long*)&t->dev().ctrs[CTR_SCRATCH];
    unsigned long long n_long[2] = {0, 0};
    HIPCHK(c, hipMemsetAsync(scratch, 0, sizeof n_long, c->stream));
    hipLaunchKernelGGL(k_rstats_count_long, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, c->stream, dev_rec_len, (uint64_t)n_rec, t->dev().k, g_stats_short, scratch);
    HIPCHK(c, hipMemcpyAsync(n_long, scratch, sizeof n_long, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    void* ws = nullptr;
    rc = launch_record_stats(t, dev_bases, n, dev_rec_start, dev_rec_len, n_rec, canonicalise, dev_out, n_long[0], n_long[1], &ws);
    if (ws) {
        const hipError_t e = hipStreamSynchronize(c->stream);
        pool_release(c, ws);
        if (!rc && e != hipSuccess) rc = fail(c, KATGPU_ERR_DEVICE, "record stats: %s", hipGetErrorString(e));
    }
    return rc;
}

// Host form: the records go through the device in batches of at most g_stats_batch bases and STATS_RECS records (a record longer than
// that is a batch of its own), so any input fits next to the table; a batch also ends where its long records would have more than
// g_stats_batch / 4 windows between them (a single record may), which bounds their count scratch by the longest record or 8 bytes x that.
// What comes back is sizeof(katgpu_record_stats) per record.
extern "C" int katgpu_table_record_stats_host(katgpu_table* t, const char* bases, size_t n, const uint64_t* rec_start, const uint64_t* rec_len,
                                              size_t n_rec, int canonicalise, katgpu_record_stats* out) {
    if (!t || (n_rec && (!rec_start || !rec_len || !out)) || (n && !bases)) return KATGPU_ERR_INVALID_ARG;
    if (!n_rec) return KATGPU_OK;
    katgpu_ctx* c = t->ctx;
    for (size_t r = 0; r < n_rec; ++r) {
        if (rec_start[r] > n || rec_len[r] > n - rec_start[r]) return fail(c, KATGPU_ERR_INVALID_ARG, "record %zu lies beyond the %zu bases", r, n);
        if (r && rec_start[r] < rec_start[r - 1] + rec_len[r - 1]) return fail(c, KATGPU_ERR_INVALID_ARG, "record %zu starts before record %zu ends: records must be in order and disjoint", r, r - 1);
    }
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    const uint32_t k = t->dev().k;
    const size_t STATS_RECS = (size_t)1 << 20;
    const size_t rec_words = 2 + RS_FIELDS;                        // start, length, the six result words
    uint8_t* db = nullptr; uint64_t* dr = nullptr;
    size_t db_bytes = 0;
    if (pool_alloc(c, (void**)&dr, std::min(n_rec, STATS_RECS) * rec_words * sizeof(uint64_t)) != hipSuccess)
        return fail(c, KATGPU_ERR_NOMEM, "record statistics: no device memory for the records of a batch");
    const size_t cap = std::min(n_rec, STATS_RECS);
    std::vector<uint64_t> st(cap), ln(cap);
    hipError_t e = hipSuccess;
    for (size_t r0 = 0; r0 < n_rec && !rc && e == hipSuccess;) {
        const uint64_t base = rec_start[r0];
        auto long_windows_of = [&](size_t r) { const uint64_t w = rec_len[r] >= k ? rec_len[r] - k + 1 : 0; return w > g_stats_short ? w : (uint64_t)0; };
        uint64_t n_long = 0, long_windows = 0;
        size_t r1 = r0;
        do {
            const uint64_t w = long_windows_of(r1);
            n_long += w != 0; long_windows += w;
            ++r1;
        } while (r1 < n_rec && r1 - r0 < STATS_RECS && rec_start[r1] + rec_len[r1] - base <= g_stats_batch &&
                 long_windows + long_windows_of(r1) <= std::max<uint64_t>(g_stats_batch / 4, 1));
        const size_t nb = rec_start[r1 - 1] + rec_len[r1 - 1] - base;
        if (nb + 64 > db_bytes) {
            pool_release(c, db); db = nullptr;
            db_bytes = std::max(nb + 64, std::min(g_stats_batch, n) + 64);
            if (pool_alloc(c, (void**)&db, db_bytes) != hipSuccess) { db_bytes = 0; rc = fail(c, KATGPU_ERR_NOMEM, "record statistics: no %zu bytes of device memory for a batch of bases", nb + 64); break; }
        }
        for (size_t r = r0; r < r1; ++r) { st[r - r0] = rec_start[r] - base; ln[r - r0] = rec_len[r]; }
        const size_t m = r1 - r0;
        katgpu_record_stats* d_out = (katgpu_record_stats*)(dr + 2 * cap);
        if (nb) e = hipMemcpyAsync(db, bases + base, nb, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(dr, st.data(), m * 8, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(dr + cap, ln.data(), m * 8, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) break;
        void* ws = nullptr;
        rc = launch_record_stats(t, db, nb, dr, dr + cap, m, canonicalise, d_out, n_long, long_windows, &ws);
        if (!rc) e = hipMemcpyAsync(out + r0, d_out, m * sizeof(katgpu_record_stats), hipMemcpyDeviceToHost, c->stream);
        const hipError_t es = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = es;
        pool_release(c, ws);
        r0 = r1;
    }
    hipStreamSynchronize(c->stream);
    pool_release(c, db); pool_release(c, dr);
    if (rc) return rc;
    if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "record stats: %s", hipGetErrorString(e));
    return KATGPU_OK;
}
