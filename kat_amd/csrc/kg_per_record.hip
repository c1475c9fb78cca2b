// kg_per_record.hip -- what `katgpu sect` and `cold` ask of a table per record of a sequence file: the coverage statistics of `sect -n` and
// `cold` (katgpu_table_record_stats_*), the count-range regions of `sect -E / -F` (katgpu_table_record_regions_*), the -counts.cvg text
// of `sect` (katgpu_table_record_cvg_text_*) and the -counts.gc text of `sect -g` (katgpu_record_gc_text_*: bases only, no table).
// Every call has a device form and a host form; the host forms send their records through the device in batches (for_record_batches).
// The statistics and regions also read their counts from a dense array instead of a table (katgpu_record_*_from_counts_device: device
// forms only), which is how they are made of a table that lies on several ranks (katgpu_table_record_stats_gathered_host, on
// kg_query.hip's gather: kg_comm.hpp).
#include "kg_comm.hpp"
#include "kg_record_stats.hpp"
#include "kg_record_regions.hpp"
#include "kg_cvg_text.hpp"
#include "kg_gc_text.hpp"

// ------------------------------------------------------------------ per-record coverage statistics (kat sect -n, kat cold) ----

static const uint32_t g_stats_short = (uint32_t)std::min<uint64_t>(hook_u64("KATGPU_TEST_STATS_SHORT", RS_SHORT_WINDOWS), RS_SHORT_WINDOWS);   // tests: the short / long limit, in windows
static const size_t g_stats_batch = (size_t)std::max<uint64_t>(hook_u64("KATGPU_TEST_STATS_BATCH", (uint64_t)32 << 20), 1);                    // tests: bases per batch of the host form
static_assert(sizeof(katgpu_record_stats) == RS_FIELDS * sizeof(uint64_t), "the kernels write a record's statistics as six words");

// Everything on the stream: the result cleared, K11 over the tiles, and, when n_long records are long (long_windows windows in all),
// their slots, K12 and the eight passes of K13 over those windows.  ws takes the workspace of the long records (none: left empty), to be
// let go once the stream has run.  Two timed sections: the second only when there are long records.
// src: where the counts come from (kg_record_stats.hpp), of k-mers of length k.
template <typename Src>
static int launch_record_stats(katgpu_ctx* c, const Src& src, uint32_t k, bool wide, const uint8_t* dev_bases, size_t n, const uint64_t* dev_start, const uint64_t* dev_len,
                               size_t n_rec, katgpu_record_stats* dev_out, uint64_t n_long, uint64_t long_windows, DevBuf& ws) {
    ws.reset();
    HIPCHK(c, hipMemsetAsync(dev_out, 0, n_rec * sizeof(katgpu_record_stats), c->stream));
    if (!n || !n_rec) return KATGPU_OK;
    const bool aligned = aligned16(dev_bases);
    const uint64_t n_out = n >= k ? n - k + 1 : 0;
    unsigned long long* o = (unsigned long long*)dev_out;
    {
        ScopedTimer tm(c, KATGPU_K_PROFILE, n_out);
        launch_aligned_wide(c, aligned, wide, n, RS_TILE_STRIDE, [&](auto A, auto W, dim3 grid, uint64_t n_tiles) {
            hipLaunchKernelGGL((k_rstats_short<decltype(A)::value, decltype(W)::value, Src>), grid, dim3(COUNT_BLOCK), 0, c->stream, src, dev_bases, (uint64_t)n, n_tiles, dev_start, dev_len, (uint64_t)n_rec, g_stats_short, o);
        });
        HIPCHK(c, hipGetLastError());
    }
    if (!n_long || !long_windows) return KATGPU_OK;
    // the long records' workspace: selection state | digit histograms | slot of every record | a count per window of a long record
    const size_t hist_off = align_up(n_long * sizeof(RsSel), 16), slot_off = hist_off + n_long * RS_DIGITS * sizeof(uint64_t);
    const size_t cnt_off = align_up(slot_off + n_rec * sizeof(uint32_t), 16), bytes = cnt_off + long_windows * sizeof(uint64_t);
    if (ws.pooled(c, bytes) != hipSuccess)
        return fail(c, KATGPU_ERR_NOMEM, "record statistics: no %zu bytes of device memory for the counts of %llu long records (%llu windows)", bytes,
                    (unsigned long long)n_long, (unsigned long long)long_windows);
    uint8_t* w = ws.as<uint8_t>();
    RsSel* sel = (RsSel*)w;
    unsigned long long* hist = (unsigned long long*)(w + hist_off);
    uint32_t* rec_slot = (uint32_t*)(w + slot_off);
    uint64_t* cnt = (uint64_t*)(w + cnt_off);
    ScopedTimer tm(c, KATGPU_K_PROFILE, 0);
    HIPCHK(c, hipMemsetAsync(w, 0, slot_off, c->stream));
    HIPCHK(c, hipMemsetAsync(rec_slot, 0xFF, n_rec * sizeof(uint32_t), c->stream));
    hipLaunchKernelGGL(k_rstats_classify, dim3(1), dim3(RS_CLASSIFY_BLOCK), 0, c->stream, dev_len, (uint64_t)n_rec, k, g_stats_short, n_long, long_windows, rec_slot, sel);
    launch_aligned_wide(c, aligned, wide, n, chunk_starts(wide), [&](auto A, auto W, dim3 grid, uint64_t n_chunks) {
        hipLaunchKernelGGL((k_rstats_long<decltype(A)::value, decltype(W)::value, Src>), grid, dim3(COUNT_BLOCK), 0, c->stream, src, dev_bases, (uint64_t)n, n_chunks, dev_start, dev_len, (uint64_t)n_rec, rec_slot, cnt, long_windows, sel, o);
    });
    const uint64_t sel_chunks = (long_windows + RS_SEL_CHUNK - 1) / RS_SEL_CHUNK;
    const dim3 hg((unsigned)std::min<uint64_t>(sel_chunks, (uint64_t)c->n_cu * 8)), pg((unsigned)((n_long + 3) / 4));
    for (int shift = 56; shift >= 0; shift -= 8) {
        hipLaunchKernelGGL(k_rstats_hist, hg, dim3(256), 0, c->stream, cnt, long_windows, sel_chunks, k, dev_len, sel, n_long, (uint32_t)shift, hist);
        hipLaunchKernelGGL(k_rstats_pick, pg, dim3(256), 0, c->stream, sel, n_long, (uint32_t)shift, hist, o);
    }
    HIPCHK(c, hipGetLastError());
    return KATGPU_OK;
}

static CountsTable counts_of(katgpu_table* t, int canonicalise) { return CountsTable{t->dev(), t->n_ovf, canonicalise}; }
static bool is_wide(const katgpu_table* t) { return t->dv.keys_b != nullptr; }
// a dense array of counts as a source: the window kernels cut their chunks by the key width of k
static CountsDense counts_of(const uint64_t* dev_counts, size_t n, uint32_t k) { return CountsDense{dev_counts, n >= k ? (uint64_t)(n - k + 1) : 0, k}; }
static int counts_check(katgpu_ctx* c, const char* what, uint32_t k, const uint64_t* dev_counts) {
    if (k < 1 || k > KATGPU_MAX_K) return fail(c, KATGPU_ERR_K, "%s: k = %u unsupported (1 <= k <= %d)", what, k, KATGPU_MAX_K);
    if (reinterpret_cast<uintptr_t>(dev_counts) & 7) return fail(c, KATGPU_ERR_INVALID_ARG, "%s: the counts are not 8-byte aligned", what);
    return KATGPU_OK;
}

// The number of long records and of their windows from the device (two words, through `scratch`), then launch_record_stats; with none, the
// rest is asynchronous on the stream, otherwise the call returns when the selection's workspace has been released.
template <typename Src>
static int record_stats_device(katgpu_ctx* c, const Src& src, uint32_t k, bool wide, unsigned long long* scratch, const uint8_t* dev_bases, size_t n,
                               const uint64_t* dev_rec_start, const uint64_t* dev_rec_len, size_t n_rec, katgpu_record_stats* dev_out) {
    unsigned long long n_long[2] = {0, 0};
    HIPCHK(c, hipMemsetAsync(scratch, 0, sizeof n_long, c->stream));
    hipLaunchKernelGGL(k_rstats_count_long, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, c->stream, dev_rec_len, (uint64_t)n_rec, k, g_stats_short, scratch);
    HIPCHK(c, hipMemcpyAsync(n_long, scratch, sizeof n_long, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    DevBuf ws;
    int rc = launch_record_stats(c, src, k, wide, dev_bases, n, dev_rec_start, dev_rec_len, n_rec, dev_out, n_long[0], n_long[1], ws);
    if (ws.p) {
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (!rc && e != hipSuccess) rc = fail(c, KATGPU_ERR_DEVICE, "record stats: %s", hipGetErrorString(e));
    }
    return rc;
}

// Device form (refresh_counters has synchronised already; the two words are two of the table's counters).
extern "C" int katgpu_table_record_stats_device(katgpu_table* t, const uint8_t* dev_bases, size_t n, const uint64_t* dev_rec_start,
                                                const uint64_t* dev_rec_len, size_t n_rec, int canonicalise, katgpu_record_stats* dev_out) {
    if (!t || !records_usable(dev_bases, n, dev_rec_start, dev_rec_len, n_rec) || (n_rec && !dev_out)) return KATGPU_ERR_INVALID_ARG;
    if (!n_rec) return KATGPU_OK;
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    return record_stats_device(c, counts_of(t, canonicalise), t->dev().k, is_wide(t), (unsigned long long*)&t->dev().ctrs[CTR_SCRATCH], dev_bases, n,
                               dev_rec_start, dev_rec_len, n_rec, dev_out);
}

// The same from a dense array of counts: no table, so a context and k, as katgpu_record_gc_text_device takes them.
extern "C" int katgpu_record_stats_from_counts_device(katgpu_ctx* c, uint32_t k, const uint8_t* dev_bases, size_t n, const uint64_t* dev_counts,
                                                      const uint64_t* dev_rec_start, const uint64_t* dev_rec_len, size_t n_rec, katgpu_record_stats* dev_out) {
    if (!c || !records_usable(dev_bases, n, dev_rec_start, dev_rec_len, n_rec) || (n_rec && !dev_out)) return KATGPU_ERR_INVALID_ARG;
    int rc = counts_check(c, "record stats from counts", k, dev_counts); if (rc) return rc;
    if (n >= k && !dev_counts) return KATGPU_ERR_INVALID_ARG;
    if (!n_rec) return KATGPU_OK;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf two;                                                    // (a table form borrows two of its table's counters for this)
    if (two.pooled(c, 16) != hipSuccess) { (void)hipGetLastError(); return fail(c, KATGPU_ERR_NOMEM, "record stats from counts: no device memory"); }
    return record_stats_device(c, counts_of(dev_counts, n, k), k, k > 32, two.as<unsigned long long>(), dev_bases, n, dev_rec_start, dev_rec_len, n_rec, dev_out);
}

// Where a batch of the host form (and of the gathered one) ends beside for_record_batches' two limits: the long records of the batch being cut
constexpr size_t STATS_RECS = (size_t)1 << 20;
struct StatsJoins {
    const uint64_t* rec_len; uint32_t k;
    uint64_t n_long = 0, long_windows = 0;
    bool operator()(size_t r, bool first) {
        if (first) n_long = long_windows = 0;
        uint64_t w = rec_len[r] >= k ? rec_len[r] - k + 1 : 0;
        if (w <= g_stats_short) w = 0;
        if (!first && long_windows + w > std::max<uint64_t>(g_stats_batch / 4, 1)) return false;
        n_long += w != 0; long_windows += w;
        return true;
    }
};

// Host form: the records go through the device in batches of at most g_stats_batch bases and STATS_RECS records (for_record_batches),
// so any input fits next to the table; a batch also ends where its long records would have more than
// g_stats_batch / 4 windows between them (a single record may), which bounds their count scratch by the longest record or 8 bytes x that.
// What comes back is sizeof(katgpu_record_stats) per record.
extern "C" int katgpu_table_record_stats_host(katgpu_table* t, const char* bases, size_t n, const uint64_t* rec_start, const uint64_t* rec_len,
                                              size_t n_rec, int canonicalise, katgpu_record_stats* out) {
    if (!t || !records_usable(bases, n, rec_start, rec_len, n_rec) || (n_rec && !out)) return KATGPU_ERR_INVALID_ARG;
    if (!n_rec) return KATGPU_OK;
    katgpu_ctx* c = t->ctx;
    int rc = check_records(c, rec_start, rec_len, n_rec, n); if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = refresh_counters(t); if (rc) return rc;
    const uint32_t k = t->dev().k;
    const size_t cap = std::min(n_rec, STATS_RECS);                // records per batch
    DevBuf ws;                                                     // the long records' workspace
    StatsJoins joins{rec_len, k};
    return for_record_batches(c, bases, n, rec_start, rec_len, n_rec, g_stats_batch, cap, RS_FIELDS, "record stats", "record statistics", joins,   // (a record's six result words)
                              [&](const uint8_t* db, size_t nb, const uint64_t* ds, const uint64_t* dl, size_t m, size_t r0, uint64_t* words) {
        katgpu_record_stats* d_out = (katgpu_record_stats*)words;
        int rc = launch_record_stats(c, counts_of(t, canonicalise), k, is_wide(t), db, nb, ds, dl, m, d_out, joins.n_long, joins.long_windows, ws);
        if (rc) return rc;
        const hipError_t e = hipMemcpyAsync(out + r0, d_out, m * sizeof(katgpu_record_stats), hipMemcpyDeviceToHost, c->stream);
        return e == hipSuccess ? KATGPU_OK : fail(c, KATGPU_ERR_DEVICE, "record stats: %s", hipGetErrorString(e));
    });
}

// ------------------------------------------------------------------ count-range regions of records (kat sect -n -E / -F) ----

static const size_t g_regions_batch = (size_t)std::max<uint64_t>(hook_u64("KATGPU_TEST_REGIONS_BATCH", (uint64_t)32 << 20), 1);   // tests: bases per batch of the host form
static_assert(sizeof(katgpu_region) == RG_FIELDS * sizeof(uint64_t), "the kernels write a region as three words");

// the workspace of one call or batch of n bases: first-window mask | a mask per range | two counters per range and mask block | a total per range
struct RegionsWork {
    DevBuf buf;
    uint64_t n_words = 0, n_blk = 0;
    uint64_t* masks = nullptr;
    unsigned long long *cnt = nullptr, *totals = nullptr;
    int fit(katgpu_ctx* c, size_t n, uint32_t n_ranges) {
        n_words = (n + 63) / 64; n_blk = (n_words + RG_BLOCK - 1) / RG_BLOCK;
        const size_t cnt_off = (1 + n_ranges) * n_words * 8, tot_off = cnt_off + n_ranges * n_blk * 16, need = tot_off + RG_MAX_RANGES * 8;
        if (buf.fit(c, need) != hipSuccess) return fail(c, KATGPU_ERR_NOMEM, "record regions: no %zu bytes of device memory for the masks of %zu bases", need, n);
        uint8_t* w = buf.as<uint8_t>();
        masks = (uint64_t*)w; cnt = (unsigned long long*)(w + cnt_off); totals = (unsigned long long*)(w + tot_off);
        return KATGPU_OK;
    }
};

static bool regions_args(const katgpu_count_range* ranges, uint32_t n_ranges, RgRanges& rg) {
    if (!ranges || n_ranges < 1 || n_ranges > RG_MAX_RANGES) return false;
    rg = RgRanges{{0, 0}, {0, 0}, n_ranges};
    for (uint32_t q = 0; q < n_ranges; ++q) { rg.min[q] = ranges[q].min; rg.max[q] = ranges[q].max; }
    return true;
}

// On the stream: K14 over the chunks of the n bases (n != 0), K15 and K16 over the masks; w.totals then holds the regions of every range.
template <typename Src>
static int launch_regions_find(katgpu_ctx* c, const Src& src, uint32_t k, bool wide, const uint8_t* dev_bases, size_t n, const uint64_t* dev_start,
                               const uint64_t* dev_len, size_t n_rec, const RgRanges& rg, RegionsWork& w) {
    ScopedTimer tm(c, KATGPU_K_PROFILE, n >= k ? n - k + 1 : 0);
    launch_aligned_wide(c, aligned16(dev_bases), wide, w.n_words * 64, chunk_starts(wide), [&](auto A, auto W, dim3 grid, uint64_t n_chunks) {
        hipLaunchKernelGGL((k_regions_mask<decltype(A)::value, decltype(W)::value, Src>), grid, dim3(COUNT_BLOCK), 0, c->stream, src, dev_bases, (uint64_t)n, n_chunks, dev_start, dev_len, (uint64_t)n_rec, rg, w.n_words, (uint16_t*)w.masks);
    });
    const dim3 grid((unsigned)std::min<uint64_t>(w.n_blk, (uint64_t)c->n_cu * 8));
    hipLaunchKernelGGL(k_regions_count, grid, dim3(RG_BLOCK), 0, c->stream, w.masks, w.n_words, w.n_blk, rg.n, w.cnt);
    hipLaunchKernelGGL(k_regions_scan, dim3(1), dim3(RG_SCAN_BLOCK), 0, c->stream, w.cnt, w.n_blk, rg.n, w.totals);
    HIPCHK(c, hipGetLastError());
    return KATGPU_OK;
}

// K17 behind it: the first `cap` regions to dev_regions, their records numbered from rec_base
static int launch_regions_emit(katgpu_ctx* c, const uint64_t* dev_start, const uint64_t* dev_len, size_t n_rec, uint64_t rec_base, const RgRanges& rg,
                               const RegionsWork& w, katgpu_region* dev_regions, size_t cap) {
    if (!cap) return KATGPU_OK;
    ScopedTimer tm(c, KATGPU_K_PROFILE, 0);
    const dim3 grid((unsigned)std::min<uint64_t>(w.n_blk, (uint64_t)c->n_cu * 8));
    hipLaunchKernelGGL(k_regions_emit, grid, dim3(RG_BLOCK), 0, c->stream, w.masks, w.n_words, w.n_blk, rg.n, w.cnt, dev_start, dev_len, (uint64_t)n_rec, rec_base, (unsigned long long*)dev_regions, (uint64_t)cap);
    HIPCHK(c, hipGetLastError());
    return KATGPU_OK;
}

// K14 - K17 over one buffer, and the true totals back
template <typename Src>
static int record_regions_device(katgpu_ctx* c, const Src& src, uint32_t k, bool wide, const uint8_t* dev_bases, size_t n, const uint64_t* dev_rec_start,
                                 const uint64_t* dev_rec_len, size_t n_rec, const RgRanges& rg, katgpu_region* dev_regions, size_t cap, size_t n_out[]) {
    RegionsWork w;
    int rc = w.fit(c, n, rg.n); if (rc) return rc;
    rc = launch_regions_find(c, src, k, wide, dev_bases, n, dev_rec_start, dev_rec_len, n_rec, rg, w);
    if (!rc) rc = launch_regions_emit(c, dev_rec_start, dev_rec_len, n_rec, 0, rg, w, dev_regions, cap);
    if (rc) return rc;                                             // (w waits for the stream before it lets its block go)
    unsigned long long totals[RG_MAX_RANGES] = {0, 0};
    rc = read_totals(c, w.totals, rg.n, "record regions", totals); if (rc) return rc;
    for (uint32_t q = 0; q < rg.n; ++q) n_out[q] = (size_t)totals[q];
    return KATGPU_OK;
}

extern "C" int katgpu_table_record_regions_device(katgpu_table* t, const uint8_t* dev_bases, size_t n, const uint64_t* dev_rec_start,
                                                  const uint64_t* dev_rec_len, size_t n_rec, int canonicalise, const katgpu_count_range* ranges,
                                                  uint32_t n_ranges, katgpu_region* dev_regions, size_t cap, size_t n_out[]) {
    RgRanges rg;
    if (!t || !n_out || !records_usable(dev_bases, n, dev_rec_start, dev_rec_len, n_rec) || (cap && !dev_regions)) return KATGPU_ERR_INVALID_ARG;
    katgpu_ctx* c = t->ctx;
    if (!regions_args(ranges, n_ranges, rg)) return fail(c, KATGPU_ERR_INVALID_ARG, "record regions: one or two count ranges, not %u", ranges ? n_ranges : 0);
    for (uint32_t q = 0; q < n_ranges; ++q) n_out[q] = 0;
    if (!n_rec || !n) return KATGPU_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    return record_regions_device(c, counts_of(t, canonicalise), t->dev().k, is_wide(t), dev_bases, n, dev_rec_start, dev_rec_len, n_rec, rg, dev_regions, cap, n_out);
}

// The same from a dense array of counts (katgpu_record_stats_from_counts_device).
extern "C" int katgpu_record_regions_from_counts_device(katgpu_ctx* c, uint32_t k, const uint8_t* dev_bases, size_t n, const uint64_t* dev_counts,
                                                        const uint64_t* dev_rec_start, const uint64_t* dev_rec_len, size_t n_rec,
                                                        const katgpu_count_range* ranges, uint32_t n_ranges, katgpu_region* dev_regions, size_t cap, size_t n_out[]) {
    RgRanges rg;
    if (!c || !n_out || !records_usable(dev_bases, n, dev_rec_start, dev_rec_len, n_rec) || (cap && !dev_regions)) return KATGPU_ERR_INVALID_ARG;
    int rc = counts_check(c, "record regions from counts", k, dev_counts); if (rc) return rc;
    if (n >= k && !dev_counts) return KATGPU_ERR_INVALID_ARG;
    if (!regions_args(ranges, n_ranges, rg)) return fail(c, KATGPU_ERR_INVALID_ARG, "record regions: one or two count ranges, not %u", ranges ? n_ranges : 0);
    for (uint32_t q = 0; q < n_ranges; ++q) n_out[q] = 0;
    if (!n_rec || !n) return KATGPU_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return record_regions_device(c, counts_of(dev_counts, n, k), k, k > 32, dev_bases, n, dev_rec_start, dev_rec_len, n_rec, rg, dev_regions, cap, n_out);
}

// One batch of a host form: the totals come back first, then room for that many regions is found (out) and K17 fills it; the copies to
// found[] are queued on the stream (the vectors grow before that and rest until the batch's synchronize).
template <typename Src>
static int regions_batch(katgpu_ctx* c, const Src& src, uint32_t k, bool wide, const uint8_t* db, size_t nb, const uint64_t* ds, const uint64_t* dl, size_t m,
                         size_t r0, const RgRanges& rg, RegionsWork& w, DevBuf& out, std::vector<katgpu_region> (&found)[RG_MAX_RANGES]) {
    if (!nb) return KATGPU_OK;
    int rc = w.fit(c, nb, rg.n); if (rc) return rc;
    rc = launch_regions_find(c, src, k, wide, db, nb, ds, dl, m, rg, w); if (rc) return rc;
    unsigned long long totals[RG_MAX_RANGES] = {0, 0};
    rc = read_totals(c, w.totals, rg.n, "record regions", totals); if (rc) return rc;
    const size_t total = (size_t)(totals[0] + totals[1]);
    if (!total) return KATGPU_OK;
    if (out.fit(c, total * sizeof(katgpu_region)) != hipSuccess)
        return fail(c, KATGPU_ERR_NOMEM, "record regions: no %zu bytes of device memory for the %zu regions of a batch", total * sizeof(katgpu_region), total);
    katgpu_region* d_out = out.as<katgpu_region>();
    rc = launch_regions_emit(c, ds, dl, m, r0, rg, w, d_out, total); if (rc) return rc;
    hipError_t e = hipSuccess;
    for (uint32_t q = 0; q < rg.n && e == hipSuccess; ++q) {
        const size_t have = found[q].size();
        found[q].resize(have + (size_t)totals[q]);
        if (totals[q]) e = hipMemcpyAsync(found[q].data() + have, d_out + (q ? totals[0] : 0), (size_t)totals[q] * sizeof(katgpu_region), hipMemcpyDeviceToHost, c->stream);
    }
    return e == hipSuccess ? KATGPU_OK : fail(c, KATGPU_ERR_DEVICE, "record regions: %s", hipGetErrorString(e));
}

// the regions of a host form, range after range, in one block for katgpu_free_host
static int regions_result(katgpu_ctx* c, const std::vector<katgpu_region> (&found)[RG_MAX_RANGES], uint32_t n_ranges, katgpu_region** regions, size_t n_out[]) {
    const size_t total = found[0].size() + found[1].size();
    katgpu_region* res = (katgpu_region*)malloc(std::max<size_t>(total, 1) * sizeof(katgpu_region));
    if (!res) return fail(c, KATGPU_ERR_NOMEM, "record regions: no host memory for %zu regions", total);
    size_t at = 0;
    for (uint32_t q = 0; q < n_ranges; ++q) {
        if (!found[q].empty()) memcpy(res + at, found[q].data(), found[q].size() * sizeof(katgpu_region));
        at += found[q].size(); n_out[q] = found[q].size();
    }
    *regions = res;
    return KATGPU_OK;
}

// Host form: the records go through the device in batches of at most g_regions_batch bases and 2^20 records (for_record_batches), so any
// input fits next to the table.  Per batch the totals come back first, then room for that many regions is found and K17 fills it; the
// regions of a batch carry the records' indices in the whole call.
extern "C" int katgpu_table_record_regions_host(katgpu_table* t, const char* bases, size_t n, const uint64_t* rec_start, const uint64_t* rec_len,
                                                size_t n_rec, int canonicalise, const katgpu_count_range* ranges, uint32_t n_ranges,
                                                katgpu_region** regions, size_t n_out[]) {
    RgRanges rg;
    if (!t || !regions || !n_out || !records_usable(bases, n, rec_start, rec_len, n_rec)) return KATGPU_ERR_INVALID_ARG;
    katgpu_ctx* c = t->ctx;
    if (!regions_args(ranges, n_ranges, rg)) return fail(c, KATGPU_ERR_INVALID_ARG, "record regions: one or two count ranges, not %u", ranges ? n_ranges : 0);
    *regions = nullptr;
    for (uint32_t q = 0; q < n_ranges; ++q) n_out[q] = 0;
    std::vector<katgpu_region> found[RG_MAX_RANGES];
    if (n_rec) {
        int rc = check_records(c, rec_start, rec_len, n_rec, n); if (rc) return rc;
        HIPCHK(c, hipSetDevice(c->device));
        rc = refresh_counters(t); if (rc) return rc;
        DevBuf out;                                                // the regions of a batch
        RegionsWork w;
        rc = for_record_batches(c, bases, n, rec_start, rec_len, n_rec, g_regions_batch, std::min(n_rec, (size_t)1 << 20), 0, "record regions", "record regions",
                                [](size_t, bool) { return true; },
                                [&](const uint8_t* db, size_t nb, const uint64_t* ds, const uint64_t* dl, size_t m, size_t r0, uint64_t*) {
            return regions_batch(c, counts_of(t, canonicalise), t->dev().k, is_wide(t), db, nb, ds, dl, m, r0, rg, w, out, found);
        });
        if (rc) return rc;
    }
    return regions_result(c, found, n_ranges, regions, n_out);
}

// ------------------------------------------------------------------ both, of a table that lies on several ranks ----

// Collective, after katgpu_exchange_merge: every rank walks the same records in the batches of katgpu_table_record_stats_host (StatsJoins).
// Per record batch the gather of katgpu_table_profile_gathered_host (kg_comm.hpp: ProfileGather) runs over the batch's bases, which are
// on every rank's device already, and leaves the dense counts of its window starts in one array on rank 0's device; rank 0 then runs the
// statistics kernels and, with ranges, the region kernels from that array (CountsDense) -- what comes back is 48 bytes per record and 24 per
// region, none per position -- and the other ranks run nothing more.  The batches are cut from the records, so the ranks first make sure
// that they hold the same ones.
// From the pool: for_record_batches' buffers (start, length and statistics per record, the batch's bases) and the gather's run (12 bytes
// per window start of a gather batch) on every rank; on rank 0 the dense counts, 8 bytes per base of a record batch, and what the two host
// forms take (the long records' workspace, the masks and regions of a batch).  The run and the dense counts are allocated before any work
// and agreed on; a rank that finds no room for the rest fails inside the batches, where comm_agree_done hears of it.
extern "C" int katgpu_table_record_stats_gathered_host(katgpu_comm* comm, katgpu_table* t, const char* bases, size_t n, const uint64_t* rec_start,
                                                       const uint64_t* rec_len, size_t n_rec, int canonicalise, const katgpu_count_range* ranges,
                                                       uint32_t n_ranges, katgpu_record_stats* stats, katgpu_region** regions, size_t n_out[]) {
    if (!comm || !t) return KATGPU_ERR_INVALID_ARG;
    katgpu_ctx* c = t->ctx;
    const int rank = katgpu_comm_rank(comm), world = katgpu_comm_world(comm);
    const uint32_t k = t->dv.k;
    RgRanges rg{{0, 0}, {0, 0}, 0};
    // ---- the same records and ranges, one k and usable pointers everywhere, before anything else: all ranks go on, or none does ----
    const bool unusable = !records_usable(bases, n, rec_start, rec_len, n_rec) || n_ranges > RG_MAX_RANGES || (n_ranges && !ranges) ||
                          (rank == 0 && ((n_rec && !stats) || (n_ranges && (!regions || !n_out))));
    uint64_t range_words[1 + 2 * RG_MAX_RANGES] = {n_ranges, 0, 0, 0, 0};          // n_ranges | min and max of every range
    if (!unusable) { regions_args(ranges, n_ranges, rg); for (uint32_t q = 0; q < n_ranges; ++q) { range_words[1 + 2 * q] = rg.min[q]; range_words[2 + 2 * q] = rg.max[q]; } }
    const CallRecords recs{rec_start, rec_len, n_rec};
    const CallWords range_call{range_words, 1 + 2 * RG_MAX_RANGES, "count ranges are not rank 0's"};
    int rc = comm_agree_on_call(comm, c, "record stats gathered", n, k, &recs, unusable, "was given no bases, no records or more than two ranges, or rank 0 no room for the results", &range_call);
    if (rc) return rc;
    if (rank == 0 && n_ranges) { *regions = nullptr; for (uint32_t q = 0; q < n_ranges; ++q) n_out[q] = 0; }
    std::vector<katgpu_region> found[RG_MAX_RANGES];
    if (!n_rec) return rank == 0 && n_ranges ? regions_result(c, found, n_ranges, regions, n_out) : KATGPU_OK;
    rc = check_records(c, rec_start, rec_len, n_rec, n); if (rc) return rc;          // (the same records everywhere: the same answer)
    // ---- the batches as they will be cut (a StatsJoins of their own): the most bases of one, and whether any reaches k bases ----
    const size_t cap = std::min(n_rec, STATS_RECS);
    const size_t max_nb = record_batches_max_bases(rec_start, rec_len, n_rec, g_stats_batch, cap, StatsJoins{rec_len, k});
    const bool gathers = max_nb >= k;
    ProfileGather g{comm, t, canonicalise};
    DevBuf dense;                                                  // rank 0: the counts of a record batch's window starts
    auto prepare = [&]() -> int {
        if (!gathers) { HIPCHK(c, hipSetDevice(c->device)); return refresh_counters(t); }
        int rc = g.prepare(max_nb - k + 1, false, false); if (rc) return rc;
        if (rank == 0 && dense.pooled(c, (max_nb - k + 1) * sizeof(uint64_t)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, KATGPU_ERR_NOMEM, "record stats gathered: no %zu bytes of device memory for the counts of a batch of %zu bases", (max_nb - k + 1) * sizeof(uint64_t), max_nb);
        }
        return KATGPU_OK;
    };
    rc = comm_agree_to_start(comm, prepare(), gathered_peer_error(comm, c, "record stats gathered", "a batch of %zu bases", max_nb));
    if (rc) return rc;

    // ---- the batches.  From here on a rank that fails raises the communicator's abort flag: its peers' waits end (comm_agree_done) ----
    uint64_t n_batches = 0;
    DevBuf ws, out;                                                // the long records' workspace | the regions of a batch
    RegionsWork w;
    StatsJoins joins{rec_len, k};
    rc = for_record_batches(c, bases, n, rec_start, rec_len, n_rec, g_stats_batch, cap, RS_FIELDS, "record stats gathered", "record stats gathered", joins,
                            [&](const uint8_t* db, size_t nb, const uint64_t* ds, const uint64_t* dl, size_t m, size_t r0, uint64_t* words) -> int {
        uint64_t* d_counts = dense.as<uint64_t>();
        int rc = g.gather(nullptr, db, nb, nullptr, d_counts); if (rc) return rc;
        ++n_batches;
        if (rank != 0) return KATGPU_OK;
        katgpu_record_stats* d_out = (katgpu_record_stats*)words;
        const CountsDense src = counts_of(d_counts, nb, k);
        rc = launch_record_stats(c, src, k, k > 32, db, nb, ds, dl, m, d_out, joins.n_long, joins.long_windows, ws); if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(stats + r0, d_out, m * sizeof(katgpu_record_stats), hipMemcpyDeviceToHost, c->stream));
        return n_ranges ? regions_batch(c, src, k, k > 32, db, nb, ds, dl, m, r0, rg, w, out, found) : KATGPU_OK;
    });
    rc = comm_agree_done(comm, rc, "record stats gathered: rank %d failed");
    if (rc) return rc;
    if (g.n_batches) g.print_timing();
    if (rank != 0) return KATGPU_OK;
    if (n_ranges) { rc = regions_result(c, found, n_ranges, regions, n_out); if (rc) return rc; }
    if (g_timing) {
        const uint64_t n_regions = found[0].size() + found[1].size();
        fprintf(stderr, "katgpu_timing {\"phase\": \"record_stats_gathered\", \"batches\": %llu, \"ranks\": %d, \"records\": %llu, \"regions\": %llu, \"back_bytes\": %llu}\n",
                (unsigned long long)n_batches, world, (unsigned long long)n_rec, (unsigned long long)n_regions,
                (unsigned long long)(sizeof(katgpu_record_stats) * n_rec + sizeof(katgpu_region) * n_regions));
    }
    return KATGPU_OK;
}

// ------------------------------------------------------------------ the text of records: -counts.cvg (kat sect) and -counts.gc (kat sect -g) ----

static const size_t g_cvg_batch = (size_t)std::max<uint64_t>(hook_u64("KATGPU_TEST_CVG_BATCH", (uint64_t)32 << 20), 1);   // tests: bases per batch of the host form
static const size_t g_gc_batch = (size_t)std::max<uint64_t>(hook_u64("KATGPU_TEST_GC_BATCH", (uint64_t)32 << 20), 1);     // tests: bases per batch of the host form

// the workspace of one call or batch of n bases and n_rec records: (the source's own counts_bytes: cvg's count per window start) | a sum per tile |
// the window-less records' bytes before every record | the two totals | (with_off: the host form's) a text offset per record and one more
struct TextWork {
    const char *what, *holds;                                      // the source's: for fit's message
    DevBuf buf;
    uint64_t n_tiles = 0;
    uint64_t *counts = nullptr, *extra = nullptr, *text_off = nullptr;
    unsigned long long *tile_sum = nullptr, *totals = nullptr;
    int fit(katgpu_ctx* c, size_t n, size_t n_rec, size_t counts_bytes, bool with_off) {
        n_tiles = n / CT_TILE + 1;                                 // positions 0 .. n
        const size_t sum_off = align_up(counts_bytes, 16), extra_off = sum_off + n_tiles * 8, tot_off = extra_off + n_rec * 8, off_off = tot_off + 16;
        const size_t need = off_off + (with_off ? (n_rec + 1) * 8 : 0);
        if (buf.fit(c, need) != hipSuccess)
            return fail(c, KATGPU_ERR_NOMEM, "%s: no %zu bytes of device memory for the %s of %zu bases and %zu records", what, need, holds, n, n_rec);
        uint8_t* w = buf.as<uint8_t>();
        counts = (uint64_t*)w; tile_sum = (unsigned long long*)(w + sum_off); extra = (uint64_t*)(w + extra_off);
        totals = (unsigned long long*)(w + tot_off); text_off = (uint64_t*)(w + off_off);
        return KATGPU_OK;
    }
};

// A text source: what differs between the two texts.  ready(): before its first launch.  size(): on the stream, w.totals then holds the bytes
// of the windows and of the window-less records.  write(): the tiles again behind it, the first `cap` bytes of the text to dev_text, the
// records' offsets (n_rec + 1, counted from text_base) to dev_text_off.

// -counts.cvg: k_profile over the n bases into w.counts (launch_profile's timed section), then K18 without writing and K19; K18 writes
struct CvgText {
    static constexpr const char *what = "cvg text", *holds = "counts";
    katgpu_table* t;
    int canonicalise;
    int ready() const { return refresh_counters(t); }
    size_t counts_bytes(size_t n) const { const uint32_t k = t->dev().k; return n >= k ? (n - k + 1) * 8 : 0; }
    dim3 grid(const TextWork& w) const { return dim3((unsigned)std::min<uint64_t>(w.n_tiles, (uint64_t)t->ctx->n_cu * 8)); }
    int size(const uint8_t* dev_bases, size_t n, const uint64_t* dev_start, const uint64_t* dev_len, size_t n_rec, const TextWork& w) const {
        katgpu_ctx* c = t->ctx;
        const uint32_t k = t->dev().k;
        if (n >= k) { int rc = launch_profile(t, dev_bases, n, canonicalise, w.counts); if (rc) return rc; }
        ScopedTimer tm(c, KATGPU_K_PROFILE, 0);                        // (launch_profile has counted the window starts)
        hipLaunchKernelGGL(k_cvg_tiles<false>, grid(w), dim3(CT_BLOCK), 0, c->stream, w.counts, (uint64_t)n, k, dev_start, dev_len, (uint64_t)n_rec, w.n_tiles, w.tile_sum,
                           w.extra, w.totals, (uint64_t)0, (uint8_t*)nullptr, (uint64_t)0, (uint64_t*)nullptr);
        hipLaunchKernelGGL(k_cvg_scan, dim3(2), dim3(CT_SCAN_BLOCK), 0, c->stream, w.tile_sum, w.n_tiles, dev_len, (uint64_t)n_rec, k, text_empty_bytes<CvgWindows>(), w.extra, w.totals);
        HIPCHK(c, hipGetLastError());
        return KATGPU_OK;
    }
    int write(const uint8_t*, size_t n, const uint64_t* dev_start, const uint64_t* dev_len, size_t n_rec, const TextWork& w, uint64_t text_base,
              uint8_t* dev_text, size_t cap, uint64_t* dev_text_off) const {
        katgpu_ctx* c = t->ctx;
        ScopedTimer tm(c, KATGPU_K_PROFILE, 0);
        hipLaunchKernelGGL(k_cvg_tiles<true>, grid(w), dim3(CT_BLOCK), 0, c->stream, w.counts, (uint64_t)n, t->dev().k, dev_start, dev_len, (uint64_t)n_rec, w.n_tiles, w.tile_sum,
                           w.extra, w.totals, text_base, dev_text, (uint64_t)cap, dev_text_off);
        HIPCHK(c, hipGetLastError());
        return KATGPU_OK;
    }
};

// the k + 2 strings of a window (kg_gc_text.hpp): glibc's "%.1f" of every percentage, and "-0.1"
static GcStrings gc_strings(uint32_t k) {
    GcStrings s{};
    auto entry = [](const char* str) {
        const size_t len = strlen(str);
        uint64_t e = (uint64_t)len << 56;
        for (size_t i = 0; i < len; ++i) e |= (uint64_t)(uint8_t)str[i] << (8 * i);
        return e;
    };
    char tmp[32];
    for (uint32_t g = 0; g <= k; ++g) { snprintf(tmp, sizeof tmp, "%.1f", ((double)g / (double)k) * 100.0); s.e[g] = entry(tmp); }
    s.e[k + 1] = entry("-0.1");
    return s;
}

// -counts.gc: no table and no counts -- K20 without writing and K19; K20 writes
struct GcText {
    static constexpr const char *what = "gc text", *holds = "tile sums";
    katgpu_ctx* c;
    uint32_t k;
    GcStrings strs;
    int ready() const { return KATGPU_OK; }
    size_t counts_bytes(size_t) const { return 0; }
    template <bool WRITE>
    void tiles(const uint8_t* dev_bases, size_t n, const uint64_t* dev_start, const uint64_t* dev_len, size_t n_rec, const TextWork& w, uint64_t text_base,
               uint8_t* dev_text, size_t cap, uint64_t* dev_text_off) const {
        const dim3 grid((unsigned)std::min<uint64_t>(w.n_tiles, (uint64_t)c->n_cu * 8));
        auto go = [&](auto A) {
            hipLaunchKernelGGL((k_gc_tiles<WRITE, decltype(A)::value>), grid, dim3(CT_BLOCK), 0, c->stream, dev_bases, (uint64_t)n, k, strs, dev_start, dev_len,
                               (uint64_t)n_rec, w.n_tiles, w.tile_sum, w.extra, w.totals, text_base, dev_text, (uint64_t)cap, dev_text_off);
        };
        if (aligned16(dev_bases)) go(std::true_type{});
        else go(std::false_type{});
    }
    int size(const uint8_t* dev_bases, size_t n, const uint64_t* dev_start, const uint64_t* dev_len, size_t n_rec, const TextWork& w) const {
        ScopedTimer tm(c, KATGPU_K_PROFILE, n >= k ? n - k + 1 : 0);
        tiles<false>(dev_bases, n, dev_start, dev_len, n_rec, w, 0, nullptr, 0, nullptr);
        hipLaunchKernelGGL(k_cvg_scan, dim3(2), dim3(CT_SCAN_BLOCK), 0, c->stream, w.tile_sum, w.n_tiles, dev_len, (uint64_t)n_rec, k, text_empty_bytes<GcWindows<true>>(), w.extra, w.totals);
        HIPCHK(c, hipGetLastError());
        return KATGPU_OK;
    }
    int write(const uint8_t* dev_bases, size_t n, const uint64_t* dev_start, const uint64_t* dev_len, size_t n_rec, const TextWork& w, uint64_t text_base,
              uint8_t* dev_text, size_t cap, uint64_t* dev_text_off) const {
        ScopedTimer tm(c, KATGPU_K_PROFILE, 0);
        tiles<true>(dev_bases, n, dev_start, dev_len, n_rec, w, text_base, dev_text, cap, dev_text_off);
        HIPCHK(c, hipGetLastError());
        return KATGPU_OK;
    }
};

static int gc_check_k(katgpu_ctx* c, uint32_t k) {
    if (k < 1 || k > KATGPU_MAX_K) return fail(c, KATGPU_ERR_K, "gc text: k = %u unsupported (1 <= k <= %d)", k, KATGPU_MAX_K);
    return KATGPU_OK;
}

// Device form of either text: sized, written, and the two totals back.
template <typename Src>
static int record_text_device(katgpu_ctx* c, const Src& src, const uint8_t* dev_bases, size_t n, const uint64_t* dev_rec_start, const uint64_t* dev_rec_len,
                              size_t n_rec, uint8_t* dev_text, size_t cap, uint64_t* dev_text_off, uint64_t* total) {
    HIPCHK(c, hipSetDevice(c->device));
    int rc = src.ready(); if (rc) return rc;
    if (!n_rec) {
        HIPCHK(c, hipMemsetAsync(dev_text_off, 0, sizeof(uint64_t), c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return KATGPU_OK;
    }
    TextWork w{src.what, src.holds};
    rc = w.fit(c, n, n_rec, src.counts_bytes(n), false); if (rc) return rc;
    rc = src.size(dev_bases, n, dev_rec_start, dev_rec_len, n_rec, w);
    if (!rc) rc = src.write(dev_bases, n, dev_rec_start, dev_rec_len, n_rec, w, 0, dev_text, cap, dev_text_off);
    if (rc) return rc;                                             // (w waits for the stream before it lets its block go)
    unsigned long long totals[2] = {0, 0};
    rc = read_totals(c, w.totals, 2, src.what, totals); if (rc) return rc;
    *total = totals[0] + totals[1];
    return KATGPU_OK;
}

// What the host form has to do with the text itself.  text_room: the result holds `need` bytes, grown by half at least.  text_fetch: `total`
// bytes of a batch's text from the device to dst through the context's two pinned buffers (ensure_pinned), piece i on its way into one
// while piece i - 1 is copied out of the other.
static int text_room(katgpu_ctx* c, const char* what, char*& res, size_t& res_cap, size_t need) {
    if (need <= res_cap) return KATGPU_OK;
    const size_t want = std::max(need, res_cap + res_cap / 2);
    char* grown = (char*)realloc(res, want);
    if (!grown) return fail(c, KATGPU_ERR_NOMEM, "%s: no host memory for %zu bytes of text", what, want);
    res = grown; res_cap = want;
    return KATGPU_OK;
}
static hipError_t text_fetch(katgpu_ctx* c, const uint8_t* dev, size_t total, char* dst) {
    hipError_t e = hipSuccess;
    const size_t piece = c->stage_bytes, n_pieces = (total + piece - 1) / piece;
    for (size_t i = 0; i <= n_pieces && e == hipSuccess; ++i) {
        if (i < n_pieces) {
            e = hipMemcpyAsync(c->pinned[i & 1], dev + i * piece, std::min(piece, total - i * piece), hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipEventRecord(c->pin_free[i & 1], c->stream);
        }
        if (i && e == hipSuccess) {
            e = hipEventSynchronize(c->pin_free[(i - 1) & 1]);
            if (e == hipSuccess) memcpy(dst + (i - 1) * piece, c->pinned[(i - 1) & 1], std::min(piece, total - (i - 1) * piece));
        }
    }
    return e;
}

// Host form of either text: the records go through the device in batches of at most max_bases bases and 2^20 records (for_record_batches), so
// any input fits next to the table.  Per batch the totals come back first, then room for the batch's text is found on the device and in the
// result, the source writes it, and it comes back through the context's two pinned buffers, one being copied out while the other fills;
// the offsets of a batch count from the call's first byte.
template <typename Src>
static int record_text_host(katgpu_ctx* c, const Src& src, size_t max_bases, const char* bases, size_t n, const uint64_t* rec_start, const uint64_t* rec_len,
                            size_t n_rec, char** text, uint64_t* text_off) {
    char* res = nullptr;
    size_t have = 0, res_cap = 0;
    if (n_rec) {
        int rc = check_records(c, rec_start, rec_len, n_rec, n); if (rc) return rc;
        HIPCHK(c, hipSetDevice(c->device));
        rc = src.ready(); if (rc) return rc;
        rc = ensure_pinned(c); if (rc) return rc;
        DevBuf out;                                                // the text of a batch
        TextWork w{src.what, src.holds};
        rc = for_record_batches(c, bases, n, rec_start, rec_len, n_rec, max_bases, std::min(n_rec, (size_t)1 << 20), 0, src.what, src.what,
                                [](size_t, bool) { return true; },
                                [&](const uint8_t* db, size_t nb, const uint64_t* ds, const uint64_t* dl, size_t m, size_t r0, uint64_t*) {
            int rc = w.fit(c, nb, m, src.counts_bytes(nb), true); if (rc) return rc;
            rc = src.size(db, nb, ds, dl, m, w); if (rc) return rc;
            unsigned long long totals[2] = {0, 0};
            rc = read_totals(c, w.totals, 2, src.what, totals); if (rc) return rc;
            const size_t total = (size_t)(totals[0] + totals[1]);
            if (out.fit(c, total) != hipSuccess) return fail(c, KATGPU_ERR_NOMEM, "%s: no %zu bytes of device memory for the text of a batch", src.what, total);
            rc = text_room(c, src.what, res, res_cap, have + total); if (rc) return rc;
            rc = src.write(db, nb, ds, dl, m, w, have, out.as<uint8_t>(), total, w.text_off); if (rc) return rc;
            hipError_t e = hipMemcpyAsync(text_off + r0, w.text_off, m * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = text_fetch(c, out.as<uint8_t>(), total, res + have);
            have += total;
            return e == hipSuccess ? (int)KATGPU_OK : fail(c, KATGPU_ERR_DEVICE, "%s: %s", src.what, hipGetErrorString(e));
        });
        if (rc) { free(res); return rc; }
    }
    if (!res) res = (char*)malloc(1);
    if (!res) return fail(c, KATGPU_ERR_NOMEM, "%s: no host memory for the text", src.what);
    text_off[n_rec] = have;
    *text = res;
    return KATGPU_OK;
}

extern "C" int katgpu_table_record_cvg_text_device(katgpu_table* t, const uint8_t* dev_bases, size_t n, const uint64_t* dev_rec_start,
                                                   const uint64_t* dev_rec_len, size_t n_rec, int canonicalise, uint8_t* dev_text, size_t cap,
                                                   uint64_t* dev_text_off, uint64_t* total) {
    if (!t || !total || !dev_text_off || !records_usable(dev_bases, n, dev_rec_start, dev_rec_len, n_rec) || (cap && !dev_text)) return KATGPU_ERR_INVALID_ARG;
    *total = 0;
    return record_text_device(t->ctx, CvgText{t, canonicalise}, dev_bases, n, dev_rec_start, dev_rec_len, n_rec, dev_text, cap, dev_text_off, total);
}

extern "C" int katgpu_table_record_cvg_text_host(katgpu_table* t, const char* bases, size_t n, const uint64_t* rec_start, const uint64_t* rec_len,
                                                 size_t n_rec, int canonicalise, char** text, uint64_t* text_off) {
    if (!t || !text || !text_off || !records_usable(bases, n, rec_start, rec_len, n_rec)) return KATGPU_ERR_INVALID_ARG;
    *text = nullptr;
    return record_text_host(t->ctx, CvgText{t, canonicalise}, g_cvg_batch, bases, n, rec_start, rec_len, n_rec, text, text_off);
}

extern "C" int katgpu_record_gc_text_device(katgpu_ctx* c, uint32_t k, const uint8_t* dev_bases, size_t n, const uint64_t* dev_rec_start,
                                            const uint64_t* dev_rec_len, size_t n_rec, uint8_t* dev_text, size_t cap, uint64_t* dev_text_off, uint64_t* total) {
    if (!c || !total || !dev_text_off || !records_usable(dev_bases, n, dev_rec_start, dev_rec_len, n_rec) || (cap && !dev_text)) return KATGPU_ERR_INVALID_ARG;
    *total = 0;
    int rc = gc_check_k(c, k); if (rc) return rc;
    return record_text_device(c, GcText{c, k, gc_strings(k)}, dev_bases, n, dev_rec_start, dev_rec_len, n_rec, dev_text, cap, dev_text_off, total);
}

extern "C" int katgpu_record_gc_text_host(katgpu_ctx* c, uint32_t k, const char* bases, size_t n, const uint64_t* rec_start, const uint64_t* rec_len,
                                          size_t n_rec, char** text, uint64_t* text_off) {
    if (!c || !text || !text_off || !records_usable(bases, n, rec_start, rec_len, n_rec)) return KATGPU_ERR_INVALID_ARG;
    *text = nullptr;
    int rc = gc_check_k(c, k); if (rc) return rc;
    return record_text_host(c, GcText{c, k, gc_strings(k)}, g_gc_batch, bases, n, rec_start, rec_len, n_rec, text, text_off);
}

