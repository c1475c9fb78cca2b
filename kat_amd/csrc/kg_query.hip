// kg_query.hip -- a sequence or keys against a table, which is left as it is: batch lookups (katgpu_table_get*), per-position profiles
// (katgpu_table_profile_*; _gathered_host: of a table that lies on several ranks, gathered on rank 0), the per-record hit counts of `kat filter seq` (katgpu_table_seq_hits_*; _gathered_host: summed over the ranks' tables on rank 0), the per-record coverage statistics
// of `kat sect -n` and `kat cold` (katgpu_table_record_stats_*) the count-range regions of `kat sect -E / -F` (katgpu_table_record_regions_*) the -counts.cvg text of `kat sect` (katgpu_table_record_cvg_text_*) and the -counts.gc text of `kat sect -g` (katgpu_record_gc_text_*: bases only, no table).  The host forms send their input through the device in batches.
#include "kg_host.hpp"
#include "kg_comm.hpp"
#include "kg_kernels.hpp"
#include "kg_query_kernels.hpp"
#include "kg_filter.hpp"
#include "kg_record_stats.hpp"
#include "kg_record_regions.hpp"
#include "kg_cvg_text.hpp"
#include "kg_gc_text.hpp"

static const bool g_forbid_profile_host = hook_u64("KATGPU_TEST_FORBID_PROFILE_HOST", 0) != 0;   // tests: a driver that should not need per-position counts asks for none
static const size_t g_profile_batch = (size_t)std::max<uint64_t>(hook_u64("KATGPU_TEST_PROFILE_BATCH", (uint64_t)32 << 20), 1);   // tests: window starts per batch of profile_host
static const size_t g_hits_batch = (size_t)std::max<uint64_t>(hook_u64("KATGPU_TEST_HITS_BATCH", (uint64_t)64 << 20), 1);        // tests: bases per batch of seq_hits_host

static const size_t g_hits_recs = (size_t)std::min<uint64_t>(std::max<uint64_t>(hook_u64("KATGPU_TEST_HITS_RECS", (uint64_t)1 << 20), 1), (uint64_t)1 << 20);   // tests: records per batch of seq_hits_host and seq_hits_gathered_host

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static uint64_t chunk_starts(bool wide) { return wide ? WIDE_CHUNK_STARTS : CHUNK_STARTS; }   // window starts per chunk of the window kernels

// keys: the caller's columns, .count == counts (where the answers go).  One staging buffer: the key column(s), then the counts
template <bool W>
static int get_records(katgpu_table* t, RecCols<W, const uint64_t> keys, size_t n, int canonicalise, uint64_t* counts) {
    if (!t || (n && keys.any_null())) return KATGPU_ERR_INVALID_ARG;
    if constexpr (W) WIDE_ONLY(t, "katgpu_table_get_wide", "katgpu_table_get");
    else NARROW_ONLY(t, "katgpu_table_get: use katgpu_table_get_wide;");
    if (!n) return KATGPU_OK;
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    DevBuf buf;
    if (buf.plain((keys.KEYS + 1) * n * 8) != hipSuccess) return fail(c, KATGPU_ERR_NOMEM, "lookup buffers");
    const RecCols<W> d = RecCols<W>::of(buf.as<uint64_t>(), n);
    for (int j = 0; j < keys.KEYS; ++j) hipMemcpyAsync(d.key[j], keys.key[j], n * 8, hipMemcpyHostToDevice, c->stream);
    hipLaunchKernelGGL(k_get<W>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, t->dev(), t->n_ovf, d, (uint64_t)n, canonicalise);
    hipMemcpyAsync(counts, d.count, n * 8, hipMemcpyDeviceToHost, c->stream);
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "%s", hipGetErrorString(e));
    return KATGPU_OK;
}

extern "C" int katgpu_table_get(katgpu_table* t, const uint64_t* keys, size_t n, int canonicalise, uint64_t* counts) {
    return get_records<false>(t, {{keys}, counts}, n, canonicalise, counts);
}

extern "C" int katgpu_table_get_wide(katgpu_table* t, const uint64_t* keys_hi, const uint64_t* keys_lo, size_t n, int canonicalise, uint64_t* counts) {
    return get_records<true>(t, {{keys_hi, keys_lo}, counts}, n, canonicalise, counts);
}

static int launch_profile(katgpu_table* t, const uint8_t* dev_bases, size_t n, int canonicalise, uint64_t* dev_counts) {
    katgpu_ctx* c = t->ctx;
    const bool wide = t->dev().keys_b != nullptr;
    const uint64_t n_out = n - t->dev().k + 1;
    ScopedTimer tm(c, KATGPU_K_PROFILE, n_out);
    launch_aligned_wide(c, aligned16(dev_bases) && aligned16(dev_counts), wide, n_out, chunk_starts(wide), [&](auto A, auto W, dim3 grid, uint64_t n_chunks) {
        hipLaunchKernelGGL((k_profile<decltype(A)::value, decltype(W)::value>), grid, dim3(COUNT_BLOCK), 0, c->stream, t->dev(), t->n_ovf, canonicalise, dev_bases, (uint64_t)n, n_chunks, dev_counts);
    });
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

// Host form: the sequence goes through the device in batches of g_profile_batch window starts (each batch re-sends the
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
    const size_t batch = std::min(n_out, g_profile_batch);
    DevBuf db, dc;
    HIPCHK(c, db.pooled(c, batch + 64));
    if (dc.pooled(c, batch * 8) != hipSuccess) return fail(c, KATGPU_ERR_NOMEM, "profile buffers");
    hipError_t e = hipSuccess;
    for (size_t pos = 0; pos < n_out && rc == KATGPU_OK && e == hipSuccess; pos += batch) {
        const size_t starts = std::min(batch, n_out - pos);
        const size_t nb = starts + k - 1;
        e = hipMemcpyAsync(db.p, bases + pos, nb, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) break;
        rc = launch_profile(t, db.as<uint8_t>(), nb, canonicalise, dc.as<uint64_t>());
        if (rc) break;
        e = hipMemcpyAsync(counts + pos, dc.p, starts * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    if (rc) return rc;
    if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "%s", hipGetErrorString(e));
    return KATGPU_OK;
}

// ------------------------------------------------------------------ the profile of a table that lies on several ranks ----

static const size_t g_gather_batch = (size_t)std::min<uint64_t>(std::max<uint64_t>(hook_u64("KATGPU_TEST_GATHER_BATCH", (uint64_t)32 << 20), 1), (uint64_t)1 << 31);   // tests: window starts per batch of profile_gathered_host (a run names a window in 32 bits)
static const int64_t g_gather_nomem = hook("KATGPU_TEST_GATHER_NOMEM") ? atoll(hook("KATGPU_TEST_GATHER_NOMEM")) : -1;   // tests: this rank reports that it could not allocate

// Collective, after katgpu_exchange_merge: every rank walks the same bases in batches of g_gather_batch window starts (each batch
// re-sends the k-1 bases it shares with the next one, as katgpu_table_profile_host does) and keeps (window, count) of the windows
// whose k-mer it owns and counts (k_profile_owned); the runs' lengths go round, the runs themselves to rank 0 -- one grouped
// transfer per batch, indices and counts of a run as two messages, behind rank 0's own run in the buffer that run was written to:
// the runs of a batch hold at most a record per window start between them, so one buffer of that size takes them all -- and rank 0
// scatters them into the batch's dense array (k_profile_scatter), which goes to `counts` through the stream.
// From the pool, per window start of a batch: 12 bytes of run on every rank and 8 of dense counts on rank 0, beside the batch's bases.
extern "C" int katgpu_table_profile_gathered_host(katgpu_comm* comm, katgpu_table* t, const char* bases, size_t n, int canonicalise, uint64_t* counts) {
    if (!comm || !t) return KATGPU_ERR_INVALID_ARG;
    katgpu_ctx* c = t->ctx;
    const int rank = katgpu_comm_rank(comm), world = katgpu_comm_world(comm);
    const uint32_t k = t->dv.k;
    const bool wide = t->dv.keys_b != nullptr;
    // ---- one sequence length, one k and usable pointers everywhere, before anything else: all ranks go on, or none does ----
    {
        const uint64_t mine[3] = {(uint64_t)n, k, (uint64_t)((n && !bases) || (rank == 0 && n >= k && !counts))};
        std::vector<uint64_t> all((size_t)world * 3, 0);
        const int crc = allgather_u64(comm, mine, 3, all.data());
        if (crc) return crc;
        for (int p = 0; p < world; ++p) {
            if (all[(size_t)p * 3] != all[0] || all[(size_t)p * 3 + 1] != all[1])
                return fail(c, KATGPU_ERR_INVALID_ARG, "profile gathered: the ranks disagree: rank 0 has %llu bases at k = %llu, rank %d %llu at k = %llu",
                            (unsigned long long)all[0], (unsigned long long)all[1], p, (unsigned long long)all[(size_t)p * 3], (unsigned long long)all[(size_t)p * 3 + 1]);
            if (all[(size_t)p * 3 + 2]) return fail(c, KATGPU_ERR_INVALID_ARG, "profile gathered: rank %d was given no bases, or rank 0 no room for the counts", p);
        }
    }
    if (n < k) return KATGPU_OK;
    const size_t n_out = n - k + 1;
    const size_t batch = std::min(n_out, g_gather_batch);
    // ---- everything a batch needs: the run's counts | its indices | its length, the dense array on rank 0 ----
    DevBuf db, run, dense;
    const size_t idx_off = batch * sizeof(uint64_t), len_off = align_up(idx_off + batch * sizeof(uint32_t), 16);
    auto prepare = [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        int rc = refresh_counters(t); if (rc) return rc;
        if (g_gather_nomem == rank || db.pooled(c, batch + k - 1 + 64) != hipSuccess || run.pooled(c, len_off + 16) != hipSuccess ||
            (rank == 0 && dense.pooled(c, batch * sizeof(uint64_t)) != hipSuccess)) {
            (void)hipGetLastError();
            return fail(c, KATGPU_ERR_NOMEM, "profile gathered: no device memory for a batch of %zu window starts", batch);
        }
        return KATGPU_OK;
    };
    int rc = comm_agree_to_start(comm, prepare(), [&](int p, int code) {
        if (code == KATGPU_ERR_NOMEM) return fail(c, code, "profile gathered: rank %d of %d has no device memory for a batch of %zu window starts", p, world, batch);
        return fail(c, code, "profile gathered: rank %d could not read its table", p);
    });
    if (rc) return rc;
    uint64_t* run_cnt = run.as<uint64_t>();
    uint32_t* run_idx = (uint32_t*)(run.as<uint8_t>() + idx_off);
    unsigned long long* run_len = (unsigned long long*)(run.as<uint8_t>() + len_off);

    // ---- the batches.  From here on a rank that fails raises the communicator's abort flag: its peers' waits end (comm_agree_done) ----
    uint64_t n_batches = 0, records = 0, wire_bytes = 0;
    std::vector<uint64_t> lens((size_t)world, 0);
    auto one_batch = [&](size_t pos) -> int {
        const size_t starts = std::min(batch, n_out - pos), nb = starts + k - 1;
        unsigned long long own = 0;
        HIPCHK(c, hipMemcpyAsync(db.p, bases + pos, nb, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(run_len, 0, sizeof own, c->stream));
        {
            ScopedTimer tm(c, KATGPU_K_PROFILE, starts);
            launch_aligned_wide(c, aligned16(db.p), wide, starts, chunk_starts(wide), [&](auto A, auto W, dim3 grid, uint64_t n_chunks) {
                hipLaunchKernelGGL((k_profile_owned<decltype(A)::value, decltype(W)::value>), grid, dim3(COUNT_BLOCK), 0, c->stream, t->dev(), t->n_ovf, canonicalise, db.as<uint8_t>(), (uint64_t)nb, n_chunks, (uint32_t)rank, (uint32_t)world, run_idx, run_cnt, run_len);
            });
            HIPCHK(c, hipGetLastError());
        }
        HIPCHK(c, hipMemcpyAsync(&own, run_len, sizeof own, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));             // (the run is whole before it travels)
        if (own > starts) return fail(c, KATGPU_ERR_DEVICE, "profile gathered: a run of %llu records from %zu windows", own, starts);
        const uint64_t mine = own;
        int rc = allgather_u64(comm, &mine, 1, lens.data());
        if (rc) return rc;
        uint64_t total = 0;
        for (uint64_t l : lens) total += l;
        const uint64_t remote = total - lens[0];
        if (total > starts) return fail(c, KATGPU_ERR_DEVICE, "profile gathered: the ranks' runs hold %llu records, the batch %zu windows", (unsigned long long)total, starts);
        if (remote) {                                            // (every rank knows: all take part in the transfer, or none does)
            std::vector<CommMsg> sends, recvs;
            if (rank != 0) { sends.push_back({0, run_idx, (size_t)own * sizeof(uint32_t)}); sends.push_back({0, run_cnt, (size_t)own * sizeof(uint64_t)}); }
            else {
                uint64_t at = lens[0];                           // the remote runs behind rank 0's own, in rank order
                for (int p = 1; p < world; at += lens[p++]) { recvs.push_back({p, run_idx + at, (size_t)lens[p] * sizeof(uint32_t)}); recvs.push_back({p, run_cnt + at, (size_t)lens[p] * sizeof(uint64_t)}); }
            }
            rc = transfer_sync(comm, sends, recvs);
            if (rc) return rc;
        }
        ++n_batches; records += total; wire_bytes += remote * (sizeof(uint32_t) + sizeof(uint64_t));
        if (rank != 0) return KATGPU_OK;
        uint64_t* d = dense.as<uint64_t>();
        {
            ScopedTimer tm(c, KATGPU_K_PROFILE, 0);
            hipLaunchKernelGGL(k_profile_scatter<true>, dim3((unsigned)grid_for(c, starts, 256, 8)), dim3(256), 0, c->stream, d, (uint64_t)starts, run_idx, run_cnt, (uint64_t)0);
            if (total) hipLaunchKernelGGL(k_profile_scatter<false>, dim3((unsigned)grid_for(c, total, 256, 8)), dim3(256), 0, c->stream, d, (uint64_t)starts, run_idx, run_cnt, total);
            HIPCHK(c, hipGetLastError());
        }
        HIPCHK(c, hipMemcpyAsync(counts + pos, d, starts * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return KATGPU_OK;
    };
    for (size_t pos = 0; pos < n_out && !rc; pos += batch) rc = one_batch(pos);
    rc = comm_agree_done(comm, rc, "profile gathered: rank %d failed");
    if (rc) return rc;
    if (rank == 0 && g_timing)
        fprintf(stderr, "katgpu_timing {\"phase\": \"profile_gathered\", \"batches\": %llu, \"ranks\": %d, \"records\": %llu, \"wire_bytes\": %llu}\n",
                (unsigned long long)n_batches, world, (unsigned long long)records, (unsigned long long)wire_bytes);
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
    unsigned long long* h = (unsigned long long*)dev_hits;
    ScopedTimer tm(c, KATGPU_K_PROFILE, n_out);
    launch_aligned_wide(c, aligned16(dev_bases), wide, n_out, chunk_starts(wide), [&](auto A, auto W, dim3 grid, uint64_t n_chunks) {
        hipLaunchKernelGGL((k_seq_hits<decltype(A)::value, decltype(W)::value>), grid, dim3(COUNT_BLOCK), 0, c->stream, t->dev(), t->n_ovf, canonicalise, dev_bases, (uint64_t)n, n_chunks, dev_start, dev_len, (uint64_t)n_rec, h);
    });
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

// Host form: the records go through the device in batches of at most g_hits_batch bases and SEQ_HITS_RECS records (for_record_batches),
// so any input fits next to the table.
extern "C" int katgpu_table_seq_hits_host(katgpu_table* t, const char* bases, size_t n, const uint64_t* rec_start, const uint64_t* rec_len,
                                          size_t n_rec, int canonicalise, uint64_t* hits) {
    if (!t || (n_rec && (!rec_start || !rec_len || !hits)) || (n && !bases)) return KATGPU_ERR_INVALID_ARG;
    if (!n_rec) return KATGPU_OK;
    katgpu_ctx* c = t->ctx;
    int rc = check_records(c, rec_start, rec_len, n_rec, n); if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = refresh_counters(t); if (rc) return rc;
    const size_t SEQ_HITS_RECS = g_hits_recs;
    DevBuf recs;                                                   // start, length and hits of every record of a batch
    HIPCHK(c, recs.pooled(c, SEQ_HITS_RECS * 3 * sizeof(uint64_t)));
    uint64_t* dr = recs.as<uint64_t>();
    return for_record_batches(c, bases, n, rec_start, rec_len, n_rec, g_hits_batch, SEQ_HITS_RECS, dr, dr + SEQ_HITS_RECS, "seq hits", nullptr,
                              [](size_t, bool) { return true; },
                              [&](const uint8_t* db, size_t nb, const uint64_t* ds, const uint64_t* dl, size_t m, size_t r0) {
        int rc = launch_seq_hits(t, db, nb, ds, dl, m, canonicalise, dr + 2 * SEQ_HITS_RECS);
        if (rc) return rc;
        const hipError_t e = hipMemcpyAsync(hits + r0, dr + 2 * SEQ_HITS_RECS, m * 8, hipMemcpyDeviceToHost, c->stream);
        return e == hipSuccess ? KATGPU_OK : fail(c, KATGPU_ERR_DEVICE, "seq hits: %s", hipGetErrorString(e));
    });
}

// ------------------------------------------------------------------ the hits of a table that lies on several ranks ----

static const int64_t g_hits_gather_nomem = hook("KATGPU_TEST_HITS_GATHER_NOMEM") ? atoll(hook("KATGPU_TEST_HITS_GATHER_NOMEM")) : -1;   // tests: this rank reports that it could not allocate

// what the ranks compare of their records: every start and length, in order, folded into one word
static uint64_t records_checksum(const uint64_t* rec_start, const uint64_t* rec_len, size_t n_rec) {
    uint64_t h = 0x9E3779B97F4A7C15ULL;
    auto fold = [&](uint64_t x) { h ^= x; h *= 0xFF51AFD7ED558CCDULL; h ^= h >> 32; };
    for (size_t r = 0; r < n_rec; ++r) { fold(rec_start[r]); fold(rec_len[r]); }
    return h;
}

// Collective, after katgpu_exchange_merge: every rank walks the same records in the batches of katgpu_table_seq_hits_host (for_record_batches:
// at most g_hits_batch bases and g_hits_recs records) and counts, per record, the hits among the windows whose k-mer it owns
// (k_seq_hits_owned).  Hits add across owners, so what travels is a record's count: the other ranks send the batch's m words to rank 0,
// which receives them behind one another, adds them to its own (k_hits_sum) and copies the sums to `hits`: 8 bytes per record and
// rank on the wire, none per window.  The batches are cut from the records, so the ranks first make sure that they hold the same ones.
// From the pool, per record of a batch: start, length and hits on every rank and world - 1 words of staging on rank 0, beside the
// batch's bases (for_record_batches' own buffer: a rank that finds no room for it fails inside the batches, where comm_agree_done hears of it).
extern "C" int katgpu_table_seq_hits_gathered_host(katgpu_comm* comm, katgpu_table* t, const char* bases, size_t n, const uint64_t* rec_start,
                                                   const uint64_t* rec_len, size_t n_rec, int canonicalise, uint64_t* hits) {
    if (!comm || !t) return KATGPU_ERR_INVALID_ARG;
    katgpu_ctx* c = t->ctx;
    const int rank = katgpu_comm_rank(comm), world = katgpu_comm_world(comm);
    const uint32_t k = t->dv.k;
    const bool wide = t->dv.keys_b != nullptr;
    // ---- the same records, one k and usable pointers everywhere, before anything else: all ranks go on, or none does ----
    {
        const bool unusable = (n && !bases) || (n_rec && (!rec_start || !rec_len)) || (rank == 0 && n_rec && !hits);
        const uint64_t mine[5] = {(uint64_t)n, (uint64_t)n_rec, k, unusable ? 0 : records_checksum(rec_start, rec_len, n_rec), (uint64_t)unusable};
        std::vector<uint64_t> all((size_t)world * 5, 0);
        const int crc = allgather_u64(comm, mine, 5, all.data());
        if (crc) return crc;
        for (int p = 0; p < world; ++p)
            if (all[(size_t)p * 5 + 4]) return fail(c, KATGPU_ERR_INVALID_ARG, "seq hits gathered: rank %d was given no bases or no records, or rank 0 no room for the hits", p);
        for (int p = 0; p < world; ++p) {
            const uint64_t* a = &all[(size_t)p * 5];
            if (a[0] != all[0] || a[1] != all[1] || a[2] != all[2])
                return fail(c, KATGPU_ERR_INVALID_ARG, "seq hits gathered: the ranks disagree: rank 0 has %llu bases in %llu records at k = %llu, rank %d %llu in %llu at k = %llu",
                            (unsigned long long)all[0], (unsigned long long)all[1], (unsigned long long)all[2], p, (unsigned long long)a[0], (unsigned long long)a[1], (unsigned long long)a[2]);
            if (a[3] != all[3]) return fail(c, KATGPU_ERR_INVALID_ARG, "seq hits gathered: the ranks disagree: rank %d's %llu records are not where rank 0's are", p, (unsigned long long)a[1]);
        }
    }
    if (!n_rec) return KATGPU_OK;
    int rc = check_records(c, rec_start, rec_len, n_rec, n); if (rc) return rc;      // (the same records everywhere: the same answer)
    // ---- everything a batch needs: start | length | hits of its records, the other ranks' hits on rank 0 ----
    const size_t cap = std::min(n_rec, g_hits_recs);               // records per batch
    DevBuf recs, stage;
    auto prepare = [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        int rc = refresh_counters(t); if (rc) return rc;
        if (g_hits_gather_nomem == rank || recs.pooled(c, cap * 3 * sizeof(uint64_t)) != hipSuccess ||
            (rank == 0 && world > 1 && stage.pooled(c, (size_t)(world - 1) * cap * sizeof(uint64_t)) != hipSuccess)) {
            (void)hipGetLastError();
            return fail(c, KATGPU_ERR_NOMEM, "seq hits gathered: no device memory for a batch of %zu records", cap);
        }
        return KATGPU_OK;
    };
    rc = comm_agree_to_start(comm, prepare(), [&](int p, int code) {
        if (code == KATGPU_ERR_NOMEM) return fail(c, code, "seq hits gathered: rank %d of %d has no device memory for a batch of %zu records", p, world, cap);
        return fail(c, code, "seq hits gathered: rank %d could not read its table", p);
    });
    if (rc) return rc;
    uint64_t* dr = recs.as<uint64_t>();
    uint64_t* d_hits = dr + 2 * cap;

    // ---- the batches.  From here on a rank that fails raises the communicator's abort flag: its peers' waits end (comm_agree_done) ----
    uint64_t n_batches = 0, records = 0;
    size_t no_room = 0;
    rc = for_record_batches(c, bases, n, rec_start, rec_len, n_rec, g_hits_batch, cap, dr, dr + cap, "seq hits gathered", &no_room,
                            [](size_t, bool) { return true; },
                            [&](const uint8_t* db, size_t nb, const uint64_t* ds, const uint64_t* dl, size_t m, size_t r0) -> int {
        HIPCHK(c, hipMemsetAsync(d_hits, 0, m * sizeof(uint64_t), c->stream));
        if (nb >= k) {
            const uint64_t n_out = nb - k + 1;
            ScopedTimer tm(c, KATGPU_K_PROFILE, n_out);
            launch_aligned_wide(c, aligned16(db), wide, n_out, chunk_starts(wide), [&](auto A, auto W, dim3 grid, uint64_t n_chunks) {
                hipLaunchKernelGGL((k_seq_hits_owned<decltype(A)::value, decltype(W)::value>), grid, dim3(COUNT_BLOCK), 0, c->stream, t->dev(), t->n_ovf, canonicalise, db, (uint64_t)nb, n_chunks, ds, dl, (uint64_t)m, (unsigned long long*)d_hits, (uint32_t)rank, (uint32_t)world);
            });
            HIPCHK(c, hipGetLastError());
        }
        if (world > 1) {
            HIPCHK(c, hipStreamSynchronize(c->stream));             // (the hits are whole before they travel)
            std::vector<CommMsg> sends, recvs;
            if (rank != 0) sends.push_back({0, d_hits, m * sizeof(uint64_t)});
            else for (int p = 1; p < world; ++p) recvs.push_back({p, stage.as<uint64_t>() + (size_t)(p - 1) * m, m * sizeof(uint64_t)});
            const int trc = transfer_sync(comm, sends, recvs);
            if (trc) return trc;
        }
        ++n_batches; records += m;
        if (rank != 0) return KATGPU_OK;
        if (world > 1) {
            ScopedTimer tm(c, KATGPU_K_PROFILE, 0);
            hipLaunchKernelGGL(k_hits_sum, dim3((unsigned)grid_for(c, m, 256, 8)), dim3(256), 0, c->stream, d_hits, stage.as<uint64_t>(), (uint64_t)m, (uint32_t)(world - 1));
            HIPCHK(c, hipGetLastError());
        }
        HIPCHK(c, hipMemcpyAsync(hits + r0, d_hits, m * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        return KATGPU_OK;
    });
    if (no_room) rc = fail(c, KATGPU_ERR_NOMEM, "seq hits gathered: no %zu bytes of device memory for a batch of bases", no_room);
    rc = comm_agree_done(comm, rc, "seq hits gathered: rank %d failed");
    if (rc) return rc;
    if (rank == 0 && g_timing)
        fprintf(stderr, "katgpu_timing {\"phase\": \"seq_hits_gathered\", \"batches\": %llu, \"ranks\": %d, \"records\": %llu, \"wire_bytes\": %llu}\n",
                (unsigned long long)n_batches, world, (unsigned long long)records, (unsigned long long)(8 * records * (uint64_t)(world - 1)));
    return KATGPU_OK;
}

// ------------------------------------------------------------------ per-record coverage statistics (kat sect -n, kat cold) ----

static const uint32_t g_stats_short = (uint32_t)std::min<uint64_t>(hook_u64("KATGPU_TEST_STATS_SHORT", RS_SHORT_WINDOWS), RS_SHORT_WINDOWS);   // tests: the short / long limit, in windows
static const size_t g_stats_batch = (size_t)std::max<uint64_t>(hook_u64("KATGPU_TEST_STATS_BATCH", (uint64_t)32 << 20), 1);                    // tests: bases per batch of the host form
static_assert(sizeof(katgpu_record_stats) == RS_FIELDS * sizeof(uint64_t), "the kernels write a record's statistics as six words");

// Everything on the stream: the result cleared, K11 over the tiles, and, when n_long records are long (long_windows windows in all),
// their slots, K12 and the eight passes of K13 over those windows.  ws takes the workspace of the long records (none: left empty), to be
// let go once the stream has run.  Two timed sections: the second only when there are long records.
static int launch_record_stats(katgpu_table* t, const uint8_t* dev_bases, size_t n, const uint64_t* dev_start, const uint64_t* dev_len, size_t n_rec,
                               int canonicalise, katgpu_record_stats* dev_out, uint64_t n_long, uint64_t long_windows, DevBuf& ws) {
    katgpu_ctx* c = t->ctx;
    ws.reset();
    HIPCHK(c, hipMemsetAsync(dev_out, 0, n_rec * sizeof(katgpu_record_stats), c->stream));
    if (!n || !n_rec) return KATGPU_OK;
    const DevTable& d = t->dev();
    const uint32_t k = d.k;
    const bool wide = d.keys_b != nullptr;
    const bool aligned = aligned16(dev_bases);
    const uint64_t n_out = n >= k ? n - k + 1 : 0;
    unsigned long long* o = (unsigned long long*)dev_out;
    {
        ScopedTimer tm(c, KATGPU_K_PROFILE, n_out);
        launch_aligned_wide(c, aligned, wide, n, RS_TILE_STRIDE, [&](auto A, auto W, dim3 grid, uint64_t n_tiles) {
            hipLaunchKernelGGL((k_rstats_short<decltype(A)::value, decltype(W)::value>), grid, dim3(COUNT_BLOCK), 0, c->stream, d, t->n_ovf, canonicalise, dev_bases, (uint64_t)n, n_tiles, dev_start, dev_len, (uint64_t)n_rec, g_stats_short, o);
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
        hipLaunchKernelGGL((k_rstats_long<decltype(A)::value, decltype(W)::value>), grid, dim3(COUNT_BLOCK), 0, c->stream, d, t->n_ovf, canonicalise, dev_bases, (uint64_t)n, n_chunks, dev_start, dev_len, (uint64_t)n_rec, rec_slot, cnt, long_windows, sel, o);
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
    DevBuf ws;
    rc = launch_record_stats(t, dev_bases, n, dev_rec_start, dev_rec_len, n_rec, canonicalise, dev_out, n_long[0], n_long[1], ws);
    if (ws.p) {
        const hipError_t e = hipStreamSynchronize(c->stream);
        if (!rc && e != hipSuccess) rc = fail(c, KATGPU_ERR_DEVICE, "record stats: %s", hipGetErrorString(e));
    }
    return rc;
}

// Host form: the records go through the device in batches of at most g_stats_batch bases and STATS_RECS records (for_record_batches),
// so any input fits next to the table; a batch also ends where its long records would have more than
// g_stats_batch / 4 windows between them (a single record may), which bounds their count scratch by the longest record or 8 bytes x that.
// What comes back is sizeof(katgpu_record_stats) per record.
extern "C" int katgpu_table_record_stats_host(katgpu_table* t, const char* bases, size_t n, const uint64_t* rec_start, const uint64_t* rec_len,
                                              size_t n_rec, int canonicalise, katgpu_record_stats* out) {
    if (!t || (n_rec && (!rec_start || !rec_len || !out)) || (n && !bases)) return KATGPU_ERR_INVALID_ARG;
    if (!n_rec) return KATGPU_OK;
    katgpu_ctx* c = t->ctx;
    int rc = check_records(c, rec_start, rec_len, n_rec, n); if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = refresh_counters(t); if (rc) return rc;
    const uint32_t k = t->dev().k;
    const size_t cap = std::min(n_rec, (size_t)1 << 20);           // records per batch
    DevBuf recs, ws;                                               // start, length and the six result words of every record of a batch; the long records' workspace
    if (recs.pooled(c, cap * (2 + RS_FIELDS) * sizeof(uint64_t)) != hipSuccess)
        return fail(c, KATGPU_ERR_NOMEM, "record statistics: no device memory for the records of a batch");
    uint64_t* dr = recs.as<uint64_t>();
    katgpu_record_stats* d_out = (katgpu_record_stats*)(dr + 2 * cap);
    uint64_t n_long = 0, long_windows = 0;                         // of the batch being cut
    auto joins = [&](size_t r, bool first) {
        if (first) n_long = long_windows = 0;
        uint64_t w = rec_len[r] >= k ? rec_len[r] - k + 1 : 0;
        if (w <= g_stats_short) w = 0;
        if (!first && long_windows + w > std::max<uint64_t>(g_stats_batch / 4, 1)) return false;
        n_long += w != 0; long_windows += w;
        return true;
    };
    size_t no_room = 0;
    rc = for_record_batches(c, bases, n, rec_start, rec_len, n_rec, g_stats_batch, cap, dr, dr + cap, "record stats", &no_room, joins,
                            [&](const uint8_t* db, size_t nb, const uint64_t* ds, const uint64_t* dl, size_t m, size_t r0) {
        int rc = launch_record_stats(t, db, nb, ds, dl, m, canonicalise, d_out, n_long, long_windows, ws);
        if (rc) return rc;
        const hipError_t e = hipMemcpyAsync(out + r0, d_out, m * sizeof(katgpu_record_stats), hipMemcpyDeviceToHost, c->stream);
        return e == hipSuccess ? KATGPU_OK : fail(c, KATGPU_ERR_DEVICE, "record stats: %s", hipGetErrorString(e));
    });
    return no_room ? fail(c, KATGPU_ERR_NOMEM, "record statistics: no %zu bytes of device memory for a batch of bases", no_room) : rc;
}

// ------------------------------------------------------------------ count-range regions of records (kat sect -n -E / -F) ----

static const size_t g_regions_batch = (size_t)std::max<uint64_t>(hook_u64("KATGPU_TEST_REGIONS_BATCH", (uint64_t)32 << 20), 1);   // tests: bases per batch of the host form
static_assert(sizeof(katgpu_region) == RG_FIELDS * sizeof(uint64_t), "the kernels write a region as three words");

// the workspace of one call or batch of n bases: first-window mask | a mask per range | two counters per range and mask block | a total per range
struct RegionsWork {
    DevBuf buf;
    size_t bytes = 0;
    uint64_t n_words = 0, n_blk = 0;
    uint64_t* masks = nullptr;
    unsigned long long *cnt = nullptr, *totals = nullptr;
    int fit(katgpu_ctx* c, size_t n, uint32_t n_ranges) {
        n_words = (n + 63) / 64; n_blk = (n_words + RG_BLOCK - 1) / RG_BLOCK;
        const size_t cnt_off = (1 + n_ranges) * n_words * 8, tot_off = cnt_off + n_ranges * n_blk * 16, need = tot_off + RG_MAX_RANGES * 8;
        if (need > bytes) {
            bytes = 0;
            if (buf.pooled(c, need) != hipSuccess)
                return fail(c, KATGPU_ERR_NOMEM, "record regions: no %zu bytes of device memory for the masks of %zu bases", need, n);
            bytes = need;
        }
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
static int launch_regions_find(katgpu_table* t, const uint8_t* dev_bases, size_t n, const uint64_t* dev_start, const uint64_t* dev_len, size_t n_rec,
                               int canonicalise, const RgRanges& rg, RegionsWork& w) {
    katgpu_ctx* c = t->ctx;
    const DevTable& d = t->dev();
    const bool wide = d.keys_b != nullptr;
    ScopedTimer tm(c, KATGPU_K_PROFILE, n >= d.k ? n - d.k + 1 : 0);
    launch_aligned_wide(c, aligned16(dev_bases), wide, w.n_words * 64, chunk_starts(wide), [&](auto A, auto W, dim3 grid, uint64_t n_chunks) {
        hipLaunchKernelGGL((k_regions_mask<decltype(A)::value, decltype(W)::value>), grid, dim3(COUNT_BLOCK), 0, c->stream, d, t->n_ovf, canonicalise, dev_bases, (uint64_t)n, n_chunks, dev_start, dev_len, (uint64_t)n_rec, rg, w.n_words, (uint16_t*)w.masks);
    });
    const dim3 grid((unsigned)std::min<uint64_t>(w.n_blk, (uint64_t)c->n_cu * 8));
    hipLaunchKernelGGL(k_regions_count, grid, dim3(RG_BLOCK), 0, c->stream, w.masks, w.n_words, w.n_blk, rg.n, w.cnt);
    hipLaunchKernelGGL(k_regions_scan, dim3(1), dim3(RG_SCAN_BLOCK), 0, c->stream, w.cnt, w.n_blk, rg.n, w.totals);
    HIPCHK(c, hipGetLastError());
    return KATGPU_OK;
}

// K17 behind it: the first `cap` regions to dev_regions, their records numbered from rec_base
static int launch_regions_emit(katgpu_table* t, const uint64_t* dev_start, const uint64_t* dev_len, size_t n_rec, uint64_t rec_base, const RgRanges& rg,
                               const RegionsWork& w, katgpu_region* dev_regions, size_t cap) {
    katgpu_ctx* c = t->ctx;
    if (!cap) return KATGPU_OK;
    ScopedTimer tm(c, KATGPU_K_PROFILE, 0);
    const dim3 grid((unsigned)std::min<uint64_t>(w.n_blk, (uint64_t)c->n_cu * 8));
    hipLaunchKernelGGL(k_regions_emit, grid, dim3(RG_BLOCK), 0, c->stream, w.masks, w.n_words, w.n_blk, rg.n, w.cnt, dev_start, dev_len, (uint64_t)n_rec, rec_base, (unsigned long long*)dev_regions, (uint64_t)cap);
    HIPCHK(c, hipGetLastError());
    return KATGPU_OK;
}

extern "C" int katgpu_table_record_regions_device(katgpu_table* t, const uint8_t* dev_bases, size_t n, const uint64_t* dev_rec_start,
                                                  const uint64_t* dev_rec_len, size_t n_rec, int canonicalise, const katgpu_count_range* ranges,
                                                  uint32_t n_ranges, katgpu_region* dev_regions, size_t cap, size_t n_out[]) {
    RgRanges rg;
    if (!t || !n_out || (n_rec && (!dev_rec_start || !dev_rec_len)) || (n && !dev_bases) || (cap && !dev_regions)) return KATGPU_ERR_INVALID_ARG;
    katgpu_ctx* c = t->ctx;
    if (!regions_args(ranges, n_ranges, rg)) return fail(c, KATGPU_ERR_INVALID_ARG, "record regions: one or two count ranges, not %u", ranges ? n_ranges : 0);
    for (uint32_t q = 0; q < n_ranges; ++q) n_out[q] = 0;
    if (!n_rec || !n) return KATGPU_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    RegionsWork w;
    rc = w.fit(c, n, n_ranges); if (rc) return rc;
    rc = launch_regions_find(t, dev_bases, n, dev_rec_start, dev_rec_len, n_rec, canonicalise, rg, w);
    if (!rc) rc = launch_regions_emit(t, dev_rec_start, dev_rec_len, n_rec, 0, rg, w, dev_regions, cap);
    unsigned long long totals[RG_MAX_RANGES] = {0, 0};
    hipError_t e = hipMemcpyAsync(totals, w.totals, n_ranges * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (rc) return rc;
    if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "record regions: %s", hipGetErrorString(e));
    for (uint32_t q = 0; q < n_ranges; ++q) n_out[q] = (size_t)totals[q];
    return KATGPU_OK;
}

// Host form: the records go through the device in batches of at most g_regions_batch bases and 2^20 records (for_record_batches), so any
// input fits next to the table.  Per batch the totals come back first, then room for that many regions is found and K17 fills it; the
// regions of a batch carry the records' indices in the whole call.
extern "C" int katgpu_table_record_regions_host(katgpu_table* t, const char* bases, size_t n, const uint64_t* rec_start, const uint64_t* rec_len,
                                                size_t n_rec, int canonicalise, const katgpu_count_range* ranges, uint32_t n_ranges,
                                                katgpu_region** regions, size_t n_out[]) {
    RgRanges rg;
    if (!t || !regions || !n_out || (n_rec && (!rec_start || !rec_len)) || (n && !bases)) return KATGPU_ERR_INVALID_ARG;
    katgpu_ctx* c = t->ctx;
    if (!regions_args(ranges, n_ranges, rg)) return fail(c, KATGPU_ERR_INVALID_ARG, "record regions: one or two count ranges, not %u", ranges ? n_ranges : 0);
    *regions = nullptr;
    for (uint32_t q = 0; q < n_ranges; ++q) n_out[q] = 0;
    std::vector<katgpu_region> found[RG_MAX_RANGES];
    if (n_rec) {
        int rc = check_records(c, rec_start, rec_len, n_rec, n); if (rc) return rc;
        HIPCHK(c, hipSetDevice(c->device));
        rc = refresh_counters(t); if (rc) return rc;
        const size_t max_recs = std::min(n_rec, (size_t)1 << 20);
        DevBuf recs, out;                                          // start and length of every record of a batch; the regions of a batch
        size_t out_cap = 0;
        if (recs.pooled(c, max_recs * 2 * sizeof(uint64_t)) != hipSuccess)
            return fail(c, KATGPU_ERR_NOMEM, "record regions: no device memory for the records of a batch");
        uint64_t* dr = recs.as<uint64_t>();
        RegionsWork w;
        size_t no_room = 0;
        rc = for_record_batches(c, bases, n, rec_start, rec_len, n_rec, g_regions_batch, max_recs, dr, dr + max_recs, "record regions", &no_room,
                                [](size_t, bool) { return true; },
                                [&](const uint8_t* db, size_t nb, const uint64_t* ds, const uint64_t* dl, size_t m, size_t r0) {
            if (!nb) return (int)KATGPU_OK;
            int rc = w.fit(c, nb, n_ranges); if (rc) return rc;
            rc = launch_regions_find(t, db, nb, ds, dl, m, canonicalise, rg, w); if (rc) return rc;
            unsigned long long totals[RG_MAX_RANGES] = {0, 0};
            hipError_t e = hipMemcpyAsync(totals, w.totals, n_ranges * 8, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "record regions: %s", hipGetErrorString(e));
            const size_t total = (size_t)(totals[0] + totals[1]);
            if (!total) return (int)KATGPU_OK;
            if (total > out_cap) {
                out_cap = 0;
                if (out.pooled(c, total * sizeof(katgpu_region)) != hipSuccess)
                    return fail(c, KATGPU_ERR_NOMEM, "record regions: no %zu bytes of device memory for the %zu regions of a batch", total * sizeof(katgpu_region), total);
                out_cap = total;
            }
            katgpu_region* d_out = out.as<katgpu_region>();
            rc = launch_regions_emit(t, ds, dl, m, r0, rg, w, d_out, total); if (rc) return rc;
            for (uint32_t q = 0; q < n_ranges && e == hipSuccess; ++q) {    // (the vectors grow before the copies are queued and rest until the batch's synchronize)
                const size_t have = found[q].size();
                found[q].resize(have + (size_t)totals[q]);
                if (totals[q]) e = hipMemcpyAsync(found[q].data() + have, d_out + (q ? totals[0] : 0), (size_t)totals[q] * sizeof(katgpu_region), hipMemcpyDeviceToHost, c->stream);
            }
            return e == hipSuccess ? (int)KATGPU_OK : fail(c, KATGPU_ERR_DEVICE, "record regions: %s", hipGetErrorString(e));
        });
        if (no_room) return fail(c, KATGPU_ERR_NOMEM, "record regions: no %zu bytes of device memory for a batch of bases", no_room);
        if (rc) return rc;
    }
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

// ------------------------------------------------------------------ the -counts.cvg text of records (kat sect) ----

static const size_t g_cvg_batch = (size_t)std::max<uint64_t>(hook_u64("KATGPU_TEST_CVG_BATCH", (uint64_t)32 << 20), 1);   // tests: bases per batch of the host form

// the workspace of one call or batch of n bases and n_rec records: a count per window start | a sum per tile | the window-less records' bytes
// before every record | the two totals | (with_off: the host form's) a text offset per record and one more
struct CvgWork {
    DevBuf buf;
    size_t bytes = 0;
    uint64_t n_tiles = 0;
    uint64_t *counts = nullptr, *extra = nullptr, *text_off = nullptr;
    unsigned long long *tile_sum = nullptr, *totals = nullptr;
    int fit(katgpu_ctx* c, size_t n, uint32_t k, size_t n_rec, bool with_off) {
        n_tiles = n / CT_TILE + 1;                                 // positions 0 .. n
        const size_t n_out = n >= k ? n - k + 1 : 0;
        const size_t sum_off = align_up(n_out * 8, 16), extra_off = sum_off + n_tiles * 8, tot_off = extra_off + n_rec * 8, off_off = tot_off + 16;
        const size_t need = off_off + (with_off ? (n_rec + 1) * 8 : 0);
        if (need > bytes) {
            bytes = 0;
            if (buf.pooled(c, need) != hipSuccess) {
                (void)hipGetLastError();
                return fail(c, KATGPU_ERR_NOMEM, "cvg text: no %zu bytes of device memory for the counts of %zu bases and %zu records", need, n, n_rec);
            }
            bytes = need;
        }
        uint8_t* w = buf.as<uint8_t>();
        counts = (uint64_t*)w; tile_sum = (unsigned long long*)(w + sum_off); extra = (uint64_t*)(w + extra_off);
        totals = (unsigned long long*)(w + tot_off); text_off = (uint64_t*)(w + off_off);
        return KATGPU_OK;
    }
};

// On the stream: k_profile over the n bases, K18 without writing, K19; w.totals then holds the bytes of the windows and of the window-less records.
static int launch_cvg_size(katgpu_table* t, const uint8_t* dev_bases, size_t n, const uint64_t* dev_start, const uint64_t* dev_len, size_t n_rec,
                           int canonicalise, CvgWork& w) {
    katgpu_ctx* c = t->ctx;
    const uint32_t k = t->dev().k;
    if (n >= k) { int rc = launch_profile(t, dev_bases, n, canonicalise, w.counts); if (rc) return rc; }
    ScopedTimer tm(c, KATGPU_K_PROFILE, 0);                        // (launch_profile has counted the window starts)
    const dim3 grid((unsigned)std::min<uint64_t>(w.n_tiles, (uint64_t)c->n_cu * 8));
    hipLaunchKernelGGL(k_cvg_tiles<false>, grid, dim3(CT_BLOCK), 0, c->stream, w.counts, (uint64_t)n, k, dev_start, dev_len, (uint64_t)n_rec, w.n_tiles, w.tile_sum,
                       w.extra, w.totals, (uint64_t)0, (uint8_t*)nullptr, (uint64_t)0, (uint64_t*)nullptr);
    hipLaunchKernelGGL(k_cvg_scan, dim3(2), dim3(CT_SCAN_BLOCK), 0, c->stream, w.tile_sum, w.n_tiles, dev_len, (uint64_t)n_rec, k, 2u, w.extra, w.totals);
    HIPCHK(c, hipGetLastError());
    return KATGPU_OK;
}

// K18 again behind it: the first `cap` bytes of the text to dev_text, the records' offsets (n_rec + 1, counted from text_base) to dev_text_off
static int launch_cvg_write(katgpu_table* t, size_t n, const uint64_t* dev_start, const uint64_t* dev_len, size_t n_rec, const CvgWork& w, uint64_t text_base,
                            uint8_t* dev_text, size_t cap, uint64_t* dev_text_off) {
    katgpu_ctx* c = t->ctx;
    ScopedTimer tm(c, KATGPU_K_PROFILE, 0);
    const dim3 grid((unsigned)std::min<uint64_t>(w.n_tiles, (uint64_t)c->n_cu * 8));
    hipLaunchKernelGGL(k_cvg_tiles<true>, grid, dim3(CT_BLOCK), 0, c->stream, w.counts, (uint64_t)n, t->dev().k, dev_start, dev_len, (uint64_t)n_rec, w.n_tiles, w.tile_sum,
                       w.extra, w.totals, text_base, dev_text, (uint64_t)cap, dev_text_off);
    HIPCHK(c, hipGetLastError());
    return KATGPU_OK;
}

extern "C" int katgpu_table_record_cvg_text_device(katgpu_table* t, const uint8_t* dev_bases, size_t n, const uint64_t* dev_rec_start,
                                                   const uint64_t* dev_rec_len, size_t n_rec, int canonicalise, uint8_t* dev_text, size_t cap,
                                                   uint64_t* dev_text_off, uint64_t* total) {
    if (!t || !total || !dev_text_off || (n_rec && (!dev_rec_start || !dev_rec_len)) || (n && !dev_bases) || (cap && !dev_text)) return KATGPU_ERR_INVALID_ARG;
    *total = 0;
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    if (!n_rec) {
        HIPCHK(c, hipMemsetAsync(dev_text_off, 0, sizeof(uint64_t), c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return KATGPU_OK;
    }
    CvgWork w;
    rc = w.fit(c, n, t->dev().k, n_rec, false); if (rc) return rc;
    rc = launch_cvg_size(t, dev_bases, n, dev_rec_start, dev_rec_len, n_rec, canonicalise, w);
    if (!rc) rc = launch_cvg_write(t, n, dev_rec_start, dev_rec_len, n_rec, w, 0, dev_text, cap, dev_text_off);
    unsigned long long totals[2] = {0, 0};
    hipError_t e = hipMemcpyAsync(totals, w.totals, sizeof totals, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (rc) return rc;
    if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "cvg text: %s", hipGetErrorString(e));
    *total = totals[0] + totals[1];
    return KATGPU_OK;
}

// What the host forms of the text calls share.  text_room: the result holds `need` bytes, grown by half at least.  text_fetch: `total`
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

// Host form: the records go through the device in batches of at most g_cvg_batch bases and 2^20 records (for_record_batches), so any input
// fits next to the table.  Per batch the totals come back first, then room for the batch's text is found on the device and in the
// result, K18 fills it, and it comes back through the context's two pinned buffers, one being copied out while the other fills;
// the offsets of a batch count from the call's first byte.
extern "C" int katgpu_table_record_cvg_text_host(katgpu_table* t, const char* bases, size_t n, const uint64_t* rec_start, const uint64_t* rec_len,
                                                 size_t n_rec, int canonicalise, char** text, uint64_t* text_off) {
    if (!t || !text || !text_off || (n_rec && (!rec_start || !rec_len)) || (n && !bases)) return KATGPU_ERR_INVALID_ARG;
    katgpu_ctx* c = t->ctx;
    *text = nullptr;
    char* res = nullptr;
    size_t have = 0, res_cap = 0;
    if (n_rec) {
        int rc = check_records(c, rec_start, rec_len, n_rec, n); if (rc) return rc;
        HIPCHK(c, hipSetDevice(c->device));
        rc = refresh_counters(t); if (rc) return rc;
        rc = ensure_pinned(c); if (rc) return rc;
        const uint32_t k = t->dev().k;
        const size_t max_recs = std::min(n_rec, (size_t)1 << 20);
        DevBuf recs, out;                                          // start and length of every record of a batch; the text of a batch
        size_t out_cap = 0;
        if (recs.pooled(c, max_recs * 2 * sizeof(uint64_t)) != hipSuccess)
            return fail(c, KATGPU_ERR_NOMEM, "cvg text: no device memory for the records of a batch");
        uint64_t* dr = recs.as<uint64_t>();
        CvgWork w;
        size_t no_room = 0;
        rc = for_record_batches(c, bases, n, rec_start, rec_len, n_rec, g_cvg_batch, max_recs, dr, dr + max_recs, "cvg text", &no_room,
                                [](size_t, bool) { return true; },
                                [&](const uint8_t* db, size_t nb, const uint64_t* ds, const uint64_t* dl, size_t m, size_t r0) {
            int rc = w.fit(c, nb, k, m, true); if (rc) return rc;
            rc = launch_cvg_size(t, db, nb, ds, dl, m, canonicalise, w); if (rc) return rc;
            unsigned long long totals[2] = {0, 0};
            hipError_t e = hipMemcpyAsync(totals, w.totals, sizeof totals, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "cvg text: %s", hipGetErrorString(e));
            const size_t total = (size_t)(totals[0] + totals[1]);
            if (total > out_cap) {
                out_cap = 0;
                if (out.pooled(c, total) != hipSuccess) {
                    (void)hipGetLastError();
                    return fail(c, KATGPU_ERR_NOMEM, "cvg text: no %zu bytes of device memory for the text of a batch", total);
                }
                out_cap = total;
            }
            rc = text_room(c, "cvg text", res, res_cap, have + total); if (rc) return rc;
            rc = launch_cvg_write(t, nb, ds, dl, m, w, have, out.as<uint8_t>(), total, w.text_off); if (rc) return rc;
            e = hipMemcpyAsync(text_off + r0, w.text_off, m * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = text_fetch(c, out.as<uint8_t>(), total, res + have);
            have += total;
            return e == hipSuccess ? (int)KATGPU_OK : fail(c, KATGPU_ERR_DEVICE, "cvg text: %s", hipGetErrorString(e));
        });
        if (no_room) rc = fail(c, KATGPU_ERR_NOMEM, "cvg text: no %zu bytes of device memory for a batch of bases", no_room);
        if (rc) { free(res); return rc; }
    }
    if (!res) res = (char*)malloc(1);
    if (!res) return fail(c, KATGPU_ERR_NOMEM, "cvg text: no host memory for the text");
    text_off[n_rec] = have;
    *text = res;
    return KATGPU_OK;
}

// ------------------------------------------------------------------ the -counts.gc text of records (kat sect -g) ----

static const size_t g_gc_batch = (size_t)std::max<uint64_t>(hook_u64("KATGPU_TEST_GC_BATCH", (uint64_t)32 << 20), 1);   // tests: bases per batch of the host form

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

// the workspace of one call or batch of n bases and n_rec records: a sum per tile | the window-less records' bytes before every record |
// the two totals | (with_off: the host form's) a text offset per record and one more
struct GcWork {
    DevBuf buf;
    size_t bytes = 0;
    uint64_t n_tiles = 0;
    GcStrings strs;
    uint64_t *extra = nullptr, *text_off = nullptr;
    unsigned long long *tile_sum = nullptr, *totals = nullptr;
    int fit(katgpu_ctx* c, size_t n, size_t n_rec, bool with_off) {
        n_tiles = n / CT_TILE + 1;                                 // positions 0 .. n
        const size_t extra_off = n_tiles * 8, tot_off = extra_off + n_rec * 8, off_off = tot_off + 16;
        const size_t need = off_off + (with_off ? (n_rec + 1) * 8 : 0);
        if (need > bytes) {
            bytes = 0;
            if (buf.pooled(c, need) != hipSuccess) {
                (void)hipGetLastError();
                return fail(c, KATGPU_ERR_NOMEM, "gc text: no %zu bytes of device memory for the tile sums of %zu bases and %zu records", need, n, n_rec);
            }
            bytes = need;
        }
        uint8_t* w = buf.as<uint8_t>();
        tile_sum = (unsigned long long*)w; extra = (uint64_t*)(w + extra_off);
        totals = (unsigned long long*)(w + tot_off); text_off = (uint64_t*)(w + off_off);
        return KATGPU_OK;
    }
};

template <bool WRITE>
static void launch_gc_tiles(katgpu_ctx* c, uint32_t k, const uint8_t* dev_bases, size_t n, const uint64_t* dev_start, const uint64_t* dev_len, size_t n_rec,
                            const GcWork& w, uint64_t text_base, uint8_t* dev_text, size_t cap, uint64_t* dev_text_off) {
    const dim3 grid((unsigned)std::min<uint64_t>(w.n_tiles, (uint64_t)c->n_cu * 8));
    auto go = [&](auto A) {
        hipLaunchKernelGGL((k_gc_tiles<WRITE, decltype(A)::value>), grid, dim3(CT_BLOCK), 0, c->stream, dev_bases, (uint64_t)n, k, w.strs, dev_start, dev_len,
                           (uint64_t)n_rec, w.n_tiles, w.tile_sum, w.extra, w.totals, text_base, dev_text, (uint64_t)cap, dev_text_off);
    };
    if (aligned16(dev_bases)) go(std::true_type{});
    else go(std::false_type{});
}

// On the stream: K20 without writing, K19; w.totals then holds the bytes of the windows and of the window-less records.
static int launch_gc_size(katgpu_ctx* c, uint32_t k, const uint8_t* dev_bases, size_t n, const uint64_t* dev_start, const uint64_t* dev_len, size_t n_rec, const GcWork& w) {
    ScopedTimer tm(c, KATGPU_K_PROFILE, n >= k ? n - k + 1 : 0);
    launch_gc_tiles<false>(c, k, dev_bases, n, dev_start, dev_len, n_rec, w, 0, nullptr, 0, nullptr);
    hipLaunchKernelGGL(k_cvg_scan, dim3(2), dim3(CT_SCAN_BLOCK), 0, c->stream, w.tile_sum, w.n_tiles, dev_len, (uint64_t)n_rec, k, 4u, w.extra, w.totals);
    HIPCHK(c, hipGetLastError());
    return KATGPU_OK;
}

// K20 again behind it: the first `cap` bytes of the text to dev_text, the records' offsets (n_rec + 1, counted from text_base) to dev_text_off
static int launch_gc_write(katgpu_ctx* c, uint32_t k, const uint8_t* dev_bases, size_t n, const uint64_t* dev_start, const uint64_t* dev_len, size_t n_rec,
                           const GcWork& w, uint64_t text_base, uint8_t* dev_text, size_t cap, uint64_t* dev_text_off) {
    ScopedTimer tm(c, KATGPU_K_PROFILE, 0);
    launch_gc_tiles<true>(c, k, dev_bases, n, dev_start, dev_len, n_rec, w, text_base, dev_text, cap, dev_text_off);
    HIPCHK(c, hipGetLastError());
    return KATGPU_OK;
}

static int gc_check_k(katgpu_ctx* c, uint32_t k) {
    if (k < 1 || k > KATGPU_MAX_K) return fail(c, KATGPU_ERR_K, "gc text: k = %u unsupported (1 <= k <= %d)", k, KATGPU_MAX_K);
    return KATGPU_OK;
}

extern "C" int katgpu_record_gc_text_device(katgpu_ctx* c, uint32_t k, const uint8_t* dev_bases, size_t n, const uint64_t* dev_rec_start,
                                            const uint64_t* dev_rec_len, size_t n_rec, uint8_t* dev_text, size_t cap, uint64_t* dev_text_off, uint64_t* total) {
    if (!c || !total || !dev_text_off || (n_rec && (!dev_rec_start || !dev_rec_len)) || (n && !dev_bases) || (cap && !dev_text)) return KATGPU_ERR_INVALID_ARG;
    *total = 0;
    int rc = gc_check_k(c, k); if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (!n_rec) {
        HIPCHK(c, hipMemsetAsync(dev_text_off, 0, sizeof(uint64_t), c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return KATGPU_OK;
    }
    GcWork w;
    w.strs = gc_strings(k);
    rc = w.fit(c, n, n_rec, false); if (rc) return rc;
    rc = launch_gc_size(c, k, dev_bases, n, dev_rec_start, dev_rec_len, n_rec, w);
    if (!rc) rc = launch_gc_write(c, k, dev_bases, n, dev_rec_start, dev_rec_len, n_rec, w, 0, dev_text, cap, dev_text_off);
    unsigned long long totals[2] = {0, 0};
    hipError_t e = hipMemcpyAsync(totals, w.totals, sizeof totals, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (rc) return rc;
    if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "gc text: %s", hipGetErrorString(e));
    *total = totals[0] + totals[1];
    return KATGPU_OK;
}

// Host form: the records go through the device in batches of at most g_gc_batch bases and 2^20 records (for_record_batches).  Per batch
// the totals come back first, then room for the batch's text is found on the device and in the result, K20 fills it, and it comes back
// through the context's two pinned buffers (text_fetch); the offsets of a batch count from the call's first byte.
extern "C" int katgpu_record_gc_text_host(katgpu_ctx* c, uint32_t k, const char* bases, size_t n, const uint64_t* rec_start, const uint64_t* rec_len,
                                          size_t n_rec, char** text, uint64_t* text_off) {
    if (!c || !text || !text_off || (n_rec && (!rec_start || !rec_len)) || (n && !bases)) return KATGPU_ERR_INVALID_ARG;
    *text = nullptr;
    int rc = gc_check_k(c, k); if (rc) return rc;
    char* res = nullptr;
    size_t have = 0, res_cap = 0;
    if (n_rec) {
        rc = check_records(c, rec_start, rec_len, n_rec, n); if (rc) return rc;
        HIPCHK(c, hipSetDevice(c->device));
        rc = ensure_pinned(c); if (rc) return rc;
        const size_t max_recs = std::min(n_rec, (size_t)1 << 20);
        DevBuf recs, out;                                          // start and length of every record of a batch; the text of a batch
        size_t out_cap = 0;
        if (recs.pooled(c, max_recs * 2 * sizeof(uint64_t)) != hipSuccess)
            return fail(c, KATGPU_ERR_NOMEM, "gc text: no device memory for the records of a batch");
        uint64_t* dr = recs.as<uint64_t>();
        GcWork w;
        w.strs = gc_strings(k);
        size_t no_room = 0;
        rc = for_record_batches(c, bases, n, rec_start, rec_len, n_rec, g_gc_batch, max_recs, dr, dr + max_recs, "gc text", &no_room,
                                [](size_t, bool) { return true; },
                                [&](const uint8_t* db, size_t nb, const uint64_t* ds, const uint64_t* dl, size_t m, size_t r0) {
            int rc = w.fit(c, nb, m, true); if (rc) return rc;
            rc = launch_gc_size(c, k, db, nb, ds, dl, m, w); if (rc) return rc;
            unsigned long long totals[2] = {0, 0};
            hipError_t e = hipMemcpyAsync(totals, w.totals, sizeof totals, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "gc text: %s", hipGetErrorString(e));
            const size_t total = (size_t)(totals[0] + totals[1]);
            if (total > out_cap) {
                out_cap = 0;
                if (out.pooled(c, total) != hipSuccess) {
                    (void)hipGetLastError();
                    return fail(c, KATGPU_ERR_NOMEM, "gc text: no %zu bytes of device memory for the text of a batch", total);
                }
                out_cap = total;
            }
            rc = text_room(c, "gc text", res, res_cap, have + total); if (rc) return rc;
            rc = launch_gc_write(c, k, db, nb, ds, dl, m, w, have, out.as<uint8_t>(), total, w.text_off); if (rc) return rc;
            e = hipMemcpyAsync(text_off + r0, w.text_off, m * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess) e = text_fetch(c, out.as<uint8_t>(), total, res + have);
            have += total;
            return e == hipSuccess ? (int)KATGPU_OK : fail(c, KATGPU_ERR_DEVICE, "gc text: %s", hipGetErrorString(e));
        });
        if (no_room) rc = fail(c, KATGPU_ERR_NOMEM, "gc text: no %zu bytes of device memory for a batch of bases", no_room);
        if (rc) { free(res); return rc; }
    }
    if (!res) res = (char*)malloc(1);
    if (!res) return fail(c, KATGPU_ERR_NOMEM, "gc text: no host memory for the text");
    text_off[n_rec] = have;
    *text = res;
    return KATGPU_OK;
}
