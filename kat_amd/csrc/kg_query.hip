// kg_query.hip -- a sequence or keys against a table, which is left as it is: batch lookups (katgpu_table_get*), per-position profiles
// (katgpu_table_profile_*; _gathered_host: of a table that lies on several ranks, gathered on rank 0), the per-record hit counts of `kat filter seq` (katgpu_table_seq_hits_*; _gathered_host: summed over the ranks' tables on rank 0).
// The host forms send their input through the device in batches.  What sect and cold ask per record is kg_per_record.hip's, the
// gathered form included: it runs this unit's gather (ProfileGather, kg_comm.hpp).
#include "kg_comm.hpp"
#include "kg_query_kernels.hpp"
#include "kg_filter.hpp"

static const bool g_forbid_profile_host = hook_u64("KATGPU_TEST_FORBID_PROFILE_HOST", 0) != 0;   // tests: a driver that should not need per-position counts asks for none
static const size_t g_profile_batch = (size_t)std::max<uint64_t>(hook_u64("KATGPU_TEST_PROFILE_BATCH", (uint64_t)32 << 20), 1);   // tests: window starts per batch of profile_host
static const size_t g_hits_batch = (size_t)std::max<uint64_t>(hook_u64("KATGPU_TEST_HITS_BATCH", (uint64_t)64 << 20), 1);        // tests: bases per batch of seq_hits_host

static const size_t g_hits_recs = (size_t)std::min<uint64_t>(std::max<uint64_t>(hook_u64("KATGPU_TEST_HITS_RECS", (uint64_t)1 << 20), 1), (uint64_t)1 << 20);   // tests: records per batch of seq_hits_host and seq_hits_gathered_host

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

int launch_profile(katgpu_table* t, const uint8_t* dev_bases, size_t n, int canonicalise, uint64_t* dev_counts) {
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

static const bool g_forbid_profile_gathered = hook_u64("KATGPU_TEST_FORBID_PROFILE_GATHERED", 0) != 0;   // tests: a driver that should gather no per-position counts on the host asks for none

// The gather itself (kg_comm.hpp: ProfileGather).  Every rank walks the same bases in batches of g_gather_batch window starts and keeps
// (window, count) of the windows whose k-mer it owns and counts (k_profile_owned); the runs' lengths go round, the runs themselves to
// rank 0 -- one grouped transfer per batch, indices and counts of a run as two messages, behind rank 0's own run in the buffer that run
// was written to: the runs of a batch hold at most a record per window start between them, so one buffer of that size takes them all --
// and rank 0 scatters them into the batch's dense array (k_profile_scatter): its own scratch, which goes to the host through the
// stream, or the batch's stretch of an array the caller keeps on the device.
int ProfileGather::prepare(size_t max_starts, bool stage_bases, bool stage_counts) {
    katgpu_ctx* c = t->ctx;
    const int rank = katgpu_comm_rank(comm);
    batch = std::max<size_t>(std::min(max_starts, g_gather_batch), 1);
    idx_off = batch * sizeof(uint64_t); len_off = align_up(idx_off + batch * sizeof(uint32_t), 16);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    if (g_gather_nomem == rank || (stage_bases && db.pooled(c, batch + t->dv.k - 1 + 64) != hipSuccess) || run.pooled(c, len_off + 16) != hipSuccess ||
        (rank == 0 && stage_counts && dense.pooled(c, batch * sizeof(uint64_t)) != hipSuccess)) {
        (void)hipGetLastError();
        return fail(c, KATGPU_ERR_NOMEM, "profile gathered: no device memory for a batch of %zu window starts", batch);
    }
    return KATGPU_OK;
}

int ProfileGather::gather(const char* bases, const uint8_t* dev_bases, size_t n, uint64_t* counts, uint64_t* dev_counts) {
    katgpu_ctx* c = t->ctx;
    const int rank = katgpu_comm_rank(comm), world = katgpu_comm_world(comm);
    const uint32_t k = t->dv.k;
    const bool wide = t->dv.keys_b != nullptr;
    if (n < k) return KATGPU_OK;
    const size_t n_out = n - k + 1;
    uint64_t* run_cnt = run.as<uint64_t>();
    uint32_t* run_idx = (uint32_t*)(run.as<uint8_t>() + idx_off);
    unsigned long long* run_len = (unsigned long long*)(run.as<uint8_t>() + len_off);
    std::vector<uint64_t> lens((size_t)world, 0);
    auto one_batch = [&](size_t pos) -> int {
        const size_t starts = std::min(batch, n_out - pos), nb = starts + k - 1;
        unsigned long long own = 0;
        const uint8_t* b = dev_bases ? dev_bases + pos : db.as<uint8_t>();
        if (!dev_bases) HIPCHK(c, hipMemcpyAsync(db.p, bases + pos, nb, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(run_len, 0, sizeof own, c->stream));
        {
            ScopedTimer tm(c, KATGPU_K_PROFILE, starts);
            launch_aligned_wide(c, aligned16(b), wide, starts, chunk_starts(wide), [&](auto A, auto W, dim3 grid, uint64_t n_chunks) {
                hipLaunchKernelGGL((k_profile_owned<decltype(A)::value, decltype(W)::value>), grid, dim3(COUNT_BLOCK), 0, c->stream, t->dev(), t->n_ovf, canonicalise, b, (uint64_t)nb, n_chunks, (uint32_t)rank, (uint32_t)world, run_idx, run_cnt, run_len);
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
        uint64_t* d = dev_counts ? dev_counts + pos : dense.as<uint64_t>();
        {
            ScopedTimer tm(c, KATGPU_K_PROFILE, 0);
            hipLaunchKernelGGL(k_profile_scatter<true>, dim3((unsigned)grid_for(c, starts, 256, 8)), dim3(256), 0, c->stream, d, (uint64_t)starts, run_idx, run_cnt, (uint64_t)0);
            if (total) hipLaunchKernelGGL(k_profile_scatter<false>, dim3((unsigned)grid_for(c, total, 256, 8)), dim3(256), 0, c->stream, d, (uint64_t)starts, run_idx, run_cnt, total);
            HIPCHK(c, hipGetLastError());
        }
        if (!dev_counts) HIPCHK(c, hipMemcpyAsync(counts + pos, d, starts * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));             // (the run buffer is the next batch's)
        return KATGPU_OK;
    };
    int rc = KATGPU_OK;
    for (size_t pos = 0; pos < n_out && !rc; pos += batch) rc = one_batch(pos);
    return rc;
}

void ProfileGather::print_timing() const {
    if (katgpu_comm_rank(comm) == 0 && g_timing)
        fprintf(stderr, "katgpu_timing {\"phase\": \"profile_gathered\", \"batches\": %llu, \"ranks\": %d, \"records\": %llu, \"wire_bytes\": %llu}\n",
                (unsigned long long)n_batches, katgpu_comm_world(comm), (unsigned long long)records, (unsigned long long)wire_bytes);
}

// Collective, after katgpu_exchange_merge: the gather above over the whole sequence (each batch re-sends the k-1 bases it shares with the
// next one, as katgpu_table_profile_host does), the dense counts of every batch to `counts` on rank 0.
// From the pool, per window start of a batch: 12 bytes of run on every rank and 8 of dense counts on rank 0, beside the batch's bases.
extern "C" int katgpu_table_profile_gathered_host(katgpu_comm* comm, katgpu_table* t, const char* bases, size_t n, int canonicalise, uint64_t* counts) {
    if (!comm || !t) return KATGPU_ERR_INVALID_ARG;
    katgpu_ctx* c = t->ctx;
    if (g_forbid_profile_gathered) return fail(c, KATGPU_ERR_INVALID_ARG, "katgpu_table_profile_gathered_host is forbidden (KATGPU_TEST_FORBID_PROFILE_GATHERED)");
    const int rank = katgpu_comm_rank(comm);
    const uint32_t k = t->dv.k;
    // ---- one sequence length, one k and usable pointers everywhere, before anything else: all ranks go on, or none does ----
    int rc = comm_agree_on_call(comm, c, "profile gathered", n, k, nullptr, (n && !bases) || (rank == 0 && n >= k && !counts), "was given no bases, or rank 0 no room for the counts");
    if (rc) return rc;
    if (n < k) return KATGPU_OK;
    // ---- everything a batch needs: the run's counts | its indices | its length, the dense array on rank 0 ----
    ProfileGather g{comm, t, canonicalise};
    rc = g.prepare(n - k + 1, true, true);
    rc = comm_agree_to_start(comm, rc, gathered_peer_error(comm, c, "profile gathered", "a batch of %zu window starts", g.batch));
    if (rc) return rc;
    // ---- the batches.  From here on a rank that fails raises the communicator's abort flag: its peers' waits end (comm_agree_done) ----
    rc = comm_agree_done(comm, g.gather(bases, nullptr, n, counts, nullptr), "profile gathered: rank %d failed");
    if (rc) return rc;
    g.print_timing();
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
    if (!t || !records_usable(dev_bases, n, dev_rec_start, dev_rec_len, n_rec) || (n_rec && !dev_hits)) return KATGPU_ERR_INVALID_ARG;
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
    if (!t || !records_usable(bases, n, rec_start, rec_len, n_rec) || (n_rec && !hits)) return KATGPU_ERR_INVALID_ARG;
    if (!n_rec) return KATGPU_OK;
    katgpu_ctx* c = t->ctx;
    int rc = check_records(c, rec_start, rec_len, n_rec, n); if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = refresh_counters(t); if (rc) return rc;
    return for_record_batches(c, bases, n, rec_start, rec_len, n_rec, g_hits_batch, g_hits_recs, 1, "seq hits", nullptr,     // (a word per record: its hits)
                              [](size_t, bool) { return true; },
                              [&](const uint8_t* db, size_t nb, const uint64_t* ds, const uint64_t* dl, size_t m, size_t r0, uint64_t* d_hits) {
        int rc = launch_seq_hits(t, db, nb, ds, dl, m, canonicalise, d_hits);
        if (rc) return rc;
        const hipError_t e = hipMemcpyAsync(hits + r0, d_hits, m * 8, hipMemcpyDeviceToHost, c->stream);
        return e == hipSuccess ? KATGPU_OK : fail(c, KATGPU_ERR_DEVICE, "seq hits: %s", hipGetErrorString(e));
    });
}

// ------------------------------------------------------------------ the hits of a table that lies on several ranks ----

static const int64_t g_hits_gather_nomem = hook("KATGPU_TEST_HITS_GATHER_NOMEM") ? atoll(hook("KATGPU_TEST_HITS_GATHER_NOMEM")) : -1;   // tests: this rank reports that it could not allocate

// Collective, after katgpu_exchange_merge: every rank walks the same records in the batches of katgpu_table_seq_hits_host (for_record_batches:
// at most g_hits_batch bases and g_hits_recs records) and counts, per record, the hits among the windows whose k-mer it owns
// (k_seq_hits_owned).  Hits add across owners, so what travels is a record's count: the other ranks send the batch's m words to rank 0,
// which receives them behind one another, adds them to its own (k_hits_sum) and copies the sums to `hits`: 8 bytes per record and
// rank on the wire, none per window.  The batches are cut from the records, so the ranks first make sure that they hold the same ones.
// From the pool, per record of a batch: world - 1 words of staging on rank 0, and for_record_batches' own buffers -- start, length and hits
// on every rank, beside the batch's bases: a rank that finds no room for those fails inside the batches, where comm_agree_done hears of it.
extern "C" int katgpu_table_seq_hits_gathered_host(katgpu_comm* comm, katgpu_table* t, const char* bases, size_t n, const uint64_t* rec_start,
                                                   const uint64_t* rec_len, size_t n_rec, int canonicalise, uint64_t* hits) {
    if (!comm || !t) return KATGPU_ERR_INVALID_ARG;
    katgpu_ctx* c = t->ctx;
    const int rank = katgpu_comm_rank(comm), world = katgpu_comm_world(comm);
    const uint32_t k = t->dv.k;
    const bool wide = t->dv.keys_b != nullptr;
    // ---- the same records, one k and usable pointers everywhere, before anything else: all ranks go on, or none does ----
    const CallRecords recs{rec_start, rec_len, n_rec};
    int rc = comm_agree_on_call(comm, c, "seq hits gathered", n, k, &recs, !records_usable(bases, n, rec_start, rec_len, n_rec) || (rank == 0 && n_rec && !hits),
                                "was given no bases or no records, or rank 0 no room for the hits");
    if (rc) return rc;
    if (!n_rec) return KATGPU_OK;
    rc = check_records(c, rec_start, rec_len, n_rec, n); if (rc) return rc;          // (the same records everywhere: the same answer)
    // ---- what a batch needs beside for_record_batches' buffers: the other ranks' hits on rank 0 ----
    const size_t cap = std::min(n_rec, g_hits_recs);               // records per batch
    DevBuf stage;
    auto prepare = [&]() -> int {
        HIPCHK(c, hipSetDevice(c->device));
        int rc = refresh_counters(t); if (rc) return rc;
        if (g_hits_gather_nomem == rank || (rank == 0 && world > 1 && stage.pooled(c, (size_t)(world - 1) * cap * sizeof(uint64_t)) != hipSuccess)) {
            (void)hipGetLastError();
            return fail(c, KATGPU_ERR_NOMEM, "seq hits gathered: no device memory for a batch of %zu records", cap);
        }
        return KATGPU_OK;
    };
    rc = comm_agree_to_start(comm, prepare(), gathered_peer_error(comm, c, "seq hits gathered", "a batch of %zu records", cap));
    if (rc) return rc;

    // ---- the batches.  From here on a rank that fails raises the communicator's abort flag: its peers' waits end (comm_agree_done) ----
    uint64_t n_batches = 0, records = 0;
    rc = for_record_batches(c, bases, n, rec_start, rec_len, n_rec, g_hits_batch, cap, 1, "seq hits gathered", "seq hits gathered",
                            [](size_t, bool) { return true; },
                            [&](const uint8_t* db, size_t nb, const uint64_t* ds, const uint64_t* dl, size_t m, size_t r0, uint64_t* d_hits) -> int {
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
    rc = comm_agree_done(comm, rc, "seq hits gathered: rank %d failed");
    if (rc) return rc;
    if (rank == 0 && g_timing)
        fprintf(stderr, "katgpu_timing {\"phase\": \"seq_hits_gathered\", \"batches\": %llu, \"ranks\": %d, \"records\": %llu, \"wire_bytes\": %llu}\n",
                (unsigned long long)n_batches, world, (unsigned long long)records, (unsigned long long)(8 * records * (uint64_t)(world - 1)));
    return KATGPU_OK;
}
