// kg_jf_device.hip -- the device side of the .jf writer and reader (kg_jf.cpp): a table's records selected, ordered by their position in
// the file and packed (katgpu_table_jf_records_device[_wide]; jf_stream_records, range by range into a file; jf_stream_gathered,
// the same for the disjoint tables of a communicator's ranks, their runs gathered on rank 0's device), and packed records unpacked and
// added to a table (katgpu_table_add_jf_records_device; jf_stream_load, chunk by chunk out of a file).
#include "kg_host.hpp"
#include "kg_comm.hpp"
#include "kg_jf_records.hpp"
#include "kg_jf_load.hpp"
#include "kg_jf.hpp"

// ------------------------------------------------------------------ .jf records in file order ----

// (the pool may be sitting on freed table arrays: give them back before giving up)
static hipError_t jf_malloc(katgpu_ctx* c, void** p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); pool_trim(c); e = hipMalloc(p, bytes); if (e != hipSuccess) (void)hipGetLastError(); }
    return e;
}

namespace {
// device scratch of the record producer, kept across the ranges of one dump
struct JfScratch {
    uint32_t* hist = nullptr; size_t nb_cap = 0;         // hist[nb_cap], cursor[nb_cap], off[nb_cap + 1]
    uint64_t* recs = nullptr; size_t rec_cap = 0;        // pos[rec_cap], (wide: hi[rec_cap],) key[rec_cap], then 32-bit counts: jf_scratch_bytes per record
    uint32_t* rank = nullptr; size_t rank_cap = 0;       // buckets beyond one LDS tile only
    ~JfScratch() { hipFree(hist); hipFree(recs); hipFree(rank); }
    template <typename T>
    bool ensure(katgpu_ctx* c, T*& p, size_t& have, size_t want, size_t bytes_for_want) {
        if (have >= want) return true;
        hipFree(p); p = nullptr; have = 0;
        if (jf_malloc(c, (void**)&p, bytes_for_want) != hipSuccess) return false;
        have = want;
        return true;
    }
};
struct JfRange { uint64_t lo, hi, n; };
struct JfRuns { const uint8_t* recs; uint64_t n; };   // n packed records of the table's k in device memory, from any byte address on: sorted runs behind one another
template <bool W> constexpr size_t jf_scratch_bytes = W ? 28 : 20;
}

// the columns of M ("matrix1": bit i of the k-mer selects column 2k-1-i) as rows over the key bits
template <bool W>
static JfRows<W> jf_rows(uint32_t k, uint32_t r, const uint64_t* cols) {
    JfRows<W> m{};
    const uint32_t c = 2 * k;
    for (uint32_t j = 0; j < r; ++j)
        for (uint32_t i = 0; i < c; ++i) {
            const uint64_t bit = (cols[c - 1 - i] >> j) & 1ULL;
            if (i < 64) m.row[j] |= bit << i;
            else if constexpr (W) m.row_hi[j] |= bit << (i - 64);
        }
    return m;
}

// buckets of 2^shift positions: at most JF_BUCKET_MEAN expected records each when `distinct` records spread evenly over 2^r positions
static uint32_t jf_bucket_shift(uint64_t distinct, uint32_t r) {
    uint32_t s = 0;
    while (s < r && std::ldexp((double)std::max<uint64_t>(distinct, 1), (int)s + 1) <= std::ldexp((double)JF_BUCKET_MEAN, (int)r)) ++s;
    return s;
}

// J1 over either source: the table's slots, or (runs) packed records in device memory
template <int MODE, bool W>
static void jf_launch_select(katgpu_table* t, const JfRuns* runs, const JfRows<W>& m, uint32_t r, uint64_t pos_lo, uint64_t pos_hi, uint32_t shift,
                             uint32_t* hist_or_cursor, unsigned long long* total, uint64_t* d_pos, uint64_t* d_hi, uint64_t* d_key, uint32_t* d_cnt) {
    katgpu_ctx* c = t->ctx;
    if (runs) {
        const dim3 grid((unsigned)std::max<uint64_t>(std::min<uint64_t>((runs->n + JR_TILE - 1) / JR_TILE, (uint64_t)c->n_cu * 8), 1));
        hipLaunchKernelGGL((k_jf_select_runs<MODE, W>), grid, dim3(JF_BLOCK), 0, c->stream, runs->recs, runs->n, 2 * t->dv.k, m, r, pos_lo, pos_hi, shift,
                           hist_or_cursor, total, d_pos, d_hi, d_key, d_cnt);
    } else
        hipLaunchKernelGGL((k_jf_select<MODE, W>), dim3(grid_for(c, t->dev().cap + 1, JF_BLOCK, 8)), dim3(JF_BLOCK), 0, c->stream, t->dev(), t->n_ovf, m, r, pos_lo, pos_hi, shift,
                           hist_or_cursor, total, d_pos, d_hi, d_key, d_cnt);
}
template <bool W>
static void jf_launch_select_hist(katgpu_table* t, const JfRows<W>& m, uint32_t r, uint64_t pos_lo, uint64_t pos_hi, uint32_t shift, uint32_t* hist, const JfRuns* runs = nullptr) {
    jf_launch_select<0, W>(t, runs, m, r, pos_lo, pos_hi, shift, hist, nullptr, nullptr, nullptr, nullptr, nullptr);
}

// Select, order and pack the records of [pos_lo, pos_hi) into dev_out (room for `cap` records).  Synchronises once, to learn how many
// the range holds (*n_out); the scatter, the sort and the pack are left running on the compute stream.  The records are the table's, or
// (runs) those of packed runs, of t's k, no two of them equal: t then lends its context and the result slot of its counters.
template <bool W>
static int jf_range(katgpu_table* t, const JfRows<W>& m, uint32_t r, uint32_t shift, uint64_t pos_lo, uint64_t pos_hi, uint8_t* dev_out, size_t cap,
                    size_t* n_out, JfScratch& s, const JfRuns* runs = nullptr) {
    katgpu_ctx* c = t->ctx;
    *n_out = 0;
    if (pos_lo == pos_hi) return KATGPU_OK;
    const uint64_t nb64 = ((pos_hi - pos_lo - 1) >> shift) + 1;
    if (nb64 >= (1ULL << 31)) return fail(c, KATGPU_ERR_INVALID_ARG, "jf records: a range of %llu buckets: ask for a narrower one", (unsigned long long)nb64);
    const uint32_t nb = (uint32_t)nb64;
    if (!s.ensure(c, s.hist, s.nb_cap, (size_t)nb, ((size_t)nb * 3 + 1) * sizeof(uint32_t))) return fail(c, KATGPU_ERR_NOMEM, "jf records: no device memory for %u bucket counters", nb);
    uint32_t *hist = s.hist, *cursor = s.hist + s.nb_cap, *off = s.hist + 2 * s.nb_cap;
    unsigned long long* res = (unsigned long long*)&t->dev().ctrs[CTR_SCRATCH];
    const DevTable dv = t->dev();
    HIPCHK(c, hipMemsetAsync(hist, 0, (size_t)nb * sizeof(uint32_t), c->stream));
    jf_launch_select_hist(t, m, r, pos_lo, pos_hi, shift, hist, runs);
    hipLaunchKernelGGL(k_jf_scan, dim3(1), dim3(JF_SCAN_BLOCK), 0, c->stream, hist, nb, off, cursor, res);
    unsigned long long h[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(h, res, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *n_out = (size_t)h[0];
    if (!h[0]) return KATGPU_OK;
    if (h[0] > cap) return fail(c, KATGPU_ERR_INVALID_ARG, "jf records: the range holds %llu records, the buffer %zu", h[0], cap);
    if (h[0] >= (1ULL << 31)) return fail(c, KATGPU_ERR_INVALID_ARG, "jf records: %llu records in one range: ask for a narrower one", h[0]);
    const size_t n = (size_t)h[0];
    if (!s.ensure(c, s.recs, s.rec_cap, n, n * jf_scratch_bytes<W>)) return fail(c, KATGPU_ERR_NOMEM, "jf records: no device memory to order %zu records", n);
    uint64_t *d_pos = s.recs, *d_hi = W ? s.recs + s.rec_cap : nullptr, *d_key = s.recs + (W ? 2 : 1) * s.rec_cap;
    uint32_t* d_cnt = (uint32_t*)(d_key + s.rec_cap);
    const uint32_t key_bytes = (2 * dv.k + 7) / 8;
    // (none of these launches is booked under a kernel class of katgpu_profile_get: the dump reports its own phases, katgpu_timing "jf_dump")
    jf_launch_select<1, W>(t, runs, m, r, pos_lo, pos_hi, shift, cursor, nullptr, d_pos, d_hi, d_key, d_cnt);
    // The ranking path compares every record of an oversized bucket with the whole bucket.  That is for the odd run of equal positions,
    // not for a matrix that piles a table onto a few of them: beyond JF_RANK_MAX records in one bucket the range is refused.
    if (h[1] > JF_RANK_MAX)
        return fail(c, KATGPU_ERR_INVALID_ARG, "jf records: %llu records share one stretch of 2^%u positions (at most %u are ordered there): the matrix does not spread this table",
                    h[1], shift, JF_RANK_MAX);
    if (h[1] > JF_TILE) {
        if (!s.ensure(c, s.rank, s.rank_cap, n, n * sizeof(uint32_t))) return fail(c, KATGPU_ERR_NOMEM, "jf records: no device memory to rank %zu records", n);
        hipLaunchKernelGGL(k_jf_rank<W>, dim3(grid_for(c, n, JF_BLOCK, 8)), dim3(JF_BLOCK), 0, c->stream, d_pos, d_hi, d_key, (uint32_t)n, pos_lo, shift, off, s.rank);
    }
    hipLaunchKernelGGL(k_jf_sort_pack<W>, dim3(std::min<uint32_t>(nb, (uint32_t)c->n_cu * 5)), dim3(JF_BLOCK), 0, c->stream, d_pos, d_hi, d_key, d_cnt, off, s.rank, nb, key_bytes, dev_out);
    HIPCHK(c, hipGetLastError());
    return KATGPU_OK;
}

// the entry point of either key width, once the table is known to be of that width
template <bool W>
static int jf_records_device(katgpu_table* t, uint32_t r, const uint64_t* cols, uint64_t pos_lo, uint64_t pos_hi, uint8_t* dev_out, size_t cap_records, size_t* n_out) {
    katgpu_ctx* c = t->ctx;
    const uint32_t k = t->dv.k;
    if (r < 1 || r > std::min<uint32_t>(2 * k, 63) || pos_lo > pos_hi || pos_hi > (1ULL << r))
        return fail(c, KATGPU_ERR_INVALID_ARG, "jf records: need 1 <= r <= min(2k, 63) and pos_lo <= pos_hi <= 2^r (r = %u, [%llu, %llu))", r, (unsigned long long)pos_lo, (unsigned long long)pos_hi);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    *n_out = 0;
    const JfRows<W> m = jf_rows<W>(k, r, cols);
    if (!dev_out || !cap_records) {
        unsigned long long* total = (unsigned long long*)&t->dev().ctrs[CTR_SCRATCH];
        HIPCHK(c, hipMemsetAsync(total, 0, sizeof(uint64_t), c->stream));
        jf_launch_select<2, W>(t, nullptr, m, r, pos_lo, pos_hi, 0u, nullptr, total, nullptr, nullptr, nullptr, nullptr);
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

extern "C" int katgpu_table_jf_records_device(katgpu_table* t, uint32_t r, const uint64_t* cols, uint64_t pos_lo, uint64_t pos_hi,
                                              uint8_t* dev_out, size_t cap_records, size_t* n_out) {
    if (!t || !cols || !n_out) return KATGPU_ERR_INVALID_ARG;
    NARROW_ONLY(t, "katgpu_table_jf_records_device: use katgpu_table_jf_records_device_wide;");
    return jf_records_device<false>(t, r, cols, pos_lo, pos_hi, dev_out, cap_records, n_out);
}

extern "C" int katgpu_table_jf_records_device_wide(katgpu_table* t, uint32_t r, const uint64_t* cols, uint64_t pos_lo, uint64_t pos_hi,
                                                   uint8_t* dev_out, size_t cap_records, size_t* n_out) {
    if (!t || !cols || !n_out) return KATGPU_ERR_INVALID_ARG;
    if (!t->dv.keys_b) return fail(t->ctx, KATGPU_ERR_K, "katgpu_table_jf_records_device_wide is for k > 32 tables (k = %u): use katgpu_table_jf_records_device", t->dv.k);
    return jf_records_device<true>(t, r, cols, pos_lo, pos_hi, dev_out, cap_records, n_out);
}

static const uint64_t g_jf_range_records = hook_u64("KATGPU_JF_RANGE_RECORDS", 0);   // tests: many ranges at tiny sizes

template <bool W>
static int jf_stream(katgpu_table* t, uint32_t r, const uint64_t* cols, FILE* f, JfDumpTiming* tm) {
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    const uint64_t distinct = t->distinct;
    if (!distinct) return KATGPU_OK;
    const uint32_t k = t->dev().k, rb = (2 * k + 7) / 8 + 4;
    const JfRows<W> m = jf_rows<W>(k, r, cols);
    const uint32_t shift = jf_bucket_shift(distinct, r);
    JfScratch s;

    // Where to cut: the records per stretch of 2^(r - cb) positions, once; ranges are whole stretches, so what each holds is known.
    const uint32_t cb = std::min<uint32_t>(r, 16), cshift = r - cb;
    const size_t nbins = (size_t)1 << cb;
    if (!s.ensure(c, s.hist, s.nb_cap, nbins, (nbins * 3 + 1) * sizeof(uint32_t))) return KG_JF_NO_SCRATCH;
    std::vector<uint32_t> bins(nbins);
    HIPCHK(c, hipMemsetAsync(s.hist, 0, nbins * sizeof(uint32_t), c->stream));
    jf_launch_select_hist(t, m, r, 0, 1ULL << r, cshift, s.hist);
    HIPCHK(c, hipMemcpyAsync(bins.data(), s.hist, nbins * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));

    // a range's records: 20 bytes (wide: 28) to order them, 4 should they need ranking, its bytes in each of the two output buffers.  Half of what
    // is free, and at most 2^25 records: the pinned buffers are what the host pays (and pinning is not free: kg_host.hpp, ScanCache).
    size_t free_b = 0, total_b = 0;
    HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
    uint64_t want = std::min<uint64_t>(std::max<uint64_t>(free_b / 2 / (jf_scratch_bytes<W> + 4 + 2 * rb), 1 << 16), 1 << 25);
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
    if (max_nb >= (1ULL << 31) || !s.ensure(c, s.hist, s.nb_cap, (size_t)max_nb, ((size_t)max_nb * 3 + 1) * sizeof(uint32_t))) return KG_JF_NO_SCRATCH;
    const int nbuf = ranges.size() > 1 ? 2 : 1;
    JfSlots io(c);                                                // events of a slot: range started, produced, copied
    if (!s.ensure(c, s.recs, s.rec_cap, (size_t)max_n, (size_t)max_n * jf_scratch_bytes<W>) ||
        !io.setup(nbuf, (size_t)max_n * rb, false, [&](void** p, size_t bytes) { return jf_malloc(c, p, bytes); })) return KG_JF_NO_SCRATCH;

    int pend = -1, slot = 0;
    size_t pend_n = 0;
    uint64_t written = 0;
    auto drain = [&]() -> int {                                   // the copy of the range before this one has landed: write it
        if (pend < 0) return KATGPU_OK;
        const hipEvent_t* ev = io.slot[pend].ev;
        HIPCHK(c, hipEventSynchronize(ev[2]));
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) tm->device_s += ms * 1e-3;
        if (hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) tm->copy_s += ms * 1e-3;
        const double t0 = now_ms();
        const bool ok = fwrite(io.slot[pend].pinned, rb, pend_n, f) == pend_n;
        tm->write_s += (now_ms() - t0) * 1e-3;
        written += pend_n; pend = -1;
        return ok ? KATGPU_OK : KATGPU_ERR_IO;
    };
    for (const JfRange& g : ranges) {
        size_t n = 0;
        const JfSlots::Slot& b = io.slot[slot];
        hipEventRecord(b.ev[0], c->stream);
        rc = jf_range(t, m, r, shift, g.lo, g.hi, b.dev, (size_t)max_n, &n, s);
        if (!rc && n != g.n) rc = fail(c, KATGPU_ERR_DEVICE, "jf dump: positions [%llu, %llu) hold %zu records, their histogram said %llu", (unsigned long long)g.lo, (unsigned long long)g.hi, n, (unsigned long long)g.n);
        if (rc == KATGPU_ERR_NOMEM || rc == KATGPU_ERR_INVALID_ARG) rc = KG_JF_NO_SCRATCH;
        if (rc) break;
        if (n) {
            hipEventRecord(b.ev[1], c->stream);
            hipStreamWaitEvent(io.copy, b.ev[1], 0);
            const hipError_t e = hipMemcpyAsync(b.pinned, b.dev, n * rb, hipMemcpyDeviceToHost, io.copy);
            hipEventRecord(b.ev[2], io.copy);
            if (e != hipSuccess) { rc = fail(c, KATGPU_ERR_DEVICE, "jf dump: %s", hipGetErrorString(e)); break; }
        }
        rc = drain();                                             // (while this range is ordered and copied)
        if (rc) break;
        if (n) { pend = slot; pend_n = n; slot = (slot + 1) % nbuf; }
        ++tm->ranges;
    }
    if (!rc) rc = drain();
    if (!rc && written != distinct) rc = fail(c, KATGPU_ERR_DEVICE, "jf dump: wrote %llu of %llu records", (unsigned long long)written, (unsigned long long)distinct);
    return rc;
}

int jf_stream_records(katgpu_table* t, uint32_t r, const uint64_t* cols, FILE* f, JfDumpTiming* tm) {
    return t->dv.keys_b ? jf_stream<true>(t, r, cols, f, tm) : jf_stream<false>(t, r, cols, f, tm);
}

// ------------------------------------------------------------------ .jf records of several ranks' tables ----

static const int64_t g_jf_gather_nomem = hook("KATGPU_TEST_JF_GATHER_NOMEM") ? atoll(hook("KATGPU_TEST_JF_GATHER_NOMEM")) : -1;   // tests: this rank reports that it could not allocate

// The ranks' tables hold disjoint k-mers: every rank orders and packs its records of a range of positions (jf_range), the runs travel
// to rank 0 (one grouped transfer per range), which orders and packs their union from the runs (jf_range over JfRuns, buckets sized
// for n_total) and streams it into the file as jf_stream does.  kg_jf.hpp says what the callers see.
template <bool W>
static int jf_gather(katgpu_comm* m, katgpu_table* t, uint32_t r, const uint64_t* cols, uint64_t n_total, const std::function<FILE*()>& open, JfGatherTiming* tm) {
    katgpu_ctx* c = t->ctx;
    const int rank = katgpu_comm_rank(m), world = katgpu_comm_world(m);
    const uint32_t k = t->dv.k, rb = (2 * k + 7) / 8 + 4;
    const JfRows<W> rows = jf_rows<W>(k, r, cols);
    JfScratch s;
    int who = -1;
    FILE* f = nullptr;
    uint64_t written = 0;
    std::vector<JfRange> ranges;
    std::vector<uint64_t> per_rank;                               // [world x n_ranges]: the records of rank p in range g
    // (what went wrong on this rank is kept until everyone has heard of it: comm_agree_to_start)
    auto current = [&]() -> int { HIPCHK(c, hipSetDevice(c->device)); return refresh_counters(t); };
    int rc = current();
    const uint64_t distinct = rc ? 0 : t->distinct;
    // senders size their buckets for their own records, rank 0 for the union it orders (its own run comes out the same under either)
    const uint32_t shift = jf_bucket_shift(rank == 0 ? n_total : distinct, r);

    // ---- cuts everyone agrees on: the all-reduced histogram over 2^min(r, 16) stretches, cut from rank 0's target of records per range ----
    const uint32_t cb = std::min<uint32_t>(r, 16), cshift = r - cb;
    const size_t nbins = (size_t)1 << cb;
    std::vector<uint32_t> bins(nbins, 0);
    std::vector<uint64_t> all(nbins + 1, 0);
    auto histogram = [&]() -> int {
        if (!distinct) return KATGPU_OK;
        if (!s.ensure(c, s.hist, s.nb_cap, nbins, (nbins * 3 + 1) * sizeof(uint32_t))) return fail(c, KATGPU_ERR_NOMEM, "jf dump: no device memory for %zu position counters", nbins);
        HIPCHK(c, hipMemsetAsync(s.hist, 0, nbins * sizeof(uint32_t), c->stream));
        jf_launch_select_hist(t, rows, r, 0, 1ULL << r, cshift, s.hist);
        HIPCHK(c, hipMemcpyAsync(bins.data(), s.hist, nbins * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        uint64_t sum = 0;
        for (uint32_t b : bins) sum += b;
        if (sum != distinct) return fail(c, KATGPU_ERR_DEVICE, "jf dump: the position histogram holds %llu records, the table %llu", (unsigned long long)sum, (unsigned long long)distinct);
        return KATGPU_OK;
    };
    if (!rc) rc = histogram();
    if (rc) std::fill(bins.begin(), bins.end(), 0);
    for (size_t b = 0; b < nbins; ++b) all[b] = bins[b];
    if (rank == 0) {
        // a range's records on rank 0: 20 bytes (wide: 28) to order them, 4 should they need ranking, their bytes as gathered runs and in each of the
        // two output buffers.  Half of what is free, and at most 2^25 records, as jf_stream has it.
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); free_b = 0; }
        uint64_t want = std::min<uint64_t>(std::max<uint64_t>(free_b / 2 / (jf_scratch_bytes<W> + 4 + 3 * rb), 1 << 16), 1 << 25);
        if (g_jf_range_records) want = g_jf_range_records;
        all[nbins] = want;
    }
    int crc = katgpu_allreduce_u64(m, all.data(), all.size());
    if (crc) return rc ? rc : crc;                                // (the communicator itself failed: its waits have ended on every rank)
    rc = comm_agree_to_start(m, rc, [&](int p, int code) {        // (no memory for the position counters is as collective as the agreement below)
        if (code == KATGPU_ERR_NOMEM) return fail(c, code, "jf dump: rank %d of %d has no device memory for its position counters", p, world);
        return fail(c, code, "jf dump: rank %d could not read its table's positions", p);
    });
    if (rc) return rc;
    {
        const uint64_t want = std::max<uint64_t>(all[nbins], 1);
        uint64_t acc = 0, start = 0, sum = 0;
        for (size_t b = 0; b < nbins; ++b) {
            if (acc && acc + all[b] > want) { ranges.push_back({start << cshift, (uint64_t)b << cshift, acc}); start = b; acc = 0; }
            acc += all[b]; sum += all[b];
        }
        ranges.push_back({start << cshift, 1ULL << r, acc});
        if (sum != n_total) return fail(c, KATGPU_ERR_DEVICE, "jf dump: the ranks' position histograms hold %llu records, their tables %llu", (unsigned long long)sum, (unsigned long long)n_total);
    }
    const size_t G = ranges.size();
    per_rank.assign((size_t)world * G, 0);
    for (size_t g = 0; g < G; ++g)
        for (uint64_t b = ranges[g].lo >> cshift; b < (ranges[g].hi >> cshift); ++b) per_rank[(size_t)rank * G + g] += bins[b];
    crc = katgpu_allreduce_u64(m, per_rank.data(), per_rank.size());     // every receive's size is known before it is posted
    if (crc) return crc;
    auto of = [&](int p, size_t g) { return per_rank[(size_t)p * G + g]; };

    // ---- everything a range can need, before a byte is written: all ranks go on, or none does ----
    uint64_t max_all = 0, max_own = 0, max_gather = 0, max_nb = 1;
    for (size_t g = 0; g < G; ++g) {
        max_all = std::max(max_all, ranges[g].n); max_own = std::max(max_own, of(rank, g));
        if (ranges[g].n > of(0, g)) max_gather = std::max(max_gather, ranges[g].n);
        max_nb = std::max(max_nb, ((ranges[g].hi - ranges[g].lo - 1) >> shift) + 1);
    }
    const uint64_t max_n = rank == 0 ? max_all : max_own;         // the most records this rank orders at once
    const int nbuf = G > 1 ? 2 : 1;
    JfSlots io(c);                                                // rank 0: events of a slot: range started, produced, copied; senders: one device buffer, their run
    struct Dev { uint8_t* p = nullptr; ~Dev() { hipFree(p); } } gather;
    hipEvent_t wire_ev[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};   // rank 0, per slot: its own run done, the runs' ordering started
    struct Events { hipEvent_t (&e)[2][2]; ~Events() { for (auto& a : e) for (hipEvent_t x : a) if (x) hipEventDestroy(x); } } wire_events{wire_ev};
    bool have = max_all < (1ULL << 31) && max_nb < (1ULL << 31);  // (a matrix that piles the tables onto one stretch of positions)
    if (have && max_n) have = s.ensure(c, s.hist, s.nb_cap, (size_t)max_nb, ((size_t)max_nb * 3 + 1) * sizeof(uint32_t)) && s.ensure(c, s.recs, s.rec_cap, (size_t)max_n, (size_t)max_n * jf_scratch_bytes<W>) &&
                             s.ensure(c, s.rank, s.rank_cap, (size_t)max_n, (size_t)max_n * sizeof(uint32_t));   // (should a bucket need ranking: nothing is allocated once the file is open)
    if (have && rank == 0) {
        have = io.setup(nbuf, std::max<size_t>((size_t)max_all * rb, 1), false, [&](void** p, size_t bytes) { return jf_malloc(c, p, bytes); });
        if (have && max_gather) have = jf_malloc(c, (void**)&gather.p, (size_t)max_gather * rb) == hipSuccess;
        for (auto& a : wire_ev) for (hipEvent_t& x : a) if (have) have = hipEventCreate(&x) == hipSuccess;
    } else if (have && max_own) have = jf_malloc(c, (void**)&io.slot[0].dev, (size_t)max_own * rb) == hipSuccess;
    if (!have) (void)hipGetLastError();
    if (g_jf_gather_nomem == rank) have = false;
    crc = comm_agree(m, have ? 0 : 1, &who);
    if (crc) return crc;
    if (who >= 0) return fail(c, KATGPU_ERR_NOMEM, "jf dump: rank %d of %d has no device or pinned memory for the buffers of a range (%llu records at most)", who, world, (unsigned long long)max_all);

    // ---- the ranges.  From here on a rank that fails raises the communicator's abort flag: its peers' waits end, and the last
    // agreement tells everyone that the file is not to be trusted (comm_agree_done) ----
    int pend = -1, slot = 0;
    size_t pend_n = 0;
    bool pend_remote = false;
    auto drain = [&]() -> int {                                   // the copy of the range before this one has landed: write it
        if (pend < 0) return KATGPU_OK;
        const hipEvent_t* ev = io.slot[pend].ev;
        HIPCHK(c, hipEventSynchronize(ev[2]));
        float ms = 0;
        if (!pend_remote) { if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) tm->device_s += ms * 1e-3; }
        else {
            if (hipEventElapsedTime(&ms, ev[0], wire_ev[pend][0]) == hipSuccess) tm->device_s += ms * 1e-3;
            if (hipEventElapsedTime(&ms, wire_ev[pend][1], ev[1]) == hipSuccess) tm->device_s += ms * 1e-3;
        }
        if (hipEventElapsedTime(&ms, ev[1], ev[2]) == hipSuccess) tm->copy_s += ms * 1e-3;
        const double t0 = now_ms();
        const bool ok = fwrite(io.slot[pend].pinned, rb, pend_n, f) == pend_n;
        tm->write_s += (now_ms() - t0) * 1e-3;
        written += pend_n; pend = -1;
        if (!ok) { tm->write_failed = true; return fail(c, KATGPU_ERR_IO, "jf dump: short write to the output file"); }
        return KATGPU_OK;
    };
    // this rank's run of a range, ordered and packed into dst
    auto own_run = [&](const JfRange& g, uint64_t expect, uint8_t* dst) -> int {
        size_t n = 0;
        int x = jf_range(t, rows, r, shift, g.lo, g.hi, dst, (size_t)max_n, &n, s);
        if (!x && n != expect) x = fail(c, KATGPU_ERR_DEVICE, "jf dump: positions [%llu, %llu) hold %zu records on rank %d, their histogram said %llu", (unsigned long long)g.lo, (unsigned long long)g.hi, n, rank, (unsigned long long)expect);
        return x;
    };
    // before a transfer: the run to travel is packed, and (rank 0) the range before this one has been read out of the gather buffer
    auto settled = [&]() -> int { HIPCHK(c, hipStreamSynchronize(c->stream)); return KATGPU_OK; };
    // rank 0 opens the file, and everyone hears of it before a run is posted: a sender must not be left with a transfer nobody takes
    crc = comm_agree(m, rank == 0 && !(f = open()) ? 1 : 0, &who);
    if (crc) return crc;
    if (who >= 0) return fail(c, KATGPU_ERR_IO, "jf dump: rank 0 cannot open the output file");
    for (size_t gi = 0; !rc && gi < G && n_total; ++gi) {
        const JfRange& g = ranges[gi];
        const uint64_t own = of(rank, gi), remote = g.n - of(0, gi);
        if (rank != 0) {
            if (own) rc = own_run(g, own, io.slot[0].dev);
            if (!rc && own) rc = settled();
            std::vector<CommMsg> sends;
            if (own) sends.push_back({0, io.slot[0].dev, (size_t)own * rb});
            if (!rc && remote) rc = transfer_sync(m, sends, {});
            continue;
        }
        const JfSlots::Slot& b = io.slot[slot];
        hipEventRecord(b.ev[0], c->stream);
        if (own) rc = own_run(g, own, remote ? gather.p : b.dev);
        if (!rc && remote) {
            // the remote runs behind rank 0's own, in rank order: a run starts wherever the one before it ended
            hipEventRecord(wire_ev[slot][0], c->stream);
            rc = settled();
            if (rc) break;
            std::vector<CommMsg> recvs;
            uint64_t at = own;
            for (int p = 1; p < world; ++p) { recvs.push_back({p, gather.p + at * rb, (size_t)of(p, gi) * rb}); at += of(p, gi); }
            const double t0 = now_ms();
            rc = transfer_sync(m, {}, recvs);
            tm->wire_s += (now_ms() - t0) * 1e-3;
            if (rc) break;
            hipEventRecord(wire_ev[slot][1], c->stream);
            const JfRuns runs{gather.p, g.n};
            size_t n = 0;
            rc = jf_range(t, rows, r, shift, g.lo, g.hi, b.dev, (size_t)max_n, &n, s, &runs);
            if (!rc && n != g.n) rc = fail(c, KATGPU_ERR_DEVICE, "jf dump: %zu of the %llu gathered records lie in positions [%llu, %llu)", n, (unsigned long long)g.n, (unsigned long long)g.lo, (unsigned long long)g.hi);
        }
        if (rc) break;
        if (g.n) {
            hipEventRecord(b.ev[1], c->stream);
            hipStreamWaitEvent(io.copy, b.ev[1], 0);
            const hipError_t e = hipMemcpyAsync(b.pinned, b.dev, g.n * rb, hipMemcpyDeviceToHost, io.copy);
            hipEventRecord(b.ev[2], io.copy);
            if (e != hipSuccess) { rc = fail(c, KATGPU_ERR_DEVICE, "jf dump: %s", hipGetErrorString(e)); break; }
        }
        rc = drain();                                             // (while this range is ordered and copied)
        if (rc) break;
        if (g.n) { pend = slot; pend_n = (size_t)g.n; pend_remote = remote != 0; slot = (slot + 1) % nbuf; }
        ++tm->ranges;
    }
    if (rank == 0 && f) {
        if (!rc) rc = drain();
        if (!rc && written != n_total) rc = fail(c, KATGPU_ERR_DEVICE, "jf dump: wrote %llu of %llu records", (unsigned long long)written, (unsigned long long)n_total);
    }
    return comm_agree_done(m, rc, "jf dump: rank %d failed, the file is incomplete");      // (no memory now is not the collective kind: the file is open)
}

int jf_stream_gathered(katgpu_comm* m, katgpu_table* t, uint32_t r, const uint64_t* cols, uint64_t n_total, const std::function<FILE*()>& open, JfGatherTiming* tm) {
    return t->dv.keys_b ? jf_gather<true>(m, t, r, cols, n_total, open, tm) : jf_gather<false>(m, t, r, cols, n_total, open, tm);
}

// ------------------------------------------------------------------ .jf records into a table ----

// n packed records at dev_recs added to t, with room made the way katgpu_table_merge_device makes it (add_in_rooms): with *unseen
// carried from chunk to chunk, a caller that feeds one after another synchronises only where the table may have to grow.
static int jf_add_records(katgpu_table* t, const uint8_t* dev_recs, size_t n, uint32_t key_len, uint32_t counter_len, uint64_t* unseen) {
    katgpu_ctx* c = t->ctx;
    const uint32_t rb = (key_len + 7) / 8 + counter_len;
    return add_in_rooms(t, n, unseen, [&](size_t pos, uint64_t take) {
        {
            ScopedTimer tm(c, KATGPU_K_MERGE, take);
            const dim3 grid((unsigned)std::min<uint64_t>((take + JL_TILE - 1) / JL_TILE, (uint64_t)c->n_cu * 8));
            if (t->dev().keys_b) hipLaunchKernelGGL(k_jf_add<true>, grid, dim3(JL_BLOCK), 0, c->stream, t->dev(), dev_recs + pos * rb, (uint64_t)take, key_len, counter_len);
            else hipLaunchKernelGGL(k_jf_add<false>, grid, dim3(JL_BLOCK), 0, c->stream, t->dev(), dev_recs + pos * rb, (uint64_t)take, key_len, counter_len);
        }
        HIPCHK(c, hipGetLastError());
        return (int)KATGPU_OK;
    });
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
    const int nbuf = n > chunk ? 2 : 1;
    bool used[2] = {false, false};
    JfSlots io(c);                                                // events of a slot: copy started, copied, add started, added
    if (!io.setup(nbuf, chunk * rb, true, [&](void** p, size_t bytes) { return pool_alloc(c, p, bytes); })) return KG_JF_NO_SCRATCH;

    auto collect = [&](int slot) -> int {                         // the chunk that went through this slot has been added: its buffers are free
        if (!used[slot]) return KATGPU_OK;
        const hipEvent_t* ev = io.slot[slot].ev;
        HIPCHK(c, hipEventSynchronize(ev[3]));
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) tm->copy_s += ms * 1e-3;
        if (hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess) tm->device_s += ms * 1e-3;
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
        const JfSlots::Slot& b = io.slot[slot];
        const double t0 = now_ms();
        const bool ok = fread(b.pinned, rb, take, f) == take;
        tm->read_s += (now_ms() - t0) * 1e-3;
        if (!ok) { rc = KATGPU_ERR_IO; break; }
        hipEventRecord(b.ev[0], io.copy);
        const hipError_t e = hipMemcpyAsync(b.dev, b.pinned, take * rb, hipMemcpyHostToDevice, io.copy);
        hipEventRecord(b.ev[1], io.copy);
        if (e != hipSuccess) { rc = fail(c, KATGPU_ERR_DEVICE, "jf load: %s", hipGetErrorString(e)); break; }
        hipStreamWaitEvent(c->stream, b.ev[1], 0);
        hipEventRecord(b.ev[2], c->stream);
        rc = jf_add_records(t, b.dev, take, key_len, counter_len, &unseen);
        hipEventRecord(b.ev[3], c->stream);
        used[slot] = true;
        pos += take;
        ++tm->chunks;
    }
    for (int i = 0; i < nbuf; ++i) { const int x = collect((slot + i) % nbuf); if (!rc) rc = x; }
    return rc ? rc : refresh_counters(t);
}
