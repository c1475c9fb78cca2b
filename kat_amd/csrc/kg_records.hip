// kg_records.hip -- records out of a table and into one: partition sizes / partition / export, merge from device or host arrays (each
// one body for one-word keys and for the two-word keys of the `_wide` entry points), and the k-mer filter of `kat filter kmer`, which
// routes a table's records into one or two new tables.
#include "kg_host.hpp"
#include "kg_record_kernels.hpp"
#include "kg_filter.hpp"

// ------------------------------------------------------------------ partition / export / merge -------
// W: the `_wide` entry point (33 <= k <= 63), whose records have two key columns (RecCols<W>)

// K6 over the table's slots.  MODE 0: d = records per part; MODE 1: d = the parts' cursors, records to `out`
template <int MODE, bool W>
static void launch_partition(katgpu_table* t, uint32_t n_parts, unsigned long long* d, RecCols<W> out) {
    katgpu_ctx* c = t->ctx;
    ScopedTimer tm(c, KATGPU_K_PARTITION, t->dev().cap);
    hipLaunchKernelGGL((k_partition<MODE, W>), dim3(grid_for(c, t->dev().cap + (W ? 0 : 1), 256, 8)), dim3(256), 0, c->stream, t->dev(), t->n_ovf, n_parts, d, out);
}

extern "C" int katgpu_table_partition_sizes(katgpu_table* t, uint32_t n_parts, uint64_t* sizes) {
    if (!t || !sizes || n_parts == 0 || n_parts > 4096) return KATGPU_ERR_INVALID_ARG;
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    DevBuf buf; HIPCHK(c, buf.plain(n_parts * 8));
    unsigned long long* d = buf.as<unsigned long long>();
    hipMemsetAsync(d, 0, n_parts * 8, c->stream);
    launch_wide(t->dev().keys_b != nullptr, [&](auto W) { launch_partition<0, decltype(W)::value>(t, n_parts, d, {}); });
    hipMemcpyAsync(sizes, d, n_parts * 8, hipMemcpyDeviceToHost, c->stream);
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "%s", hipGetErrorString(e));
    return KATGPU_OK;
}

template <bool W>
static int partition_records(katgpu_table* t, uint32_t n_parts, const uint64_t* offsets, RecCols<W> out) {
    if (!t || !offsets || n_parts == 0 || n_parts > 4096) return KATGPU_ERR_INVALID_ARG;
    if constexpr (W) WIDE_ONLY(t, "katgpu_table_partition_wide", "katgpu_table_partition");
    else NARROW_ONLY(t, "katgpu_table_partition");
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    if (t->distinct && out.any_null()) return KATGPU_ERR_INVALID_ARG;
    DevBuf buf; HIPCHK(c, buf.plain(n_parts * 8));
    unsigned long long* d = buf.as<unsigned long long>();
    hipMemcpyAsync(d, offsets, n_parts * 8, hipMemcpyHostToDevice, c->stream);
    launch_partition<1, W>(t, n_parts, d, out);
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "%s", hipGetErrorString(e));
    return KATGPU_OK;
}

extern "C" int katgpu_table_partition(katgpu_table* t, uint32_t n_parts, const uint64_t* offsets, uint64_t* dev_keys, uint64_t* dev_counts) {
    return partition_records<false>(t, n_parts, offsets, {{dev_keys}, dev_counts});
}

extern "C" int katgpu_table_partition_wide(katgpu_table* t, uint32_t n_parts, const uint64_t* offsets, uint64_t* dev_hi, uint64_t* dev_lo, uint64_t* dev_counts) {
    return partition_records<true>(t, n_parts, offsets, {{dev_hi, dev_lo}, dev_counts});
}

// What both exports check before they move anything.  *n: the records to write to `out` (0, with KATGPU_OK: nothing more to do)
template <bool W>
static int export_begin(katgpu_table* t, const RecCols<W>& out, size_t cap, size_t* n_out, size_t* n) {
    *n = 0;
    if (!t || !n_out) return KATGPU_ERR_INVALID_ARG;
    if constexpr (W) WIDE_ONLY(t, "katgpu_table_export_wide", "katgpu_table_export");
    else NARROW_ONLY(t, "katgpu_table_export: use katgpu_table_export_wide;");
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    *n_out = (size_t)t->distinct;
    if (cap == 0) return KATGPU_OK;
    if (cap < t->distinct || out.any_null()) return fail(c, KATGPU_ERR_INVALID_ARG, "export buffer too small: %zu < %llu", cap, (unsigned long long)t->distinct);
    *n = (size_t)t->distinct;
    return KATGPU_OK;
}

extern "C" int katgpu_table_export(katgpu_table* t, uint64_t* keys, uint64_t* counts, size_t cap, size_t* n_out) {
    size_t n;
    int rc = export_begin<false>(t, {{keys}, counts}, cap, n_out, &n);
    if (rc || !n) return rc;
    katgpu_ctx* c = t->ctx;
    DevBuf dk, dc;
    HIPCHK(c, dk.plain(n * 8));
    if (dc.plain(n * 8) != hipSuccess) return fail(c, KATGPU_ERR_NOMEM, "export buffers");
    uint64_t zero = 0;
    rc = katgpu_table_partition(t, 1, &zero, dk.as<uint64_t>(), dc.as<uint64_t>());
    if (rc) return rc;
    hipError_t e = hipMemcpy(keys, dk.p, n * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(counts, dc.p, n * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "export: %s", hipGetErrorString(e));
    return KATGPU_OK;
}

extern "C" int katgpu_table_export_wide(katgpu_table* t, uint64_t* keys_hi, uint64_t* keys_lo, uint64_t* counts, size_t cap, size_t* n_out) {
    size_t n;
    int rc = export_begin<true>(t, {{keys_hi, keys_lo}, counts}, cap, n_out, &n);
    if (rc || !n) return rc;
    katgpu_ctx* c = t->ctx;
    DevBuf buf; HIPCHK(c, buf.plain((3 * n + 1) * 8));
    uint64_t* d = buf.as<uint64_t>();
    unsigned long long* cursor = (unsigned long long*)(d + 3 * n);
    hipMemsetAsync(cursor, 0, 8, c->stream);
    hipLaunchKernelGGL(k_export, dim3(grid_for(c, t->dev().cap, 256, 8)), dim3(256), 0, c->stream, t->dev(), t->n_ovf, RecCols<true>::of(d, n), cursor);
    hipMemcpyAsync(keys_hi, d, n * 8, hipMemcpyDeviceToHost, c->stream);
    hipMemcpyAsync(keys_lo, d + n, n * 8, hipMemcpyDeviceToHost, c->stream);
    hipMemcpyAsync(counts, d + 2 * n, n * 8, hipMemcpyDeviceToHost, c->stream);
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "%s", hipGetErrorString(e));
    return KATGPU_OK;
}

template <bool W>
static int merge_device_records(katgpu_table* t, RecCols<W, const uint64_t> rec, size_t n) {
    if (!t || (n && rec.any_null())) return KATGPU_ERR_INVALID_ARG;
    if constexpr (W) WIDE_ONLY(t, "katgpu_table_merge_device_wide", "katgpu_table_merge_device");
    else NARROW_ONLY(t, "katgpu_table_merge_device");
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = add_in_rooms(t, n, nullptr, [&](size_t pos, uint64_t take) {
        ScopedTimer tm(c, KATGPU_K_MERGE, take);
        hipLaunchKernelGGL(k_merge<W>, dim3(grid_for(c, take, 256, 8)), dim3(256), 0, c->stream, t->dev(), rec.from(pos), take);
        return KATGPU_OK;
    });
    if (rc) return rc;
    return refresh_counters(t);
}

extern "C" int katgpu_table_merge_device(katgpu_table* t, const uint64_t* dev_keys, const uint64_t* dev_counts, size_t n) {
    return merge_device_records<false>(t, {{dev_keys}, dev_counts}, n);
}

extern "C" int katgpu_table_merge_device_wide(katgpu_table* t, const uint64_t* dev_hi, const uint64_t* dev_lo, const uint64_t* dev_counts, size_t n) {
    return merge_device_records<true>(t, {{dev_hi, dev_lo}, dev_counts}, n);
}

// the columns go up one by one into one buffer
template <bool W>
static int merge_host_records(katgpu_table* t, RecCols<W, const uint64_t> rec, size_t n) {
    if (!t || (n && rec.any_null())) return KATGPU_ERR_INVALID_ARG;
    if constexpr (W) WIDE_ONLY(t, "katgpu_table_merge_host_wide", "katgpu_table_merge_host");
    else NARROW_ONLY(t, "katgpu_table_merge_host: use katgpu_table_merge_host_wide;");
    if (!n) return KATGPU_OK;
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    if constexpr (W) {
        const uint32_t k = t->dv.k;
        const uint64_t hi_mask = (1ULL << (2 * k - 64)) - 1;           // 2 <= 2k - 64 <= 62
        for (size_t i = 0; i < n; ++i)
            if (rec.key[0][i] & ~hi_mask) return fail(c, KATGPU_ERR_INVALID_ARG, "record %zu: key wider than 2k = %u bits", i, 2 * k);
    }
    DevBuf buf;
    if (buf.plain((rec.KEYS + 1) * n * 8) != hipSuccess) return fail(c, KATGPU_ERR_NOMEM, "merge buffers");
    const RecCols<W> d = RecCols<W>::of(buf.as<uint64_t>(), n);
    hipError_t e = hipSuccess;
    for (int j = 0; j < rec.KEYS && e == hipSuccess; ++j) e = hipMemcpy(d.key[j], rec.key[j], n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d.count, rec.count, n * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "merge: %s", hipGetErrorString(e));
    return merge_device_records<W>(t, RecCols<W, const uint64_t>::of(buf.as<uint64_t>(), n), n);
}

extern "C" int katgpu_table_merge_host(katgpu_table* t, const uint64_t* keys, const uint64_t* counts, size_t n) {
    return merge_host_records<false>(t, {{keys}, counts}, n);
}

extern "C" int katgpu_table_merge_host_wide(katgpu_table* t, const uint64_t* keys_hi, const uint64_t* keys_lo, const uint64_t* counts, size_t n) {
    return merge_host_records<true>(t, {{keys_hi, keys_lo}, counts}, n);
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
            launch_wide(src.keys_b != nullptr, [&](auto W) {
                constexpr bool WIDE = decltype(W)::value;
                if (separate) hipLaunchKernelGGL((k_filter<true, WIDE>), g, dim3(256), 0, c->stream, dk, dd, src, t->n_ovf, box, invert, ctr);
                else hipLaunchKernelGGL((k_filter<false, WIDE>), g, dim3(256), 0, c->stream, dk, dd, src, t->n_ovf, box, invert, ctr);
            });
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
