// kg_records.hip -- records out of a table and into one: partition sizes / partition / export, merge from device or host arrays (one-word
// keys and their two-word `_wide` twins), and the k-mer filter of `kat filter kmer`, which routes a table's records into one or two new tables.
#include "kg_host.hpp"
#include "kg_kernels.hpp"
#include "kg_wide.hpp"
#include "kg_filter.hpp"

// ------------------------------------------------------------------ partition / export / merge -------

extern "C" int katgpu_table_partition_sizes(katgpu_table* t, uint32_t n_parts, uint64_t* sizes) {
    if (!t || !sizes || n_parts == 0 || n_parts > 4096) return KATGPU_ERR_INVALID_ARG;
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    DevBuf buf; HIPCHK(c, buf.plain(n_parts * 8));
    unsigned long long* d = buf.as<unsigned long long>();
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
    if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "%s", hipGetErrorString(e));
    return KATGPU_OK;
}

extern "C" int katgpu_table_partition(katgpu_table* t, uint32_t n_parts, const uint64_t* offsets, uint64_t* dev_keys, uint64_t* dev_counts) {
    if (!t || !offsets || n_parts == 0 || n_parts > 4096) return KATGPU_ERR_INVALID_ARG;
    NARROW_ONLY(t, "katgpu_table_partition");
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = refresh_counters(t); if (rc) return rc;
    DevBuf buf; HIPCHK(c, buf.plain(n_parts * 8));
    unsigned long long* d = buf.as<unsigned long long>();
    hipMemcpyAsync(d, offsets, n_parts * 8, hipMemcpyHostToDevice, c->stream);
    {
        ScopedTimer tm(c, KATGPU_K_PARTITION, t->dev().cap);
        hipLaunchKernelGGL(k_partition<1>, dim3(grid_for(c, t->dev().cap + 1, 256, 8)), dim3(256), 0, c->stream, t->dev(), t->n_ovf, n_parts, d, dev_keys, dev_counts);
    }
    hipError_t e = hipStreamSynchronize(c->stream);
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
    DevBuf dk, dc;
    HIPCHK(c, dk.plain(t->distinct * 8));
    if (dc.plain(t->distinct * 8) != hipSuccess) return fail(c, KATGPU_ERR_NOMEM, "export buffers");
    uint64_t zero = 0;
    rc = katgpu_table_partition(t, 1, &zero, dk.as<uint64_t>(), dc.as<uint64_t>());
    if (rc) return rc;
    hipError_t e = hipMemcpy(keys, dk.p, t->distinct * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(counts, dc.p, t->distinct * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "export: %s", hipGetErrorString(e));
    return KATGPU_OK;
}

extern "C" int katgpu_table_merge_device(katgpu_table* t, const uint64_t* dev_keys, const uint64_t* dev_counts, size_t n) {
    if (!t || (n && (!dev_keys || !dev_counts))) return KATGPU_ERR_INVALID_ARG;
    NARROW_ONLY(t, "katgpu_table_merge_device");
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    int rc = add_in_rooms(t, n, nullptr, [&](size_t pos, uint64_t take) {
        ScopedTimer tm(c, KATGPU_K_MERGE, take);
        hipLaunchKernelGGL(k_merge, dim3(grid_for(c, take, 256, 8)), dim3(256), 0, c->stream, t->dev(), dev_keys + pos, dev_counts + pos, take);
        return KATGPU_OK;
    });
    if (rc) return rc;
    return refresh_counters(t);
}

extern "C" int katgpu_table_merge_host(katgpu_table* t, const uint64_t* keys, const uint64_t* counts, size_t n) {
    if (!t || (n && (!keys || !counts))) return KATGPU_ERR_INVALID_ARG;
    NARROW_ONLY(t, "katgpu_table_merge_host: use katgpu_table_merge_host_wide;");
    if (!n) return KATGPU_OK;
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf dk, dc;
    HIPCHK(c, dk.plain(n * 8));
    if (dc.plain(n * 8) != hipSuccess) return fail(c, KATGPU_ERR_NOMEM, "merge buffers");
    hipError_t e = hipMemcpy(dk.p, keys, n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dc.p, counts, n * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "merge: %s", hipGetErrorString(e));
    return katgpu_table_merge_device(t, dk.as<uint64_t>(), dc.as<uint64_t>(), n);
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
    DevBuf buf; HIPCHK(c, buf.plain((3 * n + 1) * 8));
    uint64_t* d = buf.as<uint64_t>();
    unsigned long long* cursor = (unsigned long long*)(d + 3 * n);
    hipMemsetAsync(cursor, 0, 8, c->stream);
    hipLaunchKernelGGL(k_export_w, dim3(grid_for(c, t->dev().cap, 256, 8)), dim3(256), 0, c->stream, t->dev(), t->n_ovf, d, d + n, d + 2 * n, cursor);
    hipMemcpyAsync(keys_hi, d, n * 8, hipMemcpyDeviceToHost, c->stream);
    hipMemcpyAsync(keys_lo, d + n, n * 8, hipMemcpyDeviceToHost, c->stream);
    hipMemcpyAsync(counts, d + 2 * n, n * 8, hipMemcpyDeviceToHost, c->stream);
    hipError_t e = hipStreamSynchronize(c->stream);
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
    DevBuf buf; HIPCHK(c, buf.plain(n_parts * 8));
    unsigned long long* d = buf.as<unsigned long long>();
    hipMemcpyAsync(d, offsets, n_parts * 8, hipMemcpyHostToDevice, c->stream);
    {
        ScopedTimer tm(c, KATGPU_K_PARTITION, t->dev().cap);
        hipLaunchKernelGGL(k_partition_w<1>, dim3(grid_for(c, t->dev().cap, 256, 8)), dim3(256), 0, c->stream, t->dev(), t->n_ovf, n_parts, d, dev_hi, dev_lo, dev_counts);
    }
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "%s", hipGetErrorString(e));
    return KATGPU_OK;
}

extern "C" int katgpu_table_merge_device_wide(katgpu_table* t, const uint64_t* dev_hi, const uint64_t* dev_lo, const uint64_t* dev_counts, size_t n) {
    if (!t || (n && (!dev_hi || !dev_lo || !dev_counts))) return KATGPU_ERR_INVALID_ARG;
    katgpu_ctx* c = t->ctx;
    if (!t->dev().keys_b) return fail(c, KATGPU_ERR_K, "katgpu_table_merge_device_wide is for k > 32 tables (k = %u): use katgpu_table_merge_device", t->dev().k);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = add_in_rooms(t, n, nullptr, [&](size_t pos, uint64_t take) {
        ScopedTimer tm(c, KATGPU_K_MERGE, take);
        hipLaunchKernelGGL(k_merge_w, dim3(grid_for(c, take, 256, 8)), dim3(256), 0, c->stream, t->dev(), dev_hi + pos, dev_lo + pos, dev_counts + pos, (uint64_t)take);
        return KATGPU_OK;
    });
    if (rc) return rc;
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
    DevBuf buf; HIPCHK(c, buf.plain(3 * n * 8));
    uint64_t* d = buf.as<uint64_t>();
    hipError_t e = hipMemcpy(d, keys_hi, n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + n, keys_lo, n * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + 2 * n, counts, n * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "merge: %s", hipGetErrorString(e));
    return katgpu_table_merge_device_wide(t, d, d + n, d + 2 * n, n);
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
