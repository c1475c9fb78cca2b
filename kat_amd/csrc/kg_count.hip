// kg_count.hip -- counting: the direct kernel's launches and overflow guard, the partitioned counter's host loop (rounds, passes,
// fall backs, growth beside the arena), the host feeder (pinned staging -> device rings -> count_resident) and the katgpu_count*
// entry points that replace InputHandler::count (lib/src/input_handler.cc:180-202).
#include "kg_host.hpp"
#include "kg_ingest.hpp"
#include "kg_kernels.hpp"
#include "kg_partition.hpp"
#include "kg_partition_wide.hpp"

#include <condition_variable>
#include <deque>
#include <mutex>
#include <thread>

// ------------------------------------------------------------------ counting --------------------------

// test hooks (tests/test_gpu_parity.py): shrink the sweep threshold / the launch size so small inputs exercise them
static const uint64_t g_test_sweep_thr = hook("KATGPU_TEST_SWEEP_THR") ? strtoull(hook("KATGPU_TEST_SWEEP_THR"), nullptr, 10) : 0;
static const uint64_t g_test_max_starts = hook("KATGPU_TEST_MAX_STARTS") ? strtoull(hook("KATGPU_TEST_MAX_STARTS"), nullptr, 10) : 0;

namespace kg {
// Overflow guard for table_inc's unchecked 32-bit adds (KV12 tables; packed tables add checked): every counter >= thr gives thr to
// the side table.  Reports the largest counter left behind (scratch[0], atomicMax) so the host knows how many more unchecked adds are safe.
static __global__ void __launch_bounds__(256)
k_sweep(DevTable t, uint32_t thr, unsigned long long* scratch) {
    uint32_t mx = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < t.cap; i += stride) {
        uint32_t c = t.counts[i];
        if (c >= thr) {
            uint64_t key = t.keys[i];
            uint32_t take = (c / thr) * thr;
            c -= take;
            t.counts[i] = c;
            ovf_add(t, key, take);
        }
        mx = c > mx ? c : mx;
    }
    for (int off = 32; off > 0; off >>= 1) { uint32_t o = __shfl_down(mx, off, 64); mx = o > mx ? o : mx; }
    if ((threadIdx.x & 63) == 0) atomicMax(scratch, (unsigned long long)mx);
}
}  // namespace kg

// k_count adds with no-return atomics and cannot see a 32-bit wrap; make one impossible.  Invariant: every counter
// <= count_bound + unchecked_adds.  When the next launch could break "<= 2^32-1", k_sweep moves multiples of thr out of
// the large counters into the side table and reports the new maximum.
static int maybe_sweep(katgpu_table* t, uint64_t next_starts) {
    katgpu_ctx* c = t->ctx;
    if (t->dev().cbits) return KATGPU_OK;                          // packed tables take the checked add (kg_device.hpp: table_inc)
    const uint64_t limit = g_test_sweep_thr ? 2 * g_test_sweep_thr - 1 : 0xFFFFFFFFULL;
    if (t->count_bound + t->unchecked_adds + next_starts <= limit) return KATGPU_OK;
    const uint32_t thr = g_test_sweep_thr ? (uint32_t)g_test_sweep_thr : 0x80000000u;
    unsigned long long* scratch = (unsigned long long*)&t->dev().ctrs[CTR_SCRATCH];
    HIPCHK(c, hipMemsetAsync(scratch, 0, sizeof(uint64_t), c->stream));
    {
        ScopedTimer tm(c, KATGPU_K_REGROW, t->dev().cap);
        hipLaunchKernelGGL(k_sweep, dim3(grid_for(c, t->dev().cap, 256, 8)), dim3(256), 0, c->stream, t->dev(), thr, scratch);
    }
    uint64_t mx = 0;
    HIPCHK(c, hipMemcpyAsync(&mx, scratch, sizeof mx, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    t->count_bound = mx;
    t->unchecked_adds = 0;
    return KATGPU_OK;
}

static int launch_count(katgpu_table* t, const uint8_t* dev_bases, size_t n) {
    katgpu_ctx* c = t->ctx;
    if (n < t->dev().k) return KATGPU_OK;
    if (t->dev().keys_b) {                                         // wide k-mers: checked adds, nothing to sweep
        const uint64_t n_chunks = (n + WIDE_CHUNK_STARTS - 1) / WIDE_CHUNK_STARTS;
        const int grid = (int)std::min<uint64_t>(n_chunks, (uint64_t)c->n_cu * 4);
        ScopedTimer tm(c, KATGPU_K_COUNT, n);
        if ((reinterpret_cast<uintptr_t>(dev_bases) & 15) == 0)
            hipLaunchKernelGGL((k_count<true, true>), dim3(grid), dim3(COUNT_BLOCK), 0, c->stream, t->dev(), dev_bases, (uint64_t)n, n_chunks);
        else
            hipLaunchKernelGGL((k_count<false, true>), dim3(grid), dim3(COUNT_BLOCK), 0, c->stream, t->dev(), dev_bases, (uint64_t)n, n_chunks);
        HIPCHK(c, hipGetLastError());
        return KATGPU_OK;
    }
    int src = maybe_sweep(t, n);
    if (src) return src;
    t->unchecked_adds += n;
    const uint64_t n_chunks = (n + CHUNK_STARTS - 1) / CHUNK_STARTS;
    // exactly the resident set: a larger grid leaves a second, thinly populated wave of blocks (measured 12.7 G k-mers/s at
    // 8 blocks/CU requested vs 15.5 at the 6 that were actually resident)
    const int grid = (int)std::min<uint64_t>(n_chunks, (uint64_t)c->n_cu * c->count_blocks_per_cu);
    ScopedTimer tm(c, KATGPU_K_COUNT, n);
    if ((reinterpret_cast<uintptr_t>(dev_bases) & 15) == 0)
        hipLaunchKernelGGL(k_count<true>, dim3(grid), dim3(COUNT_BLOCK), 0, c->stream, t->dev(), dev_bases, (uint64_t)n, n_chunks);
    else
        hipLaunchKernelGGL(k_count<false>, dim3(grid), dim3(COUNT_BLOCK), 0, c->stream, t->dev(), dev_bases, (uint64_t)n, n_chunks);
    HIPCHK(c, hipGetLastError());
    return KATGPU_OK;
}


// ------------------------------------------------------------------ partitioned counter (kg_partition.hpp) ----

static const uint64_t g_part_min_starts = getenv("KATGPU_PART_MIN_STARTS") ? strtoull(getenv("KATGPU_PART_MIN_STARTS"), nullptr, 10) : (32ULL << 20);
static const uint64_t g_test_round_items = hook("KATGPU_TEST_ROUND_ITEMS") ? strtoull(hook("KATGPU_TEST_ROUND_ITEMS"), nullptr, 10) : 0;
// share of the free HBM the partition arena may take (multi-GPU runs may lower it; bench.py sets 0.75 there)
static const double g_arena_fraction = getenv("KATGPU_ARENA_FRACTION") ? std::min(0.95, std::max(0.05, atof(getenv("KATGPU_ARENA_FRACTION")))) : 0.85;
static const uint32_t g_p1_wgs = hook("KATGPU_P1_WGS") ? std::max<uint32_t>(1, (uint32_t)strtoul(hook("KATGPU_P1_WGS"), nullptr, 10)) : 3;   // level-1 workgroups per CU
// level 1 without its counting pass (kg_partition.hpp: k_p1v2_scatter<true>, one fixed-capacity segment per workgroup and bucket):
// 0 = never, 1 = for rounds of at least 64 M k-mers (the default), 2 = always (tests)
static const uint32_t g_l1_fast = hook("KATGPU_L1_FAST") ? (uint32_t)strtoul(hook("KATGPU_L1_FAST"), nullptr, 10) : 1;
static const uint32_t g_test_l1_cpb = hook("KATGPU_TEST_L1_CPB") ? (uint32_t)strtoul(hook("KATGPU_TEST_L1_CPB"), nullptr, 10) : 0;   // tests: segment capacity (forces overflow)
// level 2 without its histogram pass (kg_partition.hpp: k_p2_fast): 0 = never, 1 = when the mean run is long enough for the
// capacity slack to cover the noise, 2 = always (tests).  KATGPU_TEST_P2_OVF_CAP shrinks the overflow list (tests: forces the
// fall back to the exact kernel).
static const uint32_t g_p2_fast = hook("KATGPU_P2_FAST") ? (uint32_t)strtoul(hook("KATGPU_P2_FAST"), nullptr, 10) : 1;
static const uint64_t g_test_p2_ovf_cap = hook("KATGPU_TEST_P2_OVF_CAP") ? strtoull(hook("KATGPU_TEST_P2_OVF_CAP"), nullptr, 10) : 0;
static const uint32_t g_test_spill_mod = hook("KATGPU_TEST_SPILL_MOD") ? (uint32_t)strtoul(hook("KATGPU_TEST_SPILL_MOD"), nullptr, 10) : 0;
static const uint64_t g_test_ap_seg = hook_u64("KATGPU_TEST_AP_SEG", 0) & ~3ULL;   // tests: k-mers per walk segment of the apply kernels (several segments per run)
static const uint32_t g_apply_per_cu = (uint32_t)hook_u64("KATGPU_APPLY_PER_CU", 0);   // A/B: packed apply workgroups per CU (0: as many as the LDS holds)
static const uint64_t g_fresh_max_pct = hook_u64("KATGPU_FRESH_MAX_PCT", 100);   // A/B: a packed table's first round claims inline below this many items per 100 slots (launch_apply)
static const bool g_l1b_stamp = hook_u64("KATGPU_L1B_STAMP", 0) != 0;   // diagnostic: level 1's block edition with cycle stamps (printed per round)
static const bool g_p2x_stamp = hook_u64("KATGPU_P2X_STAMP", 0) != 0;   // diagnostic: kg_l2_blocks.hpp's kernel with cycle stamps (printed per pass)
static const bool g_p2_stamp = hook_u64("KATGPU_P2_STAMP", 0) != 0;   // diagnostic: the one-pass level 2 of 5-byte items from groups with cycle stamps (printed per pass)
static const bool g_apply_stamp = hook_u64("KATGPU_APPLY_STAMP", 0) != 0;              // diagnostic: the bench-shape apply, and a first round's small-region shape, with cycle stamps (printed per pass)

static bool part_geometry(const DevTable& d, PartGeom* g) {
    g->R = d.n_regions; g->S = d.region_slots; g->P1 = d.p1; g->P2 = d.p2; g->l2 = d.l2;
    g->b_lo = 0; g->b_hi = d.p1;
    g->l1_stride = 0; g->l1_real = 0; g->spill_cap = 0; g->l2_trim = 0;        // (a round's: count_partitioned)
    g->pl = place_make(d.k, d.p1, d.n1, d.l2);
    g->hb = l2_hi_bytes(g->pl.rb);
    g->hb1 = l2_hi_bytes(g->pl.n1);
    g->cbits = d.cbits;
    if (d.cbits && g->hb > 2) g->hb = 2;                       // (a packed table's remainder has at most 44 bits)
    // the apply kernels hold a region of whole 16-byte lines, at least a wave's worth of slots, in LDS
    return d.k <= 32 && g->pl.rb <= 63 /* all-ones is "no item" */ && g->P1 <= MAX_PARTS && g->P2 <= MAX_PARTS && g->S % 4 == 0 && g->S >= 64 && g->S <= AP2_MAX_SLOTS;
}
// (bytes of partition arena per k-mer of a round, by shape: kg_arena_plan.hpp)
static_assert(PLAN_MAX_PARTS == MAX_PARTS && PLAN_L1_TILE_STARTS == P1_TILE_STARTS && PLAN_L1B_TILE_STARTS == L1B_TILE_STARTS && PLAN_L1B_ITEMS == L1B_ITEMS && PLAN_L1B_BYTES == L1B_BYTES,
              "kg_arena_plan.hpp's copies of the kernels' constants");
// buckets per pass of level 2 + apply: a CU-full when the buckets are a whole number of those (alloc_dev_table sees to it), else all
static const uint32_t g_test_pass_buckets = hook("KATGPU_TEST_PASS_BUCKETS") ? (uint32_t)strtoul(hook("KATGPU_TEST_PASS_BUCKETS"), nullptr, 10) : 0;   // tests: passes of this many buckets
static uint32_t pass_buckets(uint32_t p1, uint32_t n_cu) {
    if (g_test_pass_buckets) return std::max<uint32_t>(1, std::min(p1, g_test_pass_buckets));
    return n_cu && p1 > n_cu && p1 % n_cu == 0 ? n_cu : p1;
}
// (the level-2 buffer holds one pass = 1 / passes of a round)
// the table's shape selects level 1's block edition (kg_l1_blocks.hpp): plan_level1 runs it, PartArena carves the level-1 buffer for it
static const bool g_l1_lean = hook_u64("KATGPU_L1_LEAN", 1) != 0;   // A/B: 0 = level 1's ranking sweep in its 64-bit form (kg_l1_lean.hpp is the 32-bit one)
static bool l1_blocks_shape(const PartGeom& g, uint32_t k) { return g_l1_lean && lean_applies(k, g.pl.n1) && g.P1 <= 512 && g.hb1 == 2; }

static const bool g_test_grow_nomem = hook("KATGPU_TEST_GROW_NOMEM") != nullptr;   // tests: table growth "fails" while the arena is busy

// keys that found no slot (8 bytes each; 16 for wide tables), in device memory, go in through the direct path
static void insert_keys(katgpu_table* t, const void* keys, uint64_t n, size_t key_bytes) {
    katgpu_ctx* c = t->ctx;
    ScopedTimer tm(c, KATGPU_K_COUNT, n);
    if (key_bytes == 16) hipLaunchKernelGGL(k_insert_keys_w, dim3(grid_for(c, n, 256, 6)), dim3(256), 0, c->stream, t->dev(), (const u64x2*)keys, n);
    else hipLaunchKernelGGL(k_insert_keys, dim3(grid_for(c, n, 256, 6)), dim3(256), 0, c->stream, t->dev(), (const uint64_t*)keys, n);
}
// Growth while a partition call holds the arena.  First with the arena protected; when the device cannot hold the old
// table, the new one and the arena at once, `stash` (spilled keys of key_bytes each that live in the arena, may be empty) is parked
// in host memory, the arena is given up, the growth retried and the keys re-inserted from the host.  *arena_lost tells the
// caller that its carve of the arena is gone.
typedef std::vector<std::pair<const void*, uint64_t>> KeyLists;
static int grow_beside_arena(katgpu_table* t, uint64_t incoming, uint64_t min_cap, const KeyLists& stash, size_t key_bytes, bool* arena_lost) {
    uint64_t n_stash = 0;
    for (auto& l : stash) n_stash += l.second;
    katgpu_ctx* c = t->ctx;
    auto grow = [&]() -> int {
        if (min_cap > t->dev().cap) {
            if (t->disable_grow) return fail(c, KATGPU_ERR_TABLE_FULL, "Hash full");
            uint64_t nc = t->dev().cap; while (nc < min_cap) nc *= 2;
            return regrow(t, nc);
        }
        return ensure_room(t, incoming);
    };
    *arena_lost = false;
    int rc = g_test_grow_nomem ? KATGPU_ERR_NOMEM : grow();
    if (rc != KATGPU_ERR_NOMEM) return rc;
    (void)hipGetLastError();
    std::vector<uint8_t> host;
    if (n_stash) {
        try { host.resize(n_stash * key_bytes); } catch (...) { return fail(c, KATGPU_ERR_NOMEM, "no host memory to park %llu spilled k-mers", (unsigned long long)n_stash); }
        uint64_t at = 0;
        for (auto& l : stash) { HIPCHK(c, hipMemcpy(host.data() + at * key_bytes, l.first, l.second * key_bytes, hipMemcpyDeviceToHost)); at += l.second; }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    release_arena(c);
    *arena_lost = true;
    if (g_trace) fprintf(stderr, "[katgpu] growth beside the partition arena failed: arena released, %llu keys parked on the host\n", (unsigned long long)n_stash);
    rc = grow();
    if (rc) return rc;
    if (n_stash) {
        const size_t chunk = std::min<size_t>(n_stash, ((size_t)256 << 20) / key_bytes);
        uint8_t* d = nullptr;
        HIPCHK(c, pool_alloc(c, (void**)&d, chunk * key_bytes));
        for (size_t i = 0; i < n_stash && rc == KATGPU_OK; i += chunk) {
            const size_t m = std::min(chunk, (size_t)n_stash - i);
            if (hipMemcpyAsync(d, host.data() + i * key_bytes, m * key_bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) { rc = fail(c, KATGPU_ERR_DEVICE, "spill upload"); break; }
            insert_keys(t, d, m, key_bytes);
            if (hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, KATGPU_ERR_DEVICE, "spill insert");
        }
        pool_release(c, d);
    }
    return rc;
}

// The partition arena (katgpu_ctx::arena, kept across calls) for a call that could use want_bytes: small_bytes of histograms and counters +
// item_bytes per k-mer of a round (want_items of them, at most; item_bytes is a rounded-up figure for the "useful round" thresholds below -- 18 for
// 8-byte keys, 32 for wide ones -- not the carve's exact bytes per item).  It is re-allocated only for a substantially larger one (fewer rounds):
// a fresh hipMalloc of this size is not free.  *usable = false: no room for a useful round -- the direct path.
static int ensure_arena(katgpu_ctx* c, size_t small_bytes, size_t item_bytes, size_t want_items, size_t want_bytes, const char* note, bool* usable) {
    *usable = false;
    if (c->arena_limit) want_bytes = std::min(want_bytes, std::max(c->arena_limit, small_bytes + item_bytes * ((size_t)64 << 20)));      // (the file feeders: more rounds, less to allocate)
    if (c->arena_bytes < want_bytes) {                                           // the arena could be more useful than it is
        size_t free_b = 0, total_b = 0;
        HIPCHK(c, hipMemGetInfo(&free_b, &total_b));
        free_b += c->arena_bytes;
        const size_t bytes = std::min<size_t>(want_bytes, (size_t)(g_arena_fraction * (double)free_b));
        if (bytes > c->arena_bytes + c->arena_bytes / 2 || c->arena_bytes < small_bytes + item_bytes * std::min<size_t>(want_items, (size_t)64 << 20)) {
            if (c->arena) { HIPCHK(c, hipFree(c->arena)); c->arena = nullptr; c->arena_bytes = 0; }
            if (!g_test_round_items && bytes < small_bytes + item_bytes * ((size_t)1 << 20)) return KATGPU_OK;
            const double t_ar = now_ms();
            if (hipMalloc((void**)&c->arena, bytes) != hipSuccess) { (void)hipGetLastError(); c->arena = nullptr; return KATGPU_OK; }
            c->arena_bytes = bytes;
            if (g_trace) fprintf(stderr, "[katgpu +%.0f ms] partition arena of %.1f GB%s: %.0f ms\n", since_load(), bytes / 1e9, note, now_ms() - t_ar);
        }
    }
    *usable = true;
    return KATGPU_OK;
}
// a partition call is using the arena: pool_alloc must not free it to satisfy a table growth
struct ArenaBusy { katgpu_ctx* c; explicit ArenaBusy(katgpu_ctx* c_) : c(c_) { c->arena_busy = true; } ~ArenaBusy() { c->arena_busy = false; } };
template <typename T> static T* carve(uint8_t*& a, size_t bytes) { T* p = (T*)a; a += align_up(bytes, 256); return p; }      // (the arena's small arrays: 256-byte steps)

// A launch with dynamic LDS: the kernel's ceiling is raised once per device (c->lds_attr holds the kernels done).
constexpr size_t LDS_BYTES = 160 * 1024, LDS_GRANULE = 1280;     // gfx950: 160 KB per CU, allocated in 320-dword granules
template <typename K, typename... Args>
static int launch_lds(katgpu_ctx* c, K kern, dim3 grid, dim3 block, size_t lds, size_t ceiling, Args... args) {
    if (!c->lds_attr.count(reinterpret_cast<const void*>(kern))) {
        HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ceiling));
        c->lds_attr.insert(reinterpret_cast<const void*>(kern));
    }
    hipLaunchKernelGGL(kern, grid, block, lds, c->stream, args...);
    return KATGPU_OK;
}

// The cycle-stamp diagnostics (KATGPU_L1B_STAMP, _P2X_STAMP, _P2_STAMP, _APPLY_STAMP): a kernel's STAMP instantiation adds its cycles per phase
// into n counters of the arena's small area (`dev`, behind spill_n; the last of the n counts tiles).  They are zeroed in front of the launch,
// fetched after it (a synchronisation: these are diagnostics) and every phase's share of phases [0, n_sum) is printed.  line == nullptr: the
// apply's nine ([0] fill, [1] walk, [2] of it drains, [3] wait for the other waves + sweep, [4] write-back, [5] regions, [6] chunks, [7] drain
// passes, [8] their phase-1 iterations).
struct StampLine { const char* head; int n_shown, n_sum; const char* phase[9]; /* a phase's text around its "%.*f" */ int digits; };
static const StampLine STAMPS_L1B = {"[katgpu] level-1 (blocks) stamps (wave 0 of every workgroup, cycles summed):", 9, 9,
    {" codes %.*f %%", "  blocks out %.*f %%", " (+ barrier %.*f %%)", "  sweep %.*f %%", " (+ %.*f %%)", "  per bucket %.*f %%", " (+ %.*f %%)", "  placing %.*f %%", " (+ %.*f %%)"}, 1};
static const StampLine STAMPS_P2X = {"[katgpu] level-2 (blocks in, blocks out) stamps (wave 0 of every workgroup, cycles summed):", 7, 9,
    {" wait for the tile %.*f %%", " (+ barrier %.*f %%)", "  ranking + blocks out %.*f %%", " (+ %.*f %%)", "  per sub-bucket %.*f %%", " (+ %.*f %%)", "  placing %.*f %%"}, 1};
static const StampLine STAMPS_P2 = {"[katgpu] level-2 stamps (lane 0 of every workgroup, cycles summed):", 5, 5,
    {" wait for the tile %.*f %%", "  digit + rank %.*f %%", "  scan %.*f %%", "  staging %.*f %%", "  copy-out %.*f %%"}, 0};
constexpr int STAMP_AT_APPLY = 8, STAMP_AT = 18;             // where they lie, in counters behind spill_n: the apply's nine, the others' (at most ten)
constexpr int STAMP_AREA = 256 / 8;                          // spill_n's carve is 256 bytes (PartArena::carve_from): 32 counters, the level-1 buffer lies behind them
static_assert(2 <= STAMP_AT_APPLY && STAMP_AT_APPLY + 9 <= STAMP_AT && STAMP_AT + 10 <= STAMP_AREA, "the stamp counters lie behind spill_n and ovf_n, apart, inside spill_n's carve");
template <typename Launch>
static int with_stamps(katgpu_ctx* c, unsigned long long* dev, int n, const StampLine* line, Launch launch) {
    unsigned long long st[10];
    HIPCHK(c, hipMemsetAsync(dev, 0, n * sizeof(unsigned long long), c->stream));
    int rc = launch(dev);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(st, dev, n * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double tot = line ? 0 : (double)(st[0] + st[1] + st[3] + st[4]);
    if (!line && st[5])
        fprintf(stderr, "[katgpu] apply stamps (wave 0 of every workgroup, cycles summed): fill %.3g (%.0f %%)  walk %.3g (%.0f %%; drains %.0f %% of the walk, %.2f iterations per pass)  barrier + sweep %.3g (%.0f %%)  write-back %.3g (%.0f %%); %llu regions, %.1f chunks per wave and region, %.0f cycles per region\n",
                (double)st[0], 100 * st[0] / tot, (double)st[1], 100 * st[1] / tot, 100.0 * st[2] / std::max(1.0, (double)st[1]), (double)st[8] / std::max(1.0, (double)st[7]), (double)st[3], 100 * st[3] / tot, (double)st[4], 100 * st[4] / tot, st[5], (double)st[6] / st[5], tot / st[5]);
    if (!line || !st[n - 1]) return KATGPU_OK;
    for (int i = 0; i < line->n_sum; ++i) tot += (double)st[i];
    char buf[768];
    int at = snprintf(buf, sizeof buf, "%s", line->head);
    for (int i = 0; i < line->n_shown; ++i) at += snprintf(buf + at, sizeof buf - at, line->phase[i], line->digits, 100 * st[i] / tot);
    fprintf(stderr, "%s; %llu tiles, %.0f cycles per tile\n", buf, st[n - 1], tot / st[n - 1]);
    return KATGPU_OK;
}

// Level 3 of a pass: one workgroup per region of buckets [g.b_lo, g.b_hi) -- region into LDS, its run applied, region written back
// (kg_partition.hpp: k_p3_apply_pk for packed tables, k_p3_apply2 for KV12).  A table's first round claims its new k-mers inside
// the probe rounds (INLINE_CLAIM); the test suite's spill hook has its own instantiations.
struct ApplyForm { bool packed; int block, kp; bool fresh /* inline claims */, hooked; };      // the instantiation that ran, for KATGPU_TRACE's "partition forms" line
struct ApplyLaunch {                                         // what every instantiation is launched with
    katgpu_table* t; const PartGeom& g; const uint64_t* off2; const uint8_t* l2_buf; uint64_t* spill_buf; unsigned long long* spill_n; const uint32_t* run_len; const uint64_t* bucket_end;
    dim3 grid; size_t lds; uint32_t qcap; uint64_t seg_len; uint32_t zero_fill; ApplyForm* form;
};
template <int B, int KP, int HB, bool INL, bool HK, bool LATE /* the next region's loads behind the end-of-walk barrier; false: with the wave */, int NR, bool STAMP = false>
static int apply_pk(const ApplyLaunch& a) {
    if (a.form) *a.form = ApplyForm{true, B, KP, INL, HK};
    return launch_lds(a.t->ctx, k_p3_apply_pk<B, KP, HB, INL, HK, LATE, NR, STAMP>, a.grid, dim3(B), a.lds, LDS_BYTES - 256, a.t->dv, a.g, a.off2, a.l2_buf, a.spill_buf, a.spill_n, a.run_len, a.bucket_end,
                      a.qcap, a.seg_len, g_test_spill_mod, a.zero_fill);
}
// probe rounds before the queue: 2 (measured at the bench size, same box: 163 ms per step against 177 with 3 and 198 with inline
// claims in every round; 1 with the drains' window of four slots: apply 115.1 ms against 110.6 with 2, profiles/apply_drain_parent_vs_branch.txt);
// a table's first round claims inline and keeps 3 -- where launch_apply calls it fresh
template <int HB>
static int apply_pk_shape(const ApplyLaunch& a, uint32_t blk, bool fresh, bool hooked) {
    if (hooked) return apply_pk<1024, 5, HB, false, true, true, 3>(a);
    if (blk == 1024) return fresh ? apply_pk<1024, 5, HB, true, false, true, 3>(a) : apply_pk<1024, 5, HB, false, false, true, 2>(a);
    if (a.g.S <= 4096) {
        if (HB == 1 && g_apply_stamp && fresh)               // diagnostic: the small-region shape of a first round (the bench's second input) with cycle stamps
            return with_stamps(a.t->ctx, a.spill_n + STAMP_AT_APPLY, 9, nullptr, [&](unsigned long long*) { return apply_pk<512, 4, 1, true, false, true, 3, true>(a); });
        return fresh ? apply_pk<512, 4, HB, true, false, true, 3>(a) : apply_pk<512, 4, HB, false, false, true, 2>(a);
    }
    if (HB == 1 && g_apply_stamp && !fresh)                  // diagnostic: the bench's shape with cycle stamps (the kernel adds them at spill_n + STAMP_AT_APPLY)
        return with_stamps(a.t->ctx, a.spill_n + STAMP_AT_APPLY, 9, nullptr, [&](unsigned long long*) { return apply_pk<512, 10, 1, false, false, false, 2, true>(a); });
    return fresh ? apply_pk<512, 10, HB, true, false, false, 3>(a) : apply_pk<512, 10, HB, false, false, false, 2>(a);
}
template <int B, int KP, int HB, bool INL, int QC, bool HK>
static int apply_kv12(const ApplyLaunch& a) {
    if (a.form) *a.form = ApplyForm{false, B, KP, INL, HK};
    return launch_lds(a.t->ctx, k_p3_apply2<B, KP, 4, 3, HB, false, INL, true, QC, HK>, a.grid, dim3(B), a.lds, LDS_BYTES - 256, a.t->dev(), a.g, a.off2, a.l2_buf, a.spill_buf, a.spill_n, a.run_len, a.bucket_end,
                      (unsigned long long*)nullptr, g_test_spill_mod, a.seg_len);
}
template <int HB>
static int apply_kv12_shape(const ApplyLaunch& a, uint32_t blk, bool big, bool fresh, bool hooked) {
    if (hooked) return apply_kv12<1024, 5, HB, false, AP2_QCAP_BIG, true>(a);
    if (blk == 512 && a.g.S <= 2048) return fresh ? apply_kv12<512, 2, HB, true, AP2_QCAP, false>(a) : apply_kv12<512, 2, HB, false, AP2_QCAP, false>(a);
    if (blk == 512) return fresh ? apply_kv12<512, 4, HB, true, AP2_QCAP, false>(a) : apply_kv12<512, 4, HB, false, AP2_QCAP, false>(a);
    if (big) return fresh ? apply_kv12<1024, 5, HB, true, AP2_QCAP_BIG, false>(a) : apply_kv12<1024, 5, HB, false, AP2_QCAP_BIG, false>(a);
    return fresh ? apply_kv12<1024, 4, HB, true, AP2_QCAP, false>(a) : apply_kv12<1024, 4, HB, false, AP2_QCAP, false>(a);
}
static int launch_apply(katgpu_table* t, const PartGeom& g, const uint64_t* off2, const uint8_t* l2_buf, uint64_t* spill_buf, unsigned long long* spill_n,
                        const uint32_t* run_len, const uint64_t* bucket_end, uint64_t round_items, ApplyForm* form = nullptr) {
    katgpu_ctx* c = t->ctx;
    const uint32_t n_cu = (uint32_t)c->n_cu, regions = (g.b_hi - g.b_lo) * g.P2;
    bool fresh = t->distinct == 0;                           // (inline claims in a table's first round; a packed table's: see below)
    const bool hooked = g_test_spill_mod != 0;
    ApplyLaunch a{t, g, off2, l2_buf, spill_buf, spill_n, run_len, bucket_end, dim3(1), 0, 0, 0, 0, form};
    int rc = KATGPU_OK;
    if (g.cbits) {
        // 512-thread workgroups, as many per CU as the LDS holds next to their queues (two at the bench's 9344-slot regions, four for
        // small regions); one of 1024 threads when a region leaves no room for a second.  (Four is what the LDS admits and what the grid is sized
        // for; by registers -- 61-72 VGPRs for the small shapes, seven waves per SIMD -- THREE are resident at a time and the rest of the grid follows:
        // two until the region loop stopped holding its slot offsets across the walk, at 85-91 VGPRs; hist, gcp and comp-rr measured the same with
        // three, profiles/apply_period_parent_vs_branch.txt.  A grid of two per CU measured inside the spread when two were resident, step
        // 371.1 -> 370.5 ms: profiles/second_input_parent_vs_branch.txt; four stays.)
        const size_t region_b = (size_t)g.S * 8;
        auto room = [&](uint32_t wgs) -> long { return (long)(LDS_BYTES / wgs / LDS_GRANULE * LDS_GRANULE) - 64 - (long)region_b; };   // bytes left for the queues
        uint32_t per_cu = 4;
        // room for the queues of eight waves: 96 entries each for a third and fourth workgroup, 72 for the second -- a second workgroup is worth
        // short queues (config 5's 9656-slot regions leave exactly 72: apply 103.5 -> 98.2 ms per step against one 1024-thread workgroup)
        auto min_q = [&](uint32_t wgs) -> long { return 8L * 8 * (wgs == 2 ? 72 : 96); };
        while (per_cu > 1 && room(per_cu) < min_q(per_cu)) --per_cu;
        if (g_apply_per_cu) per_cu = std::min(per_cu, g_apply_per_cu);
        uint32_t blk = per_cu == 1 ? 1024 : 512;
        if (hooked) { blk = 1024; per_cu = 1; }
        per_cu = std::min<uint32_t>(per_cu, 2048 / blk);
        const uint32_t nw = blk / 64;
        while (per_cu > 1 && room(per_cu) < (long)(nw * 72 * 8)) --per_cu;
        a.qcap = (uint32_t)std::min<long>(256, room(per_cu) / (long)(nw * 8));
        if (a.qcap < 72) return fail(c, KATGPU_ERR_DEVICE, "a region of %u packed slots leaves no room for the apply kernel's queues", g.S);
        a.lds = region_b + (size_t)nw * a.qcap * 8;
        // Inline claims in a table's first round -- where the round can be mostly new k-mers.  A round of more items than the table has slots is
        // mostly repeats whatever it holds (a deep read set) and takes the steady-state shape, whose claims go through the waves' queues -- if those
        // are of ordinary length: a wave leaves up to 64 entries behind a chunk, so the next chunk's survivors find qcap - 64 places.  Measured
        // per step (profiles/second_input_parent_vs_branch.txt), steady-state against inline: hist and gcp (9 items per slot, 255 entries) apply
        // 19.7 -> 15.3 and 44.0 -> 34.6 ms; the bench's reads (2.5, 111) 2 x 22.9 -> 2 x 21.5; config 5's shard (3.6, the 72 entries that min_q admits
        // for a second workgroup) 79.5 -> 116.5: it keeps inline claims; the bench's assembly (0.62) + 9.7 ms: it does too.  That the queue's length
        // is what sets config 5 apart is SUPPOSED, not measured: it also differs in k, item width and items per slot, and no shape was run with its
        // queue alone shortened.  Between the measured points the limits are min_q's 96 entries and the pigeonhole's one item per slot (no point
        // between 0.62 and 2.5 items per slot was measured).  g_fresh_max_pct is the A/B.  KV12 tables: not measured.
        if (fresh && a.qcap >= 96 && (double)round_items * 100.0 >= (double)g_fresh_max_pct * (double)t->dv.cap) fresh = false;
        const uint64_t seg_cap = (pk_half(g.cbits) - 1) & ~3ULL;                              // a walk adds less than half the count range
        a.seg_len = g_test_ap_seg ? std::min<uint64_t>(g_test_ap_seg, seg_cap) : std::min<uint64_t>(AP2_SEGMENT, seg_cap);
        a.grid = dim3(std::min<uint32_t>(regions, n_cu * per_cu));
        // A table whose slots have not been cleared yet (katgpu_table::zero_from): this pass is their first sweep when its regions are the
        // next in line -- the kernel starts every region of the pass from zeros and writes every one back; else they are cleared now.
        const uint64_t r_lo = (uint64_t)g.b_lo * g.P2, r_hi = (uint64_t)g.b_hi * g.P2;
        if (t->zero_from != ~0ULL) { if (t->zero_from == r_lo) a.zero_fill = 1; else t->zero_rest(); }
        switch (g.hb) {
        case 0: rc = apply_pk_shape<0>(a, blk, fresh, hooked); break;
        case 1: rc = apply_pk_shape<1>(a, blk, fresh, hooked); break;
        case 2: rc = apply_pk_shape<2>(a, blk, fresh, hooked); break;
        default: return fail(c, KATGPU_ERR_DEVICE, "packed apply: item width %u", g.hb);
        }
        if (rc) return rc;
        HIPCHK(c, hipGetLastError());
        if (a.zero_fill) t->zero_from = r_hi >= t->dv.n_regions ? ~0ULL : r_hi;      // (regions [r_lo, r_hi) have had their first sweep)
        return KATGPU_OK;
    }
    // KV12: as many workgroups per CU as the regions' LDS footprint (and the 2048-thread limit) admits
    const uint32_t blk = hooked ? 1024 : (g.S <= 4096 ? 512 : 1024);
    const bool big = g.S > 8192 || hooked;
    a.lds = (size_t)g.S * 12 + (size_t)(blk / 64) * (big ? AP2_QCAP_BIG : AP2_QCAP) * 12;
    const uint32_t per_cu = (uint32_t)std::max<size_t>(1, std::min<size_t>(LDS_BYTES / (a.lds + 512), 2048 / blk));
    a.grid = dim3(std::min<uint32_t>(regions, n_cu * per_cu));
    a.seg_len = g_test_ap_seg ? std::min<uint64_t>(g_test_ap_seg, AP2_SEGMENT) : AP2_SEGMENT;
    switch (g.hb) {
    case 0: rc = apply_kv12_shape<0>(a, blk, big, fresh, hooked); break;
    case 1: rc = apply_kv12_shape<1>(a, blk, big, fresh, hooked); break;
    case 2: rc = apply_kv12_shape<2>(a, blk, big, fresh, hooked); break;
    case 4: rc = apply_kv12_shape<4>(a, blk, big, fresh, hooked); break;
    }
    if (rc) return rc;
    HIPCHK(c, hipGetLastError());
    return KATGPU_OK;
}

// ---- the arena of a call: [hist1 | offs | l1_off | off2 | cnt2 | bend | spill_n, ovf_n | L1 buffer | guard | L2 buffer | guard | overflow list | guard] ----
// The three buffers' sizes are kg_arena_plan.hpp's (arena_carve): 9.70 bytes per k-mer of a round at hb = 1 (k = 27 at the bench size) with the
// dense level-1 buffer, long runs and two passes -- the level-2 buffer holds one PASS of level 2 + apply (a CU-full of buckets, see
// level2_and_apply) --; 11.9 with 8 bytes per level-1 item and the group editions' run allowance, 18.5 at hb = 4 with one pass.
constexpr uint8_t GUARD_BYTE = 0xA5;
struct PartArena {
    // sizes, from the table's geometry (the constructor): item width the level-2 buffer is carved for (a table that grows has more regions: never more
    // remainder bits), passes of a round (rounded down: the buffer never too small), the table's regions, whether its shape selects level 1's
    // block edition, the small arrays' bytes, the most a k-mer of a round can cost (what ensure_arena asks for)
    uint32_t hb, passes, n_cu; uint64_t regions; bool blocks_shape; double per_item_max; size_t small_bytes;
    // the carve (carve_from) of an arena for rounds of at most want_items k-mers; the stamp diagnostics' counters lie behind spill_n, ovf_n
    uint32_t* hist1; uint64_t* offs; uint64_t* l1_off; uint64_t* off2; uint32_t* cnt2; uint64_t* bend; unsigned long long* spill_n; unsigned long long* ovf_n;
    uint8_t* l1_buf;             // level-1 items: groups of 4 with 8 bytes of room per item (kg_partition.hpp "the level-1 buffer"), or -- cv.dense -- blocks of ten
    uint8_t* l2_buf;             // level-2 items, groups of 4 (5-byte items: 64-byte blocks of 12)
    uint64_t* ovf_buf; uint64_t ovf_cap;
    ArenaCarve cv;
    size_t round_items, l1_bytes, l2_items;
    PartArena(const PartGeom& g0, uint32_t k, uint32_t W, uint32_t n_cu_) : hb(g0.hb), passes(std::max<uint32_t>(1, g0.P1 / pass_buckets(g0.P1, n_cu_))), n_cu(n_cu_), regions(g0.R), blocks_shape(l1_blocks_shape(g0, k)) {
        per_item_max = arena_bytes_per_item(hb, passes, false, false);
        small_bytes = align_up((size_t)W * MAX_PARTS * 4, 256) + align_up((size_t)W * MAX_PARTS * 8, 256) +   /* W <= 4 * CUs */
                      align_up((MAX_PARTS + 1) * 8, 256) + align_up(((size_t)MAX_PARTS * MAX_PARTS + 1) * 8, 256) +
                      align_up((size_t)MAX_PARTS * MAX_PARTS * 4, 256) + align_up((size_t)MAX_PARTS * 8, 256) + align_up((size_t)MAX_PARTS * 4, 256) + 256;
    }
    size_t fixed_bytes(uint32_t W) const { return small_bytes + (size_t)arena_fixed_bytes(hb, passes, W, n_cu, false, false); }      // what an arena needs before its first k-mer
    // false: the buffers would end beyond the arena (cannot happen: arena_carve sizes them from arena_bytes; the caller fails the call)
    bool carve_from(uint8_t* a, size_t arena_bytes, uint32_t W, size_t want_items) {
        uint8_t* const a0 = a;
        hist1 = carve<uint32_t>(a, (size_t)W * MAX_PARTS * 4);
        offs = carve<uint64_t>(a, (size_t)W * MAX_PARTS * 8);
        l1_off = carve<uint64_t>(a, (MAX_PARTS + 1) * 8);
        off2 = carve<uint64_t>(a, ((size_t)MAX_PARTS * MAX_PARTS + 1) * 8);
        cnt2 = carve<uint32_t>(a, (size_t)MAX_PARTS * MAX_PARTS * 4);
        bend = carve<uint64_t>(a, (size_t)MAX_PARTS * 8);
        carve<uint32_t>(a, (size_t)MAX_PARTS * 4);
        spill_n = carve<unsigned long long>(a, STAMP_AREA * 8);      // (spill_n, ovf_n and the stamp diagnostics' counters: STAMP_AT_APPLY, STAMP_AT)
        ovf_n = spill_n + 1;
        if ((size_t)(a - a0) > small_bytes || arena_bytes <= small_bytes) return false;
        cv = arena_carve(arena_bytes - small_bytes, want_items, hb, passes, W, n_cu, regions, blocks_shape, g_l1_fast, g_test_p2_ovf_cap);
        round_items = cv.round_items; l1_bytes = cv.l1_bytes; l2_items = cv.l2_items; ovf_cap = cv.ovf_cap;
        l1_buf = a;
        l2_buf = l1_buf + cv.l1_bytes + ARENA_GUARD;
        ovf_buf = (uint64_t*)(l2_buf + cv.l2_bytes + ARENA_GUARD);
        return (size_t)((uint8_t*)(ovf_buf + ovf_cap) + ARENA_GUARD - a0) <= arena_bytes;
    }
    uint8_t* guard(int i) const { return i == 0 ? l1_buf + cv.l1_bytes : i == 1 ? l2_buf + cv.l2_bytes : (uint8_t*)(ovf_buf + ovf_cap); }
};
static const char* const GUARD_NAME[3] = {"level-1 buffer", "level-2 buffer", "overflow list"};
// KATGPU_TESTING: a fixed byte pattern behind each of the three buffers, checked after every round -- a kernel that wrote beyond its buffer fails the call
static int guards_set(katgpu_ctx* c, const PartArena& A) {
    if (!g_testing) return KATGPU_OK;
    for (int i = 0; i < 3; ++i) HIPCHK(c, hipMemsetAsync(A.guard(i), GUARD_BYTE, ARENA_GUARD, c->stream));
    return KATGPU_OK;
}
static int guards_check(katgpu_ctx* c, const PartArena& A) {
    if (!g_testing) return KATGPU_OK;
    std::vector<uint8_t> h(3 * ARENA_GUARD);
    for (int i = 0; i < 3; ++i) HIPCHK(c, hipMemcpyAsync(h.data() + i * ARENA_GUARD, A.guard(i), ARENA_GUARD, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < 3; ++i)
        for (size_t j = 0; j < ARENA_GUARD; ++j)
            if (h[i * ARENA_GUARD + j] != GUARD_BYTE)
                return fail(c, KATGPU_ERR_DEVICE, "partition arena: the guard behind the %s was written (byte %zu)", GUARD_NAME[i], j);
    return KATGPU_OK;
}
// level 1 tallies the all-ones key of what it reads (k = 32, not canonical; the segmented editions always write the counter): a round that is
// abandoned or repeated puts the table's own tally back
static int restore_ones(katgpu_table* t) { katgpu_ctx* c = t->ctx; HIPCHK(c, hipMemcpyAsync(&t->dv.ctrs[CTR_ONES], &t->ones, sizeof(uint64_t), hipMemcpyHostToDevice, c->stream)); return KATGPU_OK; }
// Rounds are sized in ITEMS (valid k-mers), not window starts: a cheap pre-count of a prefix measures items/starts
// (0.82 for 150 bp reads at k=27) so that the buffers are filled and the table is swept as few times as possible.
static int probe_items_per_start(katgpu_table* t, const PartGeom& g, const PartArena& A, uint32_t W, const uint8_t* p, size_t left, double* items_per_start) {
    katgpu_ctx* c = t->ctx;
    const size_t probe_m = std::min<size_t>(left, (size_t)64 << 20) / P1_TILE_STARTS * P1_TILE_STARTS;
    const uint64_t pt = probe_m / P1_TILE_STARTS, ptw = (pt + W - 1) / W;
    hipLaunchKernelGGL(k_p1v2_count, dim3(W), dim3(P1_BLOCK), 0, c->stream, t->dv, g, p, (uint64_t)(probe_m + t->dv.k - 1), pt, ptw, A.hist1);
    hipLaunchKernelGGL(k_p1_scan, dim3(1), dim3(PART_BLOCK), 0, c->stream, g, W, A.hist1, A.offs, A.l1_off);
    uint64_t probe_items = 0;
    HIPCHK(c, hipMemcpyAsync(&probe_items, &A.l1_off[g.P1], sizeof probe_items, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *items_per_start = std::max(0.05, (double)probe_items / (double)probe_m);
    // (the probe's all-ones tally must not count twice: the real count pass over the same prefix follows)
    return t->dv.k == 32 && !t->dv.canonical ? restore_ones(t) : KATGPU_OK;
}
// (window starts of the next round: kg_arena_plan.hpp's round_starts)

// ---- level 1 ----
// Segmented editions (one pass, fixed-capacity segments) when the round is big enough for their fixed costs; the exact editions
// (count + scan + scatter) otherwise, and for the rest of the call once a segmented round overflowed.  The segmented edition's BLOCK
// form (kg_l1_blocks.hpp): 6-byte items in 64-byte blocks of ten, one 1024-thread workgroup per CU, 16 K-base tiles.
enum class L1Edition { Blocks, SegLean512, SegLean1024, SegPlain512, SegPlain1024, ExactLean, ExactPlain };
static const char* const L1_EDITION_NAME[] = {"Blocks", "SegLean512", "SegLean1024", "SegPlain512", "SegPlain1024", "ExactLean", "ExactPlain"};   // (KATGPU_TRACE)
struct L1Plan {
    L1Edition edition; bool seg /* a segmented edition: level 2 reads segments (blocks of ten from Blocks, else groups) */; uint32_t wgs /* workgroups (<= W: the small arrays hold them) */; uint64_t n_tiles, tiles_per_wg;
    uint64_t seg_cap, cap_plain, stride64;   // segmented: slots of a segment; k-mers it is expected to take at most; bytes of a bucket (kg_arena_plan.hpp: l1_segments)
};
static L1Plan plan_level1(const PartGeom& g, uint32_t k, size_t m, uint64_t est_items, uint32_t W, uint32_t n_cu, size_t l1_bytes, bool seg_wanted) {
    const bool lean = g_l1_lean && lean_applies(k, g.pl.n1);
    const bool pb512 = g.P1 <= 512;
    const bool l1b = l1_blocks_shape(g, k);
    const uint64_t n_tiles = (m + P1_TILE_STARTS - 1) / P1_TILE_STARTS;
    L1Plan pl;
    pl.wgs = l1b ? n_cu : W;
    pl.n_tiles = l1b ? (m + L1B_TILE_STARTS - 1) / L1B_TILE_STARTS : n_tiles;
    // the segments' capacity and the buckets' stride (kg_arena_plan.hpp): the block edition's stride is its segments' blocks, 6.4 bytes per item
    const L1Segments sg = l1_segments(l1b, g.P1, g.hb1, pl.wgs, est_items, (pl.n_tiles + pl.wgs - 1) / pl.wgs, g_test_l1_cpb, l1_bytes);
    pl.cap_plain = sg.cap_plain; pl.seg_cap = sg.seg_cap; pl.stride64 = sg.stride;
    pl.seg = seg_wanted && sg.fits;
    if (pl.seg) pl.edition = l1b ? L1Edition::Blocks : lean ? (pb512 ? L1Edition::SegLean512 : L1Edition::SegLean1024) : (pb512 ? L1Edition::SegPlain512 : L1Edition::SegPlain1024);
    else { pl.edition = lean ? L1Edition::ExactLean : L1Edition::ExactPlain; pl.wgs = W; pl.n_tiles = n_tiles; }
    pl.tiles_per_wg = (pl.n_tiles + pl.wgs - 1) / pl.wgs;
    return pl;
}
static int launch_l1_scatter(katgpu_table* t, const PartGeom& g, const L1Plan& l1, const PartArena& A, const uint8_t* p, uint64_t nb) {
    katgpu_ctx* c = t->ctx;
    auto blocks = [&](auto kern, unsigned long long* stamps) {
        return launch_lds(c, kern, dim3(l1.wgs), dim3(L1B_THREADS), sizeof(P1BLds), sizeof(P1BLds), t->dv, g, p, nb, l1.n_tiles, l1.tiles_per_wg,
                          A.l1_buf, (uint32_t)(l1.seg_cap / L1B_ITEMS), (uint32_t)l1.stride64, A.ovf_buf, A.ovf_n, A.ovf_cap, stamps);
    };
    auto segmented = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(l1.wgs), dim3(P1_BLOCK), 0, c->stream, t->dv, g, p, nb, l1.n_tiles, l1.tiles_per_wg, (const uint64_t*)nullptr, (const uint64_t*)nullptr, A.l1_buf,
                           (uint32_t)l1.seg_cap, (uint32_t)l1.stride64, (uint32_t)l1.cap_plain, A.ovf_buf, A.ovf_n, A.ovf_cap);
        return KATGPU_OK;
    };
    auto exact = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(l1.wgs), dim3(P1_BLOCK), 0, c->stream, t->dv, g, p, nb, l1.n_tiles, l1.tiles_per_wg, (const uint64_t*)A.offs, (const uint64_t*)A.l1_off, A.l1_buf,
                           0u, 0u, 0u, (uint64_t*)nullptr, (unsigned long long*)nullptr, (uint64_t)0);
        return KATGPU_OK;
    };
    switch (l1.edition) {
    case L1Edition::Blocks:
        if (!g_l1b_stamp) return blocks(k_p1b_scatter<false>, nullptr);
        return with_stamps(c, A.spill_n + STAMP_AT, 10, &STAMPS_L1B, [&](unsigned long long* st) { return blocks(k_p1b_scatter<true>, st); });
    case L1Edition::SegLean512:   return segmented(k_p1v2_scatter<true, true, 512>);
    case L1Edition::SegLean1024:  return segmented(k_p1v2_scatter<true, true, MAX_PARTS>);
    case L1Edition::SegPlain512:  return segmented(k_p1v2_scatter<true, false, 512>);
    case L1Edition::SegPlain1024: return segmented(k_p1v2_scatter<true, false, MAX_PARTS>);
    case L1Edition::ExactLean:    return exact(k_p1v2_scatter<false, true, MAX_PARTS>);
    case L1Edition::ExactPlain:   return exact(k_p1v2_scatter<false, false, MAX_PARTS>);
    }
    return KATGPU_OK;
}
// Level 1 of a round of m starts.  A segmented edition: one launch; how many k-mers it wrote is not needed (and not known: *items stays the
// estimate).  An exact edition: count, scan, scatter; *items = the round's k-mers, and when they are more than the buffers hold (denser than
// the prefix suggested) nothing is scattered: the caller repeats the round smaller.
static int level1(katgpu_table* t, const PartGeom& g, const L1Plan& l1, const PartArena& A, size_t cap_items, const uint8_t* p, size_t m, double items_per_start, uint64_t* items) {
    katgpu_ctx* c = t->ctx;
    const uint64_t nb = m + t->dv.k - 1;
    if (l1.seg) {
        int rc;
        // (plan_level1 made the plan for this buffer: no launch on one whose last bucket ends beyond it)
        if (l1.stride64 * g.P1 > A.l1_bytes || (uint64_t)l1.wgs * (l1.edition == L1Edition::Blocks ? l1.seg_cap / L1B_ITEMS * L1B_BYTES : (4 + g.hb1) * l1.seg_cap) > l1.stride64)
            return fail(c, KATGPU_ERR_DEVICE, "partition round: %u buckets of %llu bytes end beyond the level-1 buffer of %zu bytes", g.P1, (unsigned long long)l1.stride64, A.l1_bytes);
        { ScopedTimer tm(c, KATGPU_K_PART_L1S, *items); rc = launch_l1_scatter(t, g, l1, A, p, nb); }
        if (!rc && g_trace) fprintf(stderr, "[katgpu] partition round (segmented level 1%s): %zu starts, ~%llu items, %llu k-mers per segment (arena %.1f GB; capacity %zu items, %s, stride %llu)\n", l1.edition == L1Edition::Blocks ? ", blocks of ten" : "", m,
                                    (unsigned long long)*items, (unsigned long long)l1.seg_cap, c->arena_bytes / 1e9, cap_items, L1_EDITION_NAME[(int)l1.edition], (unsigned long long)l1.stride64);
        return rc;
    }
    {
        ScopedTimer tm(c, KATGPU_K_PART_L1, m);
        hipLaunchKernelGGL(k_p1v2_count, dim3(l1.wgs), dim3(P1_BLOCK), 0, c->stream, t->dv, g, p, nb, l1.n_tiles, l1.tiles_per_wg, A.hist1);
        hipLaunchKernelGGL(k_p1_scan, dim3(1), dim3(PART_BLOCK), 0, c->stream, g, l1.wgs, A.hist1, A.offs, A.l1_off);
    }
    HIPCHK(c, hipMemcpyAsync(items, &A.l1_off[g.P1], sizeof *items, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (g_trace) fprintf(stderr, "[katgpu] partition round: %zu starts -> %llu items (buffer %zu items, arena %.1f GB, ratio %.3f; capacity %zu items, %s, stride 0)\n", m, (unsigned long long)*items, A.round_items, c->arena_bytes / 1e9, items_per_start,
                         cap_items, L1_EDITION_NAME[(int)l1.edition]);
    if (*items > cap_items) return t->dv.k == 32 && !t->dv.canonical ? restore_ones(t) : KATGPU_OK;
    if (!*items) return KATGPU_OK;
    // (the exact layout: 8 bytes per item and 32 per bucket; cap_items is sized so that this holds -- and no scatter is launched where it does not)
    if (l1_bucket_base(*items, g.P1) + 32 > A.l1_bytes)
        return fail(c, KATGPU_ERR_DEVICE, "partition round: %llu items of an exact level 1 end beyond the level-1 buffer of %zu bytes", (unsigned long long)*items, A.l1_bytes);
    ScopedTimer tm(c, KATGPU_K_PART_L1S, *items);
    return launch_l1_scatter(t, g, l1, A, p, nb);
}

// ---- level 2 ----
// One pass over the bucket when the runs are predictable (k_p2_fast, k_p2x_fast: fixed-capacity runs, an overflow list), else -- or when
// that list did not hold -- the exact two-pass kernel (k_p2).  Which instantiation: the item width g.hb and what level 1 wrote.
enum class L1Items { Groups /* of four items of at most 48 bits */, WideGroups /* g.hb1 == 4 */, Blocks /* of ten (kg_l1_blocks.hpp) */ };
static const char* const L1_ITEMS_NAME[] = {"Groups", "WideGroups", "Blocks"};                                                            // (KATGPU_TRACE)
enum L2Family : uint32_t { L2_BLOCKS = 1 /* kg_l2_blocks.hpp */, L2_ONE_PASS = 2 /* k_p2_fast */, L2_EXACT = 4 /* k_p2 */ };           // the kernel families of level 2, as bits
struct L2Pass { katgpu_ctx* c; const PartGeom& g; const PartArena& A; uint32_t grid; L1Items src; uint64_t seg_slots; uint32_t* families /* |= what ran (KATGPU_TRACE) */; };
template <typename K>
static int p2_one_pass(const L2Pass& x, K kern, size_t lds, unsigned long long* stamps = nullptr) {
    return launch_lds(x.c, kern, dim3(x.grid), dim3(PART_BLOCK), lds, lds, x.g, x.A.l1_off, x.A.l1_buf, x.A.l2_buf, x.A.off2, x.A.cnt2, x.A.ovf_buf, x.A.ovf_n, x.A.ovf_cap, x.seg_slots, stamps);
}
template <typename K>
static int p2_exact(const L2Pass& x, K kern, size_t lds) {
    return launch_lds(x.c, kern, dim3(x.grid), dim3(PART_BLOCK), lds, lds, x.g, x.A.l1_off, x.A.l1_buf, x.A.l2_buf, x.A.off2, x.seg_slots, x.A.bend);
}
template <int HB>
static int launch_l2_hb(const L2Pass& x, bool one_pass) {
    constexpr size_t lds_e = sizeof(P2Lds<HB>), lds_f = sizeof(typename P2FastLds<HB>::type);
    unsigned long long* const stamps = x.A.spill_n + STAMP_AT;
    if (x.families) *x.families |= !one_pass ? L2_EXACT : x.src == L1Items::Blocks && HB == 1 ? L2_BLOCKS : L2_ONE_PASS;
    switch (x.src) {
    case L1Items::Blocks:
        if constexpr (HB == 4) break;
        else if (!one_pass) return p2_exact(x, k_p2<HB, false, true>, lds_e);
        else if constexpr (HB != 1) return p2_one_pass(x, k_p2_fast<HB, false, false, true>, lds_f);
        else if (!g_p2x_stamp) return p2_one_pass(x, k_p2x_fast<false>, sizeof(P2XLds));             // the bench's shape: kg_l2_blocks.hpp
        else return with_stamps(x.c, stamps, 10, &STAMPS_P2X, [&](unsigned long long* st) { return p2_one_pass(x, k_p2x_fast<true>, sizeof(P2XLds), st); });
    case L1Items::WideGroups: return one_pass ? p2_one_pass(x, k_p2_fast<HB, true>, lds_f) : p2_exact(x, k_p2<HB, true>, lds_e);
    case L1Items::Groups:
        if constexpr (HB == 1) if (one_pass && g_p2_stamp) return with_stamps(x.c, stamps, 6, &STAMPS_P2, [&](unsigned long long* st) { return p2_one_pass(x, k_p2_fast<1, false, true>, lds_f, st); });
        return one_pass ? p2_one_pass(x, k_p2_fast<HB, false>, lds_f) : p2_exact(x, k_p2<HB, false>, lds_e);
    }
    return fail(x.c, KATGPU_ERR_DEVICE, "level 2 from blocked level-1 items: item width %u", x.g.hb);
}
static int launch_l2(const L2Pass& x, bool one_pass) {
    switch (x.g.hb) {
    case 0: return launch_l2_hb<0>(x, one_pass);
    case 1: return launch_l2_hb<1>(x, one_pass);
    case 2: return launch_l2_hb<2>(x, one_pass);
    case 4: return launch_l2_hb<4>(x, one_pass);
    }
    return fail(x.c, KATGPU_ERR_DEVICE, "level 2: item width %u", x.g.hb);
}
// What the overflow counter says once a pass's one-pass level 2 is through (tried_fast) -- and, in a segmented round's first pass, level 1.
// *overflowed = entries of the overflow list that are valid now (*ovf_before: those of level 1 and the earlier passes).
enum class L2Next { UseCnt2 /* the one-pass kernel's runs stand */, Exact /* it did not run */, FallBackExact /* its list did not hold: this pass and all later ones exactly */,
                    RedoRound /* level 1's list did not hold: the level-1 buffer is incomplete */ };
static int read_overflow(katgpu_table* t, const PartArena& A, bool seg, bool tried_fast, unsigned long long ovf_l1, const unsigned long long* ovf_before, unsigned long long* overflowed, L2Next* next) {
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipMemcpyAsync(overflowed, A.ovf_n, sizeof *overflowed, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (seg && ovf_l1 > A.ovf_cap) {             // (only ever in the first pass: nothing has been applied yet)
        if (g_trace) fprintf(stderr, "[katgpu] segmented level 1: %llu k-mers beyond their segments (list holds %llu): exact level 1 from here on\n", ovf_l1, (unsigned long long)A.ovf_cap);
        *next = L2Next::RedoRound;
        return restore_ones(t);                  // the scatter tallied the all-ones key
    }
    *next = !tried_fast ? L2Next::Exact : *overflowed <= A.ovf_cap ? L2Next::UseCnt2 : L2Next::FallBackExact;
    if (*next == L2Next::FallBackExact) {
        if (g_trace) fprintf(stderr, "[katgpu] k_p2_fast: %llu k-mers beyond their runs (list holds %llu): exact level 2 from here on\n", *overflowed, (unsigned long long)A.ovf_cap);
        *overflowed = *ovf_before;               // what was on the list before this pass is still there and still valid
        HIPCHK(c, hipMemcpyAsync(A.ovf_n, ovf_before, sizeof *ovf_before, hipMemcpyHostToDevice, c->stream));
    }
    return KATGPU_OK;
}

// Level 2 + apply of a round, in passes over sets of buckets: the level-2 buffer holds one pass (PartArena), a pass is a whole number of
// CU-fulls of buckets where the geometry allows (alloc_dev_table).  *lists: the k-mers that found no place (in parts of the arena that are dead).
enum class RoundEnd { Done, RedoExactL1 /* nothing was applied: the round again with an exact level 1 */, DirectPath /* a single bucket beyond the buffer */ };
static int level2_and_apply(katgpu_table* t, PartGeom& g, const L1Plan& l1, const PartArena& A, uint64_t items, bool* p2_fast_ok, KeyLists* lists, RoundEnd* end) {
    katgpu_ctx* c = t->ctx;
    const bool seg = l1.seg;
    const uint64_t seg_slots = seg ? (uint64_t)l1.wgs * l1.seg_cap : 0;        // items of one bucket
    const L1Items src = seg && l1.edition == L1Edition::Blocks ? L1Items::Blocks : g.hb1 == 4 ? L1Items::WideGroups : L1Items::Groups;
    *end = RoundEnd::Done;
    std::vector<uint64_t> h_l1_off;                                            // where bucket b starts in the level-1 buffer (exact level 1)
    unsigned long long ovf_l1 = 0;                                             // k-mers beyond their segments (segmented level 1)
    if (!seg) {
        h_l1_off.resize(g.P1 + 1);
        HIPCHK(c, hipMemcpyAsync(h_l1_off.data(), A.l1_off, (g.P1 + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    } else HIPCHK(c, hipMemcpyAsync(&ovf_l1, A.ovf_n, sizeof ovf_l1, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    auto lbeg = [&](uint32_t b) -> uint64_t { return seg ? (uint64_t)b * g.l1_real : h_l1_off[b]; };      // k-mers before bucket b (segmented: their bound)
    const uint32_t tile2 = l2_tile_items(g.hb);
    auto pass_extent = [&](uint32_t b_lo, uint32_t b_hi) -> uint64_t {       // bound of what level 2 writes for these buckets, in items (either edition: kg_arena_plan.hpp)
        return p2_pass_extent(lbeg(b_hi) - lbeg(b_lo), b_hi - b_lo, g.P2, tile2, g.l2_trim != 0);
    };
    uint32_t step = pass_buckets(g.P1, (uint32_t)c->n_cu);
    auto fits = [&](uint32_t st) { for (uint32_t b = 0; b < g.P1; b += st) if (pass_extent(b, std::min(g.P1, b + st)) > A.l2_items) return false; return true; };
    if (!seg && A.cv.big) {              // exact level 1: the caller chose the runs' form from an estimate of the buckets; now their counts are known
        g.l2_trim = 0;
        if (!fits(step) && l2_trims(g.hb, items, g.R)) g.l2_trim = 1;       // (the untrimmed passes do not fit: the trimmed form before any pass is halved)
    }
    while (step > 1 && !fits(step)) step = (step + 1) / 2;
    if (!fits(step)) {
        *end = RoundEnd::DirectPath;
        // this round's level 1 (either edition) has tallied the all-ones key of its starts, which the direct kernel will count again
        return seg || (t->dv.k == 32 && !t->dv.canonical) ? restore_ones(t) : KATGPU_OK;
    }
    const bool try_fast0 = *p2_fast_ok && (g_p2_fast == 2 || items / g.R >= 1024);
    unsigned long long ovf_total = ovf_l1;                                 // entries of the overflow list so far (level 1's, then every pass's)
    uint32_t l2_families = 0;                                              // what ran, for the trace's "partition forms" line
    ApplyForm ap{};
    if (g_trace && g.P1 > step) fprintf(stderr, "[katgpu]   level 2 + apply in %u passes of %u buckets (level-2 buffer: %zu items)\n", (g.P1 + step - 1) / step, step, A.l2_items);
    for (uint32_t b_lo = 0; b_lo < g.P1; b_lo += step) {
        g.b_lo = b_lo; g.b_hi = std::min(g.P1, b_lo + step);
        const uint64_t pass_items = std::max<uint64_t>(1, (uint64_t)((double)items * (g.b_hi - g.b_lo) / g.P1));
        // this pass's part of the level-1 buffer, dead once its level 2 is through: the pass's spill list (8-byte entries: room for one per k-mer, 0.8 per k-mer
        // behind level 1's block edition -- a list that is too short is counted, not written, and fails the call below)
        auto l1_at = [&](uint32_t b) -> uint64_t { return seg ? (uint64_t)b * g.l1_stride : l1_bucket_base(lbeg(b), b); };
        uint64_t* spill_buf = (uint64_t*)(A.l1_buf + l1_at(b_lo));
        g.spill_cap = (l1_at(g.b_hi) - l1_at(b_lo)) / 8;
        const bool try_fast = try_fast0 && *p2_fast_ok;
        const L2Pass x{c, g, A, std::min<uint32_t>(g.b_hi - g.b_lo, (uint32_t)c->n_cu), src, seg_slots, &l2_families};      // one workgroup per CU
        HIPCHK(c, hipMemsetAsync(A.spill_n, 0, sizeof(unsigned long long), c->stream));
        int rc = KATGPU_OK;
        if (try_fast) { ScopedTimer tm(c, KATGPU_K_PART_L2, pass_items); rc = launch_l2(x, true); }
        if (rc) return rc;
        L2Next next = L2Next::Exact;
        unsigned long long overflowed = ovf_total;
        if (try_fast || (seg && b_lo == 0)) {
            rc = read_overflow(t, A, seg, try_fast, ovf_l1, &ovf_total, &overflowed, &next);
            if (rc) return rc;
            if (next == L2Next::RedoRound) { *end = RoundEnd::RedoExactL1; return KATGPU_OK; }
            if (next == L2Next::FallBackExact) *p2_fast_ok = false;
        }
        const bool runs = next == L2Next::UseCnt2;                             // the one-pass kernel's runs have their lengths in cnt2
        if (!runs) { ScopedTimer tm(c, KATGPU_K_PART_L2, pass_items); rc = launch_l2(x, false); }
        if (rc) return rc;
        ovf_total = overflowed;
        {   // (exact level 2: a bucket's runs stop short of the next bucket's -- bend)
            ScopedTimer tm(c, KATGPU_K_PART_APPLY, pass_items);
            rc = launch_apply(t, g, A.off2, A.l2_buf, spill_buf, A.spill_n, runs ? A.cnt2 : nullptr, runs ? nullptr : A.bend, items, &ap);
        }
        if (rc) return rc;
        HIPCHK(c, hipGetLastError());
        unsigned long long spilled = 0;
        HIPCHK(c, hipMemcpyAsync(&spilled, A.spill_n, sizeof spilled, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (spilled > g.spill_cap)       // (more k-mers without a slot than the pass's segments were sized for: a table far too small, met by a 5-sigma round)
            return fail(c, KATGPU_ERR_TABLE_FULL, "Hash full: %llu k-mers of a partition pass found no slot (the list holds %llu); raise the size hint", spilled, (unsigned long long)g.spill_cap);
        if (spilled) lists->push_back({spill_buf, spilled});
    }
    if (ovf_total) lists->push_back({A.ovf_buf, ovf_total});                // what level 1 / level 2 could not place
    // the kernel forms this round ran (tests/test_gpu_partition_forms.py reads the line): level-1 edition, what level 2 read and the item widths,
    // level 2's kernel families in the order blocks, one-pass, exact (more than one: a pass fell back), the apply instantiation
    if (g_trace) {
        char l2[32];
        snprintf(l2, sizeof l2, "%s%s%s", l2_families & L2_BLOCKS ? "+blocks" : "", l2_families & L2_ONE_PASS ? "+one-pass" : "", l2_families & L2_EXACT ? "+exact" : "");
        fprintf(stderr, "[katgpu] partition forms: l1=%s items=%s hb1=%u hb=%u l2=%s apply=%s B=%d KP=%d fresh=%d%s\n", L1_EDITION_NAME[(int)l1.edition], L1_ITEMS_NAME[(int)src], g.hb1, g.hb,
                l2[0] ? l2 + 1 : "none", ap.packed ? "packed" : "KV12", ap.block, ap.kp, (int)ap.fresh, ap.hooked ? " hooked" : "");
    }
    return KATGPU_OK;
}
// regions that ran out of slots, runs beyond their capacity: make room, then the direct path
static int insert_spilled(katgpu_table* t, const KeyLists& lists, bool* arena_lost) {
    *arena_lost = false;
    if (lists.empty()) return KATGPU_OK;
    uint64_t total = 0;
    for (auto& l : lists) total += l.second;
    int rc = grow_beside_arena(t, total, 0, lists, 8, arena_lost);
    if (rc || *arena_lost) return rc;          // (lost: the lists went in from the host)
    for (auto& l : lists) insert_keys(t, l.first, l.second, 8);
    return KATGPU_OK;
}

// Count a resident, 16-byte aligned base stream through partition rounds.  *done = number of window starts consumed
// (all of them unless the geometry stops fitting, in which case the caller finishes with the direct kernel).
static int count_partitioned(katgpu_table* t, const uint8_t* dev_bases, size_t n, size_t* done) {
    katgpu_ctx* c = t->ctx;
    const uint32_t k = t->dv.k, n_cu = (uint32_t)c->n_cu;
    const size_t n_starts = n - k + 1;
    *done = 0;
    c->arena_borrowed = false;                    // a borrowed arena is only promised until the next count call
    if (n < 64) return KATGPU_OK;                 // (the tile loader reads whole 16-byte pieces: direct path)
    // A table hopelessly small for this input (KAT's default -H against a whole run) would spill nearly every k-mer of the
    // first round: give it room for 1/16 of the starts first -- cheap while it is still small, and before the arena exists.
    if (!g_test_round_items && !t->disable_grow && t->dv.cap < n_starts / 16) {
        uint64_t nc = t->dv.cap; while (nc < n_starts / 16) nc *= 2;
        int grc = regrow(t, nc);
        if (grc) return grc;
    }
    const uint32_t W = n_cu * std::min<uint32_t>(g_p1_wgs, 4);                     // level-1 workgroups (rows of hist1 / offs)
    PartGeom g0;
    if (!part_geometry(t->dv, &g0)) return KATGPU_OK;                              // direct path
    PartArena A(g0, k, W, n_cu);
    size_t want_items = n_starts;
    if (g_test_round_items) want_items = std::min<size_t>(want_items, g_test_round_items);
    bool usable = false;
    int rc = ensure_arena(c, A.fixed_bytes(W), 18, want_items, A.fixed_bytes(W) + (size_t)((A.per_item_max + 0.5) * (double)want_items), "", &usable);
    if (rc || !usable) return rc;                                                  // (no arena: direct path)
    ArenaBusy busy(c);
    if (!A.carve_from(c->arena, c->arena_bytes, W, want_items)) return fail(c, KATGPU_ERR_DEVICE, "partition arena: the carve of %zu bytes ends beyond the arena", c->arena_bytes);
    rc = guards_set(c, A);
    if (rc) return rc;
    if (!g_test_round_items && A.round_items < ((size_t)1 << 20) && A.round_items < n_starts) return KATGPU_OK;
    bool p2_fast_ok = g_p2_fast != 0, l1_fast_ok = g_l1_fast != 0;
    RoundCaps caps;                               // a round's capacity by the edition that runs it (kg_arena_plan.hpp): the exact one once a round ran, or has to run, the exact level 1
    double items_per_start = 1.0;
    size_t pos = 0;
    bool ratio_known = false;
    while (pos < n_starts) {
        rc = refresh_counters(t);
        if (rc) return rc;
        if ((double)t->distinct > 0.6 * (double)t->dv.cap) {
            bool lost = false;
            rc = grow_beside_arena(t, 0, t->dv.cap * 2, KeyLists(), 8, &lost);
            if (rc) return rc;
            if (lost) break;                                                      // the caller re-enters with a fresh arena
        }
        PartGeom g;
        if (!part_geometry(t->dv, &g)) break;                                      // table too large for two levels: direct path
        if (g.hb > A.hb) break;                                                   // (cannot happen: see PartArena::hb) the level-2 carve would not hold these items
        const size_t left = n_starts - pos;
        const uint8_t* p = dev_bases + pos;
        // (the segmented level 1 sizes its segments from this ratio, so it wants it even when one round takes everything)
        // what a round holds depends on the edition that runs it: the exact level 1 places fewer k-mers in a dense buffer than the block edition
        const size_t cap_items = caps.cap(A.cv, l1_fast_ok && l1_blocks_shape(g, k));
        if (!ratio_known && !g_test_round_items && (left > cap_items || (l1_fast_ok && left >= ((size_t)64 << 20)))) {
            rc = probe_items_per_start(t, g, A, W, p, left, &items_per_start);
            if (rc) return rc;
            ratio_known = true;
        }
        const size_t m = round_starts(left, cap_items, items_per_start);
        t->count_bound = 0xFFFFFFFFULL;          // the apply kernel chains its own carries; a later direct launch sweeps first
        const uint64_t est_items = (uint64_t)((double)m * items_per_start);
        const bool seg_wanted = l1_fast_ok && (g_l1_fast == 2 || (ratio_known && est_items >= ((uint64_t)64 << 20)));
        const L1Plan l1 = plan_level1(g, k, m, est_items, W, n_cu, A.l1_bytes, seg_wanted);
        if (l1.edition != L1Edition::Blocks && cap_items > caps.cap(A.cv, false)) { caps.exact_from_here(); continue; }      // sized for the block edition, which does not run: again with the exact capacity
        g.l1_stride = l1.seg ? l1.stride64 : 0;
        g.l1_real = l1.seg ? (uint64_t)l1.wgs * l1.cap_plain : 0;
        {   // the runs' slack: trimmed only where a pass does not fit the level-2 buffer with the untrimmed form (kg_arena_plan.hpp: round_trims)
            const uint32_t nb = std::min(g.P1, pass_buckets(g.P1, n_cu));
            const uint64_t nn = l1.seg ? nb * g.l1_real : (uint64_t)((double)est_items * nb / g.P1 * (1 + 1.0 / 64)) + 1024;
            g.l2_trim = round_trims(A.cv, g.hb, est_items, g.R, nn, nb, g.P2) ? 1u : 0u;
        }
        HIPCHK(c, hipMemsetAsync(A.spill_n, 0, 2 * sizeof(unsigned long long), c->stream));          // spill_n, ovf_n
        uint64_t items = est_items;
        rc = level1(t, g, l1, A, cap_items, p, m, items_per_start, &items);
        if (rc) return rc;
        if (!l1.seg && items > cap_items) {       // (exact level 1) denser than the prefix suggested: redo this round smaller, this and every later one with the exact capacity
            items_per_start = std::min(1.0, (double)items / (double)m * 1.02);
            caps.exact_from_here();
            continue;
        }
        if (items) {
            KeyLists lists;
            RoundEnd end;
            rc = level2_and_apply(t, g, l1, A, items, &p2_fast_ok, &lists, &end);
            if (rc) return rc;
            if (end == RoundEnd::RedoExactL1) { l1_fast_ok = false; caps.exact_from_here(); continue; }      // (the repeated round and every later one: the exact capacity)
            if (end == RoundEnd::DirectPath) break;
            bool lost = false;
            rc = insert_spilled(t, lists, &lost);
            if (rc) return rc;
            if (lost) { pos += m; break; }         // the caller re-enters for the rest
            rc = guards_check(c, A);
            if (rc) return rc;
        }
        pos += m;
    }
    *done = pos;
    return refresh_counters(t);
}

// The same for wide tables (kg_partition_wide.hpp): 16-byte items, exact level 1 and level 2, one pass of level 2 + apply per round.
// Arena: [hist1 | offs | l1_off | off2 | spill_n | level-1 buffer | level-2 buffer], 32 bytes per k-mer of a round; the spill list
// of a round lies in its level-1 buffer, which is dead by then.
static bool wide_part_geometry(const DevTable& d) {
    return d.keys_b && d.p1 <= (uint32_t)MAX_PARTS && d.p2 <= (uint32_t)MAX_PARTS && d.region_slots % 4 == 0 && d.region_slots >= 64 && d.region_slots <= WIDE_AP_MAX_SLOTS &&
           (uint64_t)d.p1 * d.p2 == d.n_regions;
}
static int count_partitioned_w(katgpu_table* t, const uint8_t* dev_bases, size_t n, size_t* done) {
    katgpu_ctx* c = t->ctx;
    const uint32_t k = t->dev().k;
    const size_t n_starts = n - k + 1;
    *done = 0;
    c->arena_borrowed = false;
    if (n < 4096 || !wide_part_geometry(t->dev())) return KATGPU_OK;               // direct path
    if (!g_test_round_items && !t->disable_grow && t->dev().cap < n_starts / 16) {     // (as count_partitioned: room for 1/16 of the starts first)
        uint64_t nc = t->dev().cap; while (nc < n_starts / 16) nc *= 2;
        int grc = regrow(t, nc);
        if (grc) return grc;
        if (!wide_part_geometry(t->dev())) return KATGPU_OK;
    }
    const uint32_t W = (uint32_t)c->n_cu * 3;                                  // level-1 workgroups (512 threads, 12 KB of LDS)
    const size_t tile_starts = W1_TILE_STARTS;
    const size_t small_bytes = align_up((size_t)W * MAX_PARTS * 4, 256) + align_up((size_t)W * MAX_PARTS * 8, 256) + align_up((MAX_PARTS + 1) * 8, 256) +
                               align_up(((size_t)MAX_PARTS * MAX_PARTS + 1) * 8, 256) + 256 + 4096;
    size_t want_items = n_starts;
    if (g_test_round_items) want_items = std::min<size_t>(want_items, g_test_round_items);
    bool usable = false;
    int rc = ensure_arena(c, small_bytes, 32, want_items + 64, small_bytes + 32 * (want_items + 64), " (wide k-mers)", &usable);
    if (rc || !usable) return rc;                                              // (no arena: direct path)
    ArenaBusy busy(c);
    uint8_t* a = c->arena;
    uint32_t* hist1 = carve<uint32_t>(a, (size_t)W * MAX_PARTS * 4);
    uint64_t* offs = carve<uint64_t>(a, (size_t)W * MAX_PARTS * 8);
    uint64_t* l1_off = carve<uint64_t>(a, (MAX_PARTS + 1) * 8);
    uint64_t* off2 = carve<uint64_t>(a, ((size_t)MAX_PARTS * MAX_PARTS + 1) * 8);
    unsigned long long* spill_n = carve<unsigned long long>(a, 256);
    const size_t round_items = std::min<size_t>(want_items, (c->arena_bytes - small_bytes) / 32);
    u64x2* l1_buf = (u64x2*)a;
    u64x2* l2_buf = l1_buf + round_items;
    if (!g_test_round_items && round_items < ((size_t)1 << 20) && round_items < n_starts) return KATGPU_OK;
    if (round_items < tile_starts && round_items < n_starts) return KATGPU_OK;

    size_t pos = 0;
    while (pos < n_starts) {
        rc = refresh_counters(t);
        if (rc) return rc;
        if ((double)t->distinct > 0.6 * (double)t->dev().cap) {
            bool lost = false;
            rc = grow_beside_arena(t, 0, t->dev().cap * 2, KeyLists(), 16, &lost);
            if (rc) return rc;
            if (lost) break;                                                      // the caller re-enters with a fresh arena
        }
        if (!wide_part_geometry(t->dev())) break;
        const DevTable d = t->dev();
        size_t m = std::min(n_starts - pos, round_items);                          // items <= starts: a round always fits its buffers
        if (m < n_starts - pos) {
            const size_t rounds_left = (n_starts - pos + m - 1) / m;               // balance the remaining rounds
            m = std::min(m, (n_starts - pos + rounds_left - 1) / rounds_left + tile_starts);
            m -= m % tile_starts;                                                  // whole tiles: the next round starts 16-byte aligned
            if (!m) break;
        }
        const size_t nb = m + k - 1;
        const uint8_t* p = dev_bases + pos;
        const uint64_t n_tiles = (m + tile_starts - 1) / tile_starts;
        const uint64_t tiles_per_wg = (n_tiles + W - 1) / W;
        PartGeom g{};
        g.P1 = d.p1;                                                               // (all k_p1_scan looks at)
        HIPCHK(c, hipMemsetAsync(spill_n, 0, sizeof(unsigned long long), c->stream));
        {
            ScopedTimer tm(c, KATGPU_K_PART_L1, m);
            hipLaunchKernelGGL(k_w1<false>, dim3(W), dim3(W1_BLOCK), 0, c->stream, d, d.p1, p, (uint64_t)nb, n_tiles, tiles_per_wg, hist1, (const uint64_t*)nullptr, (u64x2*)nullptr);
            hipLaunchKernelGGL(k_p1_scan, dim3(1), dim3(PART_BLOCK), 0, c->stream, g, W, hist1, offs, l1_off);
        }
        uint64_t items = 0;
        HIPCHK(c, hipMemcpyAsync(&items, &l1_off[d.p1], sizeof items, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (g_trace) fprintf(stderr, "[katgpu] partition round (wide k-mers): %zu starts -> %llu items (buffer %zu items, arena %.1f GB)\n", m, (unsigned long long)items, round_items, c->arena_bytes / 1e9);
        if (items > round_items) return fail(c, KATGPU_ERR_DEVICE, "wide partition round: %llu items from %zu starts", (unsigned long long)items, m);
        if (items) {
            {
                ScopedTimer tm(c, KATGPU_K_PART_L1S, items);
                hipLaunchKernelGGL(k_w1<true>, dim3(W), dim3(W1_BLOCK), 0, c->stream, d, d.p1, p, (uint64_t)nb, n_tiles, tiles_per_wg, (uint32_t*)nullptr, (const uint64_t*)offs, l1_buf);
            }
            {
                ScopedTimer tm(c, KATGPU_K_PART_L2, items);
                hipLaunchKernelGGL(k_w2, dim3(std::min<uint32_t>(d.p1, (uint32_t)c->n_cu)), dim3(PART_BLOCK), 0, c->stream, d.p1, d.p2, (const uint64_t*)l1_off, (const u64x2*)l1_buf, l2_buf, off2);
            }
            {
                ScopedTimer tm(c, KATGPU_K_PART_APPLY, items);
                rc = launch_lds(c, k_w3_apply, dim3(std::min<uint32_t>(d.n_regions, (uint32_t)c->n_cu)), dim3(W3_BLOCK), (size_t)d.region_slots * 20, LDS_BYTES - 256, d, (const uint64_t*)off2, (const u64x2*)l2_buf,
                                l1_buf /* the spill list: the level-1 buffer is dead */, spill_n, g_test_spill_mod);
                if (rc) return rc;
            }
            HIPCHK(c, hipGetLastError());
            unsigned long long spilled = 0;
            HIPCHK(c, hipMemcpyAsync(&spilled, spill_n, sizeof spilled, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (spilled) {                              // regions that ran out of slots: make room, then the direct path
                if (g_trace) fprintf(stderr, "[katgpu]   %llu k-mers spilled by full regions\n", spilled);
                bool lost = false;
                rc = grow_beside_arena(t, spilled, 0, KeyLists(1, {l1_buf, spilled}), 16, &lost);
                if (rc) return rc;
                if (lost) { pos += m; break; }          // the list went in from the host; the caller re-enters with a fresh arena
                insert_keys(t, l1_buf, spilled, 16);
                HIPCHK(c, hipStreamSynchronize(c->stream));
            }
        }
        pos += m;
    }
    *done = pos;
    return refresh_counters(t);
}

// Count a resident base stream.  The stream is cut into sub-batches so that "distinct + sub-batch starts" stays under
// the load limit (the table can then never fill in the middle of a launch); consecutive sub-batches overlap by k-1.
int count_resident(katgpu_table* t, const uint8_t* dev_bases, size_t n) {
    const uint32_t k = t->dv.k;                              // (dv, not dev(): a table whose slots wait for their first sweep is left to the partitioned counter)
    if (n < k) return KATGPU_OK;
    size_t pos = 0;
    const size_t n_starts = n - k + 1;
    // Large, aligned inputs go through the partitioned counter (no global atomic per k-mer); whatever it leaves (nothing,
    // normally) and everything small goes through the direct kernel below.
    while (!t->dv.keys_b && n_starts - pos >= std::max<uint64_t>(g_part_min_starts, 1) && (reinterpret_cast<uintptr_t>(dev_bases + pos) & 15) == 0) {
        size_t done = 0;                        // returns early (done < remaining) when a table growth cost it the arena
        int prc = count_partitioned(t, dev_bases + pos, n - pos, &done);
        if (prc) return prc;
        if (!done) break;
        pos += done;
    }
    while (t->dv.keys_b && n_starts - pos >= std::max<uint64_t>(g_part_min_starts, 1) && (reinterpret_cast<uintptr_t>(dev_bases + pos) & 15) == 0) {
        size_t done = 0;                        // wide tables: kg_partition_wide.hpp
        int prc = count_partitioned_w(t, dev_bases + pos, n - pos, &done);
        if (prc) return prc;
        if (!done) break;
        pos += done;
    }
    while (pos < n_starts) {
        int rc = refresh_counters(t);
        if (rc) return rc;
        // largest batch that provably fits; if even a minimal one does not, grow first
        uint64_t room = (uint64_t)(load_limit(t->dev()) * (double)t->dev().cap) > t->distinct ? (uint64_t)(load_limit(t->dev()) * (double)t->dev().cap) - t->distinct : 0;
        uint64_t want = std::min<uint64_t>(n_starts - pos, (uint64_t)CHUNK_STARTS * 65536);   // <= 266 M starts per launch
        if (g_test_max_starts) want = std::min<uint64_t>(want, g_test_max_starts);
        // As the table fills, launches shrink to the remaining room (each adds far fewer distinct k-mers than window
        // starts on real coverage, so the room shrinks slowly); only when the room is down to 1/64 of the table do we grow.
        if (room < std::min<uint64_t>(want, std::max<uint64_t>(t->dev().cap / 64, CHUNK_STARTS))) {
            rc = ensure_room(t, std::min<uint64_t>(want, std::max<uint64_t>(t->dev().cap / 2, CHUNK_STARTS)));
            if (rc) return rc;
            continue;
        }
        uint64_t starts = std::min(want, room);
        if (starts < n_starts - pos) starts -= starts % 16;            // keep the next sub-batch 16-byte aligned
        if (starts == 0) starts = std::min<uint64_t>(16, n_starts - pos);
        rc = launch_count(t, dev_bases + pos, (size_t)(starts + k - 1));
        if (rc) return rc;
        pos += starts;
    }
    return refresh_counters(t);
}

extern "C" int katgpu_count_bases_device(katgpu_table* t, const uint8_t* dev_bases, size_t n) {
    if (!t || (!dev_bases && n)) return KATGPU_ERR_INVALID_ARG;
    HIPCHK(t->ctx, hipSetDevice(t->ctx->device));
    return count_resident(t, dev_bases, n);
}

// KATGPU_RING_MB: size of each of the two device rings the host feeder fills (default 1024)
static const size_t g_ring_bytes = (getenv("KATGPU_RING_MB") ? std::max<size_t>(1, strtoull(getenv("KATGPU_RING_MB"), nullptr, 10)) : 1024) << 20;

// want: bytes of stream the caller expects (0: unknown): small inputs get small rings (two 1 GiB rings for a 100-base call, or for
// the CLI on the reference's 1000-read test files, would be most of the call's time and could fail on a full device)
static int ensure_staging(katgpu_ctx* c, size_t want = 0) {
    int rc = ensure_pinned(c); if (rc) return rc;
    size_t ring_want = g_ring_bytes;
    if (want) ring_want = std::min(g_ring_bytes, std::max<size_t>((size_t)16 << 20, align_up(want + 4096, (size_t)16 << 20)));
    if (c->ring_bytes && c->ring_bytes < ring_want) {              // grown for a bigger input
        for (int i = 0; i < 2; ++i) { hipFree(c->ring[i]); c->ring[i] = nullptr; }
        c->ring_bytes = 0;
    }
    for (; !c->ring_bytes; ring_want /= 2) {                       // halve on failure: a smaller ring is only more count calls
        if (ring_want < ((size_t)1 << 20)) return fail(c, KATGPU_ERR_NOMEM, "no device memory for the staging rings");
        bool ok = true;
        for (int i = 0; i < 2 && ok; ++i) {
            hipError_t e = hipMalloc((void**)&c->ring[i], ring_want);
            if (e != hipSuccess && c->arena && !c->arena_borrowed && !c->arena_busy) {       // the cached arena holds most of the free HBM: give it back
                (void)hipGetLastError();
                hipFree(c->arena); c->arena = nullptr; c->arena_bytes = 0;
                e = hipMalloc((void**)&c->ring[i], ring_want);
            }
            if (e != hipSuccess) { (void)hipGetLastError(); for (int j = 0; j < i; ++j) { hipFree(c->ring[j]); c->ring[j] = nullptr; } ok = false; }
        }
        if (ok) c->ring_bytes = ring_want;
    }
    return KATGPU_OK;
}

// Host base stream -> table.  The stream is copied through two pinned buffers (64 MiB each) into one of two DEVICE RINGS; a full
// ring is a resident stretch of the stream and goes to count_resident -- the partitioned counter for anything of size, exactly
// what a caller with device-resident input gets -- on a worker thread, while the feeder (and the parser team behind it) fills
// the other ring.  A ring starts with the previous ring's last k-1 bytes, so windows across the cut are counted once.
struct HostFeeder {
    katgpu_table* t; katgpu_ctx* c;
    int cur = 0; size_t fill = 0; bool pin_used[2] = {false, false};
    int ring_cur = 0; size_t ring_fill = 0;
    uint8_t tail[64]; uint32_t tail_n = 0;          // last k-1 bytes of the stream so far
    static constexpr size_t HEAD = 64;               // carry area (k - 1 <= 62 bytes) in front of a ring's payload: keeps it 16-byte aligned
    // worker
    std::thread worker;
    std::mutex mu; std::condition_variable cv;
    struct Job { int ring; size_t n; };
    std::deque<Job> jobs;
    bool ring_busy[2] = {false, false};
    bool stop = false;
    int worker_rc = KATGPU_OK; std::string worker_err;

    explicit HostFeeder(katgpu_table* t_) : t(t_), c(t_->ctx) {}
    ~HostFeeder() { shutdown(); }

    void run() {
        hipSetDevice(c->device);
        for (;;) {
            Job j;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return stop || !jobs.empty(); });
                if (jobs.empty()) return;
                j = jobs.front(); jobs.pop_front();
            }
            int rc = worker_rc ? worker_rc : count_resident(t, c->ring[j.ring], j.n);     // (after an error the queued rings are dropped, not counted)
            {
                std::lock_guard<std::mutex> lk(mu);
                if (rc && !worker_rc) { worker_rc = rc; worker_err = c->err; }
                ring_busy[j.ring] = false;
            }
            cv.notify_all();
        }
    }
    void shutdown() {
        if (!worker.joinable()) return;
        { std::lock_guard<std::mutex> lk(mu); stop = true; }
        cv.notify_all();
        worker.join();
    }
    int begin(size_t want = 0) {
        int rc = ensure_staging(c, want); if (rc) return rc;
        tail_n = 0;
        worker = std::thread([this] { run(); });
        return open_ring();
    }
    int open_ring() {                                 // ring_cur is free: seed its head with the carry
        uint8_t head[HEAD];
        memset(head, 'N', HEAD);
        memcpy(head + HEAD - tail_n, tail, tail_n);
        HIPCHK(c, hipMemcpyAsync(c->ring[ring_cur], head, HEAD, hipMemcpyHostToDevice, c->copy_stream));
        HIPCHK(c, hipStreamSynchronize(c->copy_stream));          // `head` is on this stack
        ring_fill = HEAD;
        return KATGPU_OK;
    }
    int submit_ring() {                               // hand the current ring to the worker, move on to the other one
        HIPCHK(c, hipStreamSynchronize(c->copy_stream));          // every copy into it has landed
        const int other = ring_cur ^ 1;
        {
            std::unique_lock<std::mutex> lk(mu);
            if (ring_fill > HEAD) { ring_busy[ring_cur] = true; jobs.push_back({ring_cur, ring_fill}); }
            cv.notify_all();
            cv.wait(lk, [&] { return !ring_busy[other]; });
            if (worker_rc) return fail(c, worker_rc, "%s", worker_err.c_str());
        }
        if (ring_fill > HEAD) ring_cur = other;
        return open_ring();
    }
    int push(const uint8_t* p, size_t n) {
        while (n) {
            if (fill == 0 && pin_used[cur]) { hipError_t e = hipEventSynchronize(c->pin_free[cur]); if (e != hipSuccess) return fail(c, KATGPU_ERR_DEVICE, "%s", hipGetErrorString(e)); }
            const size_t room = c->stage_bytes - fill, take = std::min(room, n);
            memcpy(c->pinned[cur] + fill, p, take);
            fill += take; p += take; n -= take;
            if (fill == c->stage_bytes) { int rc = flush(); if (rc) return rc; }
        }
        return KATGPU_OK;
    }
    int flush() {                                     // pinned[cur][0, fill) -> the current ring (asynchronously)
        if (!fill) return KATGPU_OK;
        const uint32_t want = t->dv.k - 1;
        size_t off = 0;
        while (off < fill) {
            if (ring_fill == c->ring_bytes) { int rc = submit_ring(); if (rc) return rc; }      // its head = `tail`, the k-1 bytes before `off`
            const size_t take = std::min(fill - off, c->ring_bytes - ring_fill);
            const uint8_t* src = c->pinned[cur] + off;
            HIPCHK(c, hipMemcpyAsync(c->ring[ring_cur] + ring_fill, src, take, hipMemcpyHostToDevice, c->copy_stream));
            ring_fill += take; off += take;
            // the last k-1 bytes of the stream that is in the rings so far
            if (take >= want) { memcpy(tail, src + take - want, want); tail_n = want; }
            else {
                uint8_t tmp[128]; const uint32_t keep = (uint32_t)std::min<size_t>(tail_n, want - take);
                memcpy(tmp, tail + tail_n - keep, keep); memcpy(tmp + keep, src, take);
                tail_n = keep + (uint32_t)take; memcpy(tail, tmp, tail_n);
            }
        }
        HIPCHK(c, hipEventRecord(c->pin_free[cur], c->copy_stream));
        pin_used[cur] = true;
        cur ^= 1; fill = 0;
        return KATGPU_OK;
    }
    int end_of_file() {             // files of a group never join (mer_overlap_sequence_parser.hpp:151-155: have_seam = false)
        static const uint8_t sep = 'N';
        return push(&sep, 1);
    }
    int finish() {
        int rc = flush(); if (rc) { shutdown(); return rc; }
        HIPCHK(c, hipStreamSynchronize(c->copy_stream));
        {
            std::unique_lock<std::mutex> lk(mu);
            if (ring_fill > HEAD) { ring_busy[ring_cur] = true; jobs.push_back({ring_cur, ring_fill}); }
            cv.notify_all();
            cv.wait(lk, [&] { return !ring_busy[0] && !ring_busy[1] && jobs.empty(); });
        }
        shutdown();
        if (worker_rc) return fail(c, worker_rc, "%s", worker_err.c_str());
        t->carry_n = 0;
        return refresh_counters(t);
    }
};

extern "C" int katgpu_count_bases_host(katgpu_table* t, const uint8_t* bases, size_t n) {
    if (!t || (!bases && n)) return KATGPU_ERR_INVALID_ARG;
    HIPCHK(t->ctx, hipSetDevice(t->ctx->device));
    t->carry_n = 0;
    HostFeeder f(t);
    int rc = f.begin(n); if (rc) return rc;
    rc = f.push(bases, n); if (rc) return rc;
    return f.finish();
}

// rank / world: this process's share of the group in a multi-GPU run.  Plain FASTQ files big enough for the device scan are cut
// between the ranks batch by batch (kg_scan.hip); every other file goes whole to rank (index mod world).
static int count_files_impl(katgpu_table* t, const char* const* paths, size_t n_paths, const uint16_t* trim5p, int rank, int world) {
    if (!t || !paths || world < 1 || rank < 0 || rank >= world) return KATGPU_ERR_INVALID_ARG;
    katgpu_ctx* c = t->ctx;
    HIPCHK(c, hipSetDevice(c->device));
    t->carry_n = 0;
    // Large plain FASTQ / FASTA files: raw bytes to the device, the record scan there (kg_scan.hip).  Files of a group never join and
    // the table is a multiset, so the order in which the group's files are counted is free.
    std::vector<const char*> rest;
    std::vector<uint16_t> rest_trim;
    size_t rest_bytes = 0;
    size_t whole = 0;                                              // files that are dealt whole, counted over the group
    for (size_t i = 0; i < n_paths; ++i) {
        const uint32_t trim = trim5p ? trim5p[i] : 0;
        bool took = false;
        uint8_t first = 0;
        if (world > 1 && device_scan_applies(paths[i], trim, nullptr, &first) && first == '@') {
            // a FASTQ file the ranks share out batch by batch: every rank takes this branch (the test is a property of the file), and a
            // rank that cannot -- no room for its batch buffers -- fails the run: falling back to the whole-file dealing on ONE rank
            // would count the file's batches twice or not at all, and put that rank's file counter out of step with the others'
            int rc = count_file_device_scan(t, paths[i], trim, &took, rank, world);
            if (rc) return rc;
            if (!took) return fail(c, KATGPU_ERR_NOMEM, "rank %d of %d: no device memory for the batch buffers of %s (a file the ranks share out cannot fall back to the streaming reader on one of them)", rank, world, paths[i]);
            continue;
        }
        if (world > 1 && (int)(whole++ % (size_t)world) != rank) continue;       // another rank's file
        int rc = count_file_device_scan(t, paths[i], trim, &took);
        if (rc) return rc;
        if (!took) { rest.push_back(paths[i]); rest_trim.push_back((uint16_t)trim); rest_bytes += (size_t)kg::file_size_or_zero(paths[i]); }
    }
    if (rest.empty()) { int wrc = table_wait(t); return wrc ? wrc : refresh_counters(t); }
    { int wrc = table_wait(t); if (wrc) return wrc; }                // (the streaming feeder does not overlap the allocation)
    HostFeeder f(t);
    int rc = f.begin(rest_bytes * 4); if (rc) return rc;           // (gzip inflates: be generous)
    // the group's other files -> one base stream (kg_ingest.hpp: thread team for large plain files, concurrent readers for gzip & co.)
    std::string err;
    rc = kg::stream_group(rest.data(), rest.size(), trim5p ? rest_trim.data() : nullptr, t->dv.k, [&](const uint8_t* p, size_t n) { return f.push(p, n); }, &err);
    if (rc) return err.empty() ? rc : fail(c, rc, "%s", err.c_str());
    return f.finish();
}

extern "C" int katgpu_count_files(katgpu_table* t, const char* const* paths, size_t n_paths, const uint16_t* trim5p) {
    return count_files_impl(t, paths, n_paths, trim5p, 0, 1);
}
extern "C" int katgpu_count_files_sharded(katgpu_table* t, const char* const* paths, size_t n_paths, const uint16_t* trim5p, int rank, int world) {
    return count_files_impl(t, paths, n_paths, trim5p, rank, world);
}

extern "C" int katgpu_count(katgpu_ctx* c, const char* const* paths, size_t n_paths, uint32_t k, int canonical,
                            const uint16_t* trim5p, uint64_t size_hint, int disable_grow, katgpu_table** out) {
    if (!c || !out || !paths) return KATGPU_ERR_INVALID_ARG;
    *out = nullptr;
    if (size_hint == 0) {        // every input byte starts at most one new k-mer
        uint64_t bytes = 0;
        for (size_t i = 0; i < n_paths; ++i) bytes += kg::file_size_or_zero(paths[i]);
        size_hint = std::max<uint64_t>(1u << 20, bytes);
    }
    // Big plain files: the table (and the feeders' arena) are allocated on a thread of their own while the device scan already reads
    // and parses into its accumulation buffers -- tens of GB of hipMalloc take about as long as the first GBs of the files take to arrive.
    uint64_t scan_bytes = 0;
    uint8_t scan_first = 0;
    for (size_t i = 0; i < n_paths; ++i) { uint64_t sz = 0; uint8_t fb = 0; if (device_scan_applies(paths[i], trim5p ? trim5p[i] : 0, &sz, &fb)) { scan_bytes += sz; if (!scan_first) scan_first = fb; } }
    katgpu_table* t = nullptr;
    int rc;
    if (scan_bytes >= ((uint64_t)4 << 30) && k >= 1 && k <= KATGPU_MAX_K && !getenv("KATGPU_SYNC_ALLOC")) {
        HIPCHK(c, hipSetDevice(c->device));
        t = new katgpu_table();
        t->ctx = c; t->disable_grow = disable_grow;
        t->dv.k = k; t->dv.canonical = canonical ? 1 : 0;                    // what the feeders' own threads look at before the slots exist
        const uint64_t cap = std::max<uint64_t>(size_hint, 1024);
        const size_t arena_bytes = scan_arena_bytes(scan_first);
        c->scan_waiting.store(1, std::memory_order_release);                  // the scan buffers go first (katgpu_ctx::scan_waiting; lowered by the first feeder's setup)
        c->big_alloc_running.store(1, std::memory_order_release);
        t->alloc_thread = std::thread([c, t, k, canonical, cap, arena_bytes]() {
            struct Done { katgpu_ctx* c; ~Done() { c->big_alloc_running.store(0, std::memory_order_release); } } done{c};
            hipSetDevice(c->device);
            alloc_turn(c, false, 3000.0);
            DevTable d{};
            bool lazy = false;
            const int arc = alloc_dev_table(c, k, canonical, cap, &d, 0, 0, &lazy);
            if (arc) { t->alloc_rc = arc; t->alloc_err = c->err; return; }
            t->dv = d;
            if (lazy) t->zero_from = 0;
            if (!c->arena && hipMalloc((void**)&c->arena, arena_bytes) == hipSuccess) c->arena_bytes = arena_bytes; else (void)hipGetLastError();
            if (g_trace) fprintf(stderr, "[katgpu +%.0f ms] table and arena allocated (beside the feeders)\n", since_load());
        });
        rc = KATGPU_OK;
    } else
        rc = katgpu_table_create(c, k, canonical, size_hint, disable_grow, &t);
    if (rc) return rc;
    rc = katgpu_count_files(t, paths, n_paths, trim5p);
    c->scan_waiting.store(0, std::memory_order_release);          // (a run whose files did not take the device scan after all)
    if (rc) { katgpu_table_free(t); return rc; }
    *out = t;
    return KATGPU_OK;
}

