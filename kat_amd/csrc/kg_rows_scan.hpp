// kg_rows_scan.hpp -- k_rows_scan: the exclusive scan of the rows of a u32 matrix, one workgroup per row (gfx950, wave64).
// A header of its own because two units launch it and nothing else goes with it: kg_exchange.hip (region counts -> record offsets per
// owner) and kg_scan.hip (newlines / output bytes per tile -> the tiles' first line / first byte).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kg {

// Exclusive scan of each row of a u32 matrix into u64 (row_base[r] added when given); one workgroup per row.
// off may be null (totals only); off rows have n_cols + 1 entries when `closed` (the last one is the row total).
static __global__ void __launch_bounds__(1024)
k_rows_scan(const uint32_t* __restrict__ m, uint32_t n_cols, uint64_t row_stride, const uint64_t* __restrict__ row_base,
            uint64_t* __restrict__ off, uint64_t off_stride, int closed, unsigned long long* __restrict__ totals) {
    __shared__ uint64_t s_wave[16];
    __shared__ uint64_t s_run;
    const uint32_t r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t* row = m + (uint64_t)r * row_stride;
    if (tid == 0) s_run = row_base ? row_base[r] : 0;
    __syncthreads();
    for (uint32_t c0 = 0; c0 < n_cols; c0 += 1024) {
        const uint32_t c = c0 + tid;
        const uint64_t v = c < n_cols ? row[c] : 0;
        uint64_t x = v;                                            // inclusive scan within the wave
        for (int d = 1; d < 64; d <<= 1) { uint64_t y = __shfl_up(x, d, 64); if ((int)lane >= d) x += y; }
        if (lane == 63) s_wave[w] = x;
        __syncthreads();
        uint64_t before = s_run;
        for (uint32_t q = 0; q < w; ++q) before += s_wave[q];
        if (off && c < n_cols) off[(uint64_t)r * off_stride + c] = before + x - v;
        __syncthreads();
        if (tid == 1023) s_run = before + x;
        __syncthreads();
    }
    if (tid == 0) {
        if (off && closed) off[(uint64_t)r * off_stride + n_cols] = s_run;
        if (totals) totals[r] = s_run - (row_base ? row_base[r] : 0);
    }
}

}  // namespace kg
