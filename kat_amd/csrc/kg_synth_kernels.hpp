// kg_synth_kernels.hpp -- the synthetic workload (bench / tests) made on the device, bit-identical to kat_amd/synth.py:
// k_synth_genome (a genome or an assembly's base stream) and k_synth_reads (paired reads with substitution errors).  Launched by
// kg_context.hip (katgpu_synth_*) and tools/ubench_count.hip.  They replace nothing of the reference: they stand in for input files.
#pragma once
#include "kg_device.hpp"

namespace kg {

__device__ __forceinline__ uint32_t genome_code(uint64_t seed, uint64_t i) {
    return (uint32_t)(rng2(seed, i >> 5) >> (2 * (i & 31))) & 3;
}
// contig_len == 0: n bases.  contig_len > 0: the assembly's base stream, an 'N' after every contig_len bases
// (n counts output bytes, separators included).
static __global__ void __launch_bounds__(256)
k_synth_genome(uint8_t* __restrict__ out, uint64_t n, uint64_t seed, uint64_t contig_len) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < n; x += stride) {
        uint64_t i = x;
        if (contig_len) {
            uint64_t c = x / (contig_len + 1), j = x - c * (contig_len + 1);
            if (j == contig_len) { out[x] = 'N'; continue; }
            i = c * contig_len + j;
        }
        out[x] = "ACGT"[genome_code(seed, i)];
    }
}
// one lane per base: reads are laid out with stride read_len+1 ('N' separator closes every record)
static __global__ void __launch_bounds__(256)
k_synth_reads(const uint8_t* __restrict__ genome, uint64_t genome_len, uint8_t* __restrict__ out, uint64_t first_read,
              uint64_t n_reads, uint32_t read_len, uint32_t frag_len, uint32_t err_thresh, uint64_t seed) {
    const uint64_t rec = (uint64_t)read_len + 1, total = n_reads * rec;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += stride) {
        uint64_t rl = x / rec;
        uint32_t j = (uint32_t)(x - rl * rec);
        if (j == read_len) { out[x] = 'N'; continue; }
        uint64_t r = first_read + rl, pair = r >> 1, mate = r & 1;
        uint64_t u = rng2(seed, pair);
        uint64_t start = __umul64hi(u, genome_len - frag_len + 1);
        uint64_t strand = splitmix64(u) >> 63;
        bool fwd = (strand ^ mate) == 0;
        uint8_t g = genome[fwd ? start + j : start + frag_len - 1 - j];
        uint32_t code = ((g >> 1) & 3) ^ ((g >> 2) & 1);
        if (!fwd) code = 3 - code;
        uint64_t e = rng2(seed ^ 0x5EED5EED5EED5EEDULL, r * 1024 + j);
        if ((uint32_t)e < err_thresh) code = (code + 1 + (uint32_t)((e >> 32) % 3)) & 3;
        out[x] = "ACGT"[code];
    }
}

}  // namespace kg
