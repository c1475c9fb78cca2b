// kg_windows.hpp -- the front end of every kernel that turns a base stream into k-mers, written once: one 16-byte load per lane
// (load16; byte by byte where the stream ends or is unaligned, bytes past the end read as 'N'), 2-bit codes + validity flags
// (encode16) parked in LDS with a few pad words behind them (StagedTile), and the register window a lane pulls out of LDS and slides
// sixteen times (LaneWindow for k <= 32, LaneWindowW for 33 <= k <= 63).  Barriers and unroll pragmas are the kernels' own.
// The stage kernels of the partitioned counter (k_p1v2_scatter, k_p1b_scatter) keep their own LDS layout -- 16-bit flags, the
// reverse-complement stream -- and share LaneWindow; p1_tile_fix (kg_partition.hpp) holds the one other copy of the byte-wise tail.
#pragma once
#include "kg_device.hpp"

namespace kg {

constexpr int BASES_PER_LANE = 16;               // one 16-byte global load per lane

// ---- loader ----
// the lanes whose 16 bytes cross the end of the stream, or whose stream is not 16-byte aligned: byte by byte, past the end == separator
__device__ __forceinline__ void load16_bytes(const uint8_t* __restrict__ bases, uint64_t n, uint64_t off, uint32_t (&w)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        uint32_t x = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) { uint64_t i = off + q * 4 + b; x |= (i < n ? (uint32_t)bases[i] : (uint32_t)'N') << (8 * b); }
        w[q] = x;
    }
}
template <bool ALIGNED /* bases + off is 16-byte aligned */>
__device__ __forceinline__ void load16(const uint8_t* __restrict__ bases, uint64_t n, uint64_t off, uint32_t (&w)[4]) {
    if (ALIGNED && off + BASES_PER_LANE <= n) {
        const uint4 v = *reinterpret_cast<const uint4*>(bases + off);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else load16_bytes(bases, n, off, w);
}

// 16 ASCII bytes -> 16 two-bit codes (MSB-first in a u32) + 16 "not ACGTacgt" flags (MSB-first in the low 16 bits).
// code = x ^ (x >> 1) with x = (c >> 1) & 3 maps A,C,G,T (either case) to 0,1,2,3 (mer_dna.hpp:46-63).
// Four bytes at a time (a byte-by-byte form was 200 of level 1's 1750 vector instructions per wave and tile): x per byte; the letter
// that x stands for, looked up by v_perm_b32 with x as the selector; a byte that is not that letter (case folded) is flagged; the
// four 2-bit codes / four flags of a word are gathered by one multiply each (the partial products land on distinct bits: no carries).
__device__ __forceinline__ void encode16(const uint32_t w[4], uint32_t& code, uint32_t& bad) {
    code = 0; bad = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint32_t v = w[q];
        const uint32_t x = (v >> 1) & 0x03030303u;                                   // A, C, T, G -> 0, 1, 2, 3
        const uint32_t c2 = x ^ ((x >> 1) & 0x01010101u);                            // A, C, G, T -> 0, 1, 2, 3
        const uint32_t letter = __builtin_amdgcn_perm(0u, 0x67746361u, x);           // 'a', 'c', 't', 'g' by x
        const uint32_t diff = (v | 0x20202020u) ^ letter;
        const uint32_t nz = ((((diff & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | diff) >> 7) & 0x01010101u;    // 1 per byte that is no such letter
        code = (code << 8) | ((c2 * 0x40100401u) >> 24);                             // byte 0 (the first base) into the top pair
        bad = (bad << 4) | ((nz * 0x08040201u) >> 24);
    }
}

// ---- staged tile ----
// A block's codes and flags, one word of each per lane, and PAD words behind them that read as "no base": lane t's window reaches
// PAD words beyond its own (2 for the 96-bit window, 4 for the 160-bit one -- fewer would read stale LDS).  The pad words never
// change: a kernel writes them once, before its first barrier, or along with every tile (pad() is apart from stage() because pad
// words written inside the chunk loop cost k_profile's wide shape two VGPRs and with them a wave per SIMD).
template <int BLOCK, int PAD>
struct StagedTile {
    uint32_t code[BLOCK + PAD];
    alignas(16) uint32_t bad[BLOCK + PAD];     // (where a second LDS array would start: k_seq_hits keeps its 60 VGPRs; 8 bytes more LDS for PAD = 2)
    __device__ __forceinline__ void stage(uint32_t c, uint32_t b) { code[threadIdx.x] = c; bad[threadIdx.x] = b; }
    __device__ __forceinline__ void pad() { if (threadIdx.x < PAD) { code[BLOCK + threadIdx.x] = 0; bad[BLOCK + threadIdx.x] = 0xFFFF; } }
};

// ---- windows ----
__device__ __forceinline__ uint64_t canon_if(uint64_t fwd, uint32_t k, bool canonical) {
    if (!canonical) return fwd;
    const uint64_t rc = kmer_revcomp(fwd, k);
    return rc < fwd ? rc : fwd;
}

// k <= 32.  Lane t owns the 16 window starts [16t, 16t+16): three consecutive code words (48 bases) in a 96-bit register window,
// slid 16 times -- no per-base loop, no re-reading of HBM.
struct LaneWindow {
    uint64_t hi, lo, m;
    uint32_t kshift, mshift;
    template <typename BadT>
    __device__ __forceinline__ void init(const uint32_t* code, const BadT* bad, uint32_t w, uint32_t k) {
        hi = ((uint64_t)code[w] << 32) | code[w + 1];                        // bases 16w .. 16w+31
        lo = (uint64_t)code[w + 2] << 32;                                    // bases 16w+32 .. 16w+47
        m = ((uint64_t)bad[w] << 48) | ((uint64_t)bad[w + 1] << 32) | ((uint64_t)bad[w + 2] << 16);
        kshift = 64 - 2 * k; mshift = 64 - k;
    }
    __device__ __forceinline__ bool valid() const { return (m >> mshift) == 0; }     // k valid bases from this start
    __device__ __forceinline__ uint64_t fwd() const { return hi >> kshift; }
    // what the counters count: the reverse complement recomputed from the forward word (v_bfrev, 6 VALU ops) rather than rolled
    __device__ __forceinline__ uint64_t counted(uint32_t k, bool canonical) const { return canon_if(fwd(), k, canonical); }
    __device__ __forceinline__ void step() { hi = (hi << 2) | (lo >> 62); lo <<= 2; m <<= 1; }
};

// 33 <= k <= 63.  Lane t needs bases 16t .. 16t+77: five code words = a 160-bit register window (hi, lo, nx).  The k-mer is the top
// 2k bits of (hi, lo).
struct LaneWindowW {
    uint64_t hi, lo, nx, m, mn;
    uint32_t s, mshift;
    __device__ __forceinline__ void init(const uint32_t* code, const uint32_t* bad, uint32_t w, uint32_t k) {
        hi = ((uint64_t)code[w] << 32) | code[w + 1];                        // bases 16w    .. 16w+31
        lo = ((uint64_t)code[w + 2] << 32) | code[w + 3];                    // bases 16w+32 .. 16w+63
        nx = (uint64_t)code[w + 4] << 32;                                    // bases 16w+64 .. 16w+79
        m = ((uint64_t)bad[w] << 48) | ((uint64_t)bad[w + 1] << 32) | ((uint64_t)bad[w + 2] << 16) | bad[w + 3];
        mn = (uint64_t)bad[w + 4] << 48;
        s = 128 - 2 * k; mshift = 64 - k;                                   // s: 2 .. 62, mshift: 1 .. 31
    }
    __device__ __forceinline__ bool valid() const { return (m >> mshift) == 0; }     // (k <= 63 < 64 flags)
    __device__ __forceinline__ uint64_t fwd_hi() const { return hi >> s; }
    __device__ __forceinline__ uint64_t fwd_lo() const { return (lo >> s) | (hi << (64 - s)); }
    __device__ __forceinline__ KeyW fwd() const { return keyw_from_words(fwd_hi(), fwd_lo()); }
    // what the counters count: as LaneWindow::counted, compared as words before the halves are cut
    __device__ __forceinline__ KeyW counted(uint32_t k, bool canonical) const {
        const uint64_t fhi = fwd_hi(), flo = fwd_lo();
        KeyW key = keyw_from_words(fhi, flo);
        if (canonical) {
            uint64_t rhi, rlo;
            revcomp_words(fhi, flo, k, rhi, rlo);
            if (rhi < fhi || (rhi == fhi && rlo < flo)) key = keyw_from_words(rhi, rlo);
        }
        return key;
    }
    __device__ __forceinline__ void step() {
        hi = (hi << 2) | (lo >> 62);
        lo = (lo << 2) | (nx >> 62);
        nx <<= 2;
        m = (m << 1) | (mn >> 63);
        mn <<= 1;
    }
};

}  // namespace kg
