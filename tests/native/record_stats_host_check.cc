// record_stats_host_check.cc -- kat_amd/csrc/host/record_stats_host.hpp (a record's katgpu_record_stats from its per-position counts:
// what `katgpu sect` and `katgpu cold --gpus N` compute on the host) against the vectors of tests/record_stats_model.py, as a program
// of its own: tests/test_record_stats_host.py writes the vectors, builds this with -fsanitize=address,undefined and runs it.
// argv[1]: the vectors -- u32 k, u32 records; per record u64 length, the bases, the length - k + 1 counts (u64 each; none when the
// record is shorter than k), the six expected words in the order of the struct.
#include "record_stats_host.hpp"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

static bool get(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, 1, bytes, f) == bytes; }

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <vectors>\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    uint32_t k = 0, n_rec = 0;
    if (!get(f, &k, 4) || !get(f, &n_rec, 4)) { fprintf(stderr, "short header\n"); return 2; }
    static_assert(sizeof(katgpu_record_stats) == 6 * sizeof(uint64_t), "six words");
    unsigned bad = 0;
    for (uint32_t r = 0; r < n_rec; ++r) {
        uint64_t len = 0;
        if (!get(f, &len, 8)) { fprintf(stderr, "short record %u\n", r); return 2; }
        // exactly as long as the record and its windows: a read past either end is the sanitizer's to report
        std::vector<char> seq((size_t)len);
        const size_t nb = len >= k ? (size_t)(len - k + 1) : 0;
        std::vector<uint64_t> cnt(nb);
        katgpu_record_stats want;
        if (!get(f, seq.data(), seq.size()) || !get(f, cnt.data(), nb * 8) || !get(f, &want, sizeof want)) { fprintf(stderr, "short record %u\n", r); return 2; }
        std::vector<int16_t> gc;
        const katgpu_record_stats a = kat::recordStatsFromCounts(seq.data(), seq.size(), k, nb ? cnt.data() : nullptr, &gc);
        const katgpu_record_stats b = kat::recordStatsFromCounts(seq.data(), seq.size(), k, nb ? cnt.data() : nullptr);
        uint64_t gc_invalid = 0;
        for (int16_t g : gc) gc_invalid += g < 0;
        if (memcmp(&a, &want, sizeof want) || memcmp(&b, &want, sizeof want) || gc.size() != nb || gc_invalid != want.invalid) {
            if (bad++ < 10)
                fprintf(stderr, "record %u (length %llu, k %u): sum %llu/%llu median %llu/%llu non_zero %llu/%llu invalid %llu/%llu gc %llu/%llu n %llu/%llu, %zu gc windows (%llu invalid)\n",
                        r, (unsigned long long)len, k, (unsigned long long)a.sum, (unsigned long long)want.sum, (unsigned long long)a.median, (unsigned long long)want.median,
                        (unsigned long long)a.non_zero, (unsigned long long)want.non_zero, (unsigned long long)a.invalid, (unsigned long long)want.invalid,
                        (unsigned long long)a.gc_bases, (unsigned long long)want.gc_bases, (unsigned long long)a.n_bases, (unsigned long long)want.n_bases, gc.size(),
                        (unsigned long long)gc_invalid);
        }
    }
    fclose(f);
    if (bad) { fprintf(stderr, "%u of %u records differ\n", bad, n_rec); return 1; }
    printf("record stats host ok: %u records at k = %u\n", n_rec, k);
    return 0;
}
