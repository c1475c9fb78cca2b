// record_stats_host.hpp -- a record's katgpu_record_stats from its bases and its per-position counts, on the host: the arithmetic of
// Sect::processSeq (src/sect.cc:516-579), which `katgpu sect` runs on the counts the device wrote and `katgpu cold --gpus N` on the
// counts gathered from the ranks (katgpu_table_profile_gathered_host).  Same fields as katgpu_table_record_stats_* computes on the
// device (include/katgpu.h); header-only and free of the engine, so that tests/native/record_stats_host_check.cc can run it alone.
#pragma once
#include <katgpu.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace kat {

inline bool isBase(char c) {                    // lib/include/kat/str_utils.hpp:183-201 (validKmer)
    switch (c) { case 'A': case 'a': case 'C': case 'c': case 'G': case 'g': case 'T': case 't': return true; default: return false; }
}
inline bool isGC(char c) { return c == 'G' || c == 'g' || c == 'C' || c == 'c'; }

// cnt[i] = the count of the window starting at seq[i], for the nb = len - k + 1 windows of the record (none when len < k; cnt is not
// read then and may be null).  An invalid window -- one holding a byte outside ACGTacgt -- enters the median as 0 whatever cnt says of
// it and nothing else.  gc_windows, when given, receives the G+C of every window, -1 for an invalid one (printGCCounts wants them).
inline katgpu_record_stats recordStatsFromCounts(const char* seq, size_t len, uint32_t k, const uint64_t* cnt, std::vector<int16_t>* gc_windows = nullptr) {
    katgpu_record_stats st{};
    const size_t nb = k && len >= k ? len - k + 1 : 0;
    if (gc_windows) gc_windows->assign(nb, 0);
    if (nb) {
        // validity and GC of every window by a rolling scan (the reference re-reads k characters per window)
        std::vector<uint64_t> sorted(nb);
        uint32_t bad = 0, g = 0;
        for (size_t i = 0; i < len; i++) {
            bad += !isBase(seq[i]); g += isGC(seq[i]);
            if (i >= k) { bad -= !isBase(seq[i - k]); g -= isGC(seq[i - k]); }
            if (i + 1 < k) continue;
            const size_t w = i + 1 - k;
            if (gc_windows) (*gc_windows)[w] = bad ? (int16_t)-1 : (int16_t)g;
            sorted[w] = bad ? 0 : cnt[w];
            if (bad) st.invalid++;
            else { st.sum += cnt[w]; if (cnt[w]) st.non_zero++; }
        }
        std::nth_element(sorted.begin(), sorted.begin() + nb / 2, sorted.end());                // == sort()[size/2] (:540-542)
        st.median = sorted[nb / 2];
    }
    for (size_t i = 0; i < len; i++) {
        const char c = seq[i];
        if (isGC(c)) st.gc_bases++;
        else if (c == 'N' || c == 'n') st.n_bases++;
    }
    return st;
}

}  // namespace kat
