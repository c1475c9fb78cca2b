// record_batches_check.cc -- kg_record_batches.hpp on the host, without a GPU (tests/test_record_batches.py builds this plain and with
// -fsanitize=address,undefined and runs both): every layout of at most 5 records with lengths from {0, 1, 3, 7} and gaps from {0, 1} in
// front of each, cut at max_bases from {1, 4, 8, 100} and max_recs from {1, 2, 3, 8} under three kinds of `joins`: one that always says yes,
// a window budget shaped like kg_per_record.hip's StatsJoins (k = 3, a record of more than 2 windows is long, budgets of 1 and 4 windows),
// and one that says yes and writes down what it is asked.  The cut is held against a restatement of the rule as one loop over the records.
#include <stdint.h>
#include <stdio.h>

#include "../../kat_amd/csrc/kg_record_batches.hpp"

using namespace kg;

static unsigned long long n_checks = 0, n_failed = 0, n_cuts = 0;
#define CHECK(cond, ...)                                                       \
    do {                                                                       \
        ++n_checks;                                                            \
        if (!(cond)) {                                                         \
            if (++n_failed <= 20) { printf("FAILED %s:%d %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                      \
    } while (0)

constexpr int MAX_REC = 5;
constexpr uint32_t K = 3, SHORT_WINDOWS = 2;
struct Ask { size_t r; bool first; };
struct AskLog { Ask a[4 * MAX_REC]; size_t n = 0; void add(size_t r, bool first) { if (n < 4 * MAX_REC) a[n] = Ask{r, first}; ++n; } };

// the windows a record adds to its batch's long records (0: it is a short one)
static uint64_t long_windows_of(uint64_t len) {
    const uint64_t w = len >= K ? len - K + 1 : 0;
    return w <= SHORT_WINDOWS ? 0 : w;
}

// the three kinds.  budget == 0: no budget.  Every one logs what it is asked.
struct Joins {
    const uint64_t* rec_len; uint64_t budget; AskLog* log;
    uint64_t n_long = 0, long_windows = 0;
    bool operator()(size_t r, bool first) {
        log->add(r, first);
        if (first) n_long = long_windows = 0;
        const uint64_t w = budget ? long_windows_of(rec_len[r]) : 0;
        if (!first && budget && long_windows + w > budget) return false;
        n_long += w != 0; long_windows += w;
        return true;
    }
};

// The rule again, record by record: starts[r] = record r begins a batch, and the questions that the cut must have put, in order.
struct Model { bool starts[MAX_REC + 1]; AskLog asks; };
static Model model_of(const uint64_t* st, const uint64_t* ln, size_t n_rec, size_t max_bases, size_t max_recs, uint64_t budget) {
    Model m;
    size_t first = 0, in_batch = 0;
    uint64_t windows = 0;
    for (size_t r = 0; r < n_rec; ++r) {
        bool joins = r != 0 && in_batch < max_recs && st[r] + ln[r] - st[first] <= max_bases;
        if (joins) {                                           // (only then is the callable asked)
            m.asks.add(r, false);
            joins = !budget || windows + long_windows_of(ln[r]) <= budget;
        }
        m.starts[r] = !joins;
        if (!joins) { first = r; in_batch = 0; windows = 0; m.asks.add(r, true); }
        ++in_batch; windows += budget ? long_windows_of(ln[r]) : 0;
    }
    m.starts[n_rec] = true;
    return m;
}

static void check_cut(const uint64_t* st, const uint64_t* ln, size_t n_rec, size_t max_bases, size_t max_recs, uint64_t budget) {
    ++n_cuts;
    const Model m = model_of(st, ln, n_rec, max_bases, max_recs, budget);
    AskLog log;
    Joins joins{ln, budget, &log};
    size_t most = 0, expect_r0 = 0;
    for (size_t r0 = 0; r0 < n_rec;) {
        const RecordBatch b = record_batch_at(st, ln, n_rec, max_bases, max_recs, joins, r0);
        // in order, no gap, not empty, inside the records: a partition of [0, n_rec)
        CHECK(b.r0 == expect_r0 && b.r1 > b.r0 && b.r1 <= n_rec, "batch [%zu, %zu) after %zu of %zu", b.r0, b.r1, expect_r0, n_rec);
        if (!(b.r1 > r0 && b.r1 <= n_rec)) return;
        CHECK(b.base == st[b.r0] && b.nb == st[b.r1 - 1] + ln[b.r1 - 1] - st[b.r0], "base %llu nb %zu of [%zu, %zu)", (unsigned long long)b.base, b.nb, b.r0, b.r1);
        // the two limits; a single record may be longer
        CHECK(b.r1 - b.r0 <= (max_recs ? max_recs : 1), "%zu records, max_recs %zu", b.r1 - b.r0, max_recs);
        CHECK(b.nb <= max_bases || b.r1 - b.r0 == 1, "%zu bases in %zu records, max_bases %zu", b.nb, b.r1 - b.r0, max_bases);
        // what joins has added up is this batch's, whole, when the caller sees it
        uint64_t n_long = 0, windows = 0;
        for (size_t r = b.r0; r < b.r1; ++r) { const uint64_t w = budget ? long_windows_of(ln[r]) : 0; n_long += w != 0; windows += w; }
        CHECK(joins.n_long == n_long && joins.long_windows == windows, "joins holds %llu long records of %llu windows, the batch %llu of %llu", (unsigned long long)joins.n_long,
              (unsigned long long)joins.long_windows, (unsigned long long)n_long, (unsigned long long)windows);
        CHECK(!budget || b.r1 - b.r0 == 1 || windows <= budget, "%llu long windows in %zu records, budget %llu", (unsigned long long)windows, b.r1 - b.r0, (unsigned long long)budget);
        // greedy: the batch ends at the records' end, or where one of the three reasons holds for the next record
        if (b.r1 < n_rec) {
            const bool full = b.r1 - b.r0 >= max_recs, wide = st[b.r1] + ln[b.r1] - b.base > max_bases;
            const bool refused = budget && windows + long_windows_of(ln[b.r1]) > budget;
            CHECK(full || wide || refused, "batch [%zu, %zu) ends for no reason: max_bases %zu max_recs %zu budget %llu", b.r0, b.r1, max_bases, max_recs, (unsigned long long)budget);
        }
        // the same boundaries as the record-by-record rule
        for (size_t r = b.r0; r <= b.r1; ++r) CHECK(m.starts[r] == (r == b.r0 || r == b.r1), "record %zu of batch [%zu, %zu): the model %s a batch there", r, b.r0, b.r1, m.starts[r] ? "starts" : "does not start");
        if (b.nb > most) most = b.nb;
        expect_r0 = r0 = b.r1;
    }
    CHECK(expect_r0 == n_rec, "the batches end at %zu of %zu records", expect_r0, n_rec);
    // the questions: the model's, in its order
    CHECK(log.n == m.asks.n && log.n <= 4 * MAX_REC, "%zu questions, the model has %zu", log.n, m.asks.n);
    for (size_t i = 0; i < log.n && i < m.asks.n && i < 4 * MAX_REC; ++i)
        CHECK(log.a[i].r == m.asks.a[i].r && log.a[i].first == m.asks.a[i].first, "question %zu is (%zu, %d), the model's (%zu, %d)", i, log.a[i].r, (int)log.a[i].first, m.asks.a[i].r, (int)m.asks.a[i].first);
    if (!budget) {                                             // nobody refuses: exactly once per record, in order, first exactly at the batch starts
        CHECK(log.n == n_rec, "%zu questions for %zu records", log.n, n_rec);
        for (size_t r = 0; r < n_rec && r < log.n; ++r) CHECK(log.a[r].r == r && log.a[r].first == m.starts[r], "question %zu is (%zu, %d)", r, log.a[r].r, (int)log.a[r].first);
    }
    // the sizing helper walks the same cut with a fresh callable
    AskLog log2;
    const size_t helper = record_batches_max_bases(st, ln, n_rec, max_bases, max_recs, Joins{ln, budget, &log2});
    CHECK(helper == most && log2.n == log.n, "the largest batch: helper %zu (%zu questions), walk %zu (%zu)", helper, log2.n, most, log.n);
}

int main() {
    const uint64_t lens[] = {0, 1, 3, 7}, gaps[] = {0, 1}, budgets[] = {0, 1, 4};      // (budget 0: the callable that always says yes, whose log is the third kind)
    const size_t max_bases[] = {1, 4, 8, 100}, max_recs[] = {1, 2, 3, 8};
    for (size_t n_rec = 0; n_rec <= MAX_REC; ++n_rec) {
        size_t n_layouts = 1;
        for (size_t r = 0; r < n_rec; ++r) n_layouts *= 8;
        for (size_t code = 0; code < n_layouts; ++code) {
            uint64_t st[MAX_REC + 1] = {0}, ln[MAX_REC + 1] = {0};
            uint64_t at = 0;
            size_t c = code;
            for (size_t r = 0; r < n_rec; ++r, c /= 8) { st[r] = at + gaps[c & 1]; ln[r] = lens[(c >> 1) & 3]; at = st[r] + ln[r]; }
            for (size_t mb : max_bases)
                for (size_t mr : max_recs)
                    for (uint64_t budget : budgets) check_cut(st, ln, n_rec, mb, mr, budget);
        }
    }
    printf("%llu cuts, %llu checks, %llu failed\n", n_cuts, n_checks, n_failed);
    if (n_failed) return 1;
    printf("record batches ok\n");
    return 0;
}
