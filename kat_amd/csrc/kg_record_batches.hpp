// kg_record_batches.hpp -- where the batches of a per-record host form end (kg_host.hpp: for_record_batches) and how many bases the largest
// of them spans (kg_per_record.hip: what the gathered statistics size their buffers by before any work).  Host arithmetic only (no device
// code, no context): both come from here, and tests/native/record_batches_check.cc checks the cut on the CPU.
//
// The records lie in order and disjoint (check_records).  A batch is a run of records [r0, r1): its first record always joins; further
// records join while the batch has fewer than max_recs records, the span from the first record's start to this record's end stays within
// max_bases, and joins(r, false) says yes.  joins(r, first) is asked once for every record of a batch, in order, first == true for the
// batch's first record (whatever it answers then); it is asked after the two limits, and a record it refuses is asked again as the first
// of the next batch.  All of a batch's records have been asked when the batch comes back: what joins has added up over them is the batch's.
#pragma once
#include <cstddef>
#include <cstdint>

namespace kg {

struct RecordBatch { size_t r0, r1; uint64_t base; size_t nb; };     // records [r0, r1): nb bases from `base`, the first one's start, to the last one's end

// the batch that starts at record r0 < n_rec
template <typename Joins>
RecordBatch record_batch_at(const uint64_t* rec_start, const uint64_t* rec_len, size_t n_rec, size_t max_bases, size_t max_recs, Joins&& joins, size_t r0) {
    const uint64_t base = rec_start[r0];
    size_t r1 = r0;
    joins(r1++, true);
    while (r1 < n_rec && r1 - r0 < max_recs && rec_start[r1] + rec_len[r1] - base <= max_bases && joins(r1, false)) ++r1;
    return RecordBatch{r0, r1, base, (size_t)(rec_start[r1 - 1] + rec_len[r1 - 1] - base)};
}

// the most bases of one batch over the whole cut (no records: 0)
template <typename Joins>
size_t record_batches_max_bases(const uint64_t* rec_start, const uint64_t* rec_len, size_t n_rec, size_t max_bases, size_t max_recs, Joins&& joins) {
    size_t most = 0;
    for (size_t r0 = 0; r0 < n_rec;) {
        const RecordBatch b = record_batch_at(rec_start, rec_len, n_rec, max_bases, max_recs, joins, r0);
        if (b.nb > most) most = b.nb;
        r0 = b.r1;
    }
    return most;
}

}  // namespace kg
