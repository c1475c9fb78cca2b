// kg_jf.hpp -- what the .jf reader and writer (kg_jf.cpp, pure host code) ask of the device side (kg_jf_device.hip).
#pragma once
#include "../../include/katgpu.h"
#include <cstdio>
#include <functional>

struct JfDumpTiming { double device_s = 0, copy_s = 0, write_s = 0; uint32_t ranges = 0; };
struct JfGatherTiming : JfDumpTiming { double wire_s = 0; bool write_failed = false; };
struct JfLoadTiming { double read_s = 0, copy_s = 0, device_s = 0; uint32_t chunks = 0; };

constexpr int KG_JF_NO_SCRATCH = -1;     // the device scratch or the pinned buffers could not be had, or the table's positions are too skewed to order there: use the host writer, which starts the file afresh (the load: the host reader, before a record has been added)

// The records of a table (either key width) behind a header of matrix `cols` (2k columns of r bits): ordered and packed on the device, range of
// positions by range, copied out through two pinned buffers and appended to `f`.  KATGPU_ERR_IO: a short write.
int jf_stream_records(katgpu_table* t, uint32_t r, const uint64_t* cols, FILE* f, JfDumpTiming* tm);

// The next n records of `f` (ceil(key_len/8) + counter_len bytes each) added to t: read in chunks of records straight into one of two
// pinned buffers while the chunk before is copied to one of two device buffers and added there (katgpu_table_add_jf_records_device).
// Host: 2 pinned buffers of a chunk; device: 2 buffers of a chunk beside the table -- 2^24 records a chunk, 185 MB each at k = 27,
// whatever the file's size.  KATGPU_ERR_IO: a short read.
int jf_stream_load(katgpu_table* t, FILE* f, size_t n, uint32_t key_len, uint32_t counter_len, JfLoadTiming* tm);

// Collective, after the exchange: the records of every rank's table (disjoint k-mers, one k) behind a header of matrix `cols`, made for
// their n_total records, in the one file rank 0 writes.  Per range of positions -- the cuts come from the all-reduced position
// histogram -- every rank orders and packs its own records, the runs travel to rank 0 in one grouped transfer, and rank 0 orders and
// packs their union on its device and streams it out through two pinned buffers: nothing on a host grows with the tables.  All ranks
// allocate what a range can need first and agree on it: KATGPU_ERR_NOMEM on every rank, before open() has been called, when one of them
// cannot.  open() (rank 0 only) returns the file with its header written, or null: KATGPU_ERR_IO on every rank, agreed on before a
// run travels.  A failure after that is an error on every rank, and never KATGPU_ERR_NOMEM.
int jf_stream_gathered(katgpu_comm* m, katgpu_table* t, uint32_t r, const uint64_t* cols, uint64_t n_total, const std::function<FILE*()>& open, JfGatherTiming* tm);
