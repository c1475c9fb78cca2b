// kg_jf.hpp -- what the .jf reader and writer (kg_jf.cpp, pure host code) ask of the device side (kg_jf_device.hip).
#pragma once
#include "../../include/katgpu.h"
#include <cstdio>

struct JfDumpTiming { double device_s = 0, copy_s = 0, write_s = 0; uint32_t ranges = 0; };
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
