// kg_jf.hpp -- what the .jf writer (kg_jf.cpp, pure host code) asks of the device side (kg_table.hip).
#pragma once
#include "../../include/katgpu.h"
#include <cstdio>

struct JfDumpTiming { double device_s = 0, copy_s = 0, write_s = 0; uint32_t ranges = 0; };

constexpr int KG_JF_NO_SCRATCH = -1;     // the device scratch or the pinned buffers could not be had, or the table's positions are too skewed to order there: use the host writer, which starts the file afresh

// The records of a k <= 32 table behind a header of matrix `cols` (2k columns of r bits): ordered and packed on the device, range of
// positions by range, copied out through two pinned buffers and appended to `f`.  KATGPU_ERR_IO: a short write.
int jf_stream_records(katgpu_table* t, uint32_t r, const uint64_t* cols, FILE* f, JfDumpTiming* tm);
