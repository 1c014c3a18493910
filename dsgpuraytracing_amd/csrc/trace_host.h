// trace_host.h — the host side of the device ray queries (ptgpu.h:
// pt_trace_rays*), as pure functions: the argument check, the sizes of the
// output and of the spill area, the PT_TRACE_WAVES knob and the bounded grid.
// Plain C++17, no HIP: it runs, and is tested (tests/test_trace_host.py),
// without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/ptgpu.h"

#define PT_TRACE_RAY_BYTES 32     // a ray, and a closest-hit record: two float4
#define PT_TRACE_CHUNK 64         // rays per chunk: one wave, one lane each
#define PT_TRACE_MAX_RAYS ((int64_t)1 << 40)

// ceil(n / 64); 0 for n <= 0.
int64_t trace_chunks(int64_t n);

// Bytes the call writes at `out`: 32 per ray (closest) or 8 per chunk
// (occluded); 0 for n <= 0 or an unknown mode.
size_t trace_out_bytes(int64_t n, int32_t mode);

// nullptr when a call may run, else what is wrong with its arguments: a NULL
// buffer (with n > 0), n negative or beyond PT_TRACE_MAX_RAYS, an unknown
// mode, or the ray and output ranges sharing a byte.  (The context is the
// caller's to check.)
const char* trace_args_error(int64_t n, const void* rays, const void* out, int32_t mode);

// PT_TRACE_WAVES: the cap of the grid, 0 (none) for nullptr, "" or anything
// that is not a positive decimal number; values beyond INT32_MAX are INT32_MAX.
int trace_waves_knob(const char* env);

// One-wave workgroups of a trace of n rays: min(chunks, resident), capped by a
// positive knob, at least 1 for n > 0 (a device that reports no residency
// still runs), 0 for n <= 0.  Wave b takes the chunks b, b + grid, ...
int trace_grid(int64_t n, int64_t resident, int knob);

// Spill entries (ints) of a grid over a tree whose worst-case stack is
// bvh_stack; 0 when the LDS stack (stack_lds entries) holds it.
size_t trace_spill_entries(int bvh_stack, int stack_lds, int grid);
