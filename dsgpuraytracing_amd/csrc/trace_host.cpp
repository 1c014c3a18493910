// trace_host.cpp — see trace_host.h.
#include "trace_host.h"

#include <algorithm>
#include <climits>

int64_t trace_chunks(int64_t n) { return n <= 0 ? 0 : (n - 1) / PT_TRACE_CHUNK + 1; }

size_t trace_out_bytes(int64_t n, int32_t mode) {
  if (n <= 0) return 0;
  if (mode == PT_TRACE_CLOSEST) return (size_t)n * PT_TRACE_RAY_BYTES;
  if (mode == PT_TRACE_OCCLUDED) return (size_t)trace_chunks(n) * 8;
  return 0;
}

const char* trace_args_error(int64_t n, const void* rays, const void* out, int32_t mode) {
  if (n < 0) return "n is negative";
  if (n > PT_TRACE_MAX_RAYS) return "more than 2^40 rays";
  if (mode != PT_TRACE_CLOSEST && mode != PT_TRACE_OCCLUDED) return "unknown mode";
  if (n == 0) return nullptr;
  if (!rays || !out) return "NULL buffer";
  const uintptr_t a = (uintptr_t)rays, b = (uintptr_t)out;
  const uintptr_t alen = (uintptr_t)n * PT_TRACE_RAY_BYTES, blen = (uintptr_t)trace_out_bytes(n, mode);
  // (a - b and b - a wrap instead of a + alen overflowing at the top of the address space)
  if (a >= b ? a - b < blen : b - a < alen) return "the ray and output ranges overlap";
  return nullptr;
}

int trace_waves_knob(const char* env) {
  if (!env || !*env) return 0;
  int64_t v = 0;
  for (const char* p = env; *p; ++p) {
    if (*p < '0' || *p > '9') return 0;
    v = std::min<int64_t>(v * 10 + (*p - '0'), INT32_MAX);
  }
  return (int)v;
}

int trace_grid(int64_t n, int64_t resident, int knob) {
  const int64_t chunks = trace_chunks(n);
  if (chunks == 0) return 0;
  int64_t g = std::min(chunks, std::max<int64_t>(resident, 1));
  if (knob > 0) g = std::min<int64_t>(g, knob);
  return (int)std::min<int64_t>(g, INT32_MAX);
}

size_t trace_spill_entries(int bvh_stack, int stack_lds, int grid) {
  if (bvh_stack <= stack_lds || grid <= 0) return 0;
  return (size_t)(bvh_stack - stack_lds) * (size_t)grid * PT_TRACE_CHUNK;
}
