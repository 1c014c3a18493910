// host_driver.cpp — drives the pure host parts of the device ray queries
// (csrc/trace_host.cpp) for tests/test_trace_host.py, which builds it with
// -fsanitize=address,undefined.  One case per stdin line:
//   chunks <n>                          -> {"v": chunks}
//   bytes <n> <mode>                    -> {"v": bytes}
//   args <n> <rays addr> <out addr> <mode>  -> {"error": "..."} ("" when valid)
//   knob <text or nothing>              -> {"v": knob}
//   grid <n> <resident> <knob>          -> {"v": grid}
//   spill <bvh_stack> <stack_lds> <grid>  -> {"v": entries}
#include <cinttypes>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "trace_host.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "chunks") {
      int64_t n = 0;
      in >> n;
      std::printf("{\"v\": %" PRId64 "}\n", trace_chunks(n));
    } else if (what == "bytes") {
      int64_t n = 0;
      int32_t mode = 0;
      in >> n >> mode;
      std::printf("{\"v\": %zu}\n", trace_out_bytes(n, mode));
    } else if (what == "args") {
      int64_t n = 0;
      uint64_t a = 0, b = 0;
      int32_t mode = 0;
      in >> n >> a >> b >> mode;
      const char* e = trace_args_error(n, (const void*)(uintptr_t)a, (const void*)(uintptr_t)b, mode);
      std::printf("{\"error\": \"%s\"}\n", e ? e : "");
    } else if (what == "knob") {
      std::string text;
      const bool given = (bool)(in >> text);
      std::printf("{\"v\": %d}\n", trace_waves_knob(given ? text.c_str() : nullptr));
    } else if (what == "knob_empty") {
      std::printf("{\"v\": %d}\n", trace_waves_knob(""));
    } else if (what == "grid") {
      int64_t n = 0, resident = 0;
      int knob = 0;
      in >> n >> resident >> knob;
      std::printf("{\"v\": %d}\n", trace_grid(n, resident, knob));
    } else if (what == "spill") {
      int stack = 0, lds = 0, grid = 0;
      in >> stack >> lds >> grid;
      std::printf("{\"v\": %zu}\n", trace_spill_entries(stack, lds, grid));
    } else {
      std::printf("{\"unknown\": 1}\n");
    }
  }
  return 0;
}
