// pt_api_trace.cpp — C ABI of the HIP path, third part (include/ptgpu.h): ray
// queries on the device (pt_trace_rays*, pt_camera_rays_device; kernels:
// pt_kernels.hip trace_kernel, camera_rays_kernel; pure host parts:
// trace_host.cpp).  The context is declared in pt_ctx.h.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pt_ctx.h"
#include "trace_host.h"

namespace {
int fail(int code, const std::string& msg) { return pt_fail(code, msg); }

// What both entry points refuse: first what needs no context (the arguments),
// then the context, then the scene.
int trace_check(pt_ctx* c, int64_t n, const void* rays, const void* out, int32_t mode, const char* fn) {
  if (const char* what = trace_args_error(n, rays, out, mode)) return fail(PT_E_INVALID, std::string(fn) + ": " + what);
  if (!c) return fail(PT_E_INVALID, std::string(fn) + ": NULL context");
  if (!c->have_scene) return fail(PT_E_NOSCENE, std::string(fn) + " before pt_upload_scene");
  return PT_OK;
}

// The trace of n > 0 checked rays on `s`: the grid, the spill area it needs,
// the counter zeroed, the kernel between the timing events.
int trace_launch(pt_ctx* c, int64_t n, const float4* rays, void* out, int32_t mode, hipStream_t s) {
  const bool occ = mode == PT_TRACE_OCCLUDED;
  if (c->bpc_trace[occ] <= 0) HIPCHK(ptk_trace_occupancy(&c->bpc_trace[occ], occ));
  const int grid = trace_grid(n, (int64_t)c->bpc_trace[occ] * c->n_cu, trace_waves_knob(std::getenv("PT_TRACE_WAVES")));
  const DeviceScene& sc = c->scene;
  HIPCHK_ALLOC(c->tr_counts.reserve(3));
  const size_t spill = trace_spill_entries(sc.bvh_stack, PT_STACK, grid);
  if (spill) HIPCHK_ALLOC(c->tr_spill.reserve(spill));
  HIPCHK(c->t_trace.create());
  TraceArgs a;
  std::memset(&a, 0, sizeof(a));
  a.nodes = sc.nodes.p;
  a.prims = sc.prims.p;
  a.norms = sc.norms.p;
  a.prim_map = sc.prim_map.p;
  a.rays = rays;
  a.rec = occ ? nullptr : (float4*)out;
  a.occ = occ ? (uint32_t*)out : nullptr;
  a.counts = c->tr_counts.p;
  a.stack_spill = spill ? c->tr_spill.p : nullptr;
  a.n = n;
  HIPCHK(c->tr_order.begin(s));
  HIPCHK(hipMemsetAsync(c->tr_counts.p, 0, 3 * sizeof(unsigned long long), s));
  HIPCHK(c->t_trace.begin(s));
  HIPCHK(ptk_launch_trace(&a, grid, occ, s));
  HIPCHK(c->t_trace.end(s));
  HIPCHK(c->tr_order.end(s));
  c->tr_counted = true;
  return PT_OK;
}
}  // namespace

int pt_trace_rays_device(pt_ctx* c, int64_t n, const void* rays_dev, void* out_dev, int32_t mode, void* stream) {
  if (int rc = trace_check(c, n, rays_dev, out_dev, mode, "pt_trace_rays_device")) return rc;
  if (n == 0) {
    c->tr_counted = false;
    return PT_OK;
  }
  HIPCHK(hipSetDevice(c->device));
  return trace_launch(c, n, (const float4*)rays_dev, out_dev, mode, stream_of(c, stream));
}

int pt_trace_rays(pt_ctx* c, int64_t n, const void* rays_host, void* out_host, int32_t mode) {
  if (int rc = trace_check(c, n, rays_host, out_host, mode, "pt_trace_rays")) return rc;
  if (n == 0) {
    c->tr_counted = false;
    return PT_OK;
  }
  HIPCHK(hipSetDevice(c->device));
  const size_t out_bytes = trace_out_bytes(n, mode);
  HIPCHK_ALLOC(c->tr_rays.reserve(2 * (size_t)n));
  HIPCHK_ALLOC(c->tr_out.reserve((out_bytes + sizeof(float4) - 1) / sizeof(float4)));
  hipStream_t s = c->stream;
  HIPCHK(hipMemcpyAsync(c->tr_rays.p, rays_host, (size_t)n * PT_TRACE_RAY_BYTES, hipMemcpyHostToDevice, s));
  if (int rc = trace_launch(c, n, c->tr_rays.p, c->tr_out.p, mode, s)) return rc;
  HIPCHK(hipMemcpyAsync(out_host, c->tr_out.p, out_bytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return PT_OK;
}

int pt_camera_rays_device(pt_ctx* c, const pt_tile* tiles, int32_t n_tiles, void* rays_dev, void* stream) {
  if (n_tiles < 0 || !rays_dev || (n_tiles > 0 && !tiles))
    return fail(PT_E_INVALID, "pt_camera_rays_device: bad args (NULL buffer or tiles, n_tiles < 0)");
  if (!c) return fail(PT_E_INVALID, "pt_camera_rays_device: NULL context");
  std::vector<int4> tl;
  hipStream_t s;
  if (int rc = render_begin(c, tiles, n_tiles, nullptr, stream, tl, &s)) return rc;
  if (tl.empty()) return PT_OK;
  // the tile list is the context's: a call on another stream than the last one's waits for it
  HIPCHK(c->cr_order.begin(s));
  HIPCHK(c->cr_tiles.sync(tl.data(), tl.size(), s));
  CamRayArgs a;
  std::memset(&a, 0, sizeof(a));
  set_camera_args(a, c->cam, c->params);
  a.tiles = c->cr_tiles.dev.p;
  a.rays = (float4*)rays_dev;
  HIPCHK(ptk_launch_camera_rays(&a, (int)tl.size(), s));
  HIPCHK(c->cr_order.end(s));
  return PT_OK;
}

int pt_get_trace_info(pt_ctx* c, pt_trace_info* out) {
  if (!c || !out) return fail(PT_E_INVALID, "pt_get_trace_info: NULL argument");
  std::memset(out, 0, sizeof(*out));
  if (!c->tr_counted) return PT_OK;
  HIPCHK(hipSetDevice(c->device));
  float ms = 0.f;
  HIPCHK(c->t_trace.ms(&ms));
  unsigned long long n[3] = {0, 0, 0};
  HIPCHK(hipMemcpy(n, c->tr_counts.p, sizeof(n), hipMemcpyDeviceToHost));
  out->rays = (int64_t)n[0];
  out->hits = (int64_t)n[1];
  out->invalid = (int64_t)n[2];
  out->trace_ms = ms;
  return PT_OK;
}
