// pt_api_rays.cpp — C ABI of the HIP path, fourth part (include/ptgpu.h): path
// tracing along the caller's rays (pt_render_rays*; kernel: pt_kernels.hip
// render_kernel's RAYS builds; the launch itself: pt_api.cpp launch(), which
// every render shares).  The film's pass over rays, pt_film_add_pass_rays, is
// with the film (pt_api_film.cpp).  The context is declared in pt_ctx.h.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "pt_ctx.h"

namespace {
int fail(int code, const std::string& msg) { return pt_fail(code, msg); }

// What both entry points refuse, in ptgpu.h's order: the arguments, then what
// the context lacks, then what only the params can tell.
int rays_check(pt_ctx* c, const pt_tile* tiles, int32_t n_tiles, const void* rays, const void* out, uint32_t flags,
               const char* fn) {
  const std::string f(fn);
  if (!c) return fail(PT_E_INVALID, f + ": NULL context");
  if (!rays || !out || n_tiles < 0 || (n_tiles > 0 && !tiles))
    return fail(PT_E_INVALID, f + ": bad args (NULL ray buffer, output or tiles, n_tiles < 0)");
  if (flags & ~PT_FLAG_RAYS_CAPTURE) return fail(PT_E_INVALID, f + ": flags must be 0 or PT_FLAG_RAYS_CAPTURE");
  const bool capture = (flags & PT_FLAG_RAYS_CAPTURE) != 0;
  if (!c->have_scene || !c->have_params || (capture && !c->have_cam))
    return fail(PT_E_NOSCENE, f + " before pt_upload_scene / pt_set_params" + (capture ? " / pt_set_camera" : ""));
  if (capture && c->params.spp != 1)
    return fail(PT_E_INVALID, f + ": PT_FLAG_RAYS_CAPTURE needs spp 1 (one ray per pixel), the params have " +
                                  std::to_string(c->params.spp));
  {  // (host or device: both entry points take one address space each)
    const size_t px = (size_t)c->params.width * (size_t)c->params.height;
    const uintptr_t r0 = (uintptr_t)rays, r1 = r0 + px * 2 * sizeof(float4);
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + px * 3 * sizeof(float);
    if (r0 < o1 && o0 < r1) return fail(PT_E_INVALID, f + ": the ray buffer overlaps the output");
  }
  return PT_OK;
}

// After the checks: earlier asynchronous tiles first (call order), the device
// set, the tiles clipped to the frame in <= 32x32 pieces.
int rays_begin(pt_ctx* c, const pt_tile* tiles, int32_t n_tiles, std::vector<int4>& tl) {
  if (int rc = tile_launch(c)) return rc;
  HIPCHK(hipSetDevice(c->device));
  return build_tiles(c, tiles, n_tiles, tl);
}
}  // namespace

int pt_render_rays_device(pt_ctx* c, const pt_tile* tiles, int32_t n_tiles, void* rays_dev, float* hdr_out_dev,
                          void* stream, uint32_t flags) {
  if (int rc = rays_check(c, tiles, n_tiles, rays_dev, hdr_out_dev, flags, "pt_render_rays_device")) return rc;
  std::vector<int4> tl;
  if (int rc = rays_begin(c, tiles, n_tiles, tl)) return rc;
  hipStream_t s = stream_of(c, stream);
  const RayLaunch rl{(float4*)rays_dev, (flags & PT_FLAG_RAYS_CAPTURE) != 0};
  if (int rc = launch(c, tl, &hdr_out_dev, 1, nullptr, s, 0, &rl)) return rc;
  return finish_stats(c, s, 0, false);
}

int pt_render_rays(pt_ctx* c, const pt_tile* tiles, int32_t n_tiles, void* rays_host, float* hdr_out_host,
                   uint32_t flags) {
  if (int rc = rays_check(c, tiles, n_tiles, rays_host, hdr_out_host, flags, "pt_render_rays")) return rc;
  std::vector<int4> tl;
  if (int rc = rays_begin(c, tiles, n_tiles, tl)) return rc;
  if (tl.empty()) return PT_OK;
  const bool capture = (flags & PT_FLAG_RAYS_CAPTURE) != 0;
  const size_t W = (size_t)c->params.width, H = (size_t)c->params.height;
  HIPCHK_ALLOC(c->frame.reserve(W * H * 3));
  HIPCHK_ALLOC(c->rr_rays.reserve(W * H * 2));
  hipStream_t s = c->stream;
  // every ray goes to the device (a replay reads those of the tiles' pixels
  // only, a capture overwrites them); only the tiles' pixels and captured rays
  // come back: the caller's buffers are theirs outside the tiles
  HIPCHK(hipMemcpyAsync(c->rr_rays.p, rays_host, W * H * 2 * sizeof(float4), hipMemcpyHostToDevice, s));
  float* fr = c->frame.p;
  const RayLaunch rl{c->rr_rays.p, capture};
  if (int rc = launch(c, tl, &fr, 1, nullptr, s, 0, &rl)) return rc;
  for (const int4& t : tl) {
    const size_t p = (size_t)t.y * W + (size_t)t.x;
    HIPCHK(hipMemcpy2DAsync(hdr_out_host + 3 * p, W * 3 * sizeof(float), c->frame.p + 3 * p, W * 3 * sizeof(float),
                            (size_t)t.z * 3 * sizeof(float), (size_t)t.w, hipMemcpyDeviceToHost, s));
    if (capture)
      HIPCHK(hipMemcpy2DAsync((float4*)rays_host + 2 * p, W * 2 * sizeof(float4), c->rr_rays.p + 2 * p,
                              W * 2 * sizeof(float4), (size_t)t.z * 2 * sizeof(float4), (size_t)t.w,
                              hipMemcpyDeviceToHost, s));
  }
  return finish_stats(c, s, 0, true);
}
