// pt_api_film.cpp — C ABI of the HIP path, second part (include/ptgpu.h): the
// progressive film, the first-hit feature pass, the denoiser and the
// reprojection.  The context and the render path they share with pt_api.cpp
// are declared in pt_ctx.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "denoise.h"
#include "film.h"
#include "pt_ctx.h"
#include "reproject.h"

namespace {
int fail(int code, const std::string& msg) { return pt_fail(code, msg); }
}  // namespace

// ---- progressive film (ptgpu.h: pt_film_*; kernels and record layout: film.hip, film.h)
// The toColor thresholds on the device (once per context; a blocking copy, so
// every kernel queued afterwards sees them).
static int tonemap_table(pt_ctx* c) {
  if (c->tc_thr_ready) return PT_OK;
  uint32_t thr[256];
  if (int rc = pt_to_color_thresholds(thr)) return rc;
  HIPCHK_ALLOC(c->tc_thr.reserve(256));
  HIPCHK(hipMemcpy(c->tc_thr.p, thr, sizeof(thr), hipMemcpyHostToDevice));
  c->tc_thr_ready = true;
  return PT_OK;
}

// True when no two of the non-empty rectangles r = (x0, y0, x1, y1) share a
// pixel.  Sorted by y0, each is compared with those that begin below its last
// row only -- for a grid of tiles its own row -- instead of marking W * H bytes
// (tiles_disjoint) on every pass.
static bool rects_disjoint(std::vector<int4>& r) {
  std::sort(r.begin(), r.end(), [](const int4& a, const int4& b) { return a.y != b.y ? a.y < b.y : a.x < b.x; });
  for (size_t i = 0; i < r.size(); ++i)
    for (size_t j = i + 1; j < r.size() && r[j].y < r[i].w; ++j)
      if (r[j].x < r[i].z && r[i].x < r[j].z) return false;
  return true;
}

int pt_film_create(pt_ctx* c, int32_t width, int32_t height, pt_film** out) {
  if (out) *out = nullptr;
  if (!c || !out) return fail(PT_E_INVALID, "pt_film_create: NULL argument");
  if (int rc = check_frame_dims(width, height, "pt_film_create")) return rc;
  HIPCHK(hipSetDevice(c->device));
  if (int rc = tonemap_table(c)) return rc;
  std::unique_ptr<pt_film> f(new pt_film());
  f->ctx = c;
  f->W = width;
  f->H = height;
  const size_t px = (size_t)width * (size_t)height;
  HIPCHK_ALLOC(f->rec.reserve(2 * px));
  HIPCHK_ALLOC(f->pass.reserve(3 * px));
  HIPCHK(f->t_acc.create());
  HIPCHK(f->t_res.create());
  HIPCHK(hipMemsetAsync(f->rec.p, 0, 2 * px * sizeof(uint4), c->stream));
  HIPCHK(f->order.end(c->stream));
  *out = f.get();
  c->films.push_back(std::move(f));
  return PT_OK;
}

int pt_film_destroy(pt_film* f) {
  if (!f) return PT_OK;
  pt_ctx* c = f->ctx;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();  // no kernel may still use the film's memory
  c->films.erase(std::remove_if(c->films.begin(), c->films.end(), [f](const auto& o) { return o.get() == f; }),
                 c->films.end());
  return PT_OK;
}

int pt_film_clear(pt_film* f, void* stream) {
  if (!f) return fail(PT_E_INVALID, "pt_film_clear: NULL film");
  pt_ctx* c = f->ctx;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = stream_of(c, stream);
  HIPCHK(f->order.begin(s));
  HIPCHK(hipMemsetAsync(f->rec.p, 0, 2 * (size_t)f->W * (size_t)f->H * sizeof(uint4), s));
  f->next = 0;
  f->passes = 0;
  f->have_feat = false;
  HIPCHK(f->order.end(s));
  return PT_OK;
}

int pt_film_set_next_sample(pt_film* f, uint32_t next_sample) {
  if (!f) return fail(PT_E_INVALID, "pt_film_set_next_sample: NULL film");
  f->next = next_sample;
  return PT_OK;
}

// pt_film_add_pass, and with `rays_dev` pt_film_add_pass_rays: the pass rendered
// by replay of the caller's rays (which needs no camera).
static int film_add_pass(pt_film* f, const pt_tile* tiles, int32_t n_tiles, const void* rays_dev, bool by_rays,
                         void* stream) {
  const std::string fn = by_rays ? "pt_film_add_pass_rays" : "pt_film_add_pass";
  if (!f) return fail(PT_E_INVALID, fn + ": NULL film");
  pt_ctx* c = f->ctx;
  int rc = PT_OK;
  if (!by_rays) {
    if ((rc = check_ready(c))) return rc;
  } else if (!c->have_scene || !c->have_params) {
    return fail(PT_E_NOSCENE, "pt_film_add_pass_rays before pt_upload_scene / pt_set_params");
  }
  if (n_tiles < 0 || (n_tiles > 0 && !tiles)) return fail(PT_E_INVALID, fn + ": bad args");
  if (by_rays && !rays_dev) return fail(PT_E_INVALID, fn + ": NULL ray buffer");
  const pt_params& P = c->params;
  if (P.width != f->W || P.height != f->H)
    return fail(PT_E_INVALID, fn + ": pt_params frame " + std::to_string(P.width) + " x " +
                                  std::to_string(P.height) + " differs from the film's " + std::to_string(f->W) + " x " +
                                  std::to_string(f->H));
  if (f->next + (uint64_t)P.spp > (uint64_t)1 << 32)
    return fail(PT_E_INVALID, fn + ": sample range overflow (next sample " + std::to_string(f->next) +
                                  " + spp " + std::to_string(P.spp) + " > 2^32)");
  std::vector<int4> rects;
  for (int32_t i = 0; i < n_tiles; ++i) {
    const pt_tile& t = tiles[i];
    if (t.w < 0 || t.h < 0) return fail(PT_E_INVALID, fn + ": negative tile size");
    const int x0 = std::max(0, t.x), y0 = std::max(0, t.y);
    const int x1 = (int)std::min<int64_t>(f->W, (int64_t)t.x + t.w), y1 = (int)std::min<int64_t>(f->H, (int64_t)t.y + t.h);
    if (x1 > x0 && y1 > y0) rects.push_back(make_int4(x0, y0, x1, y1));
  }
  if (!rects_disjoint(rects))
    return fail(PT_E_INVALID, fn + ": tiles overlap (their samples would be counted twice)");
  if ((rc = tile_launch(c))) return rc;  // earlier asynchronous tiles first (call order)
  HIPCHK(hipSetDevice(c->device));
  // the same <= 32x32 pieces the render resolves (build_tiles of the clipped rectangles)
  std::vector<int4> tl;
  for (const int4& r : rects)
    for (int y = r.y; y < r.w; y += 32)
      for (int x = r.x; x < r.z; x += 32) tl.push_back(make_int4(x, y, std::min(32, r.z - x), std::min(32, r.w - y)));
  hipStream_t s = stream_of(c, stream);
  HIPCHK(f->order.begin(s));
  // the pass: the context's params with the film's sample index, through the
  // render path every other entry point uses; the stored params stay the caller's
  const uint32_t base = c->params.sample_base;
  c->params.sample_base = (uint32_t)f->next;
  float* pass = f->pass.p;
  const RayLaunch rl{(float4*)const_cast<void*>(rays_dev), false};
  rc = launch(c, tl, &pass, 1, nullptr, s, 0, by_rays ? &rl : nullptr);
  c->params.sample_base = base;
  if (rc) return rc;
  if ((rc = finish_stats(c, s, 0, false))) return rc;
  if (!tl.empty()) {
    HIPCHK_ALLOC(f->tiles.sync(tl.data(), tl.size(), s));
    FilmAccArgs a;
    a.tiles = f->tiles.dev.p;
    a.rec = f->rec.p;
    a.pass = f->pass.p;
    a.W = f->W;
    a.H = f->H;
    a.spp = (uint32_t)P.spp;
    HIPCHK(f->t_acc.begin(s));
    HIPCHK(ptk_film_accumulate(&a, (int)tl.size(), s));
    HIPCHK(f->t_acc.end(s));
  }
  f->next += (uint64_t)P.spp;
  ++f->passes;
  HIPCHK(f->order.end(s));
  return PT_OK;
}

int pt_film_add_pass(pt_film* f, const pt_tile* tiles, int32_t n_tiles, void* stream) {
  return film_add_pass(f, tiles, n_tiles, nullptr, false, stream);
}

int pt_film_add_pass_rays(pt_film* f, const pt_tile* tiles, int32_t n_tiles, const void* rays_dev, void* stream) {
  return film_add_pass(f, tiles, n_tiles, rays_dev, true, stream);
}

int pt_film_resolve_device(pt_film* f, float* hdr_dev, uint32_t* rgba_dev, float* err_dev, void* stream) {
  if (!f) return fail(PT_E_INVALID, "pt_film_resolve_device: NULL film");
  if (!hdr_dev && !rgba_dev && !err_dev) return PT_OK;
  pt_ctx* c = f->ctx;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = stream_of(c, stream);
  HIPCHK(f->order.begin(s));
  FilmResolveArgs a;
  a.rec = f->rec.p;
  a.thr = c->tc_thr.p;
  a.hdr = hdr_dev;
  a.rgba = rgba_dev;
  a.err = err_dev;
  a.W = f->W;
  a.H = f->H;
  HIPCHK(f->t_res.begin(s));
  HIPCHK(ptk_film_resolve(&a, s));
  HIPCHK(f->t_res.end(s));
  HIPCHK(f->order.end(s));
  return PT_OK;
}

int pt_film_resolve(pt_film* f, float* hdr_host, uint32_t* rgba_host, float* err_host) {
  if (!f) return fail(PT_E_INVALID, "pt_film_resolve: NULL film");
  pt_ctx* c = f->ctx;
  HIPCHK(hipSetDevice(c->device));
  const size_t px = (size_t)f->W * (size_t)f->H;
  if (hdr_host) HIPCHK_ALLOC(f->out_hdr.reserve(3 * px));
  if (rgba_host) HIPCHK_ALLOC(f->out_rgba.reserve(px));
  if (err_host) HIPCHK_ALLOC(f->out_err.reserve(px));
  if (int rc = pt_film_resolve_device(f, hdr_host ? f->out_hdr.p : nullptr, rgba_host ? f->out_rgba.p : nullptr,
                                      err_host ? f->out_err.p : nullptr, nullptr))
    return rc;
  hipStream_t s = c->stream;
  if (hdr_host) HIPCHK(hipMemcpyAsync(hdr_host, f->out_hdr.p, 3 * px * sizeof(float), hipMemcpyDeviceToHost, s));
  if (rgba_host) HIPCHK(hipMemcpyAsync(rgba_host, f->out_rgba.p, px * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  if (err_host) HIPCHK(hipMemcpyAsync(err_host, f->out_err.p, px * sizeof(float), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return PT_OK;
}

int pt_film_tile_error(pt_film* f, const pt_tile* tiles, int32_t n_tiles, float* err_host) {
  if (!f) return fail(PT_E_INVALID, "pt_film_tile_error: NULL film");
  if (n_tiles < 0 || (n_tiles > 0 && (!tiles || !err_host))) return fail(PT_E_INVALID, "pt_film_tile_error: bad args");
  if (n_tiles == 0) return PT_OK;
  std::vector<int4> tl((size_t)n_tiles);
  for (int32_t i = 0; i < n_tiles; ++i) {
    const pt_tile& t = tiles[i];
    if (t.w < 0 || t.h < 0) return fail(PT_E_INVALID, "pt_film_tile_error: negative tile size");
    const int x0 = std::max(0, t.x), y0 = std::max(0, t.y);
    const int x1 = (int)std::min<int64_t>(f->W, (int64_t)t.x + t.w), y1 = (int)std::min<int64_t>(f->H, (int64_t)t.y + t.h);
    tl[i] = x1 > x0 && y1 > y0 ? make_int4(x0, y0, x1 - x0, y1 - y0) : make_int4(0, 0, 0, 0);
  }
  pt_ctx* c = f->ctx;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK_ALLOC(f->etiles.reserve(tl.size()));
  HIPCHK_ALLOC(f->emax.reserve(tl.size()));
  hipStream_t s = c->stream;
  HIPCHK(f->order.begin(s));
  HIPCHK(hipMemcpyAsync(f->etiles.p, tl.data(), tl.size() * sizeof(int4), hipMemcpyHostToDevice, s));
  FilmErrArgs a;
  a.tiles = f->etiles.p;
  a.rec = f->rec.p;
  a.out = f->emax.p;
  a.W = f->W;
  a.H = f->H;
  HIPCHK(ptk_film_tile_error(&a, n_tiles, s));
  HIPCHK(hipMemcpyAsync(err_host, f->emax.p, tl.size() * sizeof(float), hipMemcpyDeviceToHost, s));
  HIPCHK(f->order.end(s));
  HIPCHK(hipStreamSynchronize(s));
  return PT_OK;
}

int pt_film_get_info(pt_film* f, pt_film_info* out) {
  if (!f || !out) return fail(PT_E_INVALID, "pt_film_get_info: NULL argument");
  std::memset(out, 0, sizeof(*out));
  out->width = f->W;
  out->height = f->H;
  out->passes = f->passes;
  out->next_sample = f->next;
  float acc_ms = 0.f, res_ms = 0.f;
  HIPCHK(f->t_acc.ms(&acc_ms));
  out->accumulate_ms = acc_ms;
  HIPCHK(f->t_res.ms(&res_ms));
  out->resolve_ms = res_ms;
  return PT_OK;
}

// ---- the film's records out and in (ptgpu.h: pt_film_export*, pt_film_merge*; kernel: film.hip film_merge_kernel)
static size_t film_rec_bytes(const pt_film* f) { return 2 * (size_t)f->W * (size_t)f->H * sizeof(uint4); }

// True when the 2*W*H records at `p` share a byte with the film's own.
static bool overlaps_film(const pt_film* f, const void* p) {
  const uintptr_t a0 = (uintptr_t)f->rec.p, b0 = (uintptr_t)p, len = film_rec_bytes(f);
  return a0 < b0 + len && b0 < a0 + len;
}

int pt_film_export_device(pt_film* f, void* rec_out_dev, void* stream) {
  if (!f || !rec_out_dev) return fail(PT_E_INVALID, "pt_film_export_device: NULL argument");
  if (overlaps_film(f, rec_out_dev))
    return fail(PT_E_INVALID, "pt_film_export_device: the output overlaps the film's own records");
  pt_ctx* c = f->ctx;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = stream_of(c, stream);
  HIPCHK(f->order.begin(s));
  HIPCHK(hipMemcpyAsync(rec_out_dev, f->rec.p, film_rec_bytes(f), hipMemcpyDeviceToDevice, s));
  HIPCHK(f->order.end(s));
  return PT_OK;
}

int pt_film_export(pt_film* f, void* rec_out_host) {
  if (!f || !rec_out_host) return fail(PT_E_INVALID, "pt_film_export: NULL argument");
  pt_ctx* c = f->ctx;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  HIPCHK(f->order.begin(s));
  HIPCHK(hipMemcpyAsync(rec_out_host, f->rec.p, film_rec_bytes(f), hipMemcpyDeviceToHost, s));
  HIPCHK(f->order.end(s));
  HIPCHK(hipStreamSynchronize(s));
  return PT_OK;
}

int pt_film_merge_device(pt_film* f, const void* rec_dev, void* stream) {
  if (!f || !rec_dev) return fail(PT_E_INVALID, "pt_film_merge_device: NULL argument");
  if (overlaps_film(f, rec_dev))
    return fail(PT_E_INVALID, "pt_film_merge_device: the incoming records overlap the film's own");
  pt_ctx* c = f->ctx;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK_ALLOC(f->mg_counts.reserve(4));
  HIPCHK(f->t_mg.create());
  hipStream_t s = stream_of(c, stream);
  HIPCHK(f->order.begin(s));
  FilmMergeArgs a;
  a.rec = f->rec.p;
  a.in = (const uint4*)rec_dev;
  a.counts = f->mg_counts.p;
  a.W = f->W;
  a.H = f->H;
  HIPCHK(hipMemsetAsync(f->mg_counts.p, 0, 4 * sizeof(unsigned long long), s));
  HIPCHK(f->t_mg.begin(s));
  HIPCHK(ptk_film_merge(&a, s));
  HIPCHK(f->t_mg.end(s));
  HIPCHK(f->order.end(s));
  return PT_OK;
}

int pt_film_merge(pt_film* f, const void* rec_host) {
  if (!f || !rec_host) return fail(PT_E_INVALID, "pt_film_merge: NULL argument");
  pt_ctx* c = f->ctx;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK_ALLOC(f->mg_stage.reserve(2 * (size_t)f->W * (size_t)f->H));
  hipStream_t s = c->stream;
  // (the staging buffer is free: the merge that last read it was waited for below)
  HIPCHK(hipMemcpyAsync(f->mg_stage.p, rec_host, film_rec_bytes(f), hipMemcpyHostToDevice, s));
  if (int rc = pt_film_merge_device(f, f->mg_stage.p, nullptr)) return rc;
  HIPCHK(hipStreamSynchronize(s));
  return PT_OK;
}

int pt_film_get_merge_info(pt_film* f, pt_film_merge_info* out) {
  if (!f || !out) return fail(PT_E_INVALID, "pt_film_get_merge_info: NULL argument");
  std::memset(out, 0, sizeof(*out));
  if (!f->t_mg.timed) return PT_OK;
  HIPCHK(hipSetDevice(f->ctx->device));
  float ms = 0.f;
  HIPCHK(f->t_mg.ms(&ms));
  unsigned long long n[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpy(n, f->mg_counts.p, sizeof(n), hipMemcpyDeviceToHost));
  out->merged = (int64_t)n[0];
  out->taken = (int64_t)n[1];
  out->empty = (int64_t)n[2];
  out->refused = (int64_t)n[3];
  out->merge_ms = ms;
  return PT_OK;
}

int pt_debug_film_records(pt_film* f, void** rec_dev) {
  if (!f || !rec_dev) return fail(PT_E_INVALID, "pt_debug_film_records: NULL argument");
  *rec_dev = f->rec.p;
  return PT_OK;
}

int pt_to_color_device(pt_ctx* c, const float* hdr_dev, int32_t width, int32_t height, int32_t x0, int32_t y0,
                       int32_t x1, int32_t y1, uint32_t* rgba_dev, void* stream) {
  if (!c || !hdr_dev || !rgba_dev || width < 0 || height < 0) return fail(PT_E_INVALID, "pt_to_color_device: bad args");
  ToColorArgs a;
  a.x0 = std::max(0, x0);
  a.y0 = std::max(0, y0);
  a.x1 = std::min(width, x1);
  a.y1 = std::min(height, y1);
  if (a.x1 <= a.x0 || a.y1 <= a.y0) return PT_OK;
  HIPCHK(hipSetDevice(c->device));
  if (int rc = tonemap_table(c)) return rc;
  a.hdr = hdr_dev;
  a.thr = c->tc_thr.p;
  a.rgba = rgba_dev;
  a.W = width;
  HIPCHK(ptk_to_color(&a, stream_of(c, stream)));
  return PT_OK;
}

// ---- first-hit feature buffers (ptgpu.h: pt_render_features*; kernel: pt_kernels.hip features_kernel)
static int features_launch(pt_ctx* c, const std::vector<int4>& tl, float4* feat, hipStream_t s) {
  if (tl.empty()) return PT_OK;
  // the tile list and the spill area are the context's: a pass on another
  // stream than the last one's waits for it
  HIPCHK(c->feat_order.begin(s));
  HIPCHK(c->ftiles.sync(tl.data(), tl.size(), s));
  const DeviceScene& sc = c->scene;
  FeatArgs A;
  std::memset(&A, 0, sizeof(A));
  set_camera_args(A, c->cam, c->params);
  A.nodes = sc.nodes.p;
  A.prims = sc.prims.p;
  A.norms = sc.norms.p;
  A.tiles = c->ftiles.dev.p;
  A.feat = feat;
  if (sc.bvh_stack > PT_STACK) {
    HIPCHK(c->f_spill.reserve((size_t)(sc.bvh_stack - PT_STACK) * tl.size() * 16 * PT_BLOCK));
    A.stack_spill = c->f_spill.p;
  }
  HIPCHK(ptk_launch_features(&A, (int)tl.size(), s));
  HIPCHK(c->feat_order.end(s));
  return PT_OK;
}

int pt_render_features_device(pt_ctx* c, const pt_tile* tiles, int32_t n_tiles, void* feat_dev, void* stream) {
  const bool bad = n_tiles < 0 || (n_tiles > 0 && (!tiles || !feat_dev));
  std::vector<int4> tl;
  hipStream_t s;
  if (int rc = render_begin(c, tiles, n_tiles, bad ? "pt_render_features_device: bad args" : nullptr, stream, tl, &s))
    return rc;
  return features_launch(c, tl, (float4*)feat_dev, s);
}

int pt_render_features(pt_ctx* c, const pt_tile* tiles, int32_t n_tiles, void* feat_host) {
  const bool bad = n_tiles < 0 || (n_tiles > 0 && (!tiles || !feat_host));
  std::vector<int4> tl;
  hipStream_t s;  // (the context's)
  int rc = render_begin(c, tiles, n_tiles, bad ? "pt_render_features: bad args" : nullptr, nullptr, tl, &s);
  if (rc) return rc;
  const size_t W = (size_t)c->params.width, H = (size_t)c->params.height;
  HIPCHK(c->feat_out.reserve(2 * W * H));
  if ((rc = features_launch(c, tl, c->feat_out.p, s))) return rc;
  // only the tiles' records go back: the caller's buffer is theirs outside them
  for (const int4& t : tl)
    for (size_t plane = 0; plane < 2; ++plane) {
      const size_t off = plane * W * H + (size_t)t.y * W + (size_t)t.x;
      HIPCHK(hipMemcpy2DAsync((float4*)feat_host + off, W * sizeof(float4), c->feat_out.p + off, W * sizeof(float4),
                              (size_t)t.z * sizeof(float4), (size_t)t.w, hipMemcpyDeviceToHost, s));
    }
  HIPCHK(hipStreamSynchronize(s));
  return PT_OK;
}

// ---- the denoiser (ptgpu.h: pt_denoise_*, pt_film_denoise*; kernels: denoise.hip)
int pt_denoise_params_default(pt_denoise_params* out) {
  if (!out) return fail(PT_E_INVALID, "pt_denoise_params_default: out is NULL");
  out->iterations = 5;
  out->normal_squarings = 7;
  out->sigma_l = 4.0f;
  out->sigma_p = PT_DENOISE_SIGMA_P;
  return PT_OK;
}

// The parameters a call runs with: the defaults for NULL, else the caller's, checked.
static int denoise_params(const pt_denoise_params* in, pt_denoise_params* out, const char* fn) {
  if (!in) return pt_denoise_params_default(out);
  if (in->iterations < 1 || in->iterations > 6)
    return fail(PT_E_INVALID, std::string(fn) + ": iterations must be 1 .. 6");
  if (in->normal_squarings < 0 || in->normal_squarings > 10)
    return fail(PT_E_INVALID, std::string(fn) + ": normal_squarings must be 0 .. 10");
  if (!(in->sigma_l > 0.0f) || !(in->sigma_p > 0.0f))
    return fail(PT_E_INVALID, std::string(fn) + ": sigma_l and sigma_p must be > 0");
  *out = *in;
  return PT_OK;
}

// The iterations: `in` -> s0 -> s1 -> s0 ... with the last one into `out`.
static int denoise_chain(const float4* in, const float4* feat, int W, int H, const pt_denoise_params& prm, float4* s0,
                         float4* s1, float4* out, hipStream_t s) {
  DenoiseIterArgs a;
  a.feat = feat;
  a.W = W;
  a.H = H;
  a.normal_squarings = prm.normal_squarings;
  a.sigma_l = prm.sigma_l;
  a.sigma_p = prm.sigma_p;
  const float4* src = in;
  for (int i = 0; i < prm.iterations; ++i) {
    a.in = src;
    a.out = i == prm.iterations - 1 ? out : (i & 1) ? s1 : s0;
    a.step = 1 << i;
    HIPCHK(ptk_denoise_iteration(&a, s));
    src = a.out;
  }
  return PT_OK;
}

int pt_denoise_device(pt_ctx* c, const float* cv_dev, const void* feat_dev, int32_t width, int32_t height,
                      const pt_denoise_params* params, float* out_cv_dev, void* stream) {
  pt_denoise_params prm;
  if (int rc = denoise_params(params, &prm, "pt_denoise_device")) return rc;
  if (!c || !cv_dev || !feat_dev || !out_cv_dev) return fail(PT_E_INVALID, "pt_denoise_device: NULL argument");
  if (int rc = check_frame_dims(width, height, "pt_denoise_device")) return rc;
  const size_t px = (size_t)width * (size_t)height;
  const uintptr_t a0 = (uintptr_t)cv_dev, b0 = (uintptr_t)out_cv_dev, len = px * sizeof(float4);
  if (a0 < b0 + len && b0 < a0 + len) return fail(PT_E_INVALID, "pt_denoise_device: input and output overlap");
  HIPCHK(hipSetDevice(c->device));
  if (prm.iterations > 1) HIPCHK_ALLOC(c->dn_a.reserve(px));
  if (prm.iterations > 2) HIPCHK_ALLOC(c->dn_b.reserve(px));
  return denoise_chain((const float4*)cv_dev, (const float4*)feat_dev, width, height, prm, c->dn_a.p, c->dn_b.p,
                       (float4*)out_cv_dev, stream_of(c, stream));
}

static int film_frame_check(const pt_film* f, const char* fn) {
  const pt_params& P = f->ctx->params;
  if (P.width != f->W || P.height != f->H)
    return fail(PT_E_INVALID, std::string(fn) + ": pt_params frame " + std::to_string(P.width) + " x " +
                                  std::to_string(P.height) + " differs from the film's " + std::to_string(f->W) + " x " +
                                  std::to_string(f->H));
  return PT_OK;
}

int pt_film_set_features(pt_film* f, const pt_tile* tiles, int32_t n_tiles, void* stream) {
  if (!f) return fail(PT_E_INVALID, "pt_film_set_features: NULL film");
  pt_ctx* c = f->ctx;
  int rc = check_ready(c);
  if (rc) return rc;
  if (n_tiles < 0 || (n_tiles > 0 && !tiles)) return fail(PT_E_INVALID, "pt_film_set_features: bad args");
  if ((rc = film_frame_check(f, "pt_film_set_features"))) return rc;
  if ((rc = tile_launch(c))) return rc;
  HIPCHK(hipSetDevice(c->device));
  std::vector<int4> tl;
  if ((rc = build_tiles(c, tiles, n_tiles, tl))) return rc;
  HIPCHK_ALLOC(f->feat.reserve(2 * (size_t)f->W * (size_t)f->H));
  hipStream_t s = stream_of(c, stream);
  HIPCHK(f->order.begin(s));
  if (!f->have_feat) HIPCHK(ptk_features_clear(f->feat.p, f->W, f->H, s));  // a pixel never covered: the miss record
  if ((rc = features_launch(c, tl, f->feat.p, s))) return rc;
  f->have_feat = true;
  f->feat_cam = c->cam;
  HIPCHK(f->order.end(s));
  return PT_OK;
}

int pt_film_denoise_device(pt_film* f, const pt_denoise_params* params, float* hdr_dev, uint32_t* rgba_dev,
                           void* stream) {
  if (!f) return fail(PT_E_INVALID, "pt_film_denoise_device: NULL film");
  pt_denoise_params prm;
  if (int rc = denoise_params(params, &prm, "pt_film_denoise_device")) return rc;
  if (!f->have_feat)
    return fail(PT_E_INVALID, "pt_film_denoise_device: no features (pt_film_set_features after creation / pt_film_clear)");
  if (int rc = film_frame_check(f, "pt_film_denoise_device")) return rc;
  if (!hdr_dev && !rgba_dev) return PT_OK;
  pt_ctx* c = f->ctx;
  HIPCHK(hipSetDevice(c->device));
  const size_t px = (size_t)f->W * (size_t)f->H;
  HIPCHK_ALLOC(f->cv[0].reserve(px));
  HIPCHK_ALLOC(f->cv[1].reserve(px));
  hipStream_t s = stream_of(c, stream);
  HIPCHK(f->order.begin(s));
  DenoisePrepareArgs pa;
  pa.rec = f->rec.p;
  pa.cv = f->cv[0].p;
  pa.W = f->W;
  pa.H = f->H;
  HIPCHK(ptk_denoise_prepare(&pa, s));
  // cv[0] -> cv[1] -> cv[0] ...: the result is in cv[iterations & 1]
  float4* res = f->cv[prm.iterations & 1].p;
  if (int rc = denoise_chain(f->cv[0].p, f->feat.p, f->W, f->H, prm, f->cv[1].p, f->cv[0].p, res, s)) return rc;
  DenoiseFinishArgs fa;
  fa.cv = res;
  fa.thr = c->tc_thr.p;
  fa.hdr = hdr_dev;
  fa.rgba = rgba_dev;
  fa.W = f->W;
  fa.H = f->H;
  HIPCHK(ptk_denoise_finish(&fa, s));
  HIPCHK(f->order.end(s));
  return PT_OK;
}

int pt_film_denoise(pt_film* f, const pt_denoise_params* params, float* hdr_host, uint32_t* rgba_host) {
  if (!f) return fail(PT_E_INVALID, "pt_film_denoise: NULL film");
  pt_ctx* c = f->ctx;
  HIPCHK(hipSetDevice(c->device));
  const size_t px = (size_t)f->W * (size_t)f->H;
  if (hdr_host) HIPCHK_ALLOC(f->out_hdr.reserve(3 * px));
  if (rgba_host) HIPCHK_ALLOC(f->out_rgba.reserve(px));
  if (int rc = pt_film_denoise_device(f, params, hdr_host ? f->out_hdr.p : nullptr,
                                      rgba_host ? f->out_rgba.p : nullptr, nullptr))
    return rc;
  hipStream_t s = c->stream;
  if (hdr_host) HIPCHK(hipMemcpyAsync(hdr_host, f->out_hdr.p, 3 * px * sizeof(float), hipMemcpyDeviceToHost, s));
  if (rgba_host) HIPCHK(hipMemcpyAsync(rgba_host, f->out_rgba.p, px * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  return PT_OK;
}

// ---- reprojection (ptgpu.h: pt_reproject_*, pt_film_reproject; kernel: reproject.hip; host parts: reproject_host.cpp)
int pt_reproject_params_default(pt_reproject_params* out) {
  if (!out) return fail(PT_E_INVALID, "pt_reproject_params_default: out is NULL");
  reproject_params_default(out);
  return PT_OK;
}

// The parameters a call runs with: the defaults for NULL, else the caller's, checked.
static int reproject_params(const pt_reproject_params* in, pt_reproject_params* out, const char* fn) {
  if (!in) return pt_reproject_params_default(out);
  if (const char* what = reproject_params_error(*in)) return fail(PT_E_INVALID, std::string(fn) + ": " + what);
  *out = *in;
  return PT_OK;
}

static int reproject_camera_check(const pt_camera& cam, const char* fn) {
  if (!reproject_orthonormal(cam))
    return fail(PT_E_INVALID, std::string(fn) + ": the old camera's c2w is not orthonormal within 1e-9 (the projection "
                                                "into it takes coordinates by dot products with its columns)");
  return PT_OK;
}

// The gather of one frame on `s`: the keep table of `types` (uploaded when it
// changed), the counts zeroed when wanted, the kernel, timed by `span` when
// given.
static int reproject_launch(pt_ctx* c, const pt_camera& old_cam, const uint4* rec, const float4* fo, const float4* fn,
                            int W, int H, const int32_t* types, int n_types, const pt_reproject_params& prm, uint4* out,
                            unsigned long long* counts, TimedSpan* span, hipStream_t s) {
  std::vector<uint32_t> keep((size_t)n_types);
  reproject_keep_table(types, n_types, keep.data());
  HIPCHK(c->rp_order.begin(s));
  HIPCHK(c->rp_keep.sync(keep.data(), keep.size(), s));
  ReprojectArgs a;
  std::memset(&a, 0, sizeof(a));
  a.rec = rec;
  a.fo = fo;
  a.fn = fn;
  a.keep = c->rp_keep.dev.p;
  a.out = out;
  a.counts = counts;
  a.W = W;
  a.H = H;
  a.n_bsdfs = n_types;
  reproject_camera(old_cam, &a.cam);
  a.normal_cos_min = prm.normal_cos_min;
  a.sigma_p = prm.sigma_p;
  a.max_samples = prm.max_samples;
  if (counts) HIPCHK(hipMemsetAsync(counts, 0, 2 * sizeof(unsigned long long), s));
  if (span) HIPCHK(span->begin(s));
  HIPCHK(ptk_reproject(&a, s));
  if (span) HIPCHK(span->end(s));
  HIPCHK(c->rp_order.end(s));
  return PT_OK;
}

int pt_reproject_device(pt_ctx* c, const pt_camera* old_cam, const void* rec_dev, const void* feat_old_dev,
                        const void* feat_new_dev, int32_t width, int32_t height, const int32_t* bsdf_types_host,
                        int32_t n_bsdfs, const pt_reproject_params* params, void* rec_out_dev, uint64_t* counts_dev,
                        void* stream) {
  // what needs no context first
  pt_reproject_params prm;
  if (int rc = reproject_params(params, &prm, "pt_reproject_device")) return rc;
  if (!old_cam || !rec_dev || !feat_old_dev || !feat_new_dev || !rec_out_dev)
    return fail(PT_E_INVALID, "pt_reproject_device: NULL argument");
  if (int rc = check_frame_dims(width, height, "pt_reproject_device")) return rc;
  const size_t px = (size_t)width * (size_t)height;
  const uintptr_t a0 = (uintptr_t)rec_dev, b0 = (uintptr_t)rec_out_dev, len = 2 * px * sizeof(uint4);
  if (a0 < b0 + len && b0 < a0 + len)
    return fail(PT_E_INVALID, "pt_reproject_device: input and output records overlap (the gather reads any pixel)");
  if (int rc = reproject_camera_check(*old_cam, "pt_reproject_device")) return rc;
  if (bsdf_types_host && n_bsdfs < 0) return fail(PT_E_INVALID, "pt_reproject_device: negative n_bsdfs");
  if (!c) return fail(PT_E_INVALID, "pt_reproject_device: NULL context");
  if (!bsdf_types_host) {
    if (!c->have_scene) return fail(PT_E_NOSCENE, "pt_reproject_device: no BSDF types given and no scene uploaded");
    bsdf_types_host = c->scene.bsdf_types.data();
    n_bsdfs = (int32_t)c->scene.bsdf_types.size();
  }
  HIPCHK(hipSetDevice(c->device));
  return reproject_launch(c, *old_cam, (const uint4*)rec_dev, (const float4*)feat_old_dev, (const float4*)feat_new_dev,
                          width, height, bsdf_types_host, n_bsdfs, prm, (uint4*)rec_out_dev,
                          (unsigned long long*)counts_dev, nullptr, stream_of(c, stream));
}

int pt_film_reproject(pt_film* f, const pt_reproject_params* params, void* stream) {
  if (!f) return fail(PT_E_INVALID, "pt_film_reproject: NULL film");
  pt_reproject_params prm;
  int rc = reproject_params(params, &prm, "pt_film_reproject");
  if (rc) return rc;
  if (!f->have_feat)
    return fail(PT_E_INVALID, "pt_film_reproject: no features (pt_film_set_features after creation / pt_film_clear)");
  pt_ctx* c = f->ctx;
  if ((rc = check_ready(c))) return rc;
  if ((rc = film_frame_check(f, "pt_film_reproject"))) return rc;
  if ((rc = reproject_camera_check(f->feat_cam, "pt_film_reproject"))) return rc;
  if ((rc = tile_launch(c))) return rc;
  HIPCHK(hipSetDevice(c->device));
  const pt_tile whole = {0, 0, f->W, f->H};
  std::vector<int4> tl;
  if ((rc = build_tiles(c, &whole, 1, tl))) return rc;
  const size_t px = (size_t)f->W * (size_t)f->H;
  HIPCHK_ALLOC(f->rec2.reserve(2 * px));
  HIPCHK_ALLOC(f->feat2.reserve(2 * px));
  HIPCHK_ALLOC(f->rp_counts.reserve(2));
  HIPCHK(f->t_rp.create());
  hipStream_t s = stream_of(c, stream);
  HIPCHK(f->order.begin(s));
  if ((rc = features_launch(c, tl, f->feat2.p, s))) return rc;  // (the whole frame: every record is written)
  if ((rc = reproject_launch(c, f->feat_cam, f->rec.p, f->feat.p, f->feat2.p, f->W, f->H, c->scene.bsdf_types.data(),
                             (int)c->scene.bsdf_types.size(), prm, f->rec2.p, f->rp_counts.p, &f->t_rp, s)))
    return rc;
  std::swap(f->rec, f->rec2);
  std::swap(f->feat, f->feat2);
  f->feat_cam = c->cam;
  HIPCHK(f->order.end(s));
  return PT_OK;
}

int pt_film_get_reproject_info(pt_film* f, pt_reproject_info* out) {
  if (!f || !out) return fail(PT_E_INVALID, "pt_film_get_reproject_info: NULL argument");
  std::memset(out, 0, sizeof(*out));
  if (!f->t_rp.timed) return PT_OK;
  HIPCHK(hipSetDevice(f->ctx->device));
  float ms = 0.f;
  HIPCHK(f->t_rp.ms(&ms));
  unsigned long long n[2] = {0, 0};
  HIPCHK(hipMemcpy(n, f->rp_counts.p, sizeof(n), hipMemcpyDeviceToHost));
  out->kept = (int64_t)n[0];
  out->reset = (int64_t)n[1];
  out->reproject_ms = ms;
  return PT_OK;
}
