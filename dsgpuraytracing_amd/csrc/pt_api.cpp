// pt_api.cpp — C ABI of the HIP path (include/ptgpu.h): device context, scene
// upload (reference BVH -> 64-B two-child-box nodes, primitives -> 48-B float
// records), tile rendering, batched ray queries, counters.  (The film, the
// feature pass, the denoiser and the reprojection: pt_api_film.cpp; the context
// itself: pt_ctx.h.)
//
// Replaces CUDAPathTracer (cuda_src/setup.h:90-148, setup.cu:92-843): instead of
// one cudaMalloc+cudaMemcpy per BVH node (setup.cu:429-476), constant-memory
// tables capped at 20 entries (kernel.cu:3-20) and exit() on error, the scene is
// flattened on the host into four contiguous arrays, uploaded once, and every
// failure is returned as a PT_E_* code with a message in pt_last_error().
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ptgpu_scene.h"
#include "pt_ctx.h"
#include "scene_flatten.h"

namespace {

int fail(int code, const std::string& msg) { return pt_fail(code, msg); }

// reserve + blocking copy of a flattened array
template <class T>
int put(DevBuf<T>& dev, const std::vector<T>& v) {
  HIPCHK(dev.reserve(v.size()));
  HIPCHK(hipMemcpy(dev.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return PT_OK;
}

}  // namespace

// The frame sizes the kernels' 16-bit pixel coordinates and 32-bit pixel indices hold.
int check_frame_dims(int64_t width, int64_t height, const char* fn) {
  if (width < 1 || height < 1 || width > 65535 || height > 65535 || width * height > (int64_t)1 << 30)
    return fail(PT_E_INVALID, std::string(fn) + ": width and height must be 1 .. 65535 and width * height <= 2^30");
  return PT_OK;
}

int pt_create(int device, pt_ctx** out) {
  if (!out) return fail(PT_E_INVALID, "pt_create: out is NULL");
  *out = nullptr;
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(PT_E_INVALID, "pt_create: no such HIP device");
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<pt_ctx> c(new pt_ctx(device));  // (a failure below frees what was acquired so far)
  HIPCHK(c->stream.create(hipStreamNonBlocking));
  for (int k = 0; k < pt_ctx::kSlots; ++k) {
    // (slots past the first two get their stream when a small launch first
    // uses them: HIP maps streams onto GPU_MAX_HW_QUEUES hardware queues, 4 by
    // default, and two more streams per context put the render streams of
    // large frames on shared queues -- C3 pipelined -12%)
    if (k < pt_ctx::kSlotsLarge) HIPCHK(c->slots[k].open(c->stream));
    HIPCHK(c->slots[k].counter.reserve(PT_QUEUE_WORDS * PT_QUEUE_HEADS));
  }
  for (auto& tri : c->ev)
    for (auto& e : tri) HIPCHK(e.create());
  HIPCHK(c->stats.reserve(PT_STATS_SLOTS));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  // Persistent grid: as many one-wave workgroups as can be resident.  The
  // work queue needs no co-residency (no grid barrier), so a wrong occupancy
  // answer only costs speed; never size below 8 waves per CU.
  c->n_cu = prop.multiProcessorCount;
  HIPCHK(ptk_render_occupancy(&c->bpc_plain, false, false, false));
  HIPCHK(ptk_render_occupancy(&c->bpc_stats, true, false, false));
  for (int v = 0; v < 4; ++v) HIPCHK(ptk_render_occupancy(&c->bpc_variant[v], false, (v & 2) != 0, (v & 1) != 0));
  c->grid_plain = std::max(8, c->bpc_plain) * c->n_cu;
  c->grid_stats = std::max(8, c->bpc_stats) * c->n_cu;
  // counters + one trace record per wave of the largest stats grid
  HIPCHK(c->stats.reserve(PT_STATS_SLOTS + (size_t)PT_WAVE_TRACE * std::max(c->grid_stats, 64 * c->n_cu)));
  *out = c.release();
  return PT_OK;
}

int pt_destroy(pt_ctx* c) {
  if (!c) return PT_OK;
  delete c;
  return PT_OK;
}

// GPU linear-BVH build over the primitives already in sc.prims / sc.norms
// (CUDAPathTracer::buildBVH, cuda_src/setup.cu:478-686; kernels in lbvh.hip).
static int build_gpu_bvh(DeviceScene& sc, const FlatScene& f, hipStream_t s) {
  LbvhIn in{};
  in.n = (int)f.prims.size();
  in.prims = sc.prims.p;
  in.norms = sc.norms.p;
  std::copy(f.scene_min, f.scene_min + 3, in.scene_min);
  std::copy(f.scene_extent, f.scene_extent + 3, in.scene_extent);
  LbvhOut out{};
  HIPCHK(ptk_build_lbvh(&in, &out, s));
  sc.prims.adopt(out.prims, (size_t)in.n);
  sc.norms.adopt(out.norms, (size_t)in.n * 9);
  sc.prim_map.adopt(out.prim_map, (size_t)in.n);
  sc.nodes.adopt(out.nodes4, (size_t)out.n4);
  sc.nodes2.adopt(out.nodes2, (size_t)std::max(1, out.n2));
  sc.n_nodes2 = (size_t)out.n2;
  sc.n_render_nodes = (size_t)out.n4;
  if (out.max_stack > PT_STACK_MAX) return fail_stack_depth("pt_upload_scene_lbvh", out.max_stack);
  sc.bvh_stack = out.max_stack;
  sc.set_root(out.root_lo, out.root_hi, out.root_lo, out.root_hi);
  return PT_OK;
}

// Validate, flatten (scene_flatten.cpp), reserve, memcpy.
static int upload_impl(pt_ctx* c, const pt_scene* s, bool gpu_bvh) {
  if (!c || !s) return fail(PT_E_INVALID, "pt_upload_scene: NULL argument");
  if (int rc = tile_launch(c)) return rc;  // queued tiles render with the state they were submitted under
  if (s->n_prims <= 0 || !s->prim_type || !s->prim_bsdf || !s->prim_geom || !s->prim_norm ||
      (!gpu_bvh && (s->n_nodes <= 0 || !s->nodes)))
    return fail(PT_E_INVALID, "pt_upload_scene: empty scene");
  if (s->n_bsdfs <= 0 || !s->bsdfs) return fail(PT_E_INVALID, "pt_upload_scene: no BSDFs");
  if (s->n_lights < 0 || (s->n_lights > 0 && !s->lights)) return fail(PT_E_INVALID, "pt_upload_scene: bad lights");
  if (s->n_lights > 65535) return fail(PT_E_INVALID, "pt_upload_scene: more than 65535 lights");
  if (s->n_prims > (int64_t)0x3fffffff) return fail(PT_E_INVALID, "pt_upload_scene: too many primitives");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipDeviceSynchronize());  // renders in flight read the scene being replaced

  const FlattenKnobs knobs = read_flatten_knobs(gpu_bvh);
  FlatScene f;
  if (int rc = flatten_scene(s, knobs, f)) return rc;  // (a scene refused so far leaves the old one in place)

  // from here on the device holds a mix of the old scene and the new: a
  // failure half-way leaves no scene, not one whose arrays disagree
  c->have_scene = false;
  DeviceScene& sc = c->scene;
  if (int rc = put(sc.prims, f.prims)) return rc;
  if (int rc = put(sc.norms, f.norms)) return rc;
  HIPCHK(sc.bsdfs.reserve(f.bsdfs.size()));
  HIPCHK(sc.lights.reserve(std::max<size_t>(1, f.lights.size())));
  sc.prim_map.release();
  sc.prims_ref.release();
  sc.norms_ref.release();
  if (!f.prims_ref.empty()) {
    if (int rc = put(sc.prims_ref, f.prims_ref)) return rc;
    if (int rc = put(sc.norms_ref, f.norms_ref)) return rc;
  }
  if (knobs.tree == FLATTEN_GPU_TREE) {
    // the reference-count launch walks the caller's tree over a caller-order
    // copy of the primitives
    if (int rc = put(sc.prims_ref, f.prims)) return rc;
    if (int rc = put(sc.norms_ref, f.norms)) return rc;
    if (int rc = build_gpu_bvh(sc, f, c->stream)) return rc;  // adopts prims/norms/prim_map/nodes in its own order
    if (int rc = put(sc.nodes2, f.nodes2)) return rc;
    sc.n_nodes2 = f.nodes2.size();
    sc.bvh_stack = std::max(sc.bvh_stack, f.bvh_stack);
  } else if (knobs.tree == FLATTEN_LBVH_ENTRY) {
    if (int rc = build_gpu_bvh(sc, f, c->stream)) return rc;
  } else {
    if (int rc = put(sc.nodes2, f.nodes2)) return rc;
    sc.n_nodes2 = f.nodes2.size();
    if (int rc = put(sc.nodes, f.nodes4)) return rc;
    if (!f.prim_map.empty())
      if (int rc = put(sc.prim_map, f.prim_map)) return rc;
    sc.bvh_stack = f.bvh_stack;
    sc.n_render_nodes = f.nodes4.size();
    sc.set_root(f.root_lo, f.root_hi, f.root_lo_d, f.root_hi_d);
  }
  HIPCHK(hipMemcpy(sc.bsdfs.p, f.bsdfs.data(), f.bsdfs.size() * sizeof(DBsdf), hipMemcpyHostToDevice));
  if (!f.lights.empty())
    HIPCHK(hipMemcpy(sc.lights.p, f.lights.data(), f.lights.size() * sizeof(DLight), hipMemcpyHostToDevice));
  sc.env_w = f.env_w;
  sc.env_h = f.env_h;
  if (f.env_w) {
    const EnvTables& env = f.env;
    if (int rc = put(sc.env_tex, env.tex)) return rc;
    if (int rc = put(sc.env_ptheta, env.p_theta)) return rc;
    if (int rc = put(sc.env_pphi, env.p_phi)) return rc;
    if (int rc = put(sc.env_pdf, env.p_theta_phi)) return rc;
    if (int rc = put(sc.env_rtheta, env.r_theta)) return rc;
    if (int rc = put(sc.env_rphi, env.r_phi)) return rc;
  }
  sc.n_lights = (int)f.lights.size();
  sc.n_bsdfs = (int)f.bsdfs.size();
  sc.bsdf_types = f.bsdf_types;
  sc.n_prims = s->n_prims;
  sc.tri_only = f.tri_only;
  c->have_scene = true;
  return PT_OK;
}

int pt_upload_scene(pt_ctx* c, const pt_scene* s) { return upload_impl(c, s, false); }

int pt_upload_scene_lbvh(pt_ctx* c, const pt_scene* s) { return upload_impl(c, s, true); }

int pt_set_camera(pt_ctx* c, const pt_camera* cam) {
  if (!c || !cam) return fail(PT_E_INVALID, "pt_set_camera: NULL argument");
  if (int rc = tile_launch(c)) return rc;
  if (!(cam->screen_dist > 0) || !(cam->screen_w > 0) || !(cam->screen_h > 0))
    return fail(PT_E_INVALID, "pt_set_camera: non-positive screen size/distance");
  c->cam = *cam;
  c->have_cam = true;
  return PT_OK;
}

int pt_set_params(pt_ctx* c, const pt_params* p) {
  if (!c || !p) return fail(PT_E_INVALID, "pt_set_params: NULL argument");
  if (int rc = tile_launch(c)) return rc;
  if (p->width <= 0 || p->height <= 0 || p->spp <= 0 || p->max_depth < 0 || p->ns_area_light <= 0)
    return fail(PT_E_INVALID, "pt_set_params: width/height/spp/ns_area_light must be positive, max_depth >= 0");
  if (p->max_depth > 254 || p->ns_area_light > 255)  // packed in 8 bits each in the kernel's path state
    return fail(PT_E_INVALID, "pt_set_params: max_depth must be <= 254 and ns_area_light <= 255");
  if (int rc = check_frame_dims(p->width, p->height, "pt_set_params")) return rc;
  c->params = *p;
  c->have_params = true;
  return PT_OK;
}

int build_tiles(pt_ctx* c, const pt_tile* tiles, int32_t n, std::vector<int4>& out) {
  const int W = c->params.width, H = c->params.height;
  for (int32_t i = 0; i < n; ++i) {
    const pt_tile& t = tiles[i];
    if (t.w < 0 || t.h < 0) return fail(PT_E_INVALID, "pt_render_tiles: negative tile size");
    int x0 = std::max(0, t.x), y0 = std::max(0, t.y);
    int x1 = std::min(W, t.x + t.w), y1 = std::min(H, t.y + t.h);  // raytrace_tile clamps (pathtracer.cpp:594-595)
    for (int y = y0; y < y1; y += 32)
      for (int x = x0; x < x1; x += 32) out.push_back(make_int4(x, y, std::min(32, x1 - x), std::min(32, y1 - y)));
  }
  return PT_OK;
}

// What the launch policy (launch_plan.h) reads of the context, for `nf` frames of the tiles `tl`.
// A ray launch (`rays`) has no camera: no screen footprint culls its pixels or
// sizes its sample groups, its kernel has no triangle-only or pixel-trace
// build, and its grid follows the RAYS builds' own occupancy.
static PlanInput plan_input(const pt_ctx* c, const std::vector<int4>& tl, int nf, uint32_t flags, bool gpu_idle,
                            const LaunchKnobs& knobs, bool rays = false) {
  PlanInput in;
  in.W = c->params.width;
  in.H = c->params.height;
  in.spp = c->params.spp;
  in.cam = c->cam;
  const DeviceScene& sc = c->scene;
  std::copy(sc.root_lo_d, sc.root_lo_d + 3, in.box_lo);
  std::copy(sc.root_hi_d, sc.root_hi_d + 3, in.box_hi);
  in.env = sc.env_w > 0;
  in.n_bsdfs = sc.n_bsdfs;
  in.n_lights = sc.n_lights;
  in.n_render_nodes = (int64_t)sc.n_render_nodes;
  in.bvh_stack = sc.bvh_stack;
  in.tri_only = sc.tri_only;
  in.n_cu = c->n_cu;
  in.grid_plain = c->grid_plain;
  in.grid_stats = c->grid_stats;
  std::copy(c->bpc_variant, c->bpc_variant + 4, in.bpc_variant);
  in.stats_cap = c->stats.n;
  in.tiles = reinterpret_cast<const PlanRect*>(tl.data());
  in.n_tiles = tl.size();
  in.nf = nf;
  in.flags = flags;
  in.gpu_idle = gpu_idle;
  in.knobs = knobs;
  if (rays) {
    in.cam = pt_camera{};
    in.knobs.no_footprint_cull = true;
    in.knobs.no_tri_only = true;
    in.knobs.debug_x = in.knobs.debug_y = -1;
    std::copy(c->bpc_rays, c->bpc_rays + 4, in.bpc_variant);
    in.grid_plain = std::max(8, c->bpc_rays[0]) * c->n_cu;
  }
  return in;
}

// What the kernels read of the context and of the plan; launch() adds its render slot's buffers.
static KParams kernel_params(const pt_ctx* c, const LaunchPlan& plan, int nf, const uint32_t* seeds, uint32_t flags) {
  KParams P;
  std::memset(&P, 0, sizeof(P));
  const DeviceScene& sc = c->scene;
  set_camera_args(P, c->cam, c->params);
  std::copy(sc.root_lo, sc.root_lo + 3, P.root_lo);
  std::copy(sc.root_hi, sc.root_hi + 3, P.root_hi);
  P.spp = c->params.spp;
  P.max_depth = c->params.max_depth;
  P.ns_area = c->params.ns_area_light;
  P.nls_scale = (float)(1.0 / (double)P.ns_area);
  P.seed = seeds ? seeds[0] : c->params.seed;
  P.sample_base = c->params.sample_base;
  P.n_frames = nf;
  for (int f = 0; f < PT_MAX_FRAMES; ++f) P.seeds[f] = seeds && f < nf ? seeds[f] : P.seed;
  P.n_lights = sc.n_lights;
  P.n_bsdfs = sc.n_bsdfs;
  P.nodes = sc.nodes.p;
  P.nodes2 = sc.nodes2.p;
  P.prims = sc.prims.p;
  P.norms = sc.norms.p;
  if ((flags & PT_FLAG_REF_COUNTS) && sc.prims_ref.p) {  // nodes2 indexes the caller's order
    P.prims = sc.prims_ref.p;
    P.norms = sc.norms_ref.p;
  }
  P.bsdfs = sc.bsdfs.p;
  P.lights = sc.lights.p;
  P.env_w = sc.env_w;
  P.env_h = sc.env_h;
  P.env_tex = sc.env_tex.p;
  P.env_ptheta = sc.env_ptheta.p;
  P.env_pphi = sc.env_pphi.p;
  P.env_pdf = sc.env_pdf.p;
  P.env_rtheta = sc.env_rtheta.p;
  P.env_rphi = sc.env_rphi.p;
  P.packed = (flags & PT_FLAG_PACKED16) ? 16 : (flags & PT_FLAG_PACKED) ? 32 : 0;
  P.stats = c->stats.p;
  P.cull_x0 = plan.cull[0];
  P.cull_y0 = plan.cull[1];
  P.cull_x1 = plan.cull[2];
  P.cull_y1 = plan.cull[3];
  P.group_spp = plan.group_spp;
  P.group_shift = plan.group_shift;
  P.n_groups = plan.n_groups;
  P.grp_m = plan.grp_m;
  P.grp_sh = plan.grp_sh;
  P.frame_slots = (uint32_t)plan.frame_slots;
  P.frm_m = plan.frm_m;
  P.frm_sh = plan.frm_sh;
  P.chunk = plan.chunk;
  P.qbands = plan.qbands;
  P.sblocks = plan.sblocks;
  P.shade_batch = plan.shade_batch;
  P.leaf_weight = plan.leaf_weight;
  P.drain_div = plan.drain_div;
  P.tri_only = plan.tri_only;
  P.helpers = plan.helpers;
  P.census = plan.census;
  P.dbg_pix = plan.dbg_pix;
  P.n_blocks = (int)plan.blocks.size();
  return P;
}

// One render: the render kernel on the slot's render stream, then the resolve
// on the caller's stream `s`, ordered after the render (see pt_ctx: the render
// pipeline).  (The resolve on the render stream instead measured one frame
// +0.03 ms: profiles/r5/ab_resolve_reset_stream.txt.)  `nf` > 1: a frame batch
// (pt_render_frames_device) -- nf frames of these tiles, frame f keyed by
// seeds[f] into outs[f], in ONE render launch (the MF kernel) and nf resolves;
// `seeds` null: the parameters' seed.
// The launch's shape -- tile order, blocks, sample groups, grid, queue claims --
// is plan_launch's (launch_plan.cpp), from the knobs and the idle query; a
// plan that is refused returns before anything is enqueued or any slot taken.
// `rays`: a ray launch -- the RAYS kernel replays the caller's rays or captures
// into them; its render stream first waits for what `s` held at the call, so
// the rays are read (and written) in the caller's stream order.
int launch(pt_ctx* c, const std::vector<int4>& tl_in, float* const* outs, int nf, const uint32_t* seeds,
                  hipStream_t s, uint32_t flags, const RayLaunch* rays) {
  std::memset(&c->last, 0, sizeof(c->last));
  c->times_pending = false;
  if (tl_in.empty()) return PT_OK;
  const LaunchKnobs knobs = read_launch_knobs();
  // A launch that finds every slot's last resolve complete has no frame to
  // overlap with: it runs on the caller's stream, with no cross-stream waits
  // in front of the render or between the render and the resolve (a lone
  // frame's wall clock; the slots still alternate).  Only hipErrorNotReady
  // means busy: any other result is a fault of an earlier render, reported
  // here instead of being absorbed into the choice.
  bool gpu_idle = true;  // no earlier render of this context still running or queued
  for (int k = 0; k < pt_ctx::kSlots && gpu_idle; ++k) {
    if (!c->slots[k].ev_free) continue;  // (a slot never used)
    const hipError_t q = hipEventQuery(c->slots[k].ev_free);
    if (q == hipErrorNotReady) {
      (void)hipGetLastError();  // (a not-ready query is no error of this launch)
      gpu_idle = false;
    } else if (q != hipSuccess) {
      return fail(PT_E_HIP, std::string("render: an earlier launch failed: ") + hipGetErrorString(q));
    }
  }
  if (rays && c->bpc_rays[0] <= 0)
    for (int v = 0; v < 4; ++v) HIPCHK(ptk_render_occupancy_rays(&c->bpc_rays[v], (v & 2) != 0, (v & 1) != 0));
  const LaunchPlan plan = plan_launch(plan_input(c, tl_in, nf, flags, gpu_idle, knobs, rays != nullptr));
  if (!plan.error.empty()) return fail(PT_E_INVALID, plan.error);
  // PT_PIPELINE=0 and census launches: every render on the caller's stream, one slot
  const bool pipelined = knobs.pipeline && !plan.census;
  const int depth = c->small_last ? pt_ctx::kSlots : pt_ctx::kSlotsLarge;
  RenderSlot& slot = c->slots[pipelined ? (int)(c->slot_rr++ % (uint64_t)depth) : 0];
  if (!plan.stats) c->small_last = plan.small;
  const bool idle = pipelined && gpu_idle;
  HIPCHK(slot.open(c->stream));  // a small launch's first use of slots 2 and 3
  hipStream_t rs = pipelined && !idle ? (hipStream_t)slot.stream : s;
  // the slot's device state is free once the previous resolve that read it ran
  if (!idle) HIPCHK(hipStreamWaitEvent(rs, slot.ev_free, 0));
  if (rays && rs != s) {  // the rays are the caller's: everything queued on `s` so far comes first
    HIPCHK(slot.ev_rays.create(hipEventDisableTiming));
    HIPCHK(hipEventRecord(slot.ev_rays, s));
    HIPCHK(hipStreamWaitEvent(rs, slot.ev_rays, 0));
  }
  const PlanRect* tl = plan.zorder ? plan.ztiles.data() : reinterpret_cast<const PlanRect*>(tl_in.data());
  const bool tile_out = plan.zorder && (flags & (PT_FLAG_PACKED | PT_FLAG_PACKED16));  // packed outputs keep the caller's tile index
  HIPCHK(slot.tiles.sync(tl, tl_in.size(), rs));
  if (tile_out) HIPCHK(slot.tout.sync(plan.perm.data(), plan.perm.size(), rs));
  HIPCHK(slot.blocks.sync(plan.blocks.data(), plan.blocks.size(), rs));
  HIPCHK(slot.tblock0.sync(plan.tile_block0.data(), plan.tile_block0.size(), rs));
  // Queue heads: zeroed by the slot's previous resolve (a memset in front of the render is a dependent launch of its own, ~20 us
  // before the render kernel starts on a lone frame); a memset only when
  // that did not happen (first use, a launch that failed half-way)
  if (!slot.counter_clean)
    HIPCHK(hipMemsetAsync(slot.counter.p, 0, PT_QUEUE_WORDS * PT_QUEUE_HEADS * sizeof(uint32_t), rs));
  slot.counter_clean = false;
  if (plan.stats) {
    unsigned long long init[PT_STATS_SLOTS] = {0};
    init[PT_STAT_WAVE_START_MIN] = init[PT_STAT_WAVE_END_MIN] = init[PT_STAT_WAVE_EMPTY_MIN] = ~0ull;  // atomicMin slots
    HIPCHK(hipMemcpyAsync(c->stats.p, init, sizeof(init), hipMemcpyHostToDevice, rs));
    HIPCHK(hipStreamSynchronize(rs));  // `init` is a stack array
  }
  KParams P = kernel_params(c, plan, nf, seeds, flags);
  P.out = outs[0];
  P.work_counter = slot.counter.p;
  P.n_tiles = (int)tl_in.size();
  P.tiles = slot.tiles.dev.p;
  P.tile_out = tile_out ? slot.tout.dev.p : nullptr;
  P.blocks = slot.blocks.dev.p;
  P.tile_block0 = slot.tblock0.dev.p;
  P.rays = rays ? rays->rays : nullptr;
  P.rays_capture = rays && rays->capture ? 1 : 0;
  // (growing a buffer synchronises the device: a frame batch sizes every render slot's at once)
  if (nf > 1)
    for (RenderSlot& k : c->slots) {
      HIPCHK(k.partial.reserve(plan.batch_partial_floats));
      if (plan.batch_spill_ints) HIPCHK(k.spill.reserve(plan.batch_spill_ints));
    }
  HIPCHK(slot.partial.reserve(plan.partial_floats));
  P.partial = slot.partial.p;
  if (plan.spill_ints) HIPCHK(slot.spill.reserve(plan.spill_ints));
  P.stack_spill = plan.spill_ints ? slot.spill.p : nullptr;
  if (P.census)  // (a build without -DPT_CENSUS=1 leaves the drain fields 0)
    HIPCHK(hipMemsetAsync(c->stats.p + PT_STATS_SLOTS, 0, (size_t)plan.grid * PT_WAVE_TRACE * 8, rs));
  c->cur = c->ev[c->n_launches++ % pt_ctx::kRing];
  HIPCHK(hipEventRecord(c->cur[0], rs));
  HIPCHK(ptk_launch_render(&P, plan.grid, plan.stats, (flags & PT_FLAG_REF_COUNTS) != 0, rs));
  HIPCHK(hipEventRecord(c->cur[1], rs));
  if (rs != s) HIPCHK(hipStreamWaitEvent(s, c->cur[1], 0));  // the resolve reads the finished group sums
  for (int f = 0; f < nf; ++f) {  // (a frame batch: frame f's sums follow frame f - 1's)
    KParams Pf = P;
    Pf.partial = P.partial + 3 * (size_t)f * (size_t)plan.frame_slots;
    Pf.out = outs[f];
    HIPCHK(ptk_launch_resolve(&Pf, s));
  }
  slot.counter_clean = true;  // (the resolve zeroed the slot's queue heads)
  HIPCHK(hipEventRecord(c->cur[2], s));
  HIPCHK(hipEventRecord(slot.ev_free, s));
  c->census_valid = P.census != 0;
  c->culled_px = plan.culled_px;
  c->last.tile_zorder = plan.zorder ? 1 : 0;
  std::copy(plan.footprint, plan.footprint + 4, c->last.footprint);
  c->last.partial_bytes = plan.slots * PT_SUM_BYTES;
  c->last.grid_blocks = plan.grid;
  c->last.group_spp = plan.group_spp;
  c->last.blocks_per_cu = (int32_t)(plan.want / std::max(1, c->n_cu));
  c->last.pixels = plan.pixels;
  c->last.bvh_stack = c->scene.bvh_stack;
  c->last.bvh_nodes = (int64_t)c->scene.n_render_nodes;
  c->last.samples = plan.pixels * c->params.spp;
  c->last.frames_per_launch = nf;
  return PT_OK;
}

// The last launch's kernel / resolve times (waits for its events).
static int settle_times(pt_ctx* c) {
  if (!c->times_pending) return PT_OK;
  HIPCHK(hipEventSynchronize(c->cur[2]));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, c->cur[0], c->cur[1]));
  c->last.last_ms = ms;
  HIPCHK(hipEventElapsedTime(&ms, c->cur[1], c->cur[2]));
  c->last.resolve_ms = ms;
  c->times_pending = false;
  return PT_OK;
}

// After a launch: counters (and times) of a stats launch now; a plain device
// launch stays asynchronous, its times are read when asked for.
int finish_stats(pt_ctx* c, hipStream_t s, uint32_t flags, bool sync) {
  if (c->last.grid_blocks == 0) return PT_OK;  // nothing was launched
  c->times_pending = true;
  const bool counters = (flags & (PT_FLAG_STATS | PT_FLAG_REF_COUNTS)) != 0;
  if (!sync && !counters) return PT_OK;
  HIPCHK(hipStreamSynchronize(s));
  int rc = settle_times(c);
  if (rc) return rc;
  if (counters) {
    unsigned long long v[PT_STATS_SLOTS] = {0};
    HIPCHK(hipMemcpy(v, c->stats.p, sizeof(v), hipMemcpyDeviceToHost));
    c->last.camera_rays = (int64_t)v[PT_STAT_CAMERA_RAYS];
    c->last.bounce_rays = (int64_t)v[PT_STAT_BOUNCE_RAYS];
    c->last.shadow_rays = (int64_t)v[PT_STAT_SHADOW_RAYS];
    c->last.node_visits = (int64_t)v[PT_STAT_NODE_VISITS];
    c->last.tri_tests = (int64_t)v[PT_STAT_TRI_TESTS];
    c->last.sphere_tests = (int64_t)v[PT_STAT_SPHERE_TESTS];
    c->last.ext_hits = (int64_t)v[PT_STAT_EXT_HITS];
    c->last.wave_trav_steps = (int64_t)v[PT_STAT_WAVE_TRAV_STEPS];
    c->last.wave_rounds = (int64_t)v[PT_STAT_WAVE_ROUNDS];
    c->last.culled_samples = c->culled_px * c->params.spp;
    c->last.leaf_steps = (int64_t)v[PT_STAT_LEAF_STEPS];
    c->last.queue_atomics = (int64_t)v[PT_STAT_QUEUE_ATOMICS];
    c->last.shade_clocks = (int64_t)v[PT_STAT_SHADE_CLOCKS];
    c->last.trav_clocks = (int64_t)v[PT_STAT_TRAV_CLOCKS];
    c->last.max_wave_clocks = (int64_t)v[PT_STAT_MAX_WAVE_CLOCKS];
    c->last.wave_wall_sum = (int64_t)v[PT_STAT_WAVE_WALL_SUM];
    c->last.wave_wall_max = (int64_t)v[PT_STAT_WAVE_WALL_MAX];
    c->last.hitshade_clocks = (int64_t)v[PT_STAT_HITSHADE_CLOCKS];
    for (int k = 0; k < 4; ++k) c->last.section_clocks[k] = (int64_t)v[PT_STAT_SECTION_CLOCKS + k];
    for (int k = 0; k < 4; ++k) c->last.lane_iters[k] = (int64_t)v[PT_STAT_LANE_ITERS + k];
    c->last.deep_stack_steps = (int64_t)v[PT_STAT_DEEP_STACK_STEPS];
    for (int k = 0; k < 32; ++k) c->last.slot_latency_hist[k] = (int64_t)v[PT_STAT_SLOT_LATENCY_HIST + k];
    for (int k = 0; k < 8; ++k) c->last.node_census[k] = (int64_t)v[PT_STAT_NODE_CENSUS + k];
    // the launch's shape, from the first wave's start: last start, first / last end, first / last empty queue (-1: never)
    const unsigned long long t0 = v[PT_STAT_WAVE_START_MIN];
    for (int k = 0; k < 3; ++k) c->last.wave_span[k] = (int64_t)(v[PT_STAT_WAVE_START_MAX + k] - t0);
    for (int k = 0; k < 2; ++k)
      c->last.wave_span[3 + k] = v[PT_STAT_WAVE_EMPTY_MIN + k] ? (int64_t)(v[PT_STAT_WAVE_EMPTY_MIN + k] - t0) : -1;
    c->last.counters_valid = 1;
  }
  return PT_OK;
}

int check_ready(pt_ctx* c) {
  if (!c) return fail(PT_E_INVALID, "NULL context");
  if (!c->have_scene || !c->have_cam || !c->have_params)
    return fail(PT_E_NOSCENE, "render before pt_upload_scene / pt_set_camera / pt_set_params");
  return PT_OK;
}

// True when no pixel belongs to two of the (clipped) tiles.
static bool tiles_disjoint(const std::vector<int4>& tl, size_t W, size_t H) {
  std::vector<uint8_t> seen(W * H, 0);
  for (const int4& t : tl)
    for (int y = t.y; y < t.y + t.w; ++y)
      for (int x = t.x; x < t.x + t.z; ++x) {
        uint8_t& v = seen[(size_t)y * W + (size_t)x];
        if (v) return false;
        v = 1;
      }
  return true;
}

int render_begin(pt_ctx* c, const pt_tile* tiles, int32_t n_tiles, const char* bad_args, void* stream,
                 std::vector<int4>& tl, hipStream_t* s) {
  int rc = check_ready(c);
  if (rc) return rc;
  if ((rc = tile_launch(c))) return rc;  // earlier asynchronous tiles first (call order)
  if (bad_args) return fail(PT_E_INVALID, bad_args);
  HIPCHK(hipSetDevice(c->device));
  *s = stream_of(c, stream);
  return build_tiles(c, tiles, n_tiles, tl);
}

int pt_render_tiles(pt_ctx* c, const pt_tile* tiles, int32_t n_tiles, float* hdr_out_host, uint32_t flags) {
  const char* bad = n_tiles < 0 || (n_tiles > 0 && (!tiles || !hdr_out_host)) ? "pt_render_tiles: bad args"
                    : flags & (PT_FLAG_PACKED | PT_FLAG_PACKED16)
                        ? "pt_render_tiles: packed output is for pt_render_tiles_device"
                        : nullptr;
  std::vector<int4> tl;
  hipStream_t s;  // (the context's)
  int rc = render_begin(c, tiles, n_tiles, bad, nullptr, tl, &s);
  if (rc) return rc;
  const size_t W = (size_t)c->params.width, H = (size_t)c->params.height;
  HIPCHK(c->frame.reserve(W * H * 3));
  float* fr = c->frame.p;
  if ((rc = launch(c, tl, &fr, 1, nullptr, s, flags))) return rc;
  // Copy back only the tiles' pixels (the caller's buffer is theirs outside
  // them); a call whose (clipped, disjoint) tiles cover the whole frame - the
  // whole-frame batch - is one contiguous copy.
  int64_t area = 0;
  for (const int4& t : tl) area += (int64_t)t.z * t.w;
  if (area == (int64_t)(W * H) && tiles_disjoint(tl, W, H)) {
    HIPCHK(hipMemcpyAsync(hdr_out_host, c->frame.p, W * H * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
  } else {
    for (const int4& t : tl) {
      size_t off = ((size_t)t.y * W + (size_t)t.x) * 3;
      HIPCHK(hipMemcpy2DAsync(hdr_out_host + off, W * 3 * sizeof(float), c->frame.p + off, W * 3 * sizeof(float),
                              (size_t)t.z * 3 * sizeof(float), (size_t)t.w, hipMemcpyDeviceToHost, s));
    }
  }
  return finish_stats(c, s, flags, true);
}

// PT_FLAG_PACKED / PT_FLAG_PACKED16: tile i -> packed slot i, so no clipping
// or splitting may renumber tiles: every tile 1..S x 1..S and inside the frame
static int check_packed(const pt_ctx* c, const pt_tile* tiles, int32_t n_tiles, uint32_t flags, const char* fn) {
  if (!(flags & (PT_FLAG_PACKED | PT_FLAG_PACKED16))) return PT_OK;
  const int S = (flags & PT_FLAG_PACKED16) ? 16 : 32;
  const int W = c->params.width, H = c->params.height;
  for (int32_t i = 0; i < n_tiles; ++i) {
    const pt_tile& t = tiles[i];
    if (t.w < 1 || t.h < 1 || t.w > S || t.h > S || t.x < 0 || t.y < 0 || t.x + t.w > W || t.y + t.h > H)
      return fail(PT_E_INVALID, std::string(fn) + ": packed output needs tiles of 1.." + std::to_string(S) + " x 1.." +
                                    std::to_string(S) + " inside the frame");
  }
  return PT_OK;
}

int pt_render_tiles_device(pt_ctx* c, const pt_tile* tiles, int32_t n_tiles, float* hdr_out_dev, void* stream,
                           uint32_t flags) {
  const bool bad = n_tiles < 0 || (n_tiles > 0 && (!tiles || !hdr_out_dev));
  std::vector<int4> tl;
  hipStream_t s;
  int rc = render_begin(c, tiles, n_tiles, bad ? "pt_render_tiles_device: bad args" : nullptr, stream, tl, &s);
  if (rc) return rc;
  if ((rc = check_packed(c, tiles, n_tiles, flags, "pt_render_tiles_device"))) return rc;
  if ((rc = launch(c, tl, &hdr_out_dev, 1, nullptr, s, flags))) return rc;
  return finish_stats(c, s, flags, false);
}

int pt_render_frames_device(pt_ctx* c, const pt_tile* tiles, int32_t n_tiles, int32_t n_frames, const uint32_t* seeds,
                            float* const* hdr_outs_dev, void* stream, uint32_t flags) {
  auto bad_args = [&]() -> const char* {
    if (n_frames < 1 || n_frames > PT_MAX_FRAMES || !seeds || !hdr_outs_dev || n_tiles < 0 || (n_tiles > 0 && !tiles))
      return "pt_render_frames_device: bad args (1 <= n_frames <= PT_MAX_FRAMES, seeds and outputs)";
    for (int32_t f = 0; f < n_frames; ++f)
      if (n_tiles > 0 && !hdr_outs_dev[f]) return "pt_render_frames_device: NULL output";
    if (flags & (PT_FLAG_STATS | PT_FLAG_REF_COUNTS))
      return "pt_render_frames_device: counters are per frame (pt_render_tiles_device)";
    return nullptr;
  };
  std::vector<int4> tl;
  hipStream_t s;
  int rc = render_begin(c, tiles, n_tiles, bad_args(), stream, tl, &s);
  if (rc) return rc;
  if ((rc = check_packed(c, tiles, n_tiles, flags, "pt_render_frames_device"))) return rc;
  // One launch for the batch in the plain common build; the environment-light
  // and global-table builds, diagnostics and PT_FRAME_BATCH=0 render the
  // frames one launch each (the same images)
  const LaunchKnobs knobs = read_launch_knobs();
  const PlanInput in = plan_input(c, tl, 1, flags, true, knobs);
  const bool one = !knobs.frame_batch || n_frames == 1 || in.env || global_tables(in) || knobs.census || knobs.debug_pixel;
  if (one) {
    for (int32_t f = 0; f < n_frames; ++f)
      if ((rc = launch(c, tl, &hdr_outs_dev[f], 1, &seeds[f], s, flags))) return rc;
  } else {
    // (frames beyond what one launch's slot indices and group sums hold go
    // into further batches)
    for (int32_t f = 0; f < n_frames;) {
      const int nf = frames_that_fit(in, n_frames - f);
      if ((rc = launch(c, tl, hdr_outs_dev + f, nf, seeds + f, s, flags))) return rc;
      f += nf;
    }
  }
  return finish_stats(c, s, flags, false);
}

// ---- asynchronous one-tile seam (tile_seam.h)
static int tile_launch_impl(pt_ctx* c);

// A batch that could not be launched: its tiles are dropped, so the failure is
// also kept for the next pt_tile_finish (which would otherwise report PT_OK for
// tiles it never rendered), whoever called tile_launch.
int tile_launch(pt_ctx* c) {
  if (!c || !c->seam.queued()) return PT_OK;
  const int rc = tile_launch_impl(c);
  return rc ? c->seam.record_failure(rc, std::string("tile launch: ") + pt_last_error()) : PT_OK;
}

static int tile_launch_impl(pt_ctx* c) {
  TileSeam& seam = c->seam;
  std::vector<TileJob> jobs = seam.take_queue();
  if (seam.fault_injected()) return fail(PT_E_HIP, "pt_tile_submit: injected launch failure (PT_FAULT_TILE_LAUNCH)");
  HIPCHK(hipSetDevice(c->device));
  const size_t W = (size_t)c->params.width, H = (size_t)c->params.height;
  std::vector<int4> tl;
  for (const auto& j : jobs) tl.push_back(j.t);
  // the band of whole rows the batch's tiles span (a batch of the FIFO is a
  // few tile rows): one copy; pixels of the band outside the tiles land in
  // the stage only, never in the caller's buffers
  int y0 = (int)H, y1 = 0;
  for (const int4& t : tl) {
    y0 = std::min(y0, t.y);
    y1 = std::max(y1, t.y + t.w);
  }
  const size_t need = (size_t)(y1 - y0) * W * 3;
  std::unique_ptr<TileBatch> b = seam.acquire();
  // a batch that is not launched (any return before it is submitted) goes back for reuse
  struct GiveBack {
    TileSeam& seam;
    std::unique_ptr<TileBatch>& b;
    ~GiveBack() {
      if (b) seam.give_back(std::move(b));
    }
  } give_back{seam, b};
  HIPCHK(b->stage.reserve(need));
  HIPCHK(b->ev.create(hipEventDisableTiming));
  HIPCHK(c->frame.reserve(W * H * 3));
  float* fr = c->frame.p;
  if (int rc = launch(c, tl, &fr, 1, nullptr, c->stream, 0)) return rc;
  HIPCHK(hipMemcpyAsync(b->stage.p, c->frame.p + (size_t)y0 * W * 3, need * sizeof(float), hipMemcpyDeviceToHost,
                        c->stream));
  HIPCHK(hipEventRecord(b->ev, c->stream));
  b->jobs = std::move(jobs);
  b->y0 = y0;
  b->W = (int)W;
  b->H = (int)H;
  seam.submit(std::move(b));
  return finish_stats(c, c->stream, 0, false);
}

int pt_tile_submit(pt_ctx* c, const pt_tile* tile, float* hdr_out_host, uint32_t* rgba_out_host) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (!tile || !hdr_out_host) return fail(PT_E_INVALID, "pt_tile_submit: NULL tile or output");
  std::vector<int4> tl;
  if ((rc = build_tiles(c, tile, 1, tl))) return rc;  // clamped to the frame, <= 32 x 32 pieces
  bool full = false;
  for (const int4& t : tl) full = c->seam.push(TileJob{t, hdr_out_host, rgba_out_host});
  return full ? tile_launch(c) : PT_OK;
}

int pt_tile_finish(pt_ctx* c) {
  if (!c) return fail(PT_E_INVALID, "NULL context");
  // Whatever happens to the last launch, every batch already in flight is
  // waited for: the completion thread writes into the caller's buffers, which
  // the caller may free or reuse as soon as this returns.
  (void)tile_launch(c);  // (a failure is recorded in the seam)
  std::string msg;
  const int err = c->seam.drain(&msg);
  return err != PT_OK ? fail(err, msg) : PT_OK;
}

int pt_intersect(pt_ctx* c, int64_t n, const double* o, const double* d, const double* max_t, int32_t* hit, float* t,
                 int32_t* prim, int32_t* any_hit) {
  if (!c) return fail(PT_E_INVALID, "NULL context");
  if (!c->have_scene) return fail(PT_E_NOSCENE, "pt_intersect before pt_upload_scene");
  if (n < 0 || (n > 0 && (!o || !d || !max_t))) return fail(PT_E_INVALID, "pt_intersect: bad args");
  if (n == 0) return PT_OK;
  HIPCHK(hipSetDevice(c->device));
  std::vector<float> f((size_t)n * 7);
  for (int64_t i = 0; i < 3 * n; ++i) {
    f[(size_t)i] = (float)o[i];
    f[(size_t)(3 * n + i)] = (float)d[i];
  }
  // The traversal's "not entered" mark is 3.0e38f and an unused BVH4 slot is a
  // box at +inf: with max_t beyond the mark (the reference's default ray has
  // +inf) a ray with no negative direction component enters the unused slots
  // (tn = inf <= tf = inf) -- pushes the stack bound does not count and, in a
  // host-built tree whose unused slots refer to node 0, a walk that never
  // ends.  Render rays carry 3.0e38f; so do queries.
  for (int64_t i = 0; i < n; ++i) f[(size_t)(6 * n + i)] = (float)std::min(max_t[i], 3.0e38);
  HIPCHK(c->q_f.reserve((size_t)n * 8));
  HIPCHK(c->q_i.reserve((size_t)n * 3));
  HIPCHK(hipMemcpyAsync(c->q_f.p, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  float* dt = c->q_f.p + 7 * n;
  int32_t* dh = c->q_i.p;
  int32_t* dp = c->q_i.p + n;
  int32_t* da = c->q_i.p + 2 * n;
  int* spill = nullptr;
  const DeviceScene& sc = c->scene;
  if (sc.bvh_stack > PT_STACK) {
    HIPCHK(c->q_spill.reserve((size_t)(sc.bvh_stack - PT_STACK) * (size_t)((n + PT_BLOCK - 1) / PT_BLOCK * PT_BLOCK)));
    spill = c->q_spill.p;
  }
  HIPCHK(ptk_launch_intersect(sc.nodes.p, sc.prims.p, c->q_f.p, c->q_f.p + 3 * n, c->q_f.p + 6 * n, n, dh, dt, dp, da,
                              spill, sc.prim_map.p, c->stream));
  std::vector<int32_t> ib((size_t)n * 3);
  std::vector<float> tb((size_t)n);
  HIPCHK(hipMemcpyAsync(ib.data(), c->q_i.p, ib.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(tb.data(), dt, tb.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (int64_t i = 0; i < n; ++i) {
    if (hit) hit[i] = ib[(size_t)i];
    if (prim) prim[i] = ib[(size_t)(n + i)];
    if (any_hit) any_hit[i] = ib[(size_t)(2 * n + i)];
    if (t) t[i] = tb[(size_t)i];
  }
  return PT_OK;
}

int pt_debug_bvh_info(pt_ctx* c, pt_bvh_info* out) {
  if (!c || !out) return fail(PT_E_INVALID, "pt_debug_bvh_info: NULL argument");
  if (!c->have_scene) return fail(PT_E_NOSCENE, "pt_debug_bvh_info before pt_upload_scene");
  const DeviceScene& sc = c->scene;
  *out = pt_bvh_info{};
  out->n_prims = sc.n_prims;
  out->n_nodes4 = (int64_t)sc.n_render_nodes;
  out->n_nodes2 = (int64_t)sc.n_nodes2;
  out->bvh_stack = sc.bvh_stack;
  out->has_prim_map = sc.prim_map.p ? 1 : 0;
  std::copy(sc.root_lo, sc.root_lo + 3, out->root_lo);
  std::copy(sc.root_hi, sc.root_hi + 3, out->root_hi);
  return PT_OK;
}

int pt_debug_read_bvh(pt_ctx* c, void* nodes4, void* nodes2, void* prims, float* norms, int32_t* prim_map) {
  if (!c) return fail(PT_E_INVALID, "NULL context");
  if (!c->have_scene) return fail(PT_E_NOSCENE, "pt_debug_read_bvh before pt_upload_scene");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  const DeviceScene& sc = c->scene;
  const size_t n = (size_t)sc.n_prims;
  if (nodes4) HIPCHK(hipMemcpy(nodes4, sc.nodes.p, sc.n_render_nodes * sizeof(DNode), hipMemcpyDeviceToHost));
  if (nodes2 && sc.n_nodes2) HIPCHK(hipMemcpy(nodes2, sc.nodes2.p, sc.n_nodes2 * sizeof(DNode2), hipMemcpyDeviceToHost));
  if (prims) HIPCHK(hipMemcpy(prims, sc.prims.p, n * sizeof(DPrim), hipMemcpyDeviceToHost));
  if (norms) HIPCHK(hipMemcpy(norms, sc.norms.p, n * 9 * sizeof(float), hipMemcpyDeviceToHost));
  if (prim_map && sc.prim_map.p) HIPCHK(hipMemcpy(prim_map, sc.prim_map.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
  return PT_OK;
}

int pt_debug_live_resources(pt_resource_counts* out) {
  if (!out) return fail(PT_E_INVALID, "pt_debug_live_resources: out is NULL");
  const HipLiveCounts& n = hip_live();
  *out = pt_resource_counts{n.device_arrays, n.device_bytes, n.pinned_arrays, n.events, n.streams};
  return PT_OK;
}

// Host replay of the environment light's inverse-CDF searches (the kernel's
// record_lower_bound over the tables build_env_tables makes) against
// std::lower_bound, for n query pairs (u1, u2) in [0, 1): the row search over
// pTheta, then the column search over that row of pPhiGivenTheta, each checked
// for the index and the interpolation pair (prev, cur) the sampler reads.
int64_t pt_env_search_check(const float* rgb, int32_t width, int32_t height, int64_t n, const float* u1,
                            const float* u2, int64_t* long_windows) {
  if (!rgb || width <= 0 || height <= 0 || n < 0 || (n > 0 && (!u1 || !u2)))
    return fail(PT_E_INVALID, "pt_env_search_check: bad arguments");
  EnvTables t;
  build_env_tables(rgb, width, height, t);
  int64_t bad = 0, longw = 0;
  auto check = [&](const float* a, int len, const EnvRec* rec, float u) -> int {
    const float v = u * a[len - 1];
    const int k = std::min(PT_ENV_GUIDE - 1, std::max(0, (int)(u * (float)PT_ENV_GUIDE)));
    longw += rec[k].hi - rec[k].lo > 4;
    float prev = 0.f, cur = 0.f;
    const int got = record_lower_bound(a, v, u, rec, PT_ENV_GUIDE, prev, cur);
    const int want = (int)(std::lower_bound(a, a + len, v) - a);
    const float wcur = a[std::min(want, len - 1)], wprev = want > 0 ? a[want - 1] : 0.0f;
    if (got != want || std::memcmp(&cur, &wcur, 4) != 0 || std::memcmp(&prev, &wprev, 4) != 0) ++bad;
    return std::min(got, len - 1);
  };
  for (int64_t i = 0; i < n; ++i) {
    const int row = check(t.p_theta.data(), height, t.r_theta.data(), u1[i]);
    check(&t.p_phi[(size_t)row * width], width, &t.r_phi[(size_t)row * PT_ENV_GUIDE], u2[i]);
  }
  if (long_windows) *long_windows = longw;
  return bad;
}

// The float tables build_env_tables makes for a map, as the upload sends them
// to the device (host only): what a test-side reference searches and divides by.
int pt_env_tables(const float* rgb, int32_t width, int32_t height, float* p_theta, float* p_phi, float* pdf) {
  if (!rgb || width <= 0 || height <= 0) return fail(PT_E_INVALID, "pt_env_tables: bad arguments");
  EnvTables t;
  build_env_tables(rgb, width, height, t);
  if (p_theta) std::copy(t.p_theta.begin(), t.p_theta.end(), p_theta);
  if (p_phi) std::copy(t.p_phi.begin(), t.p_phi.end(), p_phi);
  if (pdf) std::copy(t.p_theta_phi.begin(), t.p_theta_phi.end(), pdf);
  return PT_OK;
}

// The environment light's device functions on the uploaded tables, one lane
// per query (env_probe_kernel).  Every query is checked here first: the kernel
// forms its table indices from them and is never launched on one it could not
// answer inside the tables.
int pt_debug_env_probe(pt_ctx* c, int64_t n, const float* u1, const float* u2, int32_t* row, int32_t* col,
                       float* row_pair, float* col_pair, float* wi, float* pdf, float* tu, float* tv, float* radiance,
                       int64_t m, const float* dirs, float* dir_radiance) {
  // (the queries first: they are refused without a device, too)
  const int64_t kMax = 1 << 24;
  if (n < 0 || m < 0 || n > kMax || m > kMax) return fail(PT_E_INVALID, "pt_debug_env_probe: bad query count");
  if (n > 0 && (!u1 || !u2 || !row || !col || !row_pair || !col_pair || !wi || !pdf || !tu || !tv || !radiance))
    return fail(PT_E_INVALID, "pt_debug_env_probe: NULL sample argument");
  if (m > 0 && (!dirs || !dir_radiance)) return fail(PT_E_INVALID, "pt_debug_env_probe: NULL direction argument");
  for (int64_t i = 0; i < n; ++i)
    if (!(u1[i] >= 0.0f && u1[i] < 1.0f && u2[i] >= 0.0f && u2[i] < 1.0f))
      return fail(PT_E_INVALID, "pt_debug_env_probe: sample query " + std::to_string(i) + " outside [0, 1)");
  for (int64_t i = 0; i < m; ++i) {
    const double x = dirs[3 * i], y = dirs[3 * i + 1], z = dirs[3 * i + 2];
    const double len = std::sqrt(x * x + y * y + z * z);
    if (!std::isfinite(len) || std::fabs(len - 1.0) > 1e-3)
      return fail(PT_E_INVALID, "pt_debug_env_probe: direction " + std::to_string(i) + " is not a unit vector");
  }
  if (!c) return fail(PT_E_INVALID, "NULL context");
  if (!c->have_scene) return fail(PT_E_NOSCENE, "pt_debug_env_probe before pt_upload_scene");
  const DeviceScene& sc = c->scene;
  if (sc.env_w <= 0 || sc.env_h <= 0) return fail(PT_E_INVALID, "pt_debug_env_probe: the scene has no environment light");
  if (n == 0 && m == 0) return PT_OK;
  HIPCHK(hipSetDevice(c->device));
  const size_t n_in = (size_t)(2 * n + 3 * m), n_out = (size_t)(13 * n + 3 * m);
  std::vector<float> in(n_in);
  std::copy(u1, u1 + n, in.begin());
  std::copy(u2, u2 + n, in.begin() + n);
  std::copy(dirs, dirs + 3 * m, in.begin() + 2 * n);
  HIPCHK(c->q_f.reserve(n_in + n_out));
  HIPCHK(c->q_i.reserve((size_t)(2 * n)));
  HIPCHK(hipMemcpyAsync(c->q_f.p, in.data(), n_in * sizeof(float), hipMemcpyHostToDevice, c->stream));
  EnvProbe a{};
  a.env_w = sc.env_w, a.env_h = sc.env_h;
  a.env_tex = sc.env_tex.p;
  a.env_ptheta = sc.env_ptheta.p, a.env_pphi = sc.env_pphi.p, a.env_pdf = sc.env_pdf.p;
  a.env_rtheta = sc.env_rtheta.p, a.env_rphi = sc.env_rphi.p;
  a.n = (int)n, a.u = c->q_f.p, a.idx = c->q_i.p, a.out = c->q_f.p + n_in;
  a.m = (int)m, a.d = c->q_f.p + 2 * n, a.rad = c->q_f.p + n_in + 13 * n;
  HIPCHK(ptk_launch_env_probe(&a, c->stream));
  std::vector<float> out(n_out);
  std::vector<int32_t> idx((size_t)(2 * n));
  HIPCHK(hipMemcpyAsync(out.data(), a.out, n_out * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (n > 0) HIPCHK(hipMemcpyAsync(idx.data(), a.idx, idx.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (n > 0) {
    const float* o = out.data();
    std::copy(idx.begin(), idx.begin() + n, row);
    std::copy(idx.begin() + n, idx.end(), col);
    std::copy(o, o + 2 * n, row_pair);
    std::copy(o + 2 * n, o + 4 * n, col_pair);
    std::copy(o + 4 * n, o + 7 * n, wi);
    std::copy(o + 7 * n, o + 8 * n, pdf);
    std::copy(o + 8 * n, o + 9 * n, tu);
    std::copy(o + 9 * n, o + 10 * n, tv);
    std::copy(o + 10 * n, o + 13 * n, radiance);
  }
  if (m > 0) std::copy(out.begin() + 13 * n, out.end(), dir_radiance);
  return PT_OK;
}

int pt_get_stats(pt_ctx* c, pt_stats* out) {
  if (!c || !out) return fail(PT_E_INVALID, "pt_get_stats: NULL argument");
  int rc = settle_times(c);
  if (rc) return rc;
  *out = c->last;
  return PT_OK;
}

int pt_get_launch_times(pt_ctx* c, float* kernel_ms, float* resolve_ms, int32_t cap, int32_t* n) {
  if (!c || !n || cap < 0 || (cap > 0 && !kernel_ms)) return fail(PT_E_INVALID, "pt_get_launch_times: bad args");
  int64_t k = std::min<int64_t>({(int64_t)cap, c->n_launches, (int64_t)pt_ctx::kRing});
  *n = (int32_t)k;
  if (k == 0) return PT_OK;
  HIPCHK(hipSetDevice(c->device));
  for (int64_t i = 0; i < k; ++i) {
    const Event* tri = c->ev[(c->n_launches - k + i) % pt_ctx::kRing];
    HIPCHK(hipEventSynchronize(tri[2]));
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, tri[0], tri[1]));
    kernel_ms[i] = ms;
    if (resolve_ms) {
      HIPCHK(hipEventElapsedTime(&ms, tri[1], tri[2]));
      resolve_ms[i] = ms;
    }
  }
  return PT_OK;
}

int pt_get_wave_trace(pt_ctx* c, int64_t* out, int64_t cap, int64_t* n_waves) {
  if (!c || !n_waves) return fail(PT_E_INVALID, "pt_get_wave_trace: NULL argument");
  if (!c->last.counters_valid && !c->census_valid)
    return fail(PT_E_INVALID, "pt_get_wave_trace: the last launch had no counters (or census)");
  const int64_t n = c->last.grid_blocks;
  *n_waves = n;
  if (!out) return PT_OK;
  if (cap < n * PT_WAVE_TRACE) return fail(PT_E_INVALID, "pt_get_wave_trace: buffer too small");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpy(out, c->stats.p + PT_STATS_SLOTS, (size_t)n * PT_WAVE_TRACE * sizeof(int64_t),
                   hipMemcpyDeviceToHost));
  return PT_OK;
}
