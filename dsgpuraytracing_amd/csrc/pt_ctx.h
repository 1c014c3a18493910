// pt_ctx.h — the device context and the film as the C ABI's translation units
// (pt_api.cpp, pt_api_film.cpp) share them: what a context owns, in parts --
// the uploaded scene (DeviceScene), the render pipeline's slots (RenderSlot),
// the asynchronous tile seam (tile_seam.h), scratch, launch timing, occupancy.
// Includes pt_device.h: HIP translation units only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ptgpu.h"
#include "hip_owned.h"
#include "launch_plan.h"
#include "pt_device.h"
#include "pt_error.h"
#include "tile_seam.h"

// A failed HIP call returns PT_E_HIP with the call's text; HIPCHK_ALLOC (the
// film, denoise and reproject entry points' reserves) returns PT_E_ALLOC when
// memory ran out, with HIP's sticky error cleared.
#define HIPCHK_AS(expr, text, alloc)                                                              \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) {                                                                       \
      if (alloc) (void)hipGetLastError();                                                         \
      return pt_fail((alloc) && _e == hipErrorOutOfMemory ? PT_E_ALLOC : PT_E_HIP, std::string(text ": ") + hipGetErrorString(_e)); \
    }                                                                                             \
  } while (0)
#define HIPCHK(expr) HIPCHK_AS(expr, #expr, false)
#define HIPCHK_ALLOC(expr) HIPCHK_AS(expr, #expr, true)

// The launch policy's rectangles are the device's int4 (x, y, w, h): tile and
// block lists go to the device, and tile lists into a plan, without conversion.
static_assert(sizeof(PlanRect) == sizeof(int4) && offsetof(PlanRect, x) == offsetof(int4, x) &&
                  offsetof(PlanRect, y) == offsetof(int4, y) && offsetof(PlanRect, w) == offsetof(int4, z) &&
                  offsetof(PlanRect, h) == offsetof(int4, w),
              "PlanRect is laid out as int4");

// The uploaded scene: what upload_impl writes and the launches read.
struct DeviceScene {
  DevBuf<DNode> nodes;    // the render tree (BVH4)
  DevBuf<DNode2> nodes2;  // binary tree for PT_FLAG_REF_COUNTS
  DevBuf<int> prim_map;   // own BVH order (SAH or GPU-built) -> uploaded primitive index (else empty)
  // primitives in the caller's (reference BVH) order, for the reference-count
  // launch over nodes2 when the render tree is our own (else empty)
  DevBuf<DPrim> prims_ref;
  DevBuf<float> norms_ref;
  DevBuf<float4> env_tex;                       // environment map RGB (w*h, .w unused)
  DevBuf<float> env_ptheta, env_pphi, env_pdf;  // EnvironmentLight tables
  DevBuf<EnvRec> env_rtheta, env_rphi;          // their guide tables' bucket records
  int env_w = 0, env_h = 0;
  DevBuf<DPrim> prims;
  DevBuf<float> norms;
  DevBuf<DBsdf> bsdfs;
  DevBuf<DLight> lights;
  int n_lights = 0, n_bsdfs = 0;
  int bvh_stack = 0;  // worst-case traversal stack entries of the uploaded BVH
  size_t n_render_nodes = 0;
  size_t n_nodes2 = 0;  // binary nodes in nodes2 (pt_debug_bvh_info)
  int64_t n_prims = 0;
  bool tri_only = false;            // every primitive a triangle
  std::vector<int32_t> bsdf_types;  // the BSDF types (reprojection's keep table)
  // the root box: rounded outward for the kernels, and as the launch policy reads it
  float root_lo[3] = {0, 0, 0}, root_hi[3] = {0, 0, 0};
  double root_lo_d[3] = {0, 0, 0}, root_hi_d[3] = {0, 0, 0};
  template <class D>
  void set_root(const float* lo, const float* hi, const D* lo_d, const D* hi_d) {
    std::copy(lo, lo + 3, root_lo), std::copy(hi, hi + 3, root_hi);
    std::copy(lo_d, lo_d + 3, root_lo_d), std::copy(hi_d, hi_d + 3, root_hi_d);
  }
};

// Render pipeline: launches alternate between kSlots slots, each with its
// own render stream and per-launch device state (tile and block lists,
// work-queue heads, sample-group sums, stack spill area).  A render waits
// only until the resolve of the previous launch of ITS slot has consumed
// the slot's group sums (ev_free), so consecutive device renders overlap:
// the next frame's waves fill the CUs the previous frame's drain leaves
// idle.  Each resolve runs on the caller's stream after its own render, so
// the caller's stream order is kept for everything it can observe.
// Small launches (a strong split's share of a frame: few work slots per
// resident lane) rotate over all kSlots slots, so up to four frames are in
// flight; larger ones over the first two (three slots measured C3 -6%, four
// -10%: profiles/r6/ab_render_slots.txt).  See plan_launch (launch_plan.cpp): small launches.
struct RenderSlot {
  Stream stream;
  Event ev_free;
  // a ray launch reads the caller's rays: its render stream waits for what the
  // caller's stream held at the call (created at the slot's first ray launch)
  Event ev_rays;
  DevList<int4, PlanRect> tiles;
  DevList<int4, PlanRect> blocks;  // footprint-clipped 8x8 pixel blocks of the tiles
  DevList<int> tblock0;            // first block of each tile (+ the end), for the resolve
  DevList<int> tout;               // caller's index of each launched tile (a Z-ordered packed launch)
  DevBuf<float> partial;           // sample-group sums
  DevBuf<int> spill;               // traversal stack entries beyond PT_STACK
  DevBuf<uint32_t> counter;        // work-queue heads, one 128-B line each
  // the queue heads are known to be zero: the last resolve of the slot reset
  // them (PT_RESOLVE_RESETS), so the next launch needs no memset
  bool counter_clean = false;
  // The slot's render stream, and ev_free recorded on the context's stream
  // (nothing to wait for yet); nothing to do for a slot that is open.
  // Render-slot streams: plain non-blocking streams at normal priority.  HIP
  // keeps one pool of GPU_MAX_HW_QUEUES (= 4) hardware queues per stream
  // priority and gives a new stream the least-used queue of its pool; kernel
  // traces and A/Bs of the C3 split's shares (profiles/r6/ab_stream_queues.txt)
  // put render slots at high priority, on CU-masked queues of their own, or
  // the caller's stream at high priority: every arm that keeps more than four
  // hardware queues busy -- counting torch's collective stream on a rank of an
  // N-GPU run -- was slower (N = 8 share 0.22 -> 0.29-0.38 ms per frame).
  hipError_t open(hipStream_t ctx_stream) {
    if (stream) return hipSuccess;
    hipError_t e = stream.create(hipStreamNonBlocking);
    if (e == hipSuccess) e = ev_free.create(hipEventDisableTiming);
    return e == hipSuccess ? hipEventRecord(ev_free, ctx_stream) : e;
  }
};

struct pt_ctx {
  explicit pt_ctx(int dev) : device(dev), seam(dev) {}
  const int device;
  Stream stream;
  // launch timing: a ring of (render start, render end, resolve end) event
  // triples so device renders need not synchronise (pt_get_launch_times)
  static constexpr int kRing = 256;
  Event ev[kRing][3];
  int64_t n_launches = 0;      // launches recorded so far (ring slot = index % kRing)
  bool census_valid = false;   // the last launch was a PT_CENSUS plain launch (its trace area holds start/end/CU)
  bool times_pending = false;  // c->last's times belong to a launch not yet synchronised
  const Event* cur = nullptr;  // the current launch's triple (of `ev`)
  DeviceScene scene;
  static constexpr int kSlots = 4;
  static constexpr int kSlotsLarge = 2;
  RenderSlot slots[kSlots];
  uint64_t slot_rr = 0;     // launches issued on the pipeline (slot rotation)
  bool small_last = false;  // the previous launch was small: rotate over every slot
  int64_t culled_px = 0;    // pixels of the last launch outside the footprint
  DevBuf<float> frame;      // device framebuffer for host-output renders
  // Declared after `frame`, so destroyed before it: the seam's destructor
  // joins the completion thread, whose batches were copied out of `frame`.
  TileSeam seam;
  DevBuf<int> q_spill;  // ray-query stack spill
  DevBuf<unsigned long long> stats;
  DevBuf<float> q_f;  // scratch of the query entry points (pt_intersect, pt_debug_env_probe): inputs and outputs
  DevBuf<int32_t> q_i;
  bool have_scene = false, have_cam = false, have_params = false;
  pt_camera cam{};
  pt_params params{};
  pt_stats last{};
  int grid_plain = 0, grid_stats = 0;
  int bpc_plain = 0, bpc_stats = 0, n_cu = 0;
  int bpc_variant[4] = {0, 0, 0, 0};  // plain builds: [env * 2 + gtab] (the common one is bpc_plain)
  std::vector<std::unique_ptr<pt_film>> films;  // films not yet destroyed
  DevBuf<uint32_t> tc_thr;  // pt_to_color_thresholds on the device (uploaded at first use)
  bool tc_thr_ready = false;
  // first-hit feature pass (pt_render_features*): its tile list, stack spill
  // area and the device side of the host entry point's output; a pass that
  // comes on another stream than the last waits for it
  DevList<int4> ftiles;
  DevBuf<int> f_spill;
  DevBuf<float4> feat_out;
  StreamOrder feat_order;
  DevBuf<float4> dn_a, dn_b;  // pt_denoise_device: the iterations' ping-pong records (grown on demand)
  // reprojection (pt_reproject_device, pt_film_reproject): the keep table on
  // the device with what it holds; a gather that comes on another stream than
  // the last waits for it
  DevList<uint32_t> rp_keep;
  StreamOrder rp_order;
  // ray queries on the device (pt_trace_rays*, pt_camera_rays_device): the
  // spill area of the bounded grid and the {rays, hits, invalid} counter, both
  // reused from call to call -- a trace that comes on another stream than the
  // last waits for it --, the last trace's kernel time, the device side of the
  // host entry point's rays and results, the camera rays' tile list
  DevBuf<int> tr_spill;
  DevBuf<unsigned long long> tr_counts;
  TimedSpan t_trace;
  bool tr_counted = false;  // the last trace launched a kernel: tr_counts and t_trace are its
  StreamOrder tr_order;
  DevBuf<float4> tr_rays, tr_out;
  int bpc_trace[2] = {0, 0};  // resident one-wave workgroups per CU: closest, occluded (asked for at first use)
  DevList<int4> cr_tiles;
  StreamOrder cr_order;
  // ray launches (pt_render_rays*): resident waves per CU of the RAYS builds,
  // [env * 2 + gtab] as bpc_variant (asked for at the first ray launch), and
  // the device side of the host entry point's rays
  int bpc_rays[4] = {0, 0, 0, 0};
  DevBuf<float4> rr_rays;
  // Every member frees itself, in reverse order of declaration; only what
  // needs ordering is done here: no kernel may still be running when the
  // first member goes.
  ~pt_ctx() {
    (void)hipSetDevice(device);
    (void)hipDeviceSynchronize();
  }
};

// A progressive film (ptgpu.h: pt_film_*; kernels and record layout: film.h).
struct pt_film {
  pt_ctx* ctx = nullptr;
  int W = 0, H = 0;
  DevBuf<uint4> rec;     // 2 * W * H records
  DevBuf<float> pass;    // the pass being added (W * H * 3, the frame layout)
  DevList<int4> tiles;   // the last pass's clipped tiles
  DevBuf<int4> etiles;   // pt_film_tile_error: the listed tiles, and their maxima
  DevBuf<float> emax;
  DevBuf<float> out_hdr, out_err;  // pt_film_resolve: device side of the host outputs
  DevBuf<uint32_t> out_rgba;
  DevBuf<float4> feat;   // 2 * W * H feature records (pt_film_set_features; allocated at first use)
  DevBuf<float4> cv[2];  // the denoiser's working records (allocated at first use)
  bool have_feat = false;  // set since creation / the last clear
  pt_camera feat_cam{};    // the camera `feat` was rendered with
  // pt_film_reproject: the second record and feature buffers it writes and then
  // swaps with rec / feat (allocated at first use), the kept / reset counts of
  // the last one and the time of its gather kernel
  DevBuf<uint4> rec2;
  DevBuf<float4> feat2;
  DevBuf<unsigned long long> rp_counts;
  TimedSpan t_rp;
  // pt_film_merge*: the device side of host records, the four class counts of
  // the last merge and the time of its kernel (allocated at first use)
  DevBuf<uint4> mg_stage;
  DevBuf<unsigned long long> mg_counts;
  TimedSpan t_mg;
  uint64_t next = 0;  // next sample index (<= 2^32)
  int64_t passes = 0;
  TimedSpan t_acc, t_res;  // the last accumulate / resolve kernel
  // the film's last operation: a later one on another stream waits for it
  StreamOrder order;
};

// The stream an entry point runs on: the caller's, or the context's for NULL.
inline hipStream_t stream_of(const pt_ctx* c, void* stream) { return stream ? (hipStream_t)stream : (hipStream_t)c->stream; }

// The camera and frame size as the kernels' argument structs (KParams, FeatArgs) hold them.
template <class Args>
void set_camera_args(Args& A, const pt_camera& cam, const pt_params& params) {
  for (int k = 0; k < 3; ++k) {
    A.cam_pos[k] = (float)cam.pos[k];
    A.c2w_col0[k] = (float)cam.c2w[3 * k + 0];
    A.c2w_col1[k] = (float)cam.c2w[3 * k + 1];
    A.c2w_col2[k] = (float)cam.c2w[3 * k + 2];
  }
  A.cam_ax = (float)(cam.screen_w / cam.screen_dist);
  A.cam_ay = (float)(cam.screen_h / cam.screen_dist);
  A.W = params.width;
  A.H = params.height;
  A.inv_w = 1.0f / (float)A.W;
  A.inv_h = 1.0f / (float)A.H;
}

// pt_api.cpp, for the film's entry points too
int check_frame_dims(int64_t width, int64_t height, const char* fn);
int check_ready(pt_ctx* c);
int tile_launch(pt_ctx* c);  // renders the queued tiles of the seam as one launch (nothing queued: nothing to do)
int build_tiles(pt_ctx* c, const pt_tile* tiles, int32_t n, std::vector<int4>& out);
// What the five render entry points begin with: the context ready, earlier
// asynchronous tiles launched (call order), `bad_args` (the caller's argument
// check: the message, or null) refused, the device set; the tiles clipped to
// the frame in <= 32x32 pieces into `tl`, and the stream to run on.
int render_begin(pt_ctx* c, const pt_tile* tiles, int32_t n_tiles, const char* bad_args, void* stream,
                 std::vector<int4>& tl, hipStream_t* s);
// A ray launch (pt_render_rays*, pt_film_add_pass_rays): the W * H rays on the
// device that the render replays, or captures into.
struct RayLaunch {
  float4* rays;
  bool capture;
};
int launch(pt_ctx* c, const std::vector<int4>& tl_in, float* const* outs, int nf, const uint32_t* seeds, hipStream_t s,
           uint32_t flags, const RayLaunch* rays = nullptr);
int finish_stats(pt_ctx* c, hipStream_t s, uint32_t flags, bool sync);
