// pt_api.cpp — C ABI of the HIP path (include/ptgpu.h): device context, scene
// upload (reference BVH -> 64-B two-child-box nodes, primitives -> 48-B float
// records), tile rendering, batched ray queries, counters.
//
// Replaces CUDAPathTracer (cuda_src/setup.h:90-148, setup.cu:92-843): instead of
// one cudaMalloc+cudaMemcpy per BVH node (setup.cu:429-476), constant-memory
// tables capped at 20 entries (kernel.cu:3-20) and exit() on error, the scene is
// flattened on the host into four contiguous arrays, uploaded once, and every
// failure is returned as a PT_E_* code with a message in pt_last_error().
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ptgpu.h"
#include "../../include/ptgpu_scene.h"
#include "denoise.h"
#include "film.h"
#include "hip_owned.h"
#include "launch_plan.h"
#include "pt_device.h"
#include "pt_error.h"
#include "reproject.h"
#include "scene_flatten.h"

namespace {

int fail(int code, const std::string& msg) { return pt_fail(code, msg); }

// A failed HIP call returns PT_E_HIP with the call's text; HIPCHK_ALLOC (the
// film, denoise and reproject entry points' reserves) returns PT_E_ALLOC when
// memory ran out, with HIP's sticky error cleared.
#define HIPCHK_AS(expr, text, alloc)                                                              \
  do {                                                                                            \
    hipError_t _e = (expr);                                                                       \
    if (_e != hipSuccess) {                                                                       \
      if (alloc) (void)hipGetLastError();                                                         \
      return fail((alloc) && _e == hipErrorOutOfMemory ? PT_E_ALLOC : PT_E_HIP, std::string(text ": ") + hipGetErrorString(_e)); \
    }                                                                                             \
  } while (0)
#define HIPCHK(expr) HIPCHK_AS(expr, #expr, false)
#define HIPCHK_ALLOC(expr) HIPCHK_AS(expr, #expr, true)

// A device list with a host mirror of what it holds: uploaded (on `s`) only
// when it changed -- the lists rarely change between frames.  Never a null
// device list: an empty one (a launch may cull every block) still has an array.
// `alloc`: a film entry point's list (PT_E_ALLOC when memory runs out).
template <class D, class T>
int sync_list(DevBuf<D>& dev, std::vector<T>& mirror, const T* list, size_t n, hipStream_t s, bool alloc = false) {
  static_assert(sizeof(D) == sizeof(T), "the list uploads without conversion");
  const D* held = dev.p;
  const hipError_t r = dev.reserve(n);
  if (dev.p != held) mirror.clear();  // (a new array holds nothing yet)
  HIPCHK_AS(r, "dev.reserve(n)", alloc);
  if (n == mirror.size() && std::memcmp(list, mirror.data(), n * sizeof(T)) == 0) return PT_OK;
  mirror.assign(list, list + n);  // (the copy's source outlives the call)
  if (n == 0) return PT_OK;
  const hipError_t e = hipMemcpyAsync(dev.p, mirror.data(), n * sizeof(T), hipMemcpyHostToDevice, s);
  if (e != hipSuccess) mirror.clear();  // (not what the device holds)
  HIPCHK(e);
  return PT_OK;
}

// reserve + blocking copy of a flattened array
template <class T>
int put(DevBuf<T>& dev, const std::vector<T>& v) {
  HIPCHK(dev.reserve(v.size()));
  HIPCHK(hipMemcpy(dev.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  return PT_OK;
}

// Render-slot streams: plain non-blocking streams at normal priority.  HIP
// keeps one pool of GPU_MAX_HW_QUEUES (= 4) hardware queues per stream
// priority and gives a new stream the least-used queue of its pool; kernel
// traces and A/Bs of the C3 split's shares (profiles/r6/ab_stream_queues.txt)
// put render slots at high priority, on CU-masked queues of their own, or
// the caller's stream at high priority: every arm that keeps more than four
// hardware queues busy -- counting torch's collective stream on a rank of an
// N-GPU run -- was slower (N = 8 share 0.22 -> 0.29-0.38 ms per frame).
hipError_t make_render_stream(Stream& s) { return s.create(hipStreamNonBlocking); }

// The frame sizes the kernels' 16-bit pixel coordinates and 32-bit pixel indices hold.
int check_frame_dims(int64_t width, int64_t height, const char* fn) {
  if (width < 1 || height < 1 || width > 65535 || height > 65535 || width * height > (int64_t)1 << 30)
    return fail(PT_E_INVALID, std::string(fn) + ": width and height must be 1 .. 65535 and width * height <= 2^30");
  return PT_OK;
}

}  // namespace

struct pt_ctx {
  int device = 0;
  Stream stream;
  // launch timing: a ring of (render start, render end, resolve end) event
  // triples so device renders need not synchronise (pt_get_launch_times)
  static constexpr int kRing = 256;
  Event ev[kRing][3];
  int64_t n_launches = 0;   // launches recorded so far (ring slot = index % kRing)
  bool census_valid = false;  // the last launch was a PT_CENSUS plain launch (its trace area holds start/end/CU)
  bool times_pending = false;  // c->last's times belong to a launch not yet synchronised
  const Event* cur = nullptr;  // the current launch's triple (of `ev`)
  DevBuf<DNode> nodes;    // the render tree (BVH4)
  DevBuf<DNode2> nodes2;  // binary tree for PT_FLAG_REF_COUNTS
  DevBuf<int> prim_map;   // own BVH order (SAH or GPU-built) -> uploaded primitive index (else empty)
  // primitives in the caller's (reference BVH) order, for the reference-count
  // launch over nodes2 when the render tree is our own (else empty)
  DevBuf<DPrim> prims_ref;
  DevBuf<float> norms_ref;
  DevBuf<float4> env_tex;          // environment map RGB (w*h, .w unused)
  DevBuf<float> env_ptheta, env_pphi, env_pdf;  // EnvironmentLight tables
  DevBuf<EnvRec> env_rtheta, env_rphi;            // their guide tables' bucket records
  int env_w = 0, env_h = 0;
  DevBuf<DPrim> prims;
  DevBuf<float> norms;
  DevBuf<DBsdf> bsdfs;
  DevBuf<DLight> lights;
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
  static constexpr int kSlots = 4;
  static constexpr int kSlotsLarge = 2;
  uint64_t slot_rr = 0;      // launches issued on the pipeline (slot rotation)
  bool small_last = false;   // the previous launch was small: rotate over every slot
  Stream rstream[kSlots];
  Event ev_free[kSlots];
  DevBuf<int4> tiles[kSlots];
  std::vector<PlanRect> tiles_host[kSlots];  // what `tiles` holds
  DevBuf<int4> blocks[kSlots];           // footprint-clipped 8x8 pixel blocks of the tiles
  std::vector<PlanRect> blocks_host[kSlots];
  DevBuf<int> tblock0[kSlots];           // first block of each tile (+ the end), for the resolve
  std::vector<int> tblock0_host[kSlots];
  DevBuf<int> tout[kSlots];              // caller's index of each launched tile (a Z-ordered packed launch)
  std::vector<int> tout_host[kSlots];
  DevBuf<float> partial[kSlots];   // per-slot sample-group sums
  DevBuf<int> spill[kSlots];       // traversal stack entries beyond PT_STACK
  DevBuf<uint32_t> counter[kSlots];
  // the slot's queue heads are known to be zero: the last resolve of the slot
  // reset them (PT_RESOLVE_RESETS), so the next launch needs no memset
  bool counter_clean[kSlots] = {};
  int64_t culled_px = 0;         // pixels of the last launch outside the footprint
  DevBuf<float> frame;  // device framebuffer for host-output renders
  // Asynchronous one-tile seam (pt_tile_submit / pt_tile_finish): submitted
  // tiles wait in `tq` until a batch of `tile_batch` is full, then render as
  // ONE launch into `frame`; the rows the batch spans are copied to the
  // batch's own pinned stage and an event is recorded behind the copy.  A
  // completion thread (`tworker`) waits on that event and completes the
  // batch -- copies its tiles into the caller's sampleBuffer and toColors them
  // into its frameBuffer -- OFF the stream, so the next batch's render never
  // waits for host work (a stream host function would serialise them).
  struct TileJob {
    int4 t;
    float* hdr;
    uint32_t* rgba;
  };
  struct TileBatch {
    std::vector<TileJob> jobs;
    PinnedBuf<float> stage;  // rows y0 .. y0 + rows - 1 of the frame
    int y0 = 0, W = 0, H = 0;
    Event ev;
  };
  std::vector<TileJob> tq;
  int tile_batch = 256;  // tiles per launch (PT_TILE_BATCH): 256 beat 16-128 and 1024 (profiles/r3/seam_native_batch_sweep.txt)
  int fault_tile_launch = 0, n_tile_launches = 0;  // PT_FAULT_TILE_LAUNCH (tests)
  std::mutex tmu;
  std::condition_variable tcv;
  std::deque<std::unique_ptr<TileBatch>> tpending;  // rendered batches awaiting completion, in launch order
  std::vector<std::unique_ptr<TileBatch>> tfree;    // completed batches: stages and events for reuse
  int tinflight = 0;                // batches launched and not yet completed
  int terr = PT_OK;                 // first completion error (reported by pt_tile_finish)
  std::string terrmsg;
  bool tstop = false;
  std::thread tworker;
  DevBuf<int> q_spill;  // ray-query stack spill
  DevBuf<unsigned long long> stats;
  DevBuf<float> q_f;    // ray-query scratch
  DevBuf<int32_t> q_i;
  int n_lights = 0, n_bsdfs = 0;
  int bvh_stack = 0;  // worst-case traversal stack entries of the uploaded BVH
  size_t n_render_nodes = 0;
  size_t n_nodes2 = 0;  // binary nodes in nodes2 (pt_debug_bvh_info)
  int64_t n_prims = 0;
  bool tri_only = false;  // every primitive a triangle
  float root_lo[3] = {0, 0, 0}, root_hi[3] = {0, 0, 0};
  double root_lo_d[3] = {0, 0, 0}, root_hi_d[3] = {0, 0, 0};
  bool have_scene = false, have_cam = false, have_params = false;
  pt_camera cam{};
  pt_params params{};
  pt_stats last{};
  int grid_plain = 0, grid_stats = 0;
  int bpc_plain = 0, bpc_stats = 0, n_cu = 0;
  int bpc_variant[4] = {0, 0, 0, 0};  // plain builds: [env * 2 + gtab] (the common one is bpc_plain)
  std::vector<std::unique_ptr<pt_film>> films;  // films not yet destroyed
  DevBuf<uint32_t> tc_thr;      // pt_to_color_thresholds on the device (uploaded at first use)
  bool tc_thr_ready = false;
  // first-hit feature pass (pt_render_features*): its tile list, stack spill
  // area and the device side of the host entry point's output; a pass that
  // comes on another stream than the last waits for it
  DevBuf<int4> ftiles;
  std::vector<int4> ftiles_host;
  DevBuf<int> f_spill;
  DevBuf<float4> feat_out;
  StreamOrder feat_order;
  DevBuf<float4> dn_a, dn_b;  // pt_denoise_device: the iterations' ping-pong records (grown on demand)
  // reprojection (pt_reproject_device, pt_film_reproject): the uploaded scene's
  // BSDF types, and the keep table on the device with what it holds; a gather
  // that comes on another stream than the last waits for it
  std::vector<int32_t> bsdf_types;
  DevBuf<uint32_t> rp_keep;
  std::vector<uint32_t> rp_keep_host;
  StreamOrder rp_order;
  // Every member frees itself, in reverse order of declaration; only what
  // needs ordering is done here: no kernel and no completion may still be
  // running when the first member goes.  (The completion thread and its
  // batches are declared after `frame`, which they read.)
  ~pt_ctx();
};

// A progressive film (ptgpu.h: pt_film_*; kernels and record layout: film.h).
struct pt_film {
  pt_ctx* ctx = nullptr;
  int W = 0, H = 0;
  DevBuf<uint4> rec;     // 2 * W * H records
  DevBuf<float> pass;    // the pass being added (W * H * 3, the frame layout)
  DevBuf<int4> tiles;    // the last pass's clipped tiles
  std::vector<int4> tiles_host;  // what `tiles` holds
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
  // the last one and the events around its gather kernel
  DevBuf<uint4> rec2;
  DevBuf<float4> feat2;
  DevBuf<unsigned long long> rp_counts;
  Event ev_rp[2];
  bool rp_timed = false;
  uint64_t next = 0;     // next sample index (<= 2^32)
  int64_t passes = 0;
  Event ev_acc[2], ev_res[2];  // around the last accumulate / resolve kernel
  bool acc_timed = false, res_timed = false;
  // the film's last operation: a later one on another stream waits for it
  StreamOrder order;
};

// The stream an entry point runs on: the caller's, or the context's for NULL.
static hipStream_t stream_of(const pt_ctx* c, void* stream) { return stream ? (hipStream_t)stream : (hipStream_t)c->stream; }

extern "C" {

int pt_create(int device, pt_ctx** out) {
  if (!out) return fail(PT_E_INVALID, "pt_create: out is NULL");
  *out = nullptr;
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(PT_E_INVALID, "pt_create: no such HIP device");
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<pt_ctx> c(new pt_ctx());  // (a failure below frees what was acquired so far)
  c->device = device;
  HIPCHK(c->stream.create(hipStreamNonBlocking));
  for (int k = 0; k < pt_ctx::kSlots; ++k) {
    // (slots past the first two get their stream when a small launch first
    // uses them: HIP maps streams onto GPU_MAX_HW_QUEUES hardware queues, 4 by
    // default, and two more streams per context put the render streams of
    // large frames on shared queues -- C3 pipelined -12%)
    if (k < pt_ctx::kSlotsLarge) {
      HIPCHK(make_render_stream(c->rstream[k]));
      HIPCHK(c->ev_free[k].create(hipEventDisableTiming));
      HIPCHK(hipEventRecord(c->ev_free[k], c->stream));
    }
    HIPCHK(c->counter[k].reserve(PT_QUEUE_WORDS * PT_QUEUE_HEADS));  // work-queue heads, one 128-B line each
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
  if (const char* tb = std::getenv("PT_TILE_BATCH")) {  // tuning knob: tiles per asynchronous launch
    int v = std::atoi(tb);
    if (v >= 1) c->tile_batch = v;
  }
  if (const char* f = std::getenv("PT_FAULT_TILE_LAUNCH")) c->fault_tile_launch = std::atoi(f);
  // counters + one trace record per wave of the largest stats grid
  HIPCHK(c->stats.reserve(PT_STATS_SLOTS + (size_t)PT_WAVE_TRACE * std::max(c->grid_stats, 64 * c->n_cu)));
  *out = c.release();
  return PT_OK;
}

pt_ctx::~pt_ctx() {
  (void)hipSetDevice(device);
  (void)hipDeviceSynchronize();  // no render of this context may still be running
  if (tworker.joinable()) {
    {
      std::lock_guard<std::mutex> lk(tmu);
      tstop = true;
    }
    tcv.notify_all();
    tworker.join();  // drains the pending batches first
  }
}

int pt_destroy(pt_ctx* c) {
  if (!c) return PT_OK;
  delete c;
  return PT_OK;
}

// GPU linear-BVH build over the primitives already in c->prims / c->norms
// (CUDAPathTracer::buildBVH, cuda_src/setup.cu:478-686; kernels in lbvh.hip).
static int build_gpu_bvh(pt_ctx* c, const FlatScene& f) {
  LbvhIn in{};
  in.n = (int)f.prims.size();
  in.prims = c->prims.p;
  in.norms = c->norms.p;
  for (int k = 0; k < 3; ++k) {
    in.scene_min[k] = f.scene_min[k];
    in.scene_extent[k] = f.scene_extent[k];
  }
  LbvhOut out{};
  HIPCHK(ptk_build_lbvh(&in, &out, c->stream));
  c->prims.adopt(out.prims, (size_t)in.n);
  c->norms.adopt(out.norms, (size_t)in.n * 9);
  c->prim_map.adopt(out.prim_map, (size_t)in.n);
  c->nodes.adopt(out.nodes4, (size_t)out.n4);
  c->nodes2.adopt(out.nodes2, (size_t)std::max(1, out.n2));
  c->n_nodes2 = (size_t)out.n2;
  c->n_render_nodes = (size_t)out.n4;
  if (out.max_stack > PT_STACK_MAX) return fail_stack_depth("pt_upload_scene_lbvh", out.max_stack);
  c->bvh_stack = out.max_stack;
  for (int k = 0; k < 3; ++k) {
    c->root_lo[k] = out.root_lo[k];
    c->root_hi[k] = out.root_hi[k];
    c->root_lo_d[k] = out.root_lo[k];
    c->root_hi_d[k] = out.root_hi[k];
  }
  return PT_OK;
}

static int tile_launch(pt_ctx* c);

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
  if (int rc = put(c->prims, f.prims)) return rc;
  if (int rc = put(c->norms, f.norms)) return rc;
  HIPCHK(c->bsdfs.reserve(f.bsdfs.size()));
  HIPCHK(c->lights.reserve(std::max<size_t>(1, f.lights.size())));
  c->prim_map.release();
  c->prims_ref.release();
  c->norms_ref.release();
  if (!f.prims_ref.empty()) {
    if (int rc = put(c->prims_ref, f.prims_ref)) return rc;
    if (int rc = put(c->norms_ref, f.norms_ref)) return rc;
  }
  if (knobs.tree == FLATTEN_GPU_TREE) {
    // the reference-count launch walks the caller's tree over a caller-order
    // copy of the primitives
    if (int rc = put(c->prims_ref, f.prims)) return rc;
    if (int rc = put(c->norms_ref, f.norms)) return rc;
    if (int rc = build_gpu_bvh(c, f)) return rc;  // adopts prims/norms/prim_map/nodes in its own order
    if (int rc = put(c->nodes2, f.nodes2)) return rc;
    c->n_nodes2 = f.nodes2.size();
    c->bvh_stack = std::max(c->bvh_stack, f.bvh_stack);
  } else if (knobs.tree == FLATTEN_LBVH_ENTRY) {
    if (int rc = build_gpu_bvh(c, f)) return rc;
  } else {
    if (int rc = put(c->nodes2, f.nodes2)) return rc;
    c->n_nodes2 = f.nodes2.size();
    if (int rc = put(c->nodes, f.nodes4)) return rc;
    if (!f.prim_map.empty())
      if (int rc = put(c->prim_map, f.prim_map)) return rc;
    c->bvh_stack = f.bvh_stack;
    c->n_render_nodes = f.nodes4.size();
    for (int k = 0; k < 3; ++k) {
      c->root_lo[k] = f.root_lo[k];
      c->root_hi[k] = f.root_hi[k];
      c->root_lo_d[k] = f.root_lo_d[k];
      c->root_hi_d[k] = f.root_hi_d[k];
    }
  }
  HIPCHK(hipMemcpy(c->bsdfs.p, f.bsdfs.data(), f.bsdfs.size() * sizeof(DBsdf), hipMemcpyHostToDevice));
  if (!f.lights.empty())
    HIPCHK(hipMemcpy(c->lights.p, f.lights.data(), f.lights.size() * sizeof(DLight), hipMemcpyHostToDevice));
  c->env_w = f.env_w;
  c->env_h = f.env_h;
  if (f.env_w) {
    const EnvTables& env = f.env;
    if (int rc = put(c->env_tex, env.tex)) return rc;
    if (int rc = put(c->env_ptheta, env.p_theta)) return rc;
    if (int rc = put(c->env_pphi, env.p_phi)) return rc;
    if (int rc = put(c->env_pdf, env.p_theta_phi)) return rc;
    if (int rc = put(c->env_rtheta, env.r_theta)) return rc;
    if (int rc = put(c->env_rphi, env.r_phi)) return rc;
  }
  c->n_lights = (int)f.lights.size();
  c->n_bsdfs = (int)f.bsdfs.size();
  c->bsdf_types = f.bsdf_types;
  c->n_prims = s->n_prims;
  c->tri_only = f.tri_only;
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

static int build_tiles(pt_ctx* c, const pt_tile* tiles, int32_t n, std::vector<int4>& out) {
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

// The launch policy's rectangles are the device's int4 (x, y, w, h): tile and
// block lists go to the device, and tile lists into a plan, without conversion.
static_assert(sizeof(PlanRect) == sizeof(int4) && offsetof(PlanRect, x) == offsetof(int4, x) &&
                  offsetof(PlanRect, y) == offsetof(int4, y) && offsetof(PlanRect, w) == offsetof(int4, z) &&
                  offsetof(PlanRect, h) == offsetof(int4, w),
              "PlanRect is laid out as int4");

// What the launch policy (launch_plan.h) reads of the context, for `nf` frames of the tiles `tl`.
static PlanInput plan_input(const pt_ctx* c, const std::vector<int4>& tl, int nf, uint32_t flags, bool gpu_idle,
                            const LaunchKnobs& knobs) {
  PlanInput in;
  in.W = c->params.width;
  in.H = c->params.height;
  in.spp = c->params.spp;
  in.cam = c->cam;
  for (int k = 0; k < 3; ++k) {
    in.box_lo[k] = c->root_lo_d[k];
    in.box_hi[k] = c->root_hi_d[k];
  }
  in.env = c->env_w > 0;
  in.n_bsdfs = c->n_bsdfs;
  in.n_lights = c->n_lights;
  in.n_render_nodes = (int64_t)c->n_render_nodes;
  in.bvh_stack = c->bvh_stack;
  in.tri_only = c->tri_only;
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
  return in;
}

// What the kernels read of the context and of the plan; launch() adds its render slot's buffers.
static KParams kernel_params(const pt_ctx* c, const LaunchPlan& plan, int nf, const uint32_t* seeds, uint32_t flags) {
  KParams P;
  std::memset(&P, 0, sizeof(P));
  for (int k = 0; k < 3; ++k) {
    P.cam_pos[k] = (float)c->cam.pos[k];
    P.c2w_col0[k] = (float)c->cam.c2w[3 * k + 0];
    P.c2w_col1[k] = (float)c->cam.c2w[3 * k + 1];
    P.c2w_col2[k] = (float)c->cam.c2w[3 * k + 2];
    P.root_lo[k] = c->root_lo[k];
    P.root_hi[k] = c->root_hi[k];
  }
  P.cam_ax = (float)(c->cam.screen_w / c->cam.screen_dist);
  P.cam_ay = (float)(c->cam.screen_h / c->cam.screen_dist);
  P.W = c->params.width;
  P.H = c->params.height;
  P.inv_w = 1.0f / (float)P.W;
  P.inv_h = 1.0f / (float)P.H;
  P.spp = c->params.spp;
  P.max_depth = c->params.max_depth;
  P.ns_area = c->params.ns_area_light;
  P.nls_scale = (float)(1.0 / (double)P.ns_area);
  P.seed = seeds ? seeds[0] : c->params.seed;
  P.sample_base = c->params.sample_base;
  P.n_frames = nf;
  for (int f = 0; f < PT_MAX_FRAMES; ++f) P.seeds[f] = seeds && f < nf ? seeds[f] : P.seed;
  P.n_lights = c->n_lights;
  P.n_bsdfs = c->n_bsdfs;
  P.nodes = c->nodes.p;
  P.nodes2 = c->nodes2.p;
  P.prims = c->prims.p;
  P.norms = c->norms.p;
  if ((flags & PT_FLAG_REF_COUNTS) && c->prims_ref.p) {  // nodes2 indexes the caller's order
    P.prims = c->prims_ref.p;
    P.norms = c->norms_ref.p;
  }
  P.bsdfs = c->bsdfs.p;
  P.lights = c->lights.p;
  P.env_w = c->env_w;
  P.env_h = c->env_h;
  P.env_tex = c->env_tex.p;
  P.env_ptheta = c->env_ptheta.p;
  P.env_pphi = c->env_pphi.p;
  P.env_pdf = c->env_pdf.p;
  P.env_rtheta = c->env_rtheta.p;
  P.env_rphi = c->env_rphi.p;
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
static int launch(pt_ctx* c, const std::vector<int4>& tl_in, float* const* outs, int nf, const uint32_t* seeds,
                  hipStream_t s, uint32_t flags) {
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
    if (!c->ev_free[k]) continue;  // (a slot never used)
    const hipError_t q = hipEventQuery(c->ev_free[k]);
    if (q == hipErrorNotReady) {
      (void)hipGetLastError();  // (a not-ready query is no error of this launch)
      gpu_idle = false;
    } else if (q != hipSuccess) {
      return fail(PT_E_HIP, std::string("render: an earlier launch failed: ") + hipGetErrorString(q));
    }
  }
  const LaunchPlan plan = plan_launch(plan_input(c, tl_in, nf, flags, gpu_idle, knobs));
  if (!plan.error.empty()) return fail(PT_E_INVALID, plan.error);
  // PT_PIPELINE=0 and census launches: every render on the caller's stream, one slot
  const bool pipelined = knobs.pipeline && !plan.census;
  const int depth = c->small_last ? pt_ctx::kSlots : pt_ctx::kSlotsLarge;
  const int slot = pipelined ? (int)(c->slot_rr++ % (uint64_t)depth) : 0;
  if (!plan.stats) c->small_last = plan.small;
  const bool idle = pipelined && gpu_idle;
  if (!c->rstream[slot]) {  // a small launch's first use of slots 2 and 3
    HIPCHK(make_render_stream(c->rstream[slot]));
    HIPCHK(c->ev_free[slot].create(hipEventDisableTiming));
    HIPCHK(hipEventRecord(c->ev_free[slot], c->stream));
  }
  hipStream_t rs = pipelined && !idle ? c->rstream[slot] : s;
  // the slot's device state is free once the previous resolve that read it ran
  if (!idle) HIPCHK(hipStreamWaitEvent(rs, c->ev_free[slot], 0));
  const PlanRect* tl = plan.zorder ? plan.ztiles.data() : reinterpret_cast<const PlanRect*>(tl_in.data());
  const bool tile_out = plan.zorder && (flags & (PT_FLAG_PACKED | PT_FLAG_PACKED16));  // packed outputs keep the caller's tile index
  if (int rc = sync_list(c->tiles[slot], c->tiles_host[slot], tl, tl_in.size(), rs)) return rc;
  if (tile_out)
    if (int rc = sync_list(c->tout[slot], c->tout_host[slot], plan.perm.data(), plan.perm.size(), rs)) return rc;
  if (int rc = sync_list(c->blocks[slot], c->blocks_host[slot], plan.blocks.data(), plan.blocks.size(), rs)) return rc;
  if (int rc = sync_list(c->tblock0[slot], c->tblock0_host[slot], plan.tile_block0.data(), plan.tile_block0.size(), rs))
    return rc;
  // Queue heads: zeroed by the slot's previous resolve (a memset in front of the render is a dependent launch of its own, ~20 us
  // before the render kernel starts on a lone frame); a memset only when
  // that did not happen (first use, a launch that failed half-way)
  if (!c->counter_clean[slot])
    HIPCHK(hipMemsetAsync(c->counter[slot].p, 0, PT_QUEUE_WORDS * PT_QUEUE_HEADS * sizeof(uint32_t), rs));
  c->counter_clean[slot] = false;
  if (plan.stats) {
    unsigned long long init[PT_STATS_SLOTS] = {0};
    init[PT_STAT_WAVE_START_MIN] = init[PT_STAT_WAVE_END_MIN] = init[PT_STAT_WAVE_EMPTY_MIN] = ~0ull;  // atomicMin slots
    HIPCHK(hipMemcpyAsync(c->stats.p, init, sizeof(init), hipMemcpyHostToDevice, rs));
    HIPCHK(hipStreamSynchronize(rs));  // `init` is a stack array
  }
  KParams P = kernel_params(c, plan, nf, seeds, flags);
  P.out = outs[0];
  P.work_counter = c->counter[slot].p;
  P.n_tiles = (int)tl_in.size();
  P.tiles = c->tiles[slot].p;
  P.tile_out = tile_out ? c->tout[slot].p : nullptr;
  P.blocks = c->blocks[slot].p;
  P.tile_block0 = c->tblock0[slot].p;
  // (growing a buffer synchronises the device: a frame batch sizes every render slot's at once)
  for (int k = 0; k < pt_ctx::kSlots && nf > 1; ++k) {
    HIPCHK(c->partial[k].reserve(plan.batch_partial_floats));
    if (plan.batch_spill_ints) HIPCHK(c->spill[k].reserve(plan.batch_spill_ints));
  }
  HIPCHK(c->partial[slot].reserve(plan.partial_floats));
  P.partial = c->partial[slot].p;
  if (plan.spill_ints) HIPCHK(c->spill[slot].reserve(plan.spill_ints));
  P.stack_spill = plan.spill_ints ? c->spill[slot].p : nullptr;
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
  c->counter_clean[slot] = true;  // (the resolve zeroed the slot's queue heads)
  HIPCHK(hipEventRecord(c->cur[2], s));
  HIPCHK(hipEventRecord(c->ev_free[slot], s));
  c->census_valid = P.census != 0;
  c->culled_px = plan.culled_px;
  c->last.tile_zorder = plan.zorder ? 1 : 0;
  std::copy(plan.footprint, plan.footprint + 4, c->last.footprint);
  c->last.partial_bytes = plan.slots * PT_SUM_BYTES;
  c->last.grid_blocks = plan.grid;
  c->last.group_spp = plan.group_spp;
  c->last.blocks_per_cu = (int32_t)(plan.want / std::max(1, c->n_cu));
  c->last.pixels = plan.pixels;
  c->last.bvh_stack = c->bvh_stack;
  c->last.bvh_nodes = (int64_t)c->n_render_nodes;
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
static int finish_stats(pt_ctx* c, hipStream_t s, uint32_t flags, bool sync) {
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

static int check_ready(pt_ctx* c) {
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

int pt_render_tiles(pt_ctx* c, const pt_tile* tiles, int32_t n_tiles, float* hdr_out_host, uint32_t flags) {
  int rc = check_ready(c);
  if (rc) return rc;
  if ((rc = tile_launch(c))) return rc;  // earlier asynchronous tiles first (call order)
  if (n_tiles < 0 || (n_tiles > 0 && (!tiles || !hdr_out_host))) return fail(PT_E_INVALID, "pt_render_tiles: bad args");
  if (flags & (PT_FLAG_PACKED | PT_FLAG_PACKED16))
    return fail(PT_E_INVALID, "pt_render_tiles: packed output is for pt_render_tiles_device");
  HIPCHK(hipSetDevice(c->device));
  std::vector<int4> tl;
  if ((rc = build_tiles(c, tiles, n_tiles, tl))) return rc;
  const size_t W = (size_t)c->params.width, H = (size_t)c->params.height;
  HIPCHK(c->frame.reserve(W * H * 3));
  float* fr = c->frame.p;
  if ((rc = launch(c, tl, &fr, 1, nullptr, c->stream, flags))) return rc;
  // Copy back only the tiles' pixels (the caller's buffer is theirs outside
  // them); a call whose (clipped, disjoint) tiles cover the whole frame - the
  // whole-frame batch - is one contiguous copy.
  int64_t area = 0;
  for (const int4& t : tl) area += (int64_t)t.z * t.w;
  if (area == (int64_t)(W * H) && tiles_disjoint(tl, W, H)) {
    HIPCHK(hipMemcpyAsync(hdr_out_host, c->frame.p, W * H * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  } else {
    for (const int4& t : tl) {
      size_t off = ((size_t)t.y * W + (size_t)t.x) * 3;
      HIPCHK(hipMemcpy2DAsync(hdr_out_host + off, W * 3 * sizeof(float), c->frame.p + off, W * 3 * sizeof(float),
                              (size_t)t.z * 3 * sizeof(float), (size_t)t.w, hipMemcpyDeviceToHost, c->stream));
    }
  }
  return finish_stats(c, c->stream, flags, true);
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
  int rc = check_ready(c);
  if (rc) return rc;
  if ((rc = tile_launch(c))) return rc;
  if (n_tiles < 0 || (n_tiles > 0 && (!tiles || !hdr_out_dev)))
    return fail(PT_E_INVALID, "pt_render_tiles_device: bad args");
  HIPCHK(hipSetDevice(c->device));
  std::vector<int4> tl;
  if ((rc = build_tiles(c, tiles, n_tiles, tl))) return rc;
  if (int rc2 = check_packed(c, tiles, n_tiles, flags, "pt_render_tiles_device")) return rc2;
  hipStream_t s = stream_of(c, stream);
  if ((rc = launch(c, tl, &hdr_out_dev, 1, nullptr, s, flags))) return rc;
  return finish_stats(c, s, flags, false);
}

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
  for (Event* e : {&f->ev_acc[0], &f->ev_acc[1], &f->ev_res[0], &f->ev_res[1]}) HIPCHK(e->create());
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

int pt_film_add_pass(pt_film* f, const pt_tile* tiles, int32_t n_tiles, void* stream) {
  if (!f) return fail(PT_E_INVALID, "pt_film_add_pass: NULL film");
  pt_ctx* c = f->ctx;
  int rc = check_ready(c);
  if (rc) return rc;
  if (n_tiles < 0 || (n_tiles > 0 && !tiles)) return fail(PT_E_INVALID, "pt_film_add_pass: bad args");
  const pt_params& P = c->params;
  if (P.width != f->W || P.height != f->H)
    return fail(PT_E_INVALID, "pt_film_add_pass: pt_params frame " + std::to_string(P.width) + " x " +
                                  std::to_string(P.height) + " differs from the film's " + std::to_string(f->W) + " x " +
                                  std::to_string(f->H));
  if (f->next + (uint64_t)P.spp > (uint64_t)1 << 32)
    return fail(PT_E_INVALID, "pt_film_add_pass: sample range overflow (next sample " + std::to_string(f->next) +
                                  " + spp " + std::to_string(P.spp) + " > 2^32)");
  std::vector<int4> rects;
  for (int32_t i = 0; i < n_tiles; ++i) {
    const pt_tile& t = tiles[i];
    if (t.w < 0 || t.h < 0) return fail(PT_E_INVALID, "pt_film_add_pass: negative tile size");
    const int x0 = std::max(0, t.x), y0 = std::max(0, t.y);
    const int x1 = (int)std::min<int64_t>(f->W, (int64_t)t.x + t.w), y1 = (int)std::min<int64_t>(f->H, (int64_t)t.y + t.h);
    if (x1 > x0 && y1 > y0) rects.push_back(make_int4(x0, y0, x1, y1));
  }
  if (!rects_disjoint(rects))
    return fail(PT_E_INVALID, "pt_film_add_pass: tiles overlap (their samples would be counted twice)");
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
  rc = launch(c, tl, &pass, 1, nullptr, s, 0);
  c->params.sample_base = base;
  if (rc) return rc;
  if ((rc = finish_stats(c, s, 0, false))) return rc;
  if (!tl.empty()) {
    if ((rc = sync_list(f->tiles, f->tiles_host, tl.data(), tl.size(), s, true))) return rc;
    FilmAccArgs a;
    a.tiles = f->tiles.p;
    a.rec = f->rec.p;
    a.pass = f->pass.p;
    a.W = f->W;
    a.H = f->H;
    a.spp = (uint32_t)P.spp;
    HIPCHK(hipEventRecord(f->ev_acc[0], s));
    HIPCHK(ptk_film_accumulate(&a, (int)tl.size(), s));
    HIPCHK(hipEventRecord(f->ev_acc[1], s));
    f->acc_timed = true;
  }
  f->next += (uint64_t)P.spp;
  ++f->passes;
  HIPCHK(f->order.end(s));
  return PT_OK;
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
  HIPCHK(hipEventRecord(f->ev_res[0], s));
  HIPCHK(ptk_film_resolve(&a, s));
  HIPCHK(hipEventRecord(f->ev_res[1], s));
  f->res_timed = true;
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
  float ms = 0.f;
  if (f->acc_timed) {
    HIPCHK(hipEventSynchronize(f->ev_acc[1]));
    HIPCHK(hipEventElapsedTime(&ms, f->ev_acc[0], f->ev_acc[1]));
    out->accumulate_ms = ms;
  }
  if (f->res_timed) {
    HIPCHK(hipEventSynchronize(f->ev_res[1]));
    HIPCHK(hipEventElapsedTime(&ms, f->ev_res[0], f->ev_res[1]));
    out->resolve_ms = ms;
  }
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
  if (int rc = sync_list(c->ftiles, c->ftiles_host, tl.data(), tl.size(), s)) return rc;
  FeatArgs A;
  std::memset(&A, 0, sizeof(A));
  for (int k = 0; k < 3; ++k) {
    A.cam_pos[k] = (float)c->cam.pos[k];
    A.c2w_col0[k] = (float)c->cam.c2w[3 * k + 0];
    A.c2w_col1[k] = (float)c->cam.c2w[3 * k + 1];
    A.c2w_col2[k] = (float)c->cam.c2w[3 * k + 2];
  }
  A.cam_ax = (float)(c->cam.screen_w / c->cam.screen_dist);
  A.cam_ay = (float)(c->cam.screen_h / c->cam.screen_dist);
  A.W = c->params.width;
  A.H = c->params.height;
  A.inv_w = 1.0f / (float)A.W;
  A.inv_h = 1.0f / (float)A.H;
  A.nodes = c->nodes.p;
  A.prims = c->prims.p;
  A.norms = c->norms.p;
  A.tiles = c->ftiles.p;
  A.feat = feat;
  if (c->bvh_stack > PT_STACK) {
    HIPCHK(c->f_spill.reserve((size_t)(c->bvh_stack - PT_STACK) * tl.size() * 16 * PT_BLOCK));
    A.stack_spill = c->f_spill.p;
  }
  HIPCHK(ptk_launch_features(&A, (int)tl.size(), s));
  HIPCHK(c->feat_order.end(s));
  return PT_OK;
}

int pt_render_features_device(pt_ctx* c, const pt_tile* tiles, int32_t n_tiles, void* feat_dev, void* stream) {
  int rc = check_ready(c);
  if (rc) return rc;
  if ((rc = tile_launch(c))) return rc;
  if (n_tiles < 0 || (n_tiles > 0 && (!tiles || !feat_dev)))
    return fail(PT_E_INVALID, "pt_render_features_device: bad args");
  HIPCHK(hipSetDevice(c->device));
  std::vector<int4> tl;
  if ((rc = build_tiles(c, tiles, n_tiles, tl))) return rc;
  return features_launch(c, tl, (float4*)feat_dev, stream_of(c, stream));
}

int pt_render_features(pt_ctx* c, const pt_tile* tiles, int32_t n_tiles, void* feat_host) {
  int rc = check_ready(c);
  if (rc) return rc;
  if ((rc = tile_launch(c))) return rc;
  if (n_tiles < 0 || (n_tiles > 0 && (!tiles || !feat_host))) return fail(PT_E_INVALID, "pt_render_features: bad args");
  HIPCHK(hipSetDevice(c->device));
  std::vector<int4> tl;
  if ((rc = build_tiles(c, tiles, n_tiles, tl))) return rc;
  const size_t W = (size_t)c->params.width, H = (size_t)c->params.height;
  HIPCHK(c->feat_out.reserve(2 * W * H));
  if ((rc = features_launch(c, tl, c->feat_out.p, c->stream))) return rc;
  // only the tiles' records go back: the caller's buffer is theirs outside them
  for (const int4& t : tl)
    for (size_t plane = 0; plane < 2; ++plane) {
      const size_t off = plane * W * H + (size_t)t.y * W + (size_t)t.x;
      HIPCHK(hipMemcpy2DAsync((float4*)feat_host + off, W * sizeof(float4), c->feat_out.p + off, W * sizeof(float4),
                              (size_t)t.z * sizeof(float4), (size_t)t.w, hipMemcpyDeviceToHost, c->stream));
    }
  HIPCHK(hipStreamSynchronize(c->stream));
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
// changed), the counts zeroed when wanted, the kernel, between ev[0] and ev[1]
// when given.
static int reproject_launch(pt_ctx* c, const pt_camera& old_cam, const uint4* rec, const float4* fo, const float4* fn,
                            int W, int H, const int32_t* types, int n_types, const pt_reproject_params& prm, uint4* out,
                            unsigned long long* counts, const Event* ev, hipStream_t s) {
  std::vector<uint32_t> keep((size_t)n_types);
  reproject_keep_table(types, n_types, keep.data());
  HIPCHK(c->rp_order.begin(s));
  if (int rc = sync_list(c->rp_keep, c->rp_keep_host, keep.data(), keep.size(), s)) return rc;
  ReprojectArgs a;
  std::memset(&a, 0, sizeof(a));
  a.rec = rec;
  a.fo = fo;
  a.fn = fn;
  a.keep = c->rp_keep.p;
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
  if (ev) HIPCHK(hipEventRecord(ev[0], s));
  HIPCHK(ptk_reproject(&a, s));
  if (ev) HIPCHK(hipEventRecord(ev[1], s));
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
    bsdf_types_host = c->bsdf_types.data();
    n_bsdfs = (int32_t)c->bsdf_types.size();
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
  for (Event& e : f->ev_rp) HIPCHK(e.create());
  hipStream_t s = stream_of(c, stream);
  HIPCHK(f->order.begin(s));
  if ((rc = features_launch(c, tl, f->feat2.p, s))) return rc;  // (the whole frame: every record is written)
  if ((rc = reproject_launch(c, f->feat_cam, f->rec.p, f->feat.p, f->feat2.p, f->W, f->H, c->bsdf_types.data(),
                             (int)c->bsdf_types.size(), prm, f->rec2.p, f->rp_counts.p, f->ev_rp, s)))
    return rc;
  f->rp_timed = true;
  std::swap(f->rec, f->rec2);
  std::swap(f->feat, f->feat2);
  f->feat_cam = c->cam;
  HIPCHK(f->order.end(s));
  return PT_OK;
}

int pt_film_get_reproject_info(pt_film* f, pt_reproject_info* out) {
  if (!f || !out) return fail(PT_E_INVALID, "pt_film_get_reproject_info: NULL argument");
  std::memset(out, 0, sizeof(*out));
  if (!f->rp_timed) return PT_OK;
  HIPCHK(hipSetDevice(f->ctx->device));
  HIPCHK(hipEventSynchronize(f->ev_rp[1]));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, f->ev_rp[0], f->ev_rp[1]));
  unsigned long long n[2] = {0, 0};
  HIPCHK(hipMemcpy(n, f->rp_counts.p, sizeof(n), hipMemcpyDeviceToHost));
  out->kept = (int64_t)n[0];
  out->reset = (int64_t)n[1];
  out->reproject_ms = ms;
  return PT_OK;
}

int pt_render_frames_device(pt_ctx* c, const pt_tile* tiles, int32_t n_tiles, int32_t n_frames, const uint32_t* seeds,
                            float* const* hdr_outs_dev, void* stream, uint32_t flags) {
  int rc = check_ready(c);
  if (rc) return rc;
  if ((rc = tile_launch(c))) return rc;
  if (n_frames < 1 || n_frames > PT_MAX_FRAMES || !seeds || !hdr_outs_dev || n_tiles < 0 || (n_tiles > 0 && !tiles))
    return fail(PT_E_INVALID, "pt_render_frames_device: bad args (1 <= n_frames <= PT_MAX_FRAMES, seeds and outputs)");
  for (int32_t f = 0; f < n_frames; ++f)
    if (n_tiles > 0 && !hdr_outs_dev[f]) return fail(PT_E_INVALID, "pt_render_frames_device: NULL output");
  if (flags & (PT_FLAG_STATS | PT_FLAG_REF_COUNTS))
    return fail(PT_E_INVALID, "pt_render_frames_device: counters are per frame (pt_render_tiles_device)");
  HIPCHK(hipSetDevice(c->device));
  std::vector<int4> tl;
  if ((rc = build_tiles(c, tiles, n_tiles, tl))) return rc;
  if (int rc2 = check_packed(c, tiles, n_tiles, flags, "pt_render_frames_device")) return rc2;
  hipStream_t s = stream_of(c, stream);
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

// ---- asynchronous one-tile seam
// Completion of one batch (on the completion thread, after the batch's event):
// the tiles' pixels go from the batch's stage into the caller's sampleBuffer
// and, as PathTracer::raytrace_tile does at its end (pathtracer.cpp:610),
// through toColor into its frameBuffer.
static void tile_complete(const pt_ctx::TileBatch* b) {
  for (const pt_ctx::TileJob& j : b->jobs) {
    for (int y = j.t.y; y < j.t.y + j.t.w; ++y) {
      const size_t dst = ((size_t)y * (size_t)b->W + (size_t)j.t.x) * 3;
      const size_t src = ((size_t)(y - b->y0) * (size_t)b->W + (size_t)j.t.x) * 3;
      std::memcpy(j.hdr + dst, b->stage.p + src, (size_t)j.t.z * 3 * sizeof(float));
    }
    if (j.rgba) (void)pt_to_color(j.hdr, b->W, b->H, j.t.x, j.t.y, j.t.x + j.t.z, j.t.y + j.t.w, j.rgba);
  }
}

// The completion thread: batches in launch order; each waits for its own
// event only, so completing batch k overlaps the render of batch k+1.
static void tile_worker(pt_ctx* c) {
  (void)hipSetDevice(c->device);
  for (;;) {
    std::unique_ptr<pt_ctx::TileBatch> b;
    {
      std::unique_lock<std::mutex> lk(c->tmu);
      c->tcv.wait(lk, [&] { return c->tstop || !c->tpending.empty(); });
      if (c->tpending.empty()) return;  // stopping, nothing left to complete
      b = std::move(c->tpending.front());
      c->tpending.pop_front();
    }
    const hipError_t e = hipEventSynchronize(b->ev);
    if (e == hipSuccess) tile_complete(b.get());
    std::lock_guard<std::mutex> lk(c->tmu);
    if (e != hipSuccess && c->terr == PT_OK) {
      c->terr = PT_E_HIP;
      c->terrmsg = std::string("tile completion: ") + hipGetErrorString(e);
    }
    b->jobs.clear();
    c->tfree.push_back(std::move(b));
    --c->tinflight;
    c->tcv.notify_all();
  }
}

// A batch that could not be launched: its tiles are dropped, so the failure is
// also kept for the next pt_tile_finish (which would otherwise report PT_OK for
// tiles it never rendered), whoever called tile_launch.
static int tile_launch_failed(pt_ctx* c, int rc) {
  std::lock_guard<std::mutex> lk(c->tmu);
  if (c->terr == PT_OK) {
    c->terr = rc;
    c->terrmsg = std::string("tile launch: ") + pt_last_error();
  }
  return rc;
}

// Fault injection for the seam's error path (tests): PT_FAULT_TILE_LAUNCH=k
// at pt_create makes the context's k-th batch launch fail before it renders.
static bool tile_fault_injected(pt_ctx* c) {
  return c->fault_tile_launch > 0 && ++c->n_tile_launches == c->fault_tile_launch;
}

static int tile_launch_impl(pt_ctx* c);

// Renders the queued tiles as one launch (nothing queued: nothing to do).
static int tile_launch(pt_ctx* c) {
  if (!c || c->tq.empty()) return PT_OK;
  const int rc = tile_launch_impl(c);
  return rc ? tile_launch_failed(c, rc) : PT_OK;
}

static int tile_launch_impl(pt_ctx* c) {
  constexpr int kMaxBatchesInFlight = 8;  // bounds the pinned staging memory
  std::vector<pt_ctx::TileJob> jobs;
  jobs.swap(c->tq);
  if (tile_fault_injected(c)) return fail(PT_E_HIP, "pt_tile_submit: injected launch failure (PT_FAULT_TILE_LAUNCH)");
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
  std::unique_ptr<pt_ctx::TileBatch> b;
  {
    std::unique_lock<std::mutex> lk(c->tmu);
    if (!c->tworker.joinable()) {
      c->tstop = false;
      c->tworker = std::thread(tile_worker, c);
    }
    c->tcv.wait(lk, [&] { return !c->tfree.empty() || c->tinflight < kMaxBatchesInFlight; });
    if (!c->tfree.empty()) {
      b = std::move(c->tfree.back());
      c->tfree.pop_back();
    }
  }
  if (!b) b.reset(new pt_ctx::TileBatch());
  // a batch that is not launched (any return before it is pending) goes back for reuse
  struct GiveBack {
    pt_ctx* c;
    std::unique_ptr<pt_ctx::TileBatch>& b;
    ~GiveBack() {
      if (!b) return;
      std::lock_guard<std::mutex> lk(c->tmu);
      c->tfree.push_back(std::move(b));
    }
  } give_back{c, b};
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
  {
    std::lock_guard<std::mutex> lk(c->tmu);
    c->tpending.push_back(std::move(b));
    ++c->tinflight;
  }
  c->tcv.notify_all();
  return finish_stats(c, c->stream, 0, false);
}

int pt_tile_submit(pt_ctx* c, const pt_tile* tile, float* hdr_out_host, uint32_t* rgba_out_host) {
  int rc = check_ready(c);
  if (rc) return rc;
  if (!tile || !hdr_out_host) return fail(PT_E_INVALID, "pt_tile_submit: NULL tile or output");
  std::vector<int4> tl;
  if ((rc = build_tiles(c, tile, 1, tl))) return rc;  // clamped to the frame, <= 32 x 32 pieces
  for (const int4& t : tl) c->tq.push_back(pt_ctx::TileJob{t, hdr_out_host, rgba_out_host});
  if ((int)c->tq.size() >= c->tile_batch) return tile_launch(c);
  return PT_OK;
}

int pt_tile_finish(pt_ctx* c) {
  if (!c) return fail(PT_E_INVALID, "NULL context");
  // Whatever happens to the last launch, every batch already in flight is
  // waited for: the completion thread writes into the caller's buffers, which
  // the caller may free or reuse as soon as this returns.
  (void)tile_launch(c);  // (a failure is recorded in terr)
  int err = PT_OK;
  std::string msg;
  {
    std::unique_lock<std::mutex> lk(c->tmu);
    c->tcv.wait(lk, [&] { return c->tinflight == 0; });  // every batch copied and completed
    err = c->terr;
    msg = c->terrmsg;
    c->terr = PT_OK;
    c->terrmsg.clear();
  }
  if (err != PT_OK) return fail(err, msg);
  return PT_OK;
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
  if (c->bvh_stack > PT_STACK) {
    HIPCHK(c->q_spill.reserve((size_t)(c->bvh_stack - PT_STACK) * (size_t)((n + PT_BLOCK - 1) / PT_BLOCK * PT_BLOCK)));
    spill = c->q_spill.p;
  }
  HIPCHK(ptk_launch_intersect(c->nodes.p, c->prims.p, c->q_f.p, c->q_f.p + 3 * n, c->q_f.p + 6 * n, n, dh, dt, dp, da,
                              spill, c->prim_map.p, c->stream));
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
  *out = pt_bvh_info{};
  out->n_prims = c->n_prims;
  out->n_nodes4 = (int64_t)c->n_render_nodes;
  out->n_nodes2 = (int64_t)c->n_nodes2;
  out->bvh_stack = c->bvh_stack;
  out->has_prim_map = c->prim_map.p ? 1 : 0;
  for (int k = 0; k < 3; ++k) {
    out->root_lo[k] = c->root_lo[k];
    out->root_hi[k] = c->root_hi[k];
  }
  return PT_OK;
}

int pt_debug_read_bvh(pt_ctx* c, void* nodes4, void* nodes2, void* prims, float* norms, int32_t* prim_map) {
  if (!c) return fail(PT_E_INVALID, "NULL context");
  if (!c->have_scene) return fail(PT_E_NOSCENE, "pt_debug_read_bvh before pt_upload_scene");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  const size_t n = (size_t)c->n_prims;
  if (nodes4) HIPCHK(hipMemcpy(nodes4, c->nodes.p, c->n_render_nodes * sizeof(DNode), hipMemcpyDeviceToHost));
  if (nodes2 && c->n_nodes2) HIPCHK(hipMemcpy(nodes2, c->nodes2.p, c->n_nodes2 * sizeof(DNode2), hipMemcpyDeviceToHost));
  if (prims) HIPCHK(hipMemcpy(prims, c->prims.p, n * sizeof(DPrim), hipMemcpyDeviceToHost));
  if (norms) HIPCHK(hipMemcpy(norms, c->norms.p, n * 9 * sizeof(float), hipMemcpyDeviceToHost));
  if (prim_map && c->prim_map.p) HIPCHK(hipMemcpy(prim_map, c->prim_map.p, n * sizeof(int32_t), hipMemcpyDeviceToHost));
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

}  // extern "C"
