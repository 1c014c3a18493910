// pt_device.h — device-side data layout of the HIP path (shared by the kernels
// and the host upload in pt_api.cpp; the records themselves are in pt_records.h).
// See DESIGN.md "Data layout in HBM".
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pt_tuning.h"  // tuning constants, launch-counter slots, pt_fastdiv_init (HIP-free)
#include "pt_records.h"  // EnvRec, DNode, DNode2, DPrim, DBsdf, DLight, PT_ENV_GUIDE

// lower_bound of v = r * a[n-1] accelerated by a guide table g[0..G] with
// g[k] = lower_bound(a, k/G * a[n-1]) (built on the host, clamped to n-1): the
// answer lies in [g[k-1], g[k+2]] for k = floor(r*G), one bucket of slack
// either side for rounding, and a[g[k+2]] >= v; the result is exactly
// std::lower_bound's.  With PT_ENV_GUIDE buckets the window is a few entries
// where the CDF carries mass (where samples land).  Bucket k's record (EnvRec)
// holds the window and its values, so the usual short window (<= 4 entries)
// costs ONE memory round trip -- two 16-B loads of one 32-B record -- and
// lower_bound = lo + #{entries < v} (the array is sorted); the caller's
// interpolation pair (prev = a[t-1] or 0, cur = a[t]) comes from the same
// registers.  A longer window -- where the CDF is nearly flat (dim regions of
// a peaky map) or the map is wider than the guide table (w > PT_ENV_GUIDE:
// several entries per bucket) -- is halved on the array down to <= 4 entries
// (answer in [lo, lo + n]) and its five values re-read.  (Guide table, then
// window: two dependent round trips, C5 -1.9%: profiles/r4/ab_env_records.txt.)
// Host and device: pt_env_search_check (pt_api.cpp) replays it against
// std::lower_bound on the host (tests/test_env_search.py).
__host__ __device__ inline int record_lower_bound(const float* __restrict__ a, float v, float r,
                                                  const EnvRec* __restrict__ rec, int G, float& prev, float& cur) {
  int k = (int)(r * (float)G);
  k = k < 0 ? 0 : k > G - 1 ? G - 1 : k;
#if defined(__HIP_DEVICE_COMPILE__)
  // the record as two 16-B vector loads, both issued before the window test:
  // read through a 32-B struct copy, the compiler loads (lo, hi, wm) first and
  // sinks the w_i loads behind the branch -- a second dependent round trip
  // (C5 -1.5%, round 5)
  typedef float rf4 __attribute__((ext_vector_type(4)));
  const rf4 q0 = ((const rf4*)(rec + k))[0];
  rf4 q1 = ((const rf4*)(rec + k))[1];
  asm volatile("" : "+v"(q1));
  int lo = __float_as_int(q0.x);
  const int hi = __float_as_int(q0.y);
  float wm = q0.z, w0 = q0.w, w1 = q1.x, w2 = q1.y, w3 = q1.z, w4 = q1.w;
#else
  // host replay: one 32-B copy of the record.  (Bit-casting the int fields
  // out of float4 elements misread the window in host code -- clang's
  // __builtin_bit_cast of a vector element returns element 0 there -- which
  // the host replay caught.)
  EnvRec e;
  __builtin_memcpy(&e, rec + k, sizeof(EnvRec));
  int lo = e.lo;
  const int hi = e.hi;
  float wm = e.wm, w0 = e.w0, w1 = e.w1, w2 = e.w2, w3 = e.w3, w4 = e.w4;
#endif
  int n = hi - lo;
  if (n > 4) {
    while (n > 4) {
      const int half = n >> 1;
      if (a[lo + half] < v) {
        lo += half + 1;
        n -= half + 1;
      } else {
        n = half;
      }
    }
    auto at = [&](int i) { return a[i < hi ? i : hi]; };
    wm = lo > 0 ? a[lo - 1] : 0.0f;
    w0 = at(lo), w1 = at(lo + 1), w2 = at(lo + 2), w3 = at(lo + 3);
    w4 = at(lo + 4);  // (the record's w4 is a[hi] of the WHOLE window: ADVICE r4)
  }
  const int c = (int)(w0 < v) + (int)(w1 < v) + (int)(w2 < v) + (int)(w3 < v);
  cur = c == 0 ? w0 : c == 1 ? w1 : c == 2 ? w2 : c == 3 ? w3 : w4;
  prev = c == 0 ? wm : c == 1 ? w0 : c == 2 ? w1 : c == 3 ? w2 : w3;
  return lo + c;
}
// The drain fields of the census of plain launches (tools/wave_trace.py
// --census) are compiled in only with -DPT_CENSUS=1 (PT_HIPCC_FLAGS): their
// bookkeeping in the persistent loop cost C3 2% even when off
// (profiles/r4/census_drain.txt).
#ifndef PT_CENSUS
#define PT_CENSUS 0
#endif

struct KParams {
  float cam_pos[3];
  float c2w_col0[3], c2w_col1[3], c2w_col2[3];
  float cam_ax, cam_ay;  // screenW/screenDist, screenH/screenDist
  int W, H, spp, max_depth, ns_area;
  float nls_scale;     // (float)(1.0 / ns_area): an area light sample's weight (pathtracer.cpp:481)
  float inv_w, inv_h;  // 1/W, 1/H
  uint32_t seed;
  uint32_t sample_base;  // first sample index of the pass (RNG keys)
  int n_lights;
  int n_bsdfs;
  int n_tiles;     // 32x32 (or smaller) tiles: 1024 pixels each
  // Sample groups (work slots) of a pixel, a function of the frame only
  // (launch_plan.cpp group_size): group j holds samples
  // [j * group_spp, min((j + 1) * group_spp, spp)).
  int group_spp;   // samples per work slot
  int group_shift;   // log2(group_spp) when a power of two, else -1 (shifts instead of divisions)
  int n_groups;    // ceil(spp / group_spp): work slots per pixel
  // Work slot / group-sum index of (block b, pixel q of the 8x8 block, group
  // j): (b * 64 + q) * n_groups + j -- a pixel's groups are consecutive, so a
  // wave's lanes hold a few pixels' groups (coherent camera rays).
  uint32_t grp_m, grp_sh;           // fastdiv by n_groups (pt_fastdiv)
  int sblocks;                      // every chunk lies in one block (64 * n_groups a multiple of chunk): scalar block loads
  int chunk;                        // slots per queue claim (PT_CHUNK or PT_CHUNK_MAX), a multiple of 64
  const int* tile_block0;           // first block of each tile (n_tiles + 1 entries), for the resolve
  const DNode* nodes;     // the render tree (BVH4)
  const DNode2* nodes2;  // the binary tree (reference-count launch only)
  const DPrim* prims;
  const float* norms;  // 9 floats per primitive (vertex normals n1,n2,n3)
  const DBsdf* bsdfs;
  const DLight* lights;
  int env_w, env_h;          // environment map size (0: no environment light)
  const float4* env_tex;     // map RGB, row 0 = +y
  const float* env_ptheta;   // EnvironmentLight::pTheta (running sums over rows)
  const float* env_pphi;     // pPhiGivenTheta (running sums within each row)
  const float* env_pdf;      // pThetaPhi
  const struct EnvRec* env_rtheta;  // bucket records of env_ptheta (PT_ENV_GUIDE)
  const struct EnvRec* env_rphi;    // bucket records of the rows of env_pphi (h x PT_ENV_GUIDE)
  const int4* tiles;  // (x, y, w, h)
  const int* tile_out;  // packed slot of launched tile i (the caller's index; null: i) -- a Z-ordered launch
  float* out;         // W*H*3, or n_tiles*1024*3 when packed
  int packed;         // packed slot edge S (PT_FLAG_PACKED: 32, PT_FLAG_PACKED16: 16; 0: the frame):
                      // tile i's pixel (x, y) -> out[3 * (i*S*S + (y-ty)*S + (x-tx))]
  float* partial;     // 3 floats per work slot: each sample group's sum, resolved into `out` in group order
  const int4* blocks;  // (x, y, w<=8, h<=8): footprint-clipped pixel blocks of the tiles
  int n_blocks;
  uint32_t* work_counter;
  unsigned long long* stats;  // counters (PT_FLAG_STATS / PT_FLAG_REF_COUNTS)
  int* stack_spill;           // traversal stack entries beyond PT_STACK (null if the BVH never needs them)
  int dbg_pix;                // diagnostic printf trace of one pixel (-1: off)
  int shade_batch;            // leave the traversal phase once this many lanes finished their ray
  int leaf_weight;            // leaf steps run when leaf_weight * leaf lanes >= 16 * node lanes
  int drain_div;              // queue drained: shade once alive/drain_div lanes are ready (0: 3/4 rule)
  int tri_only;               // every primitive is a triangle: the kernel without the sphere test
  int helpers;                // drain helpers on (PT_HELPERS; PT_NO_HELPERS turns them off per launch)
  int qbands;                 // queue heads deal contiguous bands, not interleaved chunks (large frames)
  int census;                 // plain build: record each wave's start / end / CU / drain in the trace area (PT_CENSUS)
  float root_lo[3], root_hi[3];  // scene bounds (root box, rounded outward)
  int cull_x0, cull_y0, cull_x1, cull_y1;  // pixels outside [x0,x1]x[y0,y1] see no geometry
  // Frame batch (pt_render_frames_device, the MF kernel): n_frames frames of
  // the same tiles in one launch.  Work slot g is slot g - f * frame_slots of
  // frame f = g / frame_slots; frame f keys its samples with seeds[f] and its
  // group sums follow frame f - 1's (partial + 3 * g).  One frame: unused.
  int n_frames;
  uint32_t frame_slots;
  uint32_t frm_m, frm_sh;  // fastdiv by frame_slots
  uint32_t seeds[PT_MAX_FRAMES];
  // Ray launch (pt_render_rays*, the RAYS kernel; appended, so that every
  // field above keeps its offset): W * H rays of two float4 in trace_kernel's
  // layout, ray p = x + y * W at rays[2p].  Replay: every sample of pixel p
  // follows ray p.  Capture (rays_capture != 0, spp 1): the camera ray of each
  // sample is generated as ever and stored there.  Other launches: unused.
  float4* rays;
  int rays_capture;
};

// pt_tuning.h pt_fastdiv_init's division, on the device
__device__ __forceinline__ uint32_t pt_fastdiv(uint32_t u, uint32_t m, uint32_t sh) {
  return m ? __umulhi(u, m) >> sh : u >> sh;
}

// GPU BVH build (lbvh.hip).  Inputs in upload order; outputs allocated by
// the builder and handed out on success only (the caller adopts them into
// DevBufs, hip_owned.h); after a failure `out` holds nothing.
struct LbvhIn {
  int n;
  const DPrim* prims;    // device, input order
  const float* norms;    // device, 9 per primitive
  float scene_min[3], scene_extent[3];  // scene box (rounded outward)
};
struct LbvhOut {
  DPrim* prims;          // sorted order
  float* norms;
  int* prim_map;         // sorted index -> input index
  DNode* nodes4;
  int n4;
  DNode2* nodes2;
  int n2;
  int max_stack;         // worst-case traversal stack of nodes4
  float root_lo[3], root_hi[3];
};
extern "C" hipError_t ptk_build_lbvh(const LbvhIn* in, LbvhOut* out, hipStream_t s);

extern "C" hipError_t ptk_launch_render(const KParams* P, int grid, bool stats, bool ref_counts, hipStream_t s);
extern "C" hipError_t ptk_launch_resolve(const KParams* P, hipStream_t s);
extern "C" hipError_t ptk_launch_intersect(const DNode* nodes, const DPrim* prims, const float* o, const float* d,
                                           const float* maxt, int64_t n, int32_t* hit, float* t, int32_t* prim,
                                           int32_t* anyhit, int* spill, const int* prim_map, hipStream_t s);
extern "C" hipError_t ptk_render_occupancy(int* waves_per_cu, bool stats, bool env, bool gtab);
extern "C" hipError_t ptk_render_occupancy_rays(int* waves_per_cu, bool env, bool gtab);  // the RAYS builds (P->rays set)

// Environment-light probe (env_probe_kernel; ptgpu.h pt_debug_env_probe): the
// env_* fields as KParams names them -- env_sample, env_uv and env_dir are
// templates over the parameter struct -- and the queries.  One lane per query.
struct EnvProbe {
  int env_w, env_h;
  const float4* env_tex;
  const float* env_ptheta;
  const float* env_pphi;
  const float* env_pdf;
  const struct EnvRec* env_rtheta;
  const struct EnvRec* env_rphi;
  int n;           // sample queries
  const float* u;  // u1[n], then u2[n], each in [0, 1)
  int32_t* idx;    // row[n], col[n]
  // prev / cur of the row search (2n, interleaved), of the column search (2n),
  // wi (3n), pdf (n), tu (n), tv (n), env_uv(tu, tv) (3n): 13n floats
  float* out;
  int m;           // direction queries
  const float* d;  // 3m, finite and of unit length
  float* rad;      // env_dir(d): 3m
};
extern "C" hipError_t ptk_launch_env_probe(const EnvProbe* a, hipStream_t s);

// First-hit feature pass (features_kernel; ptgpu.h pt_render_features_device):
// the camera as KParams holds it, the render tree, and the output records.
struct FeatArgs {
  float cam_pos[3];
  float c2w_col0[3], c2w_col1[3], c2w_col2[3];
  float cam_ax, cam_ay;
  float inv_w, inv_h;
  int W, H;
  const DNode* nodes;
  const DPrim* prims;
  const float* norms;
  const int4* tiles;  // (x, y, w, h), each <= 32 x 32 and inside the frame
  float4* feat;       // 2 * W * H records: {N, bsdf}, then {P, z}
  int* stack_spill;   // traversal stack entries beyond PT_STACK (null if the BVH never needs them)
};
// One wave per 64 pixels (an 8x8 block row pair) of each tile: n_tiles * 16 workgroups.
extern "C" hipError_t ptk_launch_features(const FeatArgs* a, int n_tiles, hipStream_t s);

// Ray queries on the device (trace_kernel; ptgpu.h pt_trace_rays_device): n
// rays of two float4 each, {o, tmax} and {d, unused}.  Closest mode writes two
// float4 per ray into `rec`; occluded mode one bit per ray into `occ`, two
// 32-bit words per chunk of 64 rays.
struct TraceArgs {
  const DNode* nodes;
  const DPrim* prims;
  const float* norms;
  const int* prim_map;   // own BVH order -> the caller's primitive index (null: the same)
  const float4* rays;
  float4* rec;           // closest mode: {t, u, v, prim}, {n, bsdf} per ray
  uint32_t* occ;         // occluded mode: ceil(n / 64) * 2 words
  unsigned long long* counts;  // rays, hits, invalid: added to
  int* stack_spill;      // traversal stack entries beyond PT_STACK of grid * PT_BLOCK lanes (null if the BVH never needs them)
  long long n;
};
// `grid` one-wave workgroups; wave b takes the chunks b, b + grid, ... (trace_host.h trace_grid).
extern "C" hipError_t ptk_launch_trace(const TraceArgs* a, int grid, bool occluded, hipStream_t s);
// Resident one-wave workgroups per CU of the closest / occluded build.
extern "C" hipError_t ptk_trace_occupancy(int* waves_per_cu, bool occluded);

// Pixel-centre camera rays of the listed tiles (camera_rays_kernel; ptgpu.h
// pt_camera_rays_device), in trace_kernel's ray layout at p = x + y * W.
struct CamRayArgs {
  float cam_pos[3];
  float c2w_col0[3], c2w_col1[3], c2w_col2[3];
  float cam_ax, cam_ay;
  float inv_w, inv_h;
  int W, H;
  const int4* tiles;  // (x, y, w, h), each <= 32 x 32 and inside the frame
  float4* rays;       // 2 * W * H
};
extern "C" hipError_t ptk_launch_camera_rays(const CamRayArgs* a, int n_tiles, hipStream_t s);
