// scene_flatten.h — a pt_scene flattened into the arrays pt_upload_scene puts
// on the device (scene_flatten.cpp).  Host only, no HIP runtime call: the
// upload in pt_api.cpp is "validate, flatten, reserve, memcpy", and
// tests/test_scene_flatten.py runs this unit on the CPU under sanitizers.
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/ptgpu.h"
#include "pt_records.h"

// EnvironmentLight's constructor tables (environment_light.cpp:6-48) in its own
// float arithmetic and summation order, so the GPU's inverse-CDF sampling
// picks the same texel as the reference for the same (r1, r2):
//   pThetaPhi[y][x] = illum * sin(theta_y) / C, pTheta = running row sums,
//   pPhiGivenTheta = running sums of pThetaPhi / pTheta[y] within the row.
struct EnvTables {
  std::vector<float4> tex;
  std::vector<float> p_theta, p_phi, p_theta_phi;
  std::vector<int> g_theta, g_phi;  // guide tables (PT_ENV_GUIDE buckets)
  std::vector<EnvRec> r_theta, r_phi;  // their bucket records
};
void build_env_tables(const float* rgb, int w, int h, EnvTables& t);

// The render tree: by default this library's GPU-built
// tree (Karras LBVH + treelet restructuring, lbvh.hip) over the caller's
// primitives; PT_BVH_BUILD=sah: the host binned-SAH tree; =ref: the
// caller's own (reference) tree.  pt_upload_scene_lbvh always builds on
// the GPU.  The reference-count launch walks the caller's tree in every case
// but pt_upload_scene_lbvh's.
enum FlattenTree { FLATTEN_GPU_TREE, FLATTEN_HOST_SAH, FLATTEN_REF_TREE, FLATTEN_LBVH_ENTRY };

// The flattening knobs: environment variables, read by read_flatten_knobs()
// and nowhere else.
struct FlattenKnobs {
  FlattenTree tree = FLATTEN_GPU_TREE;  // PT_BVH_BUILD unset / sah / ref
  int collapse = 3;     // PT_COLLAPSE: 0 area, 1 count, 2 sah, 3 dp (read_flatten_knobs)
  bool report = false;  // PT_BVH_REPORT (set): print the BVH4's expected steps to stderr
};
// lbvh_entry: the upload came through pt_upload_scene_lbvh (whatever PT_BVH_BUILD says)
FlattenKnobs read_flatten_knobs(bool lbvh_entry);

struct FlatScene {
  // primitives and normals (9 floats each) in the render tree's order for the
  // host trees, in the caller's for the GPU-built ones (lbvh.hip sorts them)
  std::vector<DPrim> prims;
  std::vector<float> norms;
  // the caller's order, for the reference-count launch over nodes2; empty
  // where prims / norms are in that order already (every tree but the host SAH)
  std::vector<DPrim> prims_ref;
  std::vector<float> norms_ref;
  std::vector<int> prim_map;  // host SAH order -> caller's index (else empty)
  std::vector<DNode> nodes4;  // the host-built render tree (GPU-built trees: empty)
  std::vector<DNode2> nodes2;  // the caller's tree (FLATTEN_LBVH_ENTRY: empty)
  int bvh_stack = 0;  // worst-case traversal stack of the host-built trees
  float root_lo[3] = {0, 0, 0}, root_hi[3] = {0, 0, 0};  // host trees only
  double root_lo_d[3] = {0, 0, 0}, root_hi_d[3] = {0, 0, 0};
  std::vector<DBsdf> bsdfs;
  std::vector<DLight> lights;
  std::vector<int32_t> bsdf_types;
  EnvTables env;  // empty without an environment light
  int env_w = 0, env_h = 0;
  bool tri_only = false;  // every primitive a triangle
  float scene_min[3] = {0, 0, 0}, scene_extent[3] = {0, 0, 0};  // LbvhIn's scene box (GPU-built trees only)
};

// PT_OK, or PT_E_INVALID through pt_fail.  `out` is left half-filled on failure.
int flatten_scene(const pt_scene* s, const FlattenKnobs& k, FlatScene& out);

// The one refusal of a tree deeper than PT_STACK_MAX (fn: the entry point's name).
int fail_stack_depth(const char* fn, int need);
