// pt_records.h — the records the host flattens a scene into and the kernels
// read (DESIGN.md "Data layout in HBM").  HIP-free but for the vector types:
// scene_flatten.cpp fills them on the CPU, pt_device.h hands them to the kernels.
#pragma once
#include <hip/hip_vector_types.h>

// One guide bucket k of a running-sum array a (environment-light CDFs), in
// one 32-B record so that a lower_bound whose window is short needs ONE
// memory round trip: the window [lo, hi] = [g[k-1], g[k+2]] of the guide
// table g, and the window's values w_i = a[min(lo + i, hi)] (i < 4), w4 =
// a[hi], wm = a[lo - 1] (0 at lo = 0).  Windows longer than four entries
// (hi - lo > 4) are halved on the array itself (record_lower_bound).
struct alignas(32) EnvRec {
  int lo, hi;
  float wm, w0, w1, w2, w3, w4;
};

#ifndef PT_ENV_GUIDE
#define PT_ENV_GUIDE 1024  // buckets of the environment-CDF guide tables (with the window compare: C5 +10% over 64, profiles/r3/ab_env_window_search.txt)
#endif

// BVH4 node, 128 B (one L2 line): four child boxes in SoA form, component k
// of each float4 belongs to child k, then the four child references.
//  ref >= 0 is a node index; ref < 0 is a leaf cursor ~((first << 3) | (count - 1)):
//  primitives [first, first+count) in BVH order, count <= 8 (longer leaves
//  are split into subtrees).  Unused slots hold a box at +inf (never entered).
struct alignas(16) DNode {
  float4 lox, hix, loy, hiy, loz, hiz;
  int4 ref;
  int4 pad;
};

// (Round 5 built and measured two other render-tree encodings, removed in
// round 6 with their records kept: an 8-wide node with fp16 planes from a node
// origin, C3 -8.2%, and the 4-wide node compressed the same way to 80 B, C3
// -2.4%: profiles/r5/ab_stack_fast_w8.txt, ab_sel_spill_compress.txt.)

// Binary node of the reference topology, 64 B: both child boxes + child
// references (as DNode.ref).  Only traversed by the reference-count launch
// (PT_FLAG_REF_COUNTS), whose node visits feed SURVEY.md §8(d)'s cost model.
//  a = (c0.lo.x, c0.hi.x, c0.lo.y, c0.hi.y), b = the same for c1,
//  c = (c0.lo.z, c0.hi.z, c1.lo.z, c1.hi.z), e = (c0 ref, c1 ref, 0, 0)
struct alignas(16) DNode2 {
  float4 a, b, c;
  int4 e;
};

// Primitive, 48 B.  Triangle: v0 = (p1, meta), e1 = p2-p1, e2 = p3-p1.
// Sphere: v0 = (o, meta), e1 = (r, r*r, 0, 0).  meta = (bsdf << 1) | is_triangle.
struct alignas(16) DPrim {
  float4 v0, e1, e2;
};

struct alignas(16) DBsdf {
  int type;
  float a[3];  // albedo / reflectance
  float t[3];  // transmittance
  float e[3];  // emission
  float ior;
  float pad;
};

struct alignas(16) DLight {
  int type;
  float rad[3];
  float pos[3];
  float dir[3];
  float dimx[3];
  float dimy[3];
  float area;
  float pad[2];
};
