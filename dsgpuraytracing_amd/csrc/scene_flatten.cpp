// scene_flatten.cpp — pt_scene -> the arrays the kernels read (scene_flatten.h):
// reference BVH -> 64-B two-child-box nodes and the 128-B BVH4 render tree,
// primitives -> 48-B float records, BSDF / light tables, environment tables.
// Host only (no HIP runtime call): compiled as plain C++, run on the CPU by
// tests/test_scene_flatten.py under ASan/UBSan.
#include "scene_flatten.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/ptgpu_scene.h"
#include "pt_error.h"
#include "pt_tuning.h"

namespace {

int fail(int code, const std::string& msg) { return pt_fail(code, msg); }

float round_down(double x) {
  float f = (float)x;
  if ((double)f > x) f = std::nextafter(f, -INFINITY);
  return f;
}
float round_up(double x) {
  float f = (float)x;
  if ((double)f < x) f = std::nextafter(f, INFINITY);
  return f;
}

// g[k] = lower_bound(a, k/G * a[n-1]), k = 0..G
void build_guide(const float* a, int n, int* g) {
  const float total = a[n - 1];
  for (int k = 0; k <= PT_ENV_GUIDE; ++k) {
    const float v = (float)((double)k / PT_ENV_GUIDE) * total;
    g[k] = (int)(std::lower_bound(a, a + n, v) - a);
    if (g[k] > n - 1) g[k] = n - 1;
  }
}
// The bucket records of a (n entries) from its guide table g (EnvRec).
void build_records(const float* a, const int* g, EnvRec* r) {
  for (int k = 0; k < PT_ENV_GUIDE; ++k) {
    EnvRec& e = r[k];
    e.lo = g[std::max(k - 1, 0)];
    e.hi = g[std::min(k + 2, PT_ENV_GUIDE)];
    e.wm = e.lo > 0 ? a[e.lo - 1] : 0.0f;
    e.w0 = a[std::min(e.lo, e.hi)];
    e.w1 = a[std::min(e.lo + 1, e.hi)];
    e.w2 = a[std::min(e.lo + 2, e.hi)];
    e.w3 = a[std::min(e.lo + 3, e.hi)];
    e.w4 = a[e.hi];
  }
}

}  // namespace

#pragma clang fp contract(off)
void build_env_tables(const float* rgb, int w, int h, EnvTables& t) {
  const double kPi = 3.14159265358979323;  // CMU462 PI
  t.tex.resize((size_t)w * h);
  t.p_theta.assign((size_t)h, 0.f);
  t.p_phi.assign((size_t)w * h, 0.f);
  t.p_theta_phi.assign((size_t)w * h, 0.f);
  for (size_t i = 0; i < (size_t)w * h; ++i) t.tex[i] = make_float4(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], 0.f);
  float C = 0;
  for (int y = 0; y < h; y++) {
    float theta = (y + 0.5) / h * kPi;
    float sin_theta = std::sin((double)theta);
    for (int x = 0; x < w; x++) {
      const float* p = rgb + 3 * ((size_t)x + (size_t)w * y);
      float illum = 0.2126f * p[0] + 0.7152f * p[1] + 0.0722f * p[2];  // Spectrum::illum
      t.p_theta_phi[(size_t)y * w + x] = illum * sin_theta;
      C += t.p_theta_phi[(size_t)y * w + x];
    }
  }
  for (int y = 0; y < h; y++) {
    for (int x = 0; x < w; x++) {
      t.p_theta_phi[(size_t)y * w + x] /= C;
      t.p_theta[y] += t.p_theta_phi[(size_t)y * w + x];
    }
    if (t.p_theta[y] != 0)
      for (int x = 0; x < w; x++) t.p_phi[(size_t)y * w + x] = t.p_theta_phi[(size_t)y * w + x] / t.p_theta[y];
  }
  for (int y = 0; y < h; y++) {
    if (y > 0) t.p_theta[y] += t.p_theta[y - 1];
    for (int x = 1; x < w; x++) t.p_phi[(size_t)y * w + x] += t.p_phi[(size_t)y * w + x - 1];
  }
  t.g_theta.resize(PT_ENV_GUIDE + 1);
  build_guide(t.p_theta.data(), h, t.g_theta.data());
  t.g_phi.resize((size_t)h * (PT_ENV_GUIDE + 1));
  for (int y = 0; y < h; y++) build_guide(&t.p_phi[(size_t)y * w], w, &t.g_phi[(size_t)y * (PT_ENV_GUIDE + 1)]);
  t.r_theta.resize(PT_ENV_GUIDE);
  build_records(t.p_theta.data(), t.g_theta.data(), t.r_theta.data());
  t.r_phi.resize((size_t)h * PT_ENV_GUIDE);
  for (int y = 0; y < h; y++)
    build_records(&t.p_phi[(size_t)y * w], &t.g_phi[(size_t)y * (PT_ENV_GUIDE + 1)], &t.r_phi[(size_t)y * PT_ENV_GUIDE]);
}
#pragma clang fp contract(on)

FlattenKnobs read_flatten_knobs(bool lbvh_entry) {
  FlattenKnobs k;
  const char* bb = std::getenv("PT_BVH_BUILD");
  k.tree = lbvh_entry                          ? FLATTEN_LBVH_ENTRY
           : bb && std::strcmp(bb, "sah") == 0 ? FLATTEN_HOST_SAH
           : bb && std::strcmp(bb, "ref") == 0 ? FLATTEN_REF_TREE
                                               : FLATTEN_GPU_TREE;
  // The collapse: PT_COLLAPSE=dp (default for the host trees: the SAH-optimal
  // choice of the binary nodes kept as BVH4 nodes, the DP of lbvh.hip's k_dp;
  // C3 over the host SAH tree 46.2 -> 51.0 G samples/s, +10%:
  // profiles/r5/ab_collapse_dp.txt), or greedy -- open the internal child with
  // the largest surface area (area), the most primitives (count) or area x
  // primitives (sah) until four.
  const char* cm = std::getenv("PT_COLLAPSE");
  k.collapse = !cm || std::strcmp(cm, "dp") == 0 ? 3
               : std::strcmp(cm, "count") == 0   ? 1
               : std::strcmp(cm, "sah") == 0     ? 2
                                                 : 0;
  k.report = std::getenv("PT_BVH_REPORT") != nullptr;
  return k;
}

int fail_stack_depth(const char* fn, int need) {
  return fail(PT_E_INVALID, std::string(fn) + ": BVH needs a deeper traversal stack (" + std::to_string(need) + " > " +
                                std::to_string(PT_STACK_MAX) + ")");
}

namespace {

// The double box of primitives [first, first + count) (a sphere's by |r|).
// Accumulated in locals: the out pointers may alias the geometry, which would
// send every min / max of the whole-scene box through memory.
void prim_box(const pt_scene* s, int64_t first, int64_t count, double lo_out[3], double hi_out[3]) {
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = first; i < first + count; ++i) {
    const double* g = s->prim_geom + 9 * i;
    for (int k = 0; k < 3; ++k) {
      if (s->prim_type[i] == PT_PRIM_TRIANGLE) {
        lo[k] = std::min({lo[k], g[k], g[3 + k], g[6 + k]});
        hi[k] = std::max({hi[k], g[k], g[3 + k], g[6 + k]});
      } else {
        lo[k] = std::min(lo[k], g[k] - std::fabs(g[3]));
        hi[k] = std::max(hi[k], g[k] + std::fabs(g[3]));
      }
    }
  }
  for (int k = 0; k < 3; ++k) lo_out[k] = lo[k], hi_out[k] = hi[k];
}

// ---- BVH: internal nodes only, pre-order, child boxes rounded outward;
// leaves become cursors in their parent's child references.  Leaves of more
// than 8 primitives are split into small subtrees over primitive boxes.

bool is_leaf(const pt_scene* s, int64_t i) { return s->nodes[i].left < 0 && s->nodes[i].right < 0; }

int validate_tree(const pt_scene* s) {
  const pt_bvh_node* N = s->nodes;
  const int64_t nn = s->n_nodes;
  for (int64_t i = 0; i < nn; ++i) {
    if ((N[i].left < 0) != (N[i].right < 0)) return fail(PT_E_INVALID, "pt_upload_scene: half-empty BVH node");
    if (N[i].left >= nn || N[i].right >= nn) return fail(PT_E_INVALID, "pt_upload_scene: BVH child out of range");
    if (is_leaf(s, i) && (N[i].start < 0 || N[i].range <= 0 || N[i].start + N[i].range > s->n_prims))
      return fail(PT_E_INVALID, "pt_upload_scene: bad leaf range");
  }
  if (s->n_prims >= ((int64_t)1 << 27)) return fail(PT_E_INVALID, "pt_upload_scene: too many primitives for leaf cursors");
  return PT_OK;
}

// a subtree to emit: a reference node, or a primitive range (split leaf)
struct Sub {
  int64_t ref;          // >= 0: reference node; -1: primitive range
  int64_t first, count;
  double lo[3], hi[3];
};
Sub sub_of_node(const pt_scene* s, int64_t r) {
  const pt_bvh_node* N = s->nodes;
  Sub u{r, N[r].start, N[r].range, {}, {}};
  for (int k = 0; k < 3; ++k) {
    u.lo[k] = N[r].bb_min[k];
    u.hi[k] = N[r].bb_max[k];
  }
  return u;
}
Sub sub_of_range(const pt_scene* s, int64_t first, int64_t count) {
  Sub u{-1, first, count, {}, {}};
  prim_box(s, first, count, u.lo, u.hi);
  return u;
}
bool sub_is_leaf(const pt_scene* s, const Sub& u) { return u.ref >= 0 ? is_leaf(s, u.ref) && u.count <= 8 : u.count <= 8; }
void sub_children(const pt_scene* s, const Sub& u, Sub ch[2]) {
  if (u.ref >= 0 && !is_leaf(s, u.ref)) {
    ch[0] = sub_of_node(s, s->nodes[u.ref].left);
    ch[1] = sub_of_node(s, s->nodes[u.ref].right);
  } else {  // oversized leaf: halve the primitive range
    int64_t h = u.count / 2;
    ch[0] = sub_of_range(s, u.first, h);
    ch[1] = sub_of_range(s, u.first + h, u.count - h);
  }
}

// One node of the binary tree: child boxes in fp32, child references are node
// indices or leaf cursors.  The tree is a pre-order vector of them.
struct B2 {
  float lo[2][3], hi[2][3];
  int ref[2];
};
void set_box(B2& d, int side, const Sub& u) {
  for (int k = 0; k < 3; ++k) {
    d.lo[side][k] = round_down(u.lo[k]);
    d.hi[side][k] = round_up(u.hi[k]);
  }
}
int cursor(int64_t first, int64_t count) { return (int)~((first << 3) | (count - 1)); }

// (1) binary tree over the reference topology: child boxes rounded outward
// to fp32, with the leaf split
int build_binary(const pt_scene* s, std::vector<B2>& b2) {
  Sub root = sub_of_node(s, 0);
  if (sub_is_leaf(s, root)) {  // one leaf: a root whose second child box is empty
    B2 d{};
    set_box(d, 0, root);
    for (int k = 0; k < 3; ++k) d.lo[1][k] = d.hi[1][k] = INFINITY;
    d.ref[0] = cursor(root.first, root.count);
    // the empty child is a leaf cursor (never entered: its box is at +inf),
    // never a node reference -- node 0 as its own child would be opened and
    // pushed forever by the collapse below
    d.ref[1] = cursor(0, 1);
    b2.push_back(d);
  } else {
    // explicit DFS: (subtree, parent node, side)
    struct Item { Sub u; int64_t parent; int side; };
    std::vector<Item> st = {{root, -1, 0}};
    while (!st.empty()) {
      Item it = st.back();
      st.pop_back();
      int64_t me = (int64_t)b2.size();
      b2.push_back(B2{});
      if (it.parent >= 0) b2[it.parent].ref[it.side] = (int)me;
      Sub ch[2];
      sub_children(s, it.u, ch);
      for (int side = 0; side < 2; ++side) {
        set_box(b2[me], side, ch[side]);
        if (sub_is_leaf(s, ch[side])) b2[me].ref[side] = cursor(ch[side].first, ch[side].count);
      }
      for (int side = 1; side >= 0; --side)
        if (!sub_is_leaf(s, ch[side])) st.push_back({ch[side], me, side});
    }
  }
  if ((int64_t)b2.size() >= ((int64_t)1 << 31)) return fail(PT_E_INVALID, "pt_upload_scene: too many BVH nodes");
  return PT_OK;
}

// The binary nodes of the reference-count launch keep the caller's boxes:
// its visit counts model the reference's own traversal.
void emit_nodes2(const std::vector<B2>& b2, std::vector<DNode2>& d2) {
  d2.resize(b2.size());
  for (size_t i = 0; i < b2.size(); ++i) {
    const B2& q = b2[i];
    d2[i].a = make_float4(q.lo[0][0], q.hi[0][0], q.lo[0][1], q.hi[0][1]);
    d2[i].b = make_float4(q.lo[1][0], q.hi[1][0], q.lo[1][1], q.hi[1][1]);
    d2[i].c = make_float4(q.lo[0][2], q.hi[0][2], q.lo[1][2], q.hi[1][2]);
    d2[i].e = make_int4(q.ref[0], q.ref[1], 0, 0);
  }
}

// The render tree: the kernel tests the float primitives (v0, v0 + e1,
// v0 + e2; c -+ r), whose roundings can leave the caller's double boxes by a
// few ulps (v0 and e1 are rounded apart; their sum is not the rounded
// vertex).  Every child box is widened to what lies below it: a leaf's to
// its float primitives, an inner child's to that node's own child boxes
// (pre-order: children come later).
void float_box(const pt_scene* s, int64_t first, int64_t count, float lo[3], float hi[3]) {
  for (int64_t i = first; i < first + count; ++i) {
    const double* g = s->prim_geom + 9 * i;
    for (int k = 0; k < 3; ++k) {
      double a, b;
      const double v0 = (double)(float)g[k];
      if (s->prim_type[i] == PT_PRIM_TRIANGLE) {
        const double p2 = v0 + (double)(float)(g[3 + k] - g[k]), p3 = v0 + (double)(float)(g[6 + k] - g[k]);
        a = std::min({v0, p2, p3});
        b = std::max({v0, p2, p3});
      } else {
        const double r = std::fabs((double)(float)g[3]);
        a = v0 - r;
        b = v0 + r;
      }
      lo[k] = std::min(lo[k], round_down(a));
      hi[k] = std::max(hi[k], round_up(b));
    }
  }
}
void widen_to_float_prims(const pt_scene* s, std::vector<B2>& b2) {
  for (size_t i = b2.size(); i-- > 0;)
    for (int side = 0; side < 2; ++side) {
      B2& q = b2[i];
      if (std::isinf(q.lo[side][0])) continue;  // the empty child of a one-leaf root
      float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
      const int r = q.ref[side];
      if (r < 0) {
        float_box(s, (int64_t)((~r) >> 3), (int64_t)(((~r) & 7) + 1), lo, hi);
      } else {
        for (int s2 = 0; s2 < 2; ++s2)
          for (int k = 0; k < 3; ++k) {
            lo[k] = std::min(lo[k], b2[(size_t)r].lo[s2][k]);
            hi[k] = std::max(hi[k], b2[(size_t)r].hi[s2][k]);
          }
      }
      for (int k = 0; k < 3; ++k) {
        q.lo[side][k] = std::min(q.lo[side][k], lo[k]);
        q.hi[side][k] = std::max(q.hi[side][k], hi[k]);
      }
    }
}

// (2) collapse to 4-wide nodes (the usual BVH2 -> BVH4 collapse): by the DP's
// tables (crit 3), or greedily -- repeatedly open the internal child of the
// largest weight.  Pre-order, so a node's first child follows it in memory.
struct Child {
  float lo[3], hi[3];
  int ref;
};
float area(const Child& c) {
  float dx = c.hi[0] - c.lo[0], dy = c.hi[1] - c.lo[1], dz = c.hi[2] - c.lo[2];
  return dx * dy + dy * dz + dz * dx;
}
struct Collapse {
  const std::vector<B2>& b2;
  int crit;                   // FlattenKnobs::collapse
  std::vector<double> under;  // primitives under each binary node
  // DP tables (crit 3): dpc[4n + i-1] = least expected steps of binary node
  // n's subtree in <= i slots (a node or a two-primitive leaf step costs one,
  // weighted by area); dpk = slots for its left child, -1 = as with i - 1
  std::vector<double> dpc;
  std::vector<int8_t> dpk;
};
void kids(const Collapse& c, int n, Child out[2]) {
  for (int s2 = 0; s2 < 2; ++s2) {
    for (int k = 0; k < 3; ++k) {
      out[s2].lo[k] = c.b2[(size_t)n].lo[s2][k];
      out[s2].hi[k] = c.b2[(size_t)n].hi[s2][k];
    }
    out[s2].ref = c.b2[(size_t)n].ref[s2];
  }
}
void collapse_tables(Collapse& c) {
  const std::vector<B2>& b2 = c.b2;
  // primitives under each binary node (b2 is pre-order: children follow parents)
  c.under.assign(b2.size(), 0.0);
  for (size_t i = b2.size(); i-- > 0;)
    for (int s2 = 0; s2 < 2; ++s2) {
      const int r = b2[i].ref[s2];
      c.under[i] += r >= 0 ? c.under[(size_t)r] : (double)(((~r) & 7) + 1);
    }
  if (c.crit != 3) return;
  std::vector<double>& dpc = c.dpc;
  std::vector<int8_t>& dpk = c.dpk;
  dpc.assign(b2.size() * 4, 0.0);
  dpk.assign(b2.size() * 4, 0);
  auto box_area = [](const float lo[3], const float hi[3]) {
    const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    return dx * dy + dy * dz + dz * dx;
  };
  for (size_t n = b2.size(); n-- > 0;) {  // (pre-order: children after parents)
    double a[2][5];
    for (int s2 = 0; s2 < 2; ++s2) {
      const int r = b2[n].ref[s2];
      for (int i = 1; i <= 4; ++i)
        a[s2][i] = r >= 0 ? dpc[(size_t)r * 4 + (i - 1)]
                          : box_area(b2[n].lo[s2], b2[n].hi[s2]) * (double)((((~r) & 7) + 2) / 2);
    }
    double dist[5];
    int8_t arg[5];
    for (int j = 2; j <= 4; ++j) {
      dist[j] = INFINITY;
      arg[j] = 1;
      for (int k = 1; k < j; ++k)
        if (a[0][k] + a[1][j - k] < dist[j]) {
          dist[j] = a[0][k] + a[1][j - k];
          arg[j] = (int8_t)k;
        }
    }
    float ulo[3], uhi[3];
    for (int k = 0; k < 3; ++k) {
      ulo[k] = std::min(b2[n].lo[0][k], b2[n].lo[1][k]);
      uhi[k] = std::max(b2[n].hi[0][k], b2[n].hi[1][k]);
    }
    double prev = box_area(ulo, uhi) + dist[4];
    dpc[n * 4] = prev;
    dpk[n * 4] = arg[4];
    for (int i = 2; i <= 4; ++i) {
      const bool open = dist[i] < prev;
      prev = open ? dist[i] : prev;
      dpc[n * 4 + (i - 1)] = prev;
      dpk[n * 4 + (i - 1)] = open ? arg[i] : (int8_t)-1;
    }
  }
}
// the DP's children of binary node b kept whole: its two children over four
// slots, each opened as its table says, in left-to-right order
int dp_kids(const Collapse& c, int b, Child out[4]) {
  const std::vector<B2>& b2 = c.b2;
  const std::vector<int8_t>& dpk = c.dpk;
  int sp = 0, n = 0, sb[8], ss[8], si[8];
  const int k4 = dpk[(size_t)b * 4];
  sb[sp] = b; ss[sp] = 1; si[sp++] = 4 - k4;
  sb[sp] = b; ss[sp] = 0; si[sp++] = k4;
  while (sp > 0) {
    --sp;
    const int pb = sb[sp], side = ss[sp];
    int i = si[sp];
    const int r = b2[(size_t)pb].ref[side];
    if (r >= 0) {
      while (i > 1 && dpk[(size_t)r * 4 + (i - 1)] == -1) --i;
      if (i > 1) {
        const int k = dpk[(size_t)r * 4 + (i - 1)];
        sb[sp] = r; ss[sp] = 1; si[sp++] = i - k;
        sb[sp] = r; ss[sp] = 0; si[sp++] = k;
        continue;
      }
    }
    Child ch;
    for (int k = 0; k < 3; ++k) {
      ch.lo[k] = b2[(size_t)pb].lo[side][k];
      ch.hi[k] = b2[(size_t)pb].hi[side][k];
    }
    ch.ref = r;
    out[n++] = ch;
  }
  return n;
}
double weight(const Collapse& c, const Child& ch) {
  const double n = ch.ref >= 0 ? c.under[(size_t)ch.ref] : 0.0;
  return c.crit == 0 ? (double)area(ch) : c.crit == 1 ? n : (double)area(ch) * n;
}
int greedy_kids(const Collapse& c, int b, Child ch[4]) {
  int n = 2;
  kids(c, b, ch);
  while (n < 4) {
    int best = -1;
    double ba = -1.0;
    for (int k = 0; k < n; ++k)
      if (ch[k].ref >= 0 && weight(c, ch[k]) > ba) {
        ba = weight(c, ch[k]);
        best = k;
      }
    if (best < 0) break;
    Child two[2];
    kids(c, ch[best].ref, two);
    ch[best] = two[0];
    ch[n++] = two[1];
  }
  return n;
}

// Emits the BVH4 nodes and the worst-case traversal stack.
void emit_bvh4(const Collapse& c, std::vector<DNode>& dn, int& max_stack) {
  max_stack = 0;
  struct Item4 { int b2node; int64_t parent; int slot; int stack; };
  std::vector<Item4> st = {{0, -1, 0, 0}};
  while (!st.empty()) {
    Item4 it = st.back();
    st.pop_back();
    Child ch[4];
    const int n = c.crit == 3 ? dp_kids(c, it.b2node, ch) : greedy_kids(c, it.b2node, ch);
    int64_t me = (int64_t)dn.size();
    dn.push_back(DNode{});
    if (it.parent >= 0) (&dn[(size_t)it.parent].ref.x)[it.slot] = (int)me;
    DNode& d = dn[(size_t)me];
    float* lox = &d.lox.x; float* hix = &d.hix.x; float* loy = &d.loy.x;
    float* hiy = &d.hiy.x; float* loz = &d.loz.x; float* hiz = &d.hiz.x;
    int* ref = &d.ref.x;
    for (int k = 0; k < 4; ++k) {
      if (k < n) {
        lox[k] = ch[k].lo[0]; hix[k] = ch[k].hi[0];
        loy[k] = ch[k].lo[1]; hiy[k] = ch[k].hi[1];
        loz[k] = ch[k].lo[2]; hiz[k] = ch[k].hi[2];
        ref[k] = ch[k].ref;
      } else {  // empty slot: the box at +inf, which no ray enters (an inverted
                // box would not do: the slab test orders each pair of planes)
        lox[k] = loy[k] = loz[k] = hix[k] = hiy[k] = hiz[k] = INFINITY;
        ref[k] = 0;
      }
    }
    // a visit pushes at most n-1 siblings before descending
    const int below = it.stack + (n - 1);
    max_stack = std::max(max_stack, below);
    for (int k = n - 1; k >= 0; --k)
      if (ch[k].ref >= 0) st.push_back({ch[k].ref, me, k, below});
  }
}

void report_bvh4(const std::vector<DNode>& dn, int max_stack) {
  // expected steps per random ray (surface-area heuristic over the BVH4):
  // node steps = sum of node areas / root area; leaf steps = sum over
  // leaves of area * ceil(count / 2) / root area
  auto a3 = [](float lx, float hx, float ly, float hy, float lz, float hz) {
    const double dx = hx - lx, dy = hy - ly, dz = hz - lz;
    return dx * dy + dy * dz + dz * dx;
  };
  double root = 0, nodes = 0, leaves = 0;
  for (size_t i = 0; i < dn.size(); ++i) {
    const DNode& d = dn[i];
    for (int k = 0; k < 4; ++k) {
      if (std::isinf((&d.lox.x)[k])) continue;
      const double a = a3((&d.lox.x)[k], (&d.hix.x)[k], (&d.loy.x)[k], (&d.hiy.x)[k], (&d.loz.x)[k], (&d.hiz.x)[k]);
      root += i == 0 ? a : 0.0;
      const int r = (&d.ref.x)[k];
      if (r >= 0) nodes += a;
      else leaves += a * (double)((((~r) & 7) + 2) / 2);
    }
  }
  std::fprintf(stderr, "[pt] BVH4: %zu nodes, stack %d, SAH node steps %.3f leaf steps %.3f (per root-box ray)\n",
               dn.size(), max_stack, (nodes + root) / root, leaves / root);
}

// Traversal termination rests on this: node references only point forward
// (pre-order), so a ray can never re-enter a node it has left.
int check_forward(const std::vector<DNode>& dn) {
  for (size_t i = 0; i < dn.size(); ++i)
    for (int k = 0; k < 4; ++k) {
      int r = (&dn[i].ref.x)[k];
      bool empty = std::isinf((&dn[i].lox.x)[k]);
      if (!empty && r >= 0 && (r <= (int)i || r >= (int)dn.size()))
        return fail(PT_E_INVALID, "pt_upload_scene: BVH4 child reference is not forward");
    }
  return PT_OK;
}

// Reference BVH (pt_scene.nodes) -> BVH4 nodes (dn), binary nodes (d2) and
// the worst-case traversal stack.
int build_host_bvh(const pt_scene* s, const FlattenKnobs& knobs, std::vector<DNode>& dn, std::vector<DNode2>& d2,
                   int& max_stack) {
  if (int rc = validate_tree(s)) return rc;
  std::vector<B2> b2;
  if (int rc = build_binary(s, b2)) return rc;
  emit_nodes2(b2, d2);
  widen_to_float_prims(s, b2);
  Collapse c{b2, knobs.collapse, {}, {}, {}};
  collapse_tables(c);
  emit_bvh4(c, dn, max_stack);
  if (knobs.report) report_bvh4(dn, max_stack);
  if (int rc = check_forward(dn)) return rc;
  if (max_stack > PT_STACK_MAX) return fail_stack_depth("pt_upload_scene", max_stack);
  return PT_OK;
}

// The caller's double primitives as DPrim records and float normals.
int convert_prims(const pt_scene* s, std::vector<DPrim>& prims, std::vector<float>& norms) {
  prims.resize((size_t)s->n_prims);
  norms.assign((size_t)s->n_prims * 9, 0.f);
  for (int64_t i = 0; i < s->n_prims; ++i) {
    const double* g = s->prim_geom + 9 * i;
    const double* n = s->prim_norm + 9 * i;
    int b = s->prim_bsdf[i];
    if (b < 0 || b >= s->n_bsdfs) return fail(PT_E_INVALID, "pt_upload_scene: primitive BSDF index out of range");
    DPrim& P = prims[(size_t)i];
    if (s->prim_type[i] == PT_PRIM_TRIANGLE) {
      int meta = (b << 1) | 1;
      float mf;
      std::memcpy(&mf, &meta, 4);
      P.v0 = make_float4((float)g[0], (float)g[1], (float)g[2], mf);
      P.e1 = make_float4((float)(g[3] - g[0]), (float)(g[4] - g[1]), (float)(g[5] - g[2]), 0.f);
      P.e2 = make_float4((float)(g[6] - g[0]), (float)(g[7] - g[1]), (float)(g[8] - g[2]), 0.f);
      for (int k = 0; k < 9; ++k) norms[9 * i + k] = (float)n[k];
    } else if (s->prim_type[i] == PT_PRIM_SPHERE) {
      int meta = (b << 1);
      float mf;
      std::memcpy(&mf, &meta, 4);
      P.v0 = make_float4((float)g[0], (float)g[1], (float)g[2], mf);
      P.e1 = make_float4((float)g[3], (float)(g[3] * g[3]), 0.f, 0.f);
      P.e2 = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      return fail(PT_E_INVALID, "pt_upload_scene: unknown primitive type");
    }
  }
  return PT_OK;
}

int flatten_bsdfs(const pt_scene* s, std::vector<DBsdf>& bs) {
  bs.resize((size_t)s->n_bsdfs);
  for (int i = 0; i < s->n_bsdfs; ++i) {
    const pt_bsdf& B = s->bsdfs[i];
    if (B.type < 0 || B.type > 4) return fail(PT_E_INVALID, "pt_upload_scene: unknown BSDF type");
    DBsdf& d = bs[(size_t)i];
    d.type = B.type;
    for (int k = 0; k < 3; ++k) {
      d.a[k] = B.albedo[k];
      d.t[k] = B.transmittance[k];
      d.e[k] = B.emission[k];
    }
    d.ior = B.ior;
    d.pad = 0.f;
  }
  return PT_OK;
}

int flatten_lights(const pt_scene* s, std::vector<DLight>& ls, int& n_env) {
  ls.resize((size_t)std::max(0, s->n_lights));
  n_env = 0;
  for (int i = 0; i < s->n_lights; ++i) {
    const pt_light& L = s->lights[i];
    if (L.type < 0 || L.type > 4) return fail(PT_E_INVALID, "pt_upload_scene: unsupported light type");
    if (L.type == PT_LIGHT_ENVIRONMENT && ++n_env > 1)
      return fail(PT_E_INVALID, "pt_upload_scene: more than one environment light");
    DLight& d = ls[(size_t)i];
    std::memset(&d, 0, sizeof(d));
    d.type = L.type;
    for (int k = 0; k < 3; ++k) {
      d.rad[k] = L.radiance[k];
      d.pos[k] = (float)L.position[k];
      d.dir[k] = (float)L.direction[k];
      d.dimx[k] = (float)L.dim_x[k];
      d.dimy[k] = (float)L.dim_y[k];
    }
    d.area = L.area;
  }
  return PT_OK;
}

// Own SAH tree (PT_BVH_BUILD=sah): the primitives are permuted into its
// leaf order and uploaded that way; prim_map takes ray-query ids back.
struct SahScene {
  std::vector<pt_bvh_node> nodes;
  std::vector<int64_t> perm;
  std::vector<int32_t> ptype, pbsdf;
  std::vector<double> pgeom, pnorm;
  pt_scene scene;
};
int build_sah_scene(const pt_scene* s, SahScene& o) {
  o.nodes.resize((size_t)std::max<int64_t>(1, 2 * s->n_prims - 1));
  o.perm.resize((size_t)s->n_prims);
  int64_t nn = 0;
  if (int rc = pt_host_build_render_tree(s, o.nodes.data(), &nn, o.perm.data())) return rc;
  o.nodes.resize((size_t)nn);
  const size_t np = (size_t)s->n_prims;
  o.ptype.resize(np);
  o.pbsdf.resize(np);
  o.pgeom.resize(np * 9);
  o.pnorm.resize(np * 9);
  for (size_t i = 0; i < np; ++i) {
    const size_t p = (size_t)o.perm[i];
    o.ptype[i] = s->prim_type[p];
    o.pbsdf[i] = s->prim_bsdf[p];
    std::memcpy(&o.pgeom[9 * i], s->prim_geom + 9 * p, 9 * sizeof(double));
    std::memcpy(&o.pnorm[9 * i], s->prim_norm + 9 * p, 9 * sizeof(double));
  }
  o.scene = *s;
  o.scene.prim_type = o.ptype.data();
  o.scene.prim_bsdf = o.pbsdf.data();
  o.scene.prim_geom = o.pgeom.data();
  o.scene.prim_norm = o.pnorm.data();
  o.scene.nodes = o.nodes.data();
  o.scene.n_nodes = (int64_t)o.nodes.size();
  return PT_OK;
}

// The root box of a host tree: the root node's, rounded outward ...
void root_box(const pt_scene* s, const std::vector<DNode>& dn, FlatScene& f) {
  const pt_bvh_node* N = s->nodes;
  for (int k = 0; k < 3; ++k) {
    f.root_lo[k] = round_down(N[0].bb_min[k]);
    f.root_hi[k] = round_up(N[0].bb_max[k]);
    f.root_lo_d[k] = N[0].bb_min[k];
    f.root_hi_d[k] = N[0].bb_max[k];
  }
  // ... and the root's child boxes, which build_host_bvh widened to the float primitives
  for (int slot = 0; slot < 4 && !dn.empty(); ++slot) {
    const float* lo[3] = {&dn[0].lox.x, &dn[0].loy.x, &dn[0].loz.x};
    const float* hi[3] = {&dn[0].hix.x, &dn[0].hiy.x, &dn[0].hiz.x};
    if (std::isinf(lo[0][slot])) continue;
    for (int k = 0; k < 3; ++k) {
      f.root_lo[k] = std::min(f.root_lo[k], lo[k][slot]);
      f.root_hi[k] = std::max(f.root_hi[k], hi[k][slot]);
      f.root_lo_d[k] = std::min(f.root_lo_d[k], (double)lo[k][slot]);
      f.root_hi_d[k] = std::max(f.root_hi_d[k], (double)hi[k][slot]);
    }
  }
}

// The GPU build's scene box: sceneBox.expand(prim->get_bbox()) (setup.cu:482-487)
void scene_box(const pt_scene* s, FlatScene& f) {
  double lo[3], hi[3];
  prim_box(s, 0, s->n_prims, lo, hi);
  for (int k = 0; k < 3; ++k) {
    f.scene_min[k] = round_down(lo[k]);
    f.scene_extent[k] = (float)(hi[k] - lo[k]);
  }
}

}  // namespace

int flatten_scene(const pt_scene* s, const FlattenKnobs& knobs, FlatScene& f) {
  f = FlatScene{};
  const pt_scene* const s0 = s;  // the caller's scene (reference BVH order)
  SahScene sah;
  if (knobs.tree == FLATTEN_HOST_SAH) {
    if (int rc = build_sah_scene(s, sah)) return rc;
    s = &sah.scene;
  }

  // ---- primitives (already in BVH order)
  if (int rc = convert_prims(s, f.prims, f.norms)) return rc;
  if (s != s0)
    if (int rc = convert_prims(s0, f.prims_ref, f.norms_ref)) return rc;

  int n_env = 0;
  if (int rc = flatten_bsdfs(s, f.bsdfs)) return rc;
  if (int rc = flatten_lights(s, f.lights, n_env)) return rc;
  if (n_env && (!s->env_rgb || s->env_width <= 0 || s->env_height <= 0))
    return fail(PT_E_INVALID, "pt_upload_scene: environment light without a map (env_rgb/env_width/env_height)");
  if (!n_env && s->env_rgb) return fail(PT_E_INVALID, "pt_upload_scene: env_rgb given but no PT_LIGHT_ENVIRONMENT light");
  if (n_env) build_env_tables(s->env_rgb, s->env_width, s->env_height, f.env);
  f.env_w = n_env ? s->env_width : 0;
  f.env_h = n_env ? s->env_height : 0;

  if (knobs.tree == FLATTEN_GPU_TREE) {
    // the caller's tree: validated, kept as the binary nodes of the
    // reference-count launch over a caller-order copy of the primitives
    std::vector<DNode> dn0;
    if (int rc = build_host_bvh(s0, knobs, dn0, f.nodes2, f.bvh_stack)) return rc;
    scene_box(s0, f);
  } else if (knobs.tree != FLATTEN_LBVH_ENTRY) {
    if (int rc = build_host_bvh(s, knobs, f.nodes4, f.nodes2, f.bvh_stack)) return rc;
    if (s != s0) {  // the reference-count launch walks the caller's (reference) tree
      std::vector<DNode> dn0;
      int ms0 = 0;
      f.nodes2.clear();
      if (int rc = build_host_bvh(s0, knobs, dn0, f.nodes2, ms0)) return rc;
      f.bvh_stack = std::max(f.bvh_stack, ms0);
    }
    f.prim_map.assign(sah.perm.begin(), sah.perm.end());
    root_box(s, f.nodes4, f);
  } else {
    scene_box(s, f);
  }
  f.bsdf_types.resize(f.bsdfs.size());
  for (size_t i = 0; i < f.bsdfs.size(); ++i) f.bsdf_types[i] = f.bsdfs[i].type;
  f.tri_only = std::all_of(s->prim_type, s->prim_type + s->n_prims, [](int t) { return t == PT_PRIM_TRIANGLE; });
  return PT_OK;
}
