// plan_driver.cpp — runs the launch policy (csrc/launch_plan.cpp) on the CPU
// for tests/test_launch_plan.py: one case per input line, one JSON object per
// output line.  A case is a list of key=value tokens:
//   op=plan|group|rect      (default plan)
//   W H spp env nf flags idle ncu grid_plain grid_stats bpc=a,b,c,d nodes stack
//   tri_only stats_cap nbsdfs nlights cam=pos(3),c2w(9),w,h,dist box=lo(3),hi(3)
//   tiles=SPEC[+SPEC...]    SPEC: grid:E (edge-E tiles over the frame), grid:E:k/n
//                           (every n-th of them from k), or x,y,w,h
//   env.NAME=VALUE          set in the environment while the knobs are read
//   pipeline=0 small_launch=0   (the knobs read once per process)
//   lists=1                 print the permutation, blocks and tile_block0
//   fit_nf=N                frames_that_fit's nf (default PT_MAX_FRAMES)
//   op=group: traced env spp sample_group lanes frame_blocks budget
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "launch_plan.h"

using Case = std::map<std::string, std::string>;

static double num(const Case& c, const char* k, double dflt) {
  auto it = c.find(k);
  return it == c.end() ? dflt : std::atof(it->second.c_str());
}
static std::vector<double> nums(const std::string& s, char sep = ',') {
  std::vector<double> v;
  std::stringstream ss(s);
  std::string t;
  while (std::getline(ss, t, sep)) v.push_back(std::atof(t.c_str()));
  return v;
}
template <class T>
static void arr(const char* name, const T* v, size_t n) {
  std::printf("\"%s\": [", name);
  for (size_t i = 0; i < n; ++i) std::printf("%s%lld", i ? ", " : "", (long long)v[i]);
  std::printf("], ");
}
static void rects(const char* name, const std::vector<PlanRect>& v) {
  std::printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) std::printf("%s[%d, %d, %d, %d]", i ? ", " : "", v[i].x, v[i].y, v[i].w, v[i].h);
  std::printf("], ");
}

static std::vector<PlanRect> tiles_of(const std::string& spec, int W, int H) {
  std::vector<PlanRect> out;
  std::stringstream ss(spec);
  std::string part;
  while (std::getline(ss, part, '+')) {
    if (part.rfind("grid:", 0) == 0) {
      int e = 32, k = 0, n = 1;
      std::sscanf(part.c_str(), "grid:%d:%d/%d", &e, &k, &n);
      int i = 0;
      for (int y = 0; y < H; y += e)
        for (int x = 0; x < W; x += e, ++i)
          if (i % n == k) out.push_back({x, y, std::min(e, W - x), std::min(e, H - y)});
    } else {
      std::vector<double> v = nums(part);
      if (v.size() == 4) out.push_back({(int)v[0], (int)v[1], (int)v[2], (int)v[3]});
    }
  }
  return out;
}

static void run(const Case& c) {
  const std::string op = c.count("op") ? c.at("op") : "plan";
  if (op == "group") {
    std::printf("{\"group_spp\": %d}\n",
                group_size((int64_t)num(c, "traced", 0), num(c, "env", 0) != 0, (int)num(c, "spp", 1),
                           (int)num(c, "sample_group", 0), (int64_t)num(c, "lanes", PT_GROUP_REF_LANES),
                           (int64_t)num(c, "frame_blocks", 1), (int64_t)num(c, "budget", 5120)));
    return;
  }
  PlanInput in;
  in.W = (int)num(c, "W", 64);
  in.H = (int)num(c, "H", 64);
  in.spp = (int)num(c, "spp", 1);
  std::vector<double> cam = nums(c.count("cam") ? c.at("cam") : "0,0,0,1,0,0,0,1,0,0,0,1,1,1,1");
  cam.resize(15);
  for (int k = 0; k < 3; ++k) in.cam.pos[k] = cam[k];
  for (int k = 0; k < 9; ++k) in.cam.c2w[k] = cam[3 + k];
  in.cam.screen_w = cam[12];
  in.cam.screen_h = cam[13];
  in.cam.screen_dist = cam[14];
  std::vector<double> box = nums(c.count("box") ? c.at("box") : "-1,-1,-1,1,1,1");  // (around the default pinhole: no cull)
  box.resize(6);
  for (int k = 0; k < 3; ++k) in.box_lo[k] = box[k], in.box_hi[k] = box[3 + k];
  in.env = num(c, "env", 0) != 0;
  in.n_bsdfs = (int)num(c, "nbsdfs", 4);
  in.n_lights = (int)num(c, "nlights", 1);
  in.n_render_nodes = (int64_t)num(c, "nodes", 1000);
  in.bvh_stack = (int)num(c, "stack", 16);
  in.tri_only = num(c, "tri_only", 1) != 0;
  in.n_cu = (int)num(c, "ncu", 256);
  in.grid_plain = (int)num(c, "grid_plain", 20 * in.n_cu);
  in.grid_stats = (int)num(c, "grid_stats", 12 * in.n_cu);
  std::vector<double> bpc = nums(c.count("bpc") ? c.at("bpc") : "20,16,16,12");
  bpc.resize(4);
  for (int k = 0; k < 4; ++k) in.bpc_variant[k] = (int)bpc[k];
  in.stats_cap = (size_t)num(c, "stats_cap", PT_STATS_SLOTS + (double)PT_WAVE_TRACE * 64 * in.n_cu);
  const std::vector<PlanRect> tiles = tiles_of(c.count("tiles") ? c.at("tiles") : "grid:32", in.W, in.H);
  in.tiles = tiles.data();
  in.n_tiles = tiles.size();
  in.nf = (int)num(c, "nf", 1);
  in.flags = (uint32_t)num(c, "flags", 0);
  in.gpu_idle = num(c, "idle", 1) != 0;
  std::vector<std::string> set;
  for (const auto& kv : c)
    if (kv.first.rfind("env.", 0) == 0) {
      set.push_back(kv.first.substr(4));
      setenv(set.back().c_str(), kv.second.c_str(), 1);
    }
  in.knobs = read_launch_knobs();
  for (const std::string& n : set) unsetenv(n.c_str());
  if (c.count("pipeline")) in.knobs.pipeline = num(c, "pipeline", 1) != 0;
  if (c.count("small_launch")) in.knobs.small_launch = num(c, "small_launch", 1) != 0;

  if (op == "rect") {
    int r[4] = {0, 0, 0, 0};
    const bool ok = footprint_rect(in.cam, in.box_lo, in.box_hi, in.W, in.H, r);
    std::printf("{\"ok\": %d, \"rect\": [%d, %d, %d, %d]}\n", ok ? 1 : 0, r[0], r[1], r[2], r[3]);
    return;
  }
  const LaunchPlan p = plan_launch(in);
  int64_t fit_slots = -1;
  const int fit = frames_that_fit(in, (int)num(c, "fit_nf", PT_MAX_FRAMES), &fit_slots);
  std::printf("{\"error\": \"%s\", ", p.error.c_str());
  if (num(c, "lists", 0) != 0) {
    rects("tiles", tiles);
    arr("perm", p.perm.data(), p.perm.size());
    rects("ztiles", p.ztiles);
    rects("blocks", p.blocks);
    arr("tile_block0", p.tile_block0.data(), p.tile_block0.size());
  }
  arr("cull", p.cull, 4);
  arr("footprint", p.footprint, 4);
  const std::pair<const char*, long long> f[] = {
      {"n_tiles", (long long)in.n_tiles}, {"zorder", p.zorder}, {"n_perm", (long long)p.perm.size()},
      {"n_blocks", (long long)p.blocks.size()}, {"n_tile_block0", (long long)p.tile_block0.size()},
      {"pixels", p.pixels}, {"culled_px", p.culled_px}, {"traced_px", traced_px(in)},
      {"group_spp", p.group_spp}, {"n_groups", p.n_groups}, {"group_shift", p.group_shift},
      {"grp_m", p.grp_m}, {"grp_sh", p.grp_sh}, {"frm_m", p.frm_m}, {"frm_sh", p.frm_sh},
      {"frame_slots", p.frame_slots}, {"slots", p.slots}, {"want", p.want}, {"grid", p.grid},
      {"gtab", p.gtab}, {"stats", p.stats}, {"small", p.small}, {"chunk", p.chunk}, {"qbands", p.qbands},
      {"sblocks", p.sblocks}, {"shade_batch", p.shade_batch}, {"leaf_weight", p.leaf_weight},
      {"drain_div", p.drain_div}, {"tri_only", p.tri_only}, {"helpers", p.helpers}, {"census", p.census},
      {"dbg_pix", p.dbg_pix}, {"partial_floats", (long long)p.partial_floats}, {"spill_ints", (long long)p.spill_ints},
      {"batch_partial_floats", (long long)p.batch_partial_floats}, {"batch_spill_ints", (long long)p.batch_spill_ints},
      {"fit", fit}, {"fit_frame_slots", fit_slots}};
  for (const auto& kv : f) std::printf("\"%s\": %lld, ", kv.first, kv.second);
  std::printf("\"n_cu\": %d}\n", in.n_cu);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    Case c;
    std::stringstream ss(line);
    std::string tok;
    while (ss >> tok) {
      const size_t eq = tok.find('=');
      if (eq != std::string::npos) c[tok.substr(0, eq)] = tok.substr(eq + 1);
    }
    if (!c.empty()) run(c);
  }
  return 0;
}
