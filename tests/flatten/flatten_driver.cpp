// flatten_driver.cpp — runs csrc/scene_flatten.cpp on the CPU for
// tests/test_scene_flatten.py (built there with ASan/UBSan; no GPU, no HIP
// runtime).  Usage: flatten_driver OUTDIR, cases on stdin, one per line:
//   name=ID (dae=PATH [env=EXR] | dump=PATH) [tree=ref|sah|lbvh] [collapse=dp|area|count|sah]
// tree / collapse are put into PT_BVH_BUILD / PT_COLLAPSE (absent: unset) and
// read back through read_flatten_knobs().  Per case the driver writes each
// array of the FlatScene as raw bytes to OUTDIR/ID.<array> and prints one JSON
// line: rc, the error message, bvh_stack and the boxes as hex floats.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/ptgpu.h"
#include "../../include/ptgpu_scene.h"
#include "ptdump.h"
#include "scene_flatten.h"

namespace {

// A scene dump (dsgpuraytracing_amd/native.py SceneArrays) as a pt_scene.
struct DumpScene {
  std::vector<int32_t> ptype, pbsdf, btype, ltype;
  std::vector<double> geom, norm, nbb, lgeom;
  std::vector<int64_t> ninfo, eshape;
  std::vector<float> bparams, lrad, larea, env;
  std::vector<pt_bvh_node> nodes;
  std::vector<pt_bsdf> bsdfs;
  std::vector<pt_light> lights;
  pt_scene scene{};
};

template <class T>
bool rec(const std::vector<ptdump::Record>& recs, const char* name, const char* dtype, std::vector<T>& v) {
  for (const ptdump::Record& r : recs)
    if (r.name == name) return r.dtype == dtype && ptdump::get(recs, name, v);
  return false;
}

bool load_dump(const char* path, DumpScene& d) {
  std::vector<ptdump::Record> recs;
  if (!ptdump::read_all(path, recs)) return false;
  bool ok = rec(recs, "prim_type", "i4", d.ptype) && rec(recs, "prim_bsdf", "i4", d.pbsdf) &&
            rec(recs, "prim_geom", "f8", d.geom) && rec(recs, "prim_norm", "f8", d.norm) &&
            rec(recs, "node_bb", "f8", d.nbb) && rec(recs, "node_info", "i8", d.ninfo) &&
            rec(recs, "bsdf_type", "i4", d.btype) && rec(recs, "bsdf_params", "f4", d.bparams) &&
            rec(recs, "light_type", "i4", d.ltype) && rec(recs, "light_rad", "f4", d.lrad) &&
            rec(recs, "light_geom", "f8", d.lgeom) && rec(recs, "light_area", "f4", d.larea);
  const size_t np = d.ptype.size(), nn = d.ninfo.size() / 4, nb = d.btype.size(), nl = d.ltype.size();
  ok = ok && d.pbsdf.size() == np && d.geom.size() == 9 * np && d.norm.size() == 9 * np && d.nbb.size() == 6 * nn &&
       d.bparams.size() == 12 * nb && d.lrad.size() == 3 * nl && d.lgeom.size() == 12 * nl && d.larea.size() == nl;
  if (!ok) return false;
  d.nodes.resize(nn);
  for (size_t i = 0; i < nn; ++i) {
    pt_bvh_node& n = d.nodes[i];
    for (int k = 0; k < 3; ++k) {
      n.bb_min[k] = d.nbb[6 * i + k];
      n.bb_max[k] = d.nbb[6 * i + 3 + k];
    }
    n.start = d.ninfo[4 * i], n.range = d.ninfo[4 * i + 1], n.left = d.ninfo[4 * i + 2], n.right = d.ninfo[4 * i + 3];
  }
  d.bsdfs.resize(nb);
  for (size_t i = 0; i < nb; ++i) {
    pt_bsdf& b = d.bsdfs[i];
    const float* p = &d.bparams[12 * i];
    b.type = d.btype[i];
    for (int k = 0; k < 3; ++k) b.albedo[k] = p[k], b.transmittance[k] = p[3 + k], b.emission[k] = p[6 + k];
    b.ior = p[9], b.roughness = p[10];
  }
  d.lights.resize(nl);
  for (size_t i = 0; i < nl; ++i) {
    pt_light& L = d.lights[i];
    const double* g = &d.lgeom[12 * i];
    L.type = d.ltype[i];
    for (int k = 0; k < 3; ++k)
      L.radiance[k] = d.lrad[3 * i + k], L.position[k] = g[k], L.direction[k] = g[3 + k], L.dim_x[k] = g[6 + k],
      L.dim_y[k] = g[9 + k];
    L.area = d.larea[i];
  }
  pt_scene& s = d.scene;
  s.n_prims = (int64_t)np;
  s.prim_type = d.ptype.data(), s.prim_bsdf = d.pbsdf.data(), s.prim_geom = d.geom.data(), s.prim_norm = d.norm.data();
  s.n_nodes = (int64_t)nn, s.nodes = d.nodes.data();
  s.n_bsdfs = (int32_t)nb, s.bsdfs = d.bsdfs.data();
  s.n_lights = (int32_t)nl, s.lights = d.lights.data();
  if (rec(recs, "env_rgb", "f4", d.env)) {
    if (!rec(recs, "env_shape", "i8", d.eshape) || d.eshape.size() != 2 ||
        d.env.size() != (size_t)(3 * d.eshape[0] * d.eshape[1]))
      return false;
    s.env_height = (int32_t)d.eshape[0], s.env_width = (int32_t)d.eshape[1], s.env_rgb = d.env.data();
  }
  return true;
}

template <class T>
void put(const std::string& base, const char* what, const std::vector<T>& v) {
  FILE* f = std::fopen((base + "." + what).c_str(), "wb");
  if (!f) std::exit(3);
  if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) std::exit(3);
  std::fclose(f);
}

void hex3(const char* key, const float v[3]) { std::printf(", \"%s\": [\"%a\", \"%a\", \"%a\"]", key, v[0], v[1], v[2]); }
void hex3(const char* key, const double v[3]) { std::printf(", \"%s\": [\"%a\", \"%a\", \"%a\"]", key, v[0], v[1], v[2]); }

void knob(const char* var, const std::map<std::string, std::string>& kv, const char* key) {
  auto it = kv.find(key);
  if (it == kv.end()) unsetenv(var);
  else setenv(var, it->second.c_str(), 1);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::string line, loaded;
  pt_host_scene* hs = nullptr;
  DumpScene dump;
  pt_scene scene{};
  while (std::getline(std::cin, line)) {
    std::map<std::string, std::string> kv;
    std::istringstream in(line);
    for (std::string tok; in >> tok;) kv[tok.substr(0, tok.find('='))] = tok.substr(tok.find('=') + 1);
    const std::string src = kv.count("dae") ? kv["dae"] + "|" + (kv.count("env") ? kv["env"] : "") : kv["dump"];
    if (src != loaded) {  // (consecutive cases over one scene load it once)
      pt_host_scene_free(hs);
      hs = nullptr;
      if (kv.count("dae")) {
        if (pt_host_scene_load(kv["dae"].c_str(), 64, 64, nullptr, &hs)) return std::fprintf(stderr, "%s\n", pt_last_error()), 4;
        if (kv.count("env") && pt_host_scene_set_envmap(hs, kv["env"].c_str())) return 4;
        if (pt_host_scene_view(hs, &scene, nullptr)) return 4;
      } else {
        dump = DumpScene{};
        if (!load_dump(kv["dump"].c_str(), dump)) return 4;
        scene = dump.scene;
      }
      loaded = src;
    }
    const bool lbvh = kv.count("tree") && kv["tree"] == "lbvh";
    if (lbvh) kv.erase("tree");
    knob("PT_BVH_BUILD", kv, "tree");
    knob("PT_COLLAPSE", kv, "collapse");
    FlatScene f;
    const int rc = flatten_scene(&scene, read_flatten_knobs(lbvh), f);
    std::printf("{\"name\": \"%s\", \"rc\": %d, \"error\": \"%s\"", kv["name"].c_str(), rc, rc ? pt_last_error() : "");
    if (rc == PT_OK) {
      const std::string base = std::string(argv[1]) + "/" + kv["name"];
      put(base, "prims", f.prims), put(base, "norms", f.norms);
      put(base, "prims_ref", f.prims_ref), put(base, "norms_ref", f.norms_ref), put(base, "prim_map", f.prim_map);
      put(base, "nodes4", f.nodes4), put(base, "nodes2", f.nodes2);
      put(base, "bsdfs", f.bsdfs), put(base, "lights", f.lights), put(base, "bsdf_types", f.bsdf_types);
      put(base, "env_tex", f.env.tex), put(base, "env_p_theta", f.env.p_theta), put(base, "env_p_phi", f.env.p_phi);
      put(base, "env_p_theta_phi", f.env.p_theta_phi), put(base, "env_g_theta", f.env.g_theta);
      put(base, "env_g_phi", f.env.g_phi), put(base, "env_r_theta", f.env.r_theta), put(base, "env_r_phi", f.env.r_phi);
      std::printf(", \"bvh_stack\": %d, \"tri_only\": %d, \"env_w\": %d, \"env_h\": %d", f.bvh_stack, (int)f.tri_only,
                  f.env_w, f.env_h);
      hex3("root_lo", f.root_lo), hex3("root_hi", f.root_hi), hex3("root_lo_d", f.root_lo_d), hex3("root_hi_d", f.root_hi_d);
      hex3("scene_min", f.scene_min), hex3("scene_extent", f.scene_extent);
    }
    std::printf("}\n");
  }
  pt_host_scene_free(hs);
  return 0;
}
