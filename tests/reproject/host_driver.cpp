// host_driver.cpp — drives the pure host parts of the film's reprojection
// (csrc/reproject_host.cpp) for tests/test_reproject_host.py, which builds it
// with -fsanitize=address,undefined.  One case per stdin line:
//   cam <15 doubles>            -> {"ortho": 0|1, "f32": [14 floats as uint32 bits]}
//   params <cos> <sigma> <max>  -> {"error": "..."} ("" when valid)
//   keep <n> <types...>         -> {"keep": [...]}
//   default                     -> {"params": [cos bits, sigma bits, max]}
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include <iostream>

#include "reproject_host.h"

static uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string what;
    in >> what;
    if (what == "cam") {
      pt_camera cam;
      double v[15];
      for (double& d : v) {
        std::string tok;
        in >> tok;
        d = std::strtod(tok.c_str(), nullptr);  // (accepts nan / inf)
      }
      std::memcpy(cam.pos, v, 3 * sizeof(double));
      std::memcpy(cam.c2w, v + 3, 9 * sizeof(double));
      cam.screen_w = v[12];
      cam.screen_h = v[13];
      cam.screen_dist = v[14];
      ReprojectCam rc;
      reproject_camera(cam, &rc);
      const float f[14] = {rc.pos[0], rc.pos[1], rc.pos[2], rc.c0[0], rc.c0[1], rc.c0[2], rc.c1[0],
                           rc.c1[1],  rc.c1[2],  rc.c2[0],  rc.c2[1], rc.c2[2], rc.ax,    rc.ay};
      std::printf("{\"ortho\": %d, \"f32\": [", reproject_orthonormal(cam) ? 1 : 0);
      for (int i = 0; i < 14; ++i) std::printf("%s%" PRIu32, i ? ", " : "", bits(f[i]));
      std::printf("]}\n");
    } else if (what == "params") {
      pt_reproject_params p;
      std::string a, b;
      unsigned long m = 0;
      in >> a >> b >> m;
      p.normal_cos_min = std::strtof(a.c_str(), nullptr);
      p.sigma_p = std::strtof(b.c_str(), nullptr);
      p.max_samples = (uint32_t)m;
      const char* e = reproject_params_error(p);
      std::printf("{\"error\": \"%s\"}\n", e ? e : "");
    } else if (what == "keep") {
      int n = 0;
      in >> n;
      std::vector<int32_t> t((size_t)n);
      for (int32_t& x : t) in >> x;
      std::vector<uint32_t> k((size_t)n);
      reproject_keep_table(t.data(), n, k.data());
      std::printf("{\"keep\": [");
      for (int i = 0; i < n; ++i) std::printf("%s%" PRIu32, i ? ", " : "", k[(size_t)i]);
      std::printf("]}\n");
    } else if (what == "default") {
      pt_reproject_params p;
      reproject_params_default(&p);
      std::printf("{\"params\": [%" PRIu32 ", %" PRIu32 ", %" PRIu32 "]}\n", bits(p.normal_cos_min), bits(p.sigma_p),
                  p.max_samples);
    } else {
      std::printf("{\"unknown\": 1}\n");
    }
  }
  return 0;
}
