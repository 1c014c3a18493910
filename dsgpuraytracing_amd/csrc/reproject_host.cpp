// reproject_host.cpp — the host side of the film's reprojection (reproject_host.h).
#include "reproject_host.h"

#include <cmath>

void reproject_camera(const pt_camera& cam, ReprojectCam* out) {
  for (int k = 0; k < 3; ++k) {
    out->pos[k] = (float)cam.pos[k];
    out->c0[k] = (float)cam.c2w[3 * k + 0];
    out->c1[k] = (float)cam.c2w[3 * k + 1];
    out->c2[k] = (float)cam.c2w[3 * k + 2];
  }
  out->ax = (float)(cam.screen_w / cam.screen_dist);
  out->ay = (float)(cam.screen_h / cam.screen_dist);
}

bool reproject_orthonormal(const pt_camera& cam) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double dp = 0;
      for (int k = 0; k < 3; ++k) dp += cam.c2w[3 * k + i] * cam.c2w[3 * k + j];
      if (!(std::fabs(dp - (i == j ? 1.0 : 0.0)) <= 1e-9)) return false;
    }
  return true;
}

void reproject_params_default(pt_reproject_params* out) {
  out->normal_cos_min = PT_REPROJECT_NORMAL_COS_MIN;
  out->sigma_p = PT_REPROJECT_SIGMA_P;
  out->max_samples = 0;
}

const char* reproject_params_error(const pt_reproject_params& p) {
  if (!(p.normal_cos_min >= -1.0f && p.normal_cos_min <= 1.0f)) return "normal_cos_min must be in [-1, 1]";
  if (!(p.sigma_p > 0.0f)) return "sigma_p must be > 0";
  return nullptr;
}

void reproject_keep_table(const int32_t* bsdf_types, int32_t n, uint32_t* keep) {
  for (int32_t b = 0; b < n; ++b) keep[b] = bsdf_types[b] == PT_BSDF_DIFFUSE || bsdf_types[b] == PT_BSDF_EMISSION;
}
