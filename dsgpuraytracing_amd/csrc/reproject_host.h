// reproject_host.h — the host side of the film's reprojection, as pure
// functions: the camera as the kernel's f32 arguments, the orthonormality test
// projection by dot products needs, the parameter check and the keep table of
// a BSDF list.  Plain C++17, no HIP: it runs, and is tested
// (tests/test_reproject_host.py), without a GPU.
#pragma once
#include <stdint.h>

#include "../../include/ptgpu.h"

// The camera as features_launch (pt_api.cpp) hands it to the feature kernel:
// every double rounded to f32 once, a = (float)(screen / screen_dist).
struct ReprojectCam {
  float pos[3];
  float c0[3], c1[3], c2[3];  // the columns of c2w
  float ax, ay;
};
void reproject_camera(const pt_camera& cam, ReprojectCam* out);

// |column_i . column_j - delta_ij| <= 1e-9 for every pair: the test of
// footprint_rect (launch_plan.cpp).  False for a NaN.
bool reproject_orthonormal(const pt_camera& cam);

void reproject_params_default(pt_reproject_params* out);
// nullptr when the parameters are valid, else what is wrong with them.
const char* reproject_params_error(const pt_reproject_params& p);

// keep[b] = 1 for PT_BSDF_DIFFUSE and PT_BSDF_EMISSION, 0 for every other type.
void reproject_keep_table(const int32_t* bsdf_types, int32_t n, uint32_t* keep);
