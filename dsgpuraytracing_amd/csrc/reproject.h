// reproject.h — the film's reprojection across a camera move (reproject.hip), as
// pt_api.cpp drives it.  Buffers (include/ptgpu.h: "Reprojection"):
//   rec, out      the film's 2 * W * H records (film.h); `out` never aliases `rec`
//   fo, fn        the feature buffers of the old and of the new camera (denoise.h)
//   keep[b]       1: the radiance of BSDF b's first hit does not depend on the view
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ptgpu.h"
#include "reproject_host.h"

struct ReprojectArgs {
  const uint4* rec;
  const float4* fo;
  const float4* fn;
  const uint32_t* keep;        // n_bsdfs entries (never read when n_bsdfs is 0)
  uint4* out;
  unsigned long long* counts;  // nullable: [kept, reset], added to
  int W, H;
  int n_bsdfs;
  ReprojectCam cam;            // the OLD camera
  float normal_cos_min, sigma_p;
  uint32_t max_samples;
};

extern "C" hipError_t ptk_reproject(const ReprojectArgs* a, hipStream_t s);
