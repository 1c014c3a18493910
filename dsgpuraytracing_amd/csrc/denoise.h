// denoise.h — the edge-avoiding a-trous film denoiser (denoise.hip), as pt_api.cpp
// drives it.  Buffers (include/ptgpu.h: "Feature buffers" / "Denoiser"):
//   feat[p], feat[W*H + p]   the first-hit feature records {N, bsdf}, {P, z}
//   cv[p] = {r, g, b, v}     the working record: colour and the variance of the
//                            mean luminance (+inf: unknown, !(v >= 0): invalid)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ptgpu.h"

struct DenoiseIterArgs {
  const float4* in;    // W * H records, read
  float4* out;         // W * H records, written (never `in`)
  const float4* feat;  // 2 * W * H feature records
  int W, H;
  int step;            // 1 << iteration
  int normal_squarings;
  float sigma_l, sigma_p;
};

struct DenoisePrepareArgs {
  const uint4* rec;  // the film's 2 * W * H records (film.h)
  float4* cv;
  int W, H;
};

struct DenoiseFinishArgs {
  const float4* cv;
  const uint32_t* thr;  // the 256 toColor thresholds
  float* hdr;           // each output nullable
  uint32_t* rgba;
  int W, H;
};

extern "C" hipError_t ptk_denoise_iteration(const DenoiseIterArgs* a, hipStream_t s);
extern "C" hipError_t ptk_denoise_prepare(const DenoisePrepareArgs* a, hipStream_t s);
extern "C" hipError_t ptk_denoise_finish(const DenoiseFinishArgs* a, hipStream_t s);
// Every record of the feature buffer to the miss record.
extern "C" hipError_t ptk_features_clear(float4* feat, int W, int H, hipStream_t s);
