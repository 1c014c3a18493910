// tonemap.h — the device tonemap shared by the film's resolve, pt_to_color_device
// (film.hip) and the denoiser's finish kernel (denoise.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ptk {

// HDRImageBuffer::toColor's 8-bit code of one channel, as the host's pt_to_color
// (image_out.cpp) computes it: the code is a non-decreasing step function of
// the float's bit pattern, so it is the number of thresholds thr[1..255] at or
// below the bits (thr[0] = 0): the largest k with thr[k] <= bits, by an 8-step
// branchless search of the table in LDS.  Sign bit set: the host's powf path
// gives 0 for -0.0f and 255 (NaN -> 255) for everything else; a positive NaN's
// bits lie above every threshold (255).
__device__ __forceinline__ uint32_t to_color_code(const uint32_t* thr, float v) {
  const uint32_t b = __float_as_uint(v);
  uint32_t k = 0;
#pragma unroll
  for (uint32_t s = 128; s; s >>= 1) k += thr[k + s] <= b ? s : 0u;
  return b == 0x80000000u ? 0u : k;  // (any other bits >= 2^31 are above every threshold: 255)
}

__device__ __forceinline__ uint32_t to_color_rgba(const uint32_t* thr, float r, float g, float b) {
  return (255u << 24) + (to_color_code(thr, b) << 16) + (to_color_code(thr, g) << 8) + to_color_code(thr, r);
}

}  // namespace ptk
