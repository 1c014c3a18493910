// denoise.hip — the film's edge-avoiding a-trous wavelet denoiser (Dammertz et
// al. 2010, with the variance-guided luminance weight of SVGF's spatial pass):
// the prepare kernel (film records -> working records), one kernel per
// iteration, the finish kernel (working records -> HDR / RGBA8), and the fill
// of a feature buffer with the miss record (include/ptgpu.h: pt_denoise_*,
// pt_film_denoise_*).
//
// Like the film's, the arithmetic is a definition (ptgpu.h), restated in numpy
// by tests/denoise_helpers.py and compared bit for bit: every operation is one
// separately rounded IEEE f32 operation in the order written there, so this
// translation unit is built without fast-math and with contraction off; `/`
// and sqrtf are the correctly rounded sequences.  A skipped tap leaves the
// sums untouched (a select), it is never multiplied by zero.
//
// Launch shape, as the film kernels: one 256-thread workgroup per 32x32 tile
// of the frame's grid, lane = pixel of a 32-pixel row, each lane four rows.
// The centre's records stay in registers; a tap is three dwordx4 loads (the
// working record and the two feature records) from plain global memory: at
// step >= 4 the 25 taps span more than any LDS tile would hold, and rows of a
// wave's taps are contiguous 512-B runs served by L1/L2.  A tap row's fifteen
// loads are issued together, at coordinates clamped into the frame (the tap
// itself is dropped by a flag).  Register and LDS figures: DESIGN.md.
#include <hip/hip_runtime.h>

#include <math.h>

#include "denoise.h"
#include "tonemap.h"

#pragma clang fp contract(off)

namespace ptk {

__device__ __forceinline__ bool is_finite(float x) { return fabsf(x) < INFINITY; }  // (false for NaN)

__device__ __forceinline__ float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

__global__ __launch_bounds__(256) void denoise_prepare_kernel(DenoisePrepareArgs a) {
  const int tx = (a.W + 31) >> 5;
  const int x = (((int)blockIdx.x % tx) << 5) + ((int)threadIdx.x & 31);
  const int y0 = ((int)blockIdx.x / tx) << 5;
  if (x >= a.W) return;
  const size_t plane = (size_t)a.W * (size_t)a.H;
  const int y1 = min(y0 + 32, a.H);
  for (int y = y0 + ((int)threadIdx.x >> 5); y < y1; y += 8) {
    const size_t p = (size_t)x + (size_t)y * (size_t)a.W;
    const uint4 s = a.rec[p];
    const uint4 e = a.rec[plane + p];
    float4 o = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
    if (s.w) {
      const float n = (float)s.w;
      o.x = __uint_as_float(s.x) / n;
      o.y = __uint_as_float(s.y) / n;
      o.z = __uint_as_float(s.z) / n;
      o.w = e.z >= 2u ? (fmaxf(__uint_as_float(e.y), 0.0f) / n) / (float)(e.z - 1u) : INFINITY;
    }
    a.cv[p] = o;
  }
}

__global__ __launch_bounds__(256) void denoise_iteration_kernel(DenoiseIterArgs a) {
  const int tx = (a.W + 31) >> 5;
  const int x = (((int)blockIdx.x % tx) << 5) + ((int)threadIdx.x & 31);
  const int y0 = ((int)blockIdx.x / tx) << 5;
  if (x >= a.W) return;
  const size_t plane = (size_t)a.W * (size_t)a.H;
  const int y1 = min(y0 + 32, a.H);
  for (int y = y0 + ((int)threadIdx.x >> 5); y < y1; y += 8) {
    const size_t p = (size_t)x + (size_t)y * (size_t)a.W;
    const float4 cp = a.in[p];
    if (!(cp.w >= 0.0f)) {  // invalid: never rendered, or NaN
      a.out[p] = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
      continue;
    }
    if (!(is_finite(cp.x) && is_finite(cp.y) && is_finite(cp.z))) {
      a.out[p] = cp;
      continue;
    }
    const float4 np = a.feat[p];
    const float4 pp = a.feat[plane + p];
    const int bp = __float_as_int(np.w);
    const bool hit = bp >= 0;
    const bool known = cp.w < INFINITY;
    // ---- variance prefilter: 3x3 at distance 1, weights 1/4, 1/8, 1/16
    float den = 1.0f;
    if (known) {
      float sv = 0.0f, sg = 0.0f;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
        const int qy = y + dy;
        const bool rowin = qy >= 0 && qy < a.H;
        const int cy = min(max(qy, 0), a.H - 1);
        float v[3];
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const int cx = min(max(x + dx, 0), a.W - 1);
          v[dx + 1] = a.in[(size_t)cx + (size_t)cy * (size_t)a.W].w;
        }
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const int qx = x + dx;
          const float g = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
          const float vq = v[dx + 1];
          const bool use = rowin && qx >= 0 && qx < a.W && vq >= 0.0f && vq < INFINITY;
          const float t = g * vq;
          sv = use ? sv + t : sv;
          sg = use ? sg + g : sg;
        }
      }
      const float vf = sv / sg;
      const float sd = sqrtf(vf);
      den = a.sigma_l * sd + 1e-6f;
    }
    const float Lp = lum(cp.x, cp.y, cp.z);
    const float pden = a.sigma_p * pp.w;
    // ---- the 5x5 taps at distance `step`
    float sr = 0.0f, sgn = 0.0f, sb = 0.0f, sw = 0.0f, sv2 = 0.0f;
#pragma unroll 1
    for (int dy = -2; dy <= 2; ++dy) {
      const int qy = y + dy * a.step;
      if (qy < 0 || qy >= a.H) continue;
      const float ky = dy == 0 ? 0.375f : (dy == 1 || dy == -1) ? 0.25f : 0.0625f;
      float4 cq[5], nq[5], pq[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const int cx = min(max(x + (j - 2) * a.step, 0), a.W - 1);
        const size_t q = (size_t)cx + (size_t)qy * (size_t)a.W;
        cq[j] = a.in[q];
        nq[j] = a.feat[q];
        pq[j] = a.feat[plane + q];
      }
      float c[5];
#pragma unroll
      for (int j = 0; j < 5; ++j)
        c[j] = fmaxf(0.0f, (np.x * nq[j].x + np.y * nq[j].y) + np.z * nq[j].z);
      for (int i = 0; i < a.normal_squarings; ++i) {
#pragma unroll
        for (int j = 0; j < 5; ++j) c[j] = c[j] * c[j];
      }
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const int qx = x + (j - 2) * a.step;
        const float kx = j == 2 ? 0.375f : (j == 1 || j == 3) ? 0.25f : 0.0625f;
        const float h = kx * ky;
        const bool use = qx >= 0 && qx < a.W && cq[j].w >= 0.0f && is_finite(cq[j].x) && is_finite(cq[j].y) &&
                         is_finite(cq[j].z) && __float_as_int(nq[j].w) == bp;
        const float ddx = pq[j].x - pp.x, ddy = pq[j].y - pp.y, ddz = pq[j].z - pp.z;
        const float xp = fabsf((np.x * ddx + np.y * ddy) + np.z * ddz) / pden;
        const float w_n = hit ? c[j] : 1.0f;
        const float w_p = hit ? fmaxf(0.0f, 1.0f - xp) : 1.0f;
        const float xl = fabsf(lum(cq[j].x, cq[j].y, cq[j].z) - Lp) / den;
        const float w_l = known ? 1.0f / (1.0f + xl * xl) : 1.0f;
        float w = ((h * w_n) * w_p) * w_l;
        w = (j == 2 && dy == 0) ? h : w;  // the centre tap
        const float vq = cq[j].w == INFINITY ? cp.w : cq[j].w;
        const float tr = w * cq[j].x, tg = w * cq[j].y, tb = w * cq[j].z, tv = (w * w) * vq;
        sr = use ? sr + tr : sr;
        sgn = use ? sgn + tg : sgn;
        sb = use ? sb + tb : sb;
        sw = use ? sw + w : sw;
        sv2 = use ? sv2 + tv : sv2;
      }
    }
    float4 o;
    o.x = sr / sw;
    o.y = sgn / sw;
    o.z = sb / sw;
    o.w = known ? sv2 / (sw * sw) : INFINITY;
    a.out[p] = o;
  }
}

__global__ __launch_bounds__(256) void denoise_finish_kernel(DenoiseFinishArgs a) {
  __shared__ uint32_t s_thr[256];
  if (a.rgba) {  // (uniform)
    s_thr[threadIdx.x] = a.thr[threadIdx.x];
    __syncthreads();
  }
  const int tx = (a.W + 31) >> 5;
  const int x = (((int)blockIdx.x % tx) << 5) + ((int)threadIdx.x & 31);
  const int y0 = ((int)blockIdx.x / tx) << 5;
  if (x >= a.W) return;
  const int y1 = min(y0 + 32, a.H);
  for (int y = y0 + ((int)threadIdx.x >> 5); y < y1; y += 8) {
    const size_t p = (size_t)x + (size_t)y * (size_t)a.W;
    const float4 c = a.cv[p];
    if (a.hdr) {
      float* o = a.hdr + 3 * p;
      o[0] = c.x;
      o[1] = c.y;
      o[2] = c.z;
    }
    if (a.rgba) a.rgba[p] = to_color_rgba(s_thr, c.x, c.y, c.z);
  }
}

__global__ __launch_bounds__(256) void features_clear_kernel(float4* feat, size_t plane) {
  const size_t p = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (p >= plane) return;
  feat[p] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
  feat[plane + p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

}  // namespace ptk

static int frame_grid(int W, int H) { return ((W + 31) / 32) * ((H + 31) / 32); }

extern "C" hipError_t ptk_denoise_prepare(const DenoisePrepareArgs* a, hipStream_t s) {
  hipLaunchKernelGGL(ptk::denoise_prepare_kernel, dim3(frame_grid(a->W, a->H)), dim3(256), 0, s, *a);
  return hipGetLastError();
}

extern "C" hipError_t ptk_denoise_iteration(const DenoiseIterArgs* a, hipStream_t s) {
  hipLaunchKernelGGL(ptk::denoise_iteration_kernel, dim3(frame_grid(a->W, a->H)), dim3(256), 0, s, *a);
  return hipGetLastError();
}

extern "C" hipError_t ptk_denoise_finish(const DenoiseFinishArgs* a, hipStream_t s) {
  hipLaunchKernelGGL(ptk::denoise_finish_kernel, dim3(frame_grid(a->W, a->H)), dim3(256), 0, s, *a);
  return hipGetLastError();
}

extern "C" hipError_t ptk_features_clear(float4* feat, int W, int H, hipStream_t s) {
  const size_t plane = (size_t)W * (size_t)H;
  hipLaunchKernelGGL(ptk::features_clear_kernel, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, s, feat, plane);
  return hipGetLastError();
}
