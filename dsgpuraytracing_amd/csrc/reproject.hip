// reproject.hip — the film's reprojection across a camera move: the temporal
// half of SVGF (denoise.hip is the spatial half).  For every pixel of the NEW
// camera's frame, the first hit's world-space point is projected into the OLD
// camera, and the old pixel's Welford records are taken over when the two
// first hits agree (same BSDF, close normals, the same plane); the pixel is
// reset otherwise (include/ptgpu.h: pt_reproject_device, pt_film_reproject).
//
// Like the film's, the arithmetic is a definition (ptgpu.h), restated in numpy
// by tests/reproject_helpers.py and compared bit for bit: every operation is
// one separately rounded IEEE f32 operation in the order written there, so
// this translation unit is built without fast-math and with contraction off;
// `/` is the correctly rounded sequence.
//
// Launch shape, as the film kernels: one 256-thread workgroup per 32x32 block
// of the frame's grid, lane = pixel of a 32-pixel row, each lane four rows.
// The two feature loads of the new frame and the two record stores are one
// dwordx4 per lane over contiguous rows; the old pixel q is arbitrary, so the
// old features and records at q are four gathered 16-B loads, issued together
// and only by lanes whose projection landed in the frame.  The output is a
// second record buffer: q is some other lane's p, so in place would race.
// The kept / reset counts are reduced per wave by ballot and popcount, the
// four waves through LDS, and added to the device counter by one two-lane
// vector atomic per workgroup.  Register and LDS figures: DESIGN.md.
#include <hip/hip_runtime.h>

#include <math.h>

#include "reproject.h"

#pragma clang fp contract(off)

namespace ptk {

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
  return (ax * bx + ay * by) + az * bz;
}

__global__ __launch_bounds__(256) void reproject_kernel(ReprojectArgs a) {
  __shared__ uint32_t s_cnt[4][2];
  const int tx = (a.W + 31) >> 5;
  const int x = (((int)blockIdx.x % tx) << 5) + ((int)threadIdx.x & 31);
  const int y0 = (((int)blockIdx.x / tx) << 5) + ((int)threadIdx.x >> 5);
  const size_t plane = (size_t)a.W * (size_t)a.H;
  const float fW = (float)a.W, fH = (float)a.H;
  const ReprojectCam& cam = a.cam;
  uint32_t n_kept = 0, n_reset = 0;  // of the wave (uniform)
  // (every lane takes every trip: the ballots below are whole-wave)
#pragma unroll 1
  for (int i = 0; i < 4; ++i) {
    const int y = y0 + 8 * i;
    const bool in_frame = x < a.W && y < a.H;
    bool ok = false;
    uint4 s = make_uint4(0u, 0u, 0u, 0u), e = make_uint4(0u, 0u, 0u, 0u);
    const size_t p = (size_t)x + (size_t)y * (size_t)a.W;
    if (in_frame) {
      const float4 np = a.fn[p];
      const float4 pp = a.fn[plane + p];
      const int bp = __float_as_int(np.w);
      ok = bp >= 0 && bp < a.n_bsdfs;
      if (ok) ok = a.keep[bp] != 0u;
      // ---- into the old camera
      const float vx = pp.x - cam.pos[0], vy = pp.y - cam.pos[1], vz = pp.z - cam.pos[2];
      const float cx = dot3(vx, vy, vz, cam.c0[0], cam.c0[1], cam.c0[2]);
      const float cy = dot3(vx, vy, vz, cam.c1[0], cam.c1[1], cam.c1[2]);
      const float cz = dot3(vx, vy, vz, cam.c2[0], cam.c2[1], cam.c2[2]);
      ok = ok && cz < 0.0f;
      const float iz = 0.0f - cz;
      const float u = ((cx / iz) / cam.ax + 0.5f) * fW;
      const float w = ((cy / iz) / cam.ay + 0.5f) * fH;
      ok = ok && u >= 0.0f && u < fW && w >= 0.0f && w < fH;  // (a NaN fails)
      if (ok) {
        const size_t q = (size_t)(int)u + (size_t)(int)w * (size_t)a.W;
        const float4 nq = a.fo[q];
        const float4 pq = a.fo[plane + q];
        s = a.rec[q];
        e = a.rec[plane + q];
        // ---- the two first hits agree
        const float c = dot3(np.x, np.y, np.z, nq.x, nq.y, nq.z);
        const float dx = pq.x - pp.x, dy = pq.y - pp.y, dz = pq.z - pp.z;
        const float dist = fabsf(dot3(np.x, np.y, np.z, dx, dy, dz));
        ok = __float_as_int(nq.w) == bp && c >= a.normal_cos_min && dist <= a.sigma_p * pp.w && s.w > 0u;
      }
      if (ok && a.max_samples != 0u && s.w > a.max_samples) {  // the per-pass variance M2 / n stays, the confidence shrinks
        const uint32_t n1 = a.max_samples;
        const float f = (float)n1 / (float)s.w;
        s.x = __float_as_uint(__uint_as_float(s.x) * f);
        s.y = __float_as_uint(__uint_as_float(s.y) * f);
        s.z = __float_as_uint(__uint_as_float(s.z) * f);
        e.y = __float_as_uint(__uint_as_float(e.y) * f);
        const uint32_t k1 = (uint32_t)(((uint64_t)e.z * (uint64_t)n1) / (uint64_t)s.w);
        e.z = k1 > 1u ? k1 : 1u;
        s.w = n1;
      }
      if (!ok) {
        s = make_uint4(0u, 0u, 0u, 0u);
        e = make_uint4(0u, 0u, 0u, 0u);
      }
      a.out[p] = s;
      a.out[plane + p] = e;
    }
    n_kept += (uint32_t)__popcll(__ballot(in_frame && ok));
    n_reset += (uint32_t)__popcll(__ballot(in_frame && !ok));
  }
  if (!a.counts) return;  // (uniform)
  if (((int)threadIdx.x & 63) == 0) {
    s_cnt[threadIdx.x >> 6][0] = n_kept;
    s_cnt[threadIdx.x >> 6][1] = n_reset;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const uint32_t v = (s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x]) + (s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x]);
    if (v) atomicAdd(a.counts + threadIdx.x, (unsigned long long)v);
  }
}

}  // namespace ptk

extern "C" hipError_t ptk_reproject(const ReprojectArgs* a, hipStream_t s) {
  const int grid = ((a->W + 31) / 32) * ((a->H + 31) / 32);
  hipLaunchKernelGGL(ptk::reproject_kernel, dim3(grid), dim3(256), 0, s, *a);
  return hipGetLastError();
}
