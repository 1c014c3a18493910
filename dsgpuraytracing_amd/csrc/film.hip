// film.hip — the device-resident progressive film: accumulate a pass, resolve
// to the HDR mean / the RGBA8 toColor codes / the per-pixel error, and the
// per-tile maximum of that error, and the merge of another film's records into
// it (include/ptgpu.h: pt_film_*), plus pt_to_color_device, which shares the
// resolve's tonemap.
//
// The film arithmetic is a definition (ptgpu.h), restated in numpy by
// tests/film_helpers.py and compared bit for bit: every operation is one
// separately rounded IEEE f32 operation, so this translation unit is built
// without fast-math and with contraction off (x*y+z would become v_fma_f32);
// `/` and sqrtf are the correctly rounded sequences.
//
// Launch shape, as resolve_kernel (pt_kernels.hip): one 256-thread workgroup
// per <= 32x32 tile, lane = pixel of a 32-pixel row, so each record plane and
// each output is read or written as whole contiguous rows (16 B per lane: one
// dwordx4 per record).  The kernels stay small (VGPR and LDS figures in
// DESIGN.md): they run beside the next pass's persistent render waves.
#include <hip/hip_runtime.h>

#include <math.h>

#include "film.h"
#include "tonemap.h"

#pragma clang fp contract(off)

namespace ptk {

// Standard error of the pass-weighted mean luminance relative to the mean.
__device__ __forceinline__ float film_error(uint32_t n, float mu, float M2, uint32_t k) {
  if (k < 2u) return INFINITY;
  return sqrtf((fmaxf(M2, 0.0f) / (float)n) / (float)(k - 1u)) / fmaxf(mu, PT_FILM_LUM_FLOOR);
}

__global__ __launch_bounds__(256) void film_accumulate_kernel(FilmAccArgs a) {
  const int4 t = a.tiles[blockIdx.x];
  const size_t plane = (size_t)a.W * (size_t)a.H;
  const float w = (float)a.spp;
  const int dx = (int)threadIdx.x & 31;
  if (dx >= t.z) return;
  for (int dy = (int)threadIdx.x >> 5; dy < t.w; dy += 8) {
    const size_t p = (size_t)(t.x + dx) + (size_t)(t.y + dy) * (size_t)a.W;
    const float* m = a.pass + 3 * p;
    const float mr = m[0], mg = m[1], mb = m[2];
    uint4 s = a.rec[p];
    uint4 e = a.rec[plane + p];
    s.x = __float_as_uint(__uint_as_float(s.x) + mr * w);
    s.y = __float_as_uint(__uint_as_float(s.y) + mg * w);
    s.z = __float_as_uint(__uint_as_float(s.z) + mb * w);
    s.w += a.spp;
    const float L = (0.2126f * mr + 0.7152f * mg) + 0.0722f * mb;  // Spectrum::illum
    const float Wn = (float)s.w;
    float mu = __uint_as_float(e.x);
    const float d = L - mu;
    mu = mu + d * (w / Wn);
    e.x = __float_as_uint(mu);
    e.y = __float_as_uint(__uint_as_float(e.y) + (w * d) * (L - mu));
    e.z += 1u;
    a.rec[p] = s;
    a.rec[plane + p] = e;
  }
}

// Whole frame, one workgroup per tile of the 32x32 grid.
__global__ __launch_bounds__(256) void film_resolve_kernel(FilmResolveArgs a) {
  __shared__ uint32_t s_thr[256];
  if (a.rgba) {  // (uniform)
    s_thr[threadIdx.x] = a.thr[threadIdx.x];
    __syncthreads();
  }
  const int tx = (a.W + 31) >> 5;
  const int x = (((int)blockIdx.x % tx) << 5) + ((int)threadIdx.x & 31);
  const int y0 = ((int)blockIdx.x / tx) << 5;
  if (x >= a.W) return;
  const size_t plane = (size_t)a.W * (size_t)a.H;
  const int y1 = min(y0 + 32, a.H);
  for (int y = y0 + ((int)threadIdx.x >> 5); y < y1; y += 8) {
    const size_t p = (size_t)x + (size_t)y * (size_t)a.W;
    const uint4 s = a.rec[p];
    if (a.hdr || a.rgba) {
      float r = 0.0f, g = 0.0f, b = 0.0f;
      if (s.w) {
        const float n = (float)s.w;
        r = __uint_as_float(s.x) / n;
        g = __uint_as_float(s.y) / n;
        b = __uint_as_float(s.z) / n;
      }
      if (a.hdr) {
        float* o = a.hdr + 3 * p;
        o[0] = r;
        o[1] = g;
        o[2] = b;
      }
      if (a.rgba) a.rgba[p] = to_color_rgba(s_thr, r, g, b);
    }
    if (a.err) {
      const uint4 e = a.rec[plane + p];
      a.err[p] = film_error(s.w, __uint_as_float(e.x), __uint_as_float(e.y), e.z);
    }
  }
}

// One workgroup per listed tile (any size): the maximum of the error over its
// pixels, lanes reduced by shuffles, the four waves through LDS.  The error is
// >= 0 or +inf; an empty tile gives 0.
__global__ __launch_bounds__(256) void film_tile_error_kernel(FilmErrArgs a) {
  __shared__ float s_max[4];
  const int4 t = a.tiles[blockIdx.x];
  const size_t plane = (size_t)a.W * (size_t)a.H;
  float v = 0.0f;
  for (int dy = (int)threadIdx.x >> 5; dy < t.w; dy += 8)
    for (int dx = (int)threadIdx.x & 31; dx < t.z; dx += 32) {
      const size_t p = (size_t)(t.x + dx) + (size_t)(t.y + dy) * (size_t)a.W;
      const uint32_t n = a.rec[p].w;
      const uint4 e = a.rec[plane + p];
      v = fmaxf(v, film_error(n, __uint_as_float(e.x), __uint_as_float(e.y), e.z));
    }
#pragma unroll
  for (int off = 32; off; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  if (((int)threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) a.out[blockIdx.x] = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
}

// pt_film_merge_device: film <- film (+) incoming records, the pairwise
// combine of two Welford states (Chan et al.) as ptgpu.h defines it.  Whole
// frame, the resolve's shape; each lane four rows.  A pixel's four records
// are loaded together; only a taken or merged pixel stores.  The four class
// counts are reduced per wave by ballot and popcount, the four waves through
// LDS, and added to the device counter by one four-lane vector atomic per
// workgroup (as reproject.hip counts kept and reset).
__global__ __launch_bounds__(256) void film_merge_kernel(FilmMergeArgs a) {
  __shared__ uint32_t s_cnt[4][4];
  const int tx = (a.W + 31) >> 5;
  const int x = (((int)blockIdx.x % tx) << 5) + ((int)threadIdx.x & 31);
  const int y0 = (((int)blockIdx.x / tx) << 5) + ((int)threadIdx.x >> 5);
  const size_t plane = (size_t)a.W * (size_t)a.H;
  uint32_t n_cls[4] = {0, 0, 0, 0};  // merged, taken, empty, refused of the wave (uniform)
  // (every lane takes every trip: the ballots below are whole-wave)
#pragma unroll 1
  for (int i = 0; i < 4; ++i) {
    const int y = y0 + 8 * i;
    const bool in_frame = x < a.W && y < a.H;
    int cls = -1;
    if (in_frame) {
      const size_t p = (size_t)x + (size_t)y * (size_t)a.W;
      const uint4 sb = a.in[p];
      const uint4 eb = a.in[plane + p];
      uint4 s = a.rec[p];
      uint4 e = a.rec[plane + p];
      const uint32_t n = s.w + sb.w;
      if (sb.w == 0u) {
        cls = 2;
      } else if (s.w == 0u) {
        cls = 1;
        s = sb;
        e = eb;
      } else if (n < s.w) {  // n_a + n_b does not fit in 32 bits
        cls = 3;
      } else {
        cls = 0;
        const float na = (float)s.w, nb = (float)sb.w;
        const float Wn = (float)n;
        s.x = __float_as_uint(__uint_as_float(s.x) + __uint_as_float(sb.x));
        s.y = __float_as_uint(__uint_as_float(s.y) + __uint_as_float(sb.y));
        s.z = __float_as_uint(__uint_as_float(s.z) + __uint_as_float(sb.z));
        s.w = n;
        const float mu_a = __uint_as_float(e.x);
        const float d = __uint_as_float(eb.x) - mu_a;
        e.x = __float_as_uint(mu_a + d * (nb / Wn));
        e.y = __float_as_uint((__uint_as_float(e.y) + __uint_as_float(eb.y)) + (d * d) * ((na * nb) / Wn));
        e.z += eb.z;
      }
      if (cls < 2) {
        a.rec[p] = s;
        a.rec[plane + p] = e;
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) n_cls[c] += (uint32_t)__popcll(__ballot(cls == c));
  }
  if (((int)threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 4; ++c) s_cnt[threadIdx.x >> 6][c] = n_cls[c];
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const uint32_t v = (s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x]) + (s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x]);
    if (v) atomicAdd(a.counts + threadIdx.x, (unsigned long long)v);
  }
}

// pt_to_color_device: one workgroup per 32x32 block of the rectangle.
__global__ __launch_bounds__(256) void to_color_kernel(ToColorArgs a) {
  __shared__ uint32_t s_thr[256];
  s_thr[threadIdx.x] = a.thr[threadIdx.x];
  __syncthreads();
  const int tx = (a.x1 - a.x0 + 31) >> 5;
  const int x = a.x0 + (((int)blockIdx.x % tx) << 5) + ((int)threadIdx.x & 31);
  const int y0 = a.y0 + (((int)blockIdx.x / tx) << 5);
  if (x >= a.x1) return;
  const int y1 = min(y0 + 32, a.y1);
  for (int y = y0 + ((int)threadIdx.x >> 5); y < y1; y += 8) {
    const size_t p = (size_t)x + (size_t)y * (size_t)a.W;
    const float* c = a.hdr + 3 * p;
    a.rgba[p] = to_color_rgba(s_thr, c[0], c[1], c[2]);
  }
}

}  // namespace ptk

extern "C" hipError_t ptk_film_accumulate(const FilmAccArgs* a, int n_tiles, hipStream_t s) {
  if (n_tiles <= 0) return hipSuccess;
  hipLaunchKernelGGL(ptk::film_accumulate_kernel, dim3(n_tiles), dim3(256), 0, s, *a);
  return hipGetLastError();
}

extern "C" hipError_t ptk_film_resolve(const FilmResolveArgs* a, hipStream_t s) {
  const int grid = ((a->W + 31) / 32) * ((a->H + 31) / 32);
  hipLaunchKernelGGL(ptk::film_resolve_kernel, dim3(grid), dim3(256), 0, s, *a);
  return hipGetLastError();
}

extern "C" hipError_t ptk_film_tile_error(const FilmErrArgs* a, int n_tiles, hipStream_t s) {
  if (n_tiles <= 0) return hipSuccess;
  hipLaunchKernelGGL(ptk::film_tile_error_kernel, dim3(n_tiles), dim3(256), 0, s, *a);
  return hipGetLastError();
}

extern "C" hipError_t ptk_film_merge(const FilmMergeArgs* a, hipStream_t s) {
  const int grid = ((a->W + 31) / 32) * ((a->H + 31) / 32);
  hipLaunchKernelGGL(ptk::film_merge_kernel, dim3(grid), dim3(256), 0, s, *a);
  return hipGetLastError();
}

extern "C" hipError_t ptk_to_color(const ToColorArgs* a, hipStream_t s) {
  const int grid = ((a->x1 - a->x0 + 31) / 32) * ((a->y1 - a->y0 + 31) / 32);
  if (grid <= 0) return hipSuccess;
  hipLaunchKernelGGL(ptk::to_color_kernel, dim3(grid), dim3(256), 0, s, *a);
  return hipGetLastError();
}
