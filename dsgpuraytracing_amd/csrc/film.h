// film.h — the device-resident progressive film (film.hip), as pt_api.cpp drives it.
//
// Per pixel p = x + y*W the film keeps two 16-B records in two planes of one
// allocation, so a wave's 64 records are one contiguous 1-KB run per plane:
//   rec[p]       = {sum.r, sum.g, sum.b, n}   f32 f32 f32 u32
//   rec[W*H + p] = {mu, M2, k, pad}           f32 f32 u32 u32
// all zero when clear.  The arithmetic is defined in include/ptgpu.h
// (pt_film_add_pass / pt_film_resolve_device / pt_film_merge_device).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ptgpu.h"

struct FilmAccArgs {
  const int4* tiles;  // clipped tiles (x, y, w, h), each <= 32 x 32 and inside the frame
  uint4* rec;         // 2 * W * H records
  const float* pass;  // the pass: W * H * 3 floats, the frame layout
  int W, H;
  uint32_t spp;
};

struct FilmResolveArgs {
  const uint4* rec;
  const uint32_t* thr;  // the 256 toColor thresholds (pt_to_color_thresholds)
  float* hdr;           // each output nullable
  uint32_t* rgba;
  float* err;
  int W, H;
};

struct FilmErrArgs {
  const int4* tiles;  // clipped tiles (x, y, w, h) of any size, inside the frame (w or h may be 0)
  const uint4* rec;
  float* out;         // one maximum per tile
  int W, H;
};

struct FilmMergeArgs {
  uint4* rec;                  // the film's 2 * W * H records: a, and the result
  const uint4* in;             // the incoming 2 * W * H records: b (no overlap with rec)
  unsigned long long* counts;  // merged, taken, empty, refused: added to
  int W, H;
};

struct ToColorArgs {
  const float* hdr;
  const uint32_t* thr;
  uint32_t* rgba;
  int W;
  int x0, y0, x1, y1;  // clamped to the frame, x0 < x1 and y0 < y1
};

extern "C" hipError_t ptk_film_accumulate(const FilmAccArgs* a, int n_tiles, hipStream_t s);
extern "C" hipError_t ptk_film_resolve(const FilmResolveArgs* a, hipStream_t s);
extern "C" hipError_t ptk_film_tile_error(const FilmErrArgs* a, int n_tiles, hipStream_t s);
extern "C" hipError_t ptk_film_merge(const FilmMergeArgs* a, hipStream_t s);
extern "C" hipError_t ptk_to_color(const ToColorArgs* a, hipStream_t s);
