// LDS tile staging shared by the row-per-lane loss kernels (ppo_loss.hip,
// disc_gh.hip): a 256-thread block moves a [rows][width] contiguous global
// stream into padded (odd-stride, bank-conflict-free) LDS rows and back.
// Everything is in an anonymous namespace: each .hip that includes this gets
// its own copy.
#pragma once

#include "common.h"

namespace {

// Stage a [rows][width] contiguous global stream into padded LDS rows.
// Global side is float4 where width >= 8 (the caller guarantees the
// base is 16-B aligned: tile_base*width is a multiple of 4), LDS side
// is 4 scalar writes with an at-most-one row wrap per group.  row/col
// kept by increment — one div/mod per stream, not per element.
DEV_INLINE void stage_tile(const float* __restrict__ src,
                           float* __restrict__ dst, int width, int stride,
                           int rows, int tid) {
  const int n = rows * width;
  if (width >= 8) {
    const float4* s4 = reinterpret_cast<const float4*>(src);
    const int n4 = n >> 2;
    const int dr = 1024 / width, dc = 1024 % width;
    int r = (tid * 4) / width, c = (tid * 4) % width;
    for (int q = tid; q < n4; q += 256) {
      const float4 v = s4[q];
      int rr = r, cc = c;
      const float vv[4] = {v.x, v.y, v.z, v.w};
      #pragma unroll
      for (int k = 0; k < 4; ++k) {
        dst[rr * stride + cc] = vv[k];
        if (++cc == width) { cc = 0; ++rr; }
      }
      r += dr; c += dc;
      if (c >= width) { c -= width; ++r; }
    }
    for (int g = (n4 << 2) + tid; g < n; g += 256)
      dst[(g / width) * stride + g % width] = src[g];
  } else {
    const int dr = 256 / width, dc = 256 % width;
    for (int g = tid, r = tid / width, c = tid % width; g < n; g += 256) {
      dst[r * stride + c] = src[g];
      r += dr; c += dc;
      if (c >= width) { c -= width; r += 1; }
    }
  }
}

// The same for an int64 stream, narrowed to int32 on the LDS side (action
// indices: half the LDS of the global form).  One 8-B load per lane.
DEV_INLINE void stage_tile_i64(const int64_t* __restrict__ src,
                               int* __restrict__ dst, int width, int stride,
                               int rows, int tid) {
  const int n = rows * width;
  const int dr = 256 / width, dc = 256 % width;
  for (int g = tid, r = tid / width, c = tid % width; g < n; g += 256) {
    dst[r * stride + c] = static_cast<int>(src[g]);
    r += dr; c += dc;
    if (c >= width) { c -= width; r += 1; }
  }
}

// Store padded LDS rows [rows][width] (row stride `stride`) to a contiguous
// global [rows][width], float4 on the global side.  width is a multiple of
// 4 and >= 4, so rows*width is too and a group wraps at most once; dst is
// 16-B aligned (tile_base*width floats into an aligned buffer).
DEV_INLINE void store_tile(const float* __restrict__ src,
                           float* __restrict__ dst, int width, int stride,
                           int rows, int tid) {
  const int n4 = (rows * width) >> 2;
  float4* d4 = reinterpret_cast<float4*>(dst);
  const int dr = 1024 / width, dc = 1024 % width;
  int r = (tid * 4) / width, c = (tid * 4) % width;
  for (int q = tid; q < n4; q += 256) {
    float vv[4];
    int rr = r, cc = c;
    #pragma unroll
    for (int k = 0; k < 4; ++k) {
      vv[k] = src[rr * stride + cc];
      if (++cc == width) { cc = 0; ++rr; }
    }
    d4[q] = make_float4(vv[0], vv[1], vv[2], vv[3]);
    r += dr; c += dc;
    if (c >= width) { c -= width; ++r; }
  }
}

}  // namespace
