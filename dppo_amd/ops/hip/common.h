// Common device helpers for dppo_amd CDNA4 (gfx950) kernels.
//
// Written for MI355X: 64-wide wavefronts (every warp idiom uses width 64),
// wave-level __shfl reductions, one atomic per wave (guideline 12), and
// double-precision global accumulators (global_atomic_add_f64 is native on
// CDNA) so large-batch loss reductions keep fp32-class accuracy.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdlib>

#define DEV_INLINE __device__ __forceinline__

constexpr int WAVE = 64;  // CDNA wavefront width (not 32)
constexpr int N_CU = 256;  // MI355X: 256 CUs in 8 XCDs

DEV_INLINE float wave_reduce_sum(float x) {
  #pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) x += __shfl_down(x, off, WAVE);
  return x;
}

// Per-wave reduce then ONE double atomic per wave.
DEV_INLINE void wave_atomic_add(double* dst, float val) {
  float w = wave_reduce_sum(val);
  if ((threadIdx.x & (WAVE - 1)) == 0) atomicAdd(dst, static_cast<double>(w));
}

// Fast tanh: 1 - 2/(e^{2x}+1) via the hardware exp. ~6 instructions vs
// ocml tanhf's branchy ~35; |rel err| ~2e-7, saturates correctly for
// |x| >~ 10 (e^{2x} -> inf -> 1).
DEV_INLINE float fast_tanhf(float x) {
  const float e = __expf(2.0f * x);
  return 1.0f - 2.0f / (e + 1.0f);
}

// x^2+y^2+z^2+w^2 with the contraction spelled out: the split and fused
// env-step kernels must round the reward's chunk sums identically.
DEV_INLINE float sq4(float4 v) {
  return __fmaf_rn(v.w, v.w,
                   __fmaf_rn(v.z, v.z, __fmaf_rn(v.y, v.y, __fmul_rn(v.x, v.x))));
}

DEV_INLINE int64_t gidx() {
  return static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
}

DEV_INLINE int64_t gstride() {
  return static_cast<int64_t>(gridDim.x) * blockDim.x;
}

// Integer tuning knob from the environment (docs/KNOBS.md); `def` when
// unset.  Call sites that must not re-read per call cache the result in a
// function-local static.
inline int env_int(const char* name, int def) {
  const char* e = getenv(name);
  return e ? atoi(e) : def;
}

// Grid sizing for memory-bound elementwise/reduction kernels: cap the
// grid and grid-stride the rest (guideline 11).
inline int elementwise_grid(int64_t n, int block) {
  int64_t g = (n + block - 1) / block;
  const int64_t cap = 2048;
  return static_cast<int>(g < cap ? (g > 0 ? g : 1) : cap);
}
