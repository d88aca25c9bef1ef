// Pieces shared by the wave-per-row PPO loss kernels (cat_loss.hip,
// multi_loss.hip): butterfly wave reductions that leave the result in every
// lane, and the kernel that turns the three double-precision row sums into
// the four losses.  Everything is in an anonymous namespace: each .hip that
// includes this gets its own copy of the kernel.
#pragma once

#include "common.h"

namespace {

constexpr float NEG_INF = -3.0e38f;

DEV_INLINE float wave_allreduce_sum(float x) {
  #pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) x += __shfl_xor(x, off, WAVE);
  return x;
}

DEV_INLINE float wave_allreduce_max(float x) {
  #pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1)
    x = fmaxf(x, __shfl_xor(x, off, WAVE));
  return x;
}

// acc: {policy_min_sum, ent_sum, value_max_sum} over B rows
__global__ void ppo_rows_finalize_kernel(
    const double* __restrict__ acc, float* __restrict__ losses,  // [4]
    int64_t B, float entcoeff, float vcoeff) {
  const double ib = 1.0 / static_cast<double>(B);
  const float pol = static_cast<float>(-acc[0] * ib);
  const float ent = static_cast<float>(-entcoeff * acc[1] * ib);
  const float val = static_cast<float>(vcoeff * acc[2] * ib);
  losses[0] = pol;
  losses[1] = ent;
  losses[2] = val;
  losses[3] = pol + ent + val;
}

}  // namespace
