// v_mfma_f32_32x32x2_f32 fragment helpers and the activation derivative
// shared by the MLP kernels (mfma_gemm.hip, mlp_mid.hip, mlp_train.hip).
//
// Fragment layout (cdna guide §3):
//   lane l: A[i = l&31][k = l>>5], B[k = l>>5][j = l&31]
//   C/D reg r (of 16): row = (r&3) + 8*(r>>2) + 4*(l>>5), col = l&31.
#pragma once

#include "common.h"

using f32x16 = __attribute__((ext_vector_type(16))) float;

DEV_INLINE int cd_row(int reg, int lane) {
  return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
}

// act'(z) from the saved activation h = act(z): tanh or relu.  The two
// expressions are the ones every backward path has always used; results
// move if they are respelled.
DEV_INLINE float act_grad(float h, bool is_tanh) {
  return is_tanh ? (1.f - h * h) : (h > 0.f ? 1.f : 0.f);
}
