// Classic-control device math: the CartPole-v0 and Pendulum-v1 transitions,
// their reset draws and observations, as functions of scalars.  The float32
// expressions are those of envs/classic.py (cartpole_step, pendulum_step),
// which the tests hold the kernel to.  sinf / cosf / floorf are the accurate
// forms on purpose: the state is integrated over hundreds of steps.
// RNG, slot scheme and samplers are rollout_math.h's.
#pragma once

#include "rollout_math.h"

constexpr int ENV_CARTPOLE = 0;
constexpr int ENV_PENDULUM = 1;

// per-env shapes: S state scalars, D observation scalars
template <int ENV>
struct ClassicEnv;

template <>
struct ClassicEnv<ENV_CARTPOLE> {
  static constexpr int S = 4;  // x, x_dot, theta, theta_dot
  static constexpr int D = 4;  // the state itself
};

template <>
struct ClassicEnv<ENV_PENDULUM> {
  static constexpr int S = 2;  // theta, theta_dot
  static constexpr int D = 3;  // cos theta, sin theta, theta_dot
};

// One Euler step (tau = 0.02) under action a (1 pushes right, else left),
// all from the old state.  Reward 1; returns the termination flag of the
// new state (|x| > 2.4 or |theta| > 12 degrees).
DEV_INLINE int cartpole_step(float* s, int a, float& reward) {
  const float x = s[0], xd = s[1], th = s[2], thd = s[3];
  const float force = (a == 1) ? 10.0f : -10.0f;
  const float sn = sinf(th), cs = cosf(th);
  const float temp = (force + 0.05f * thd * thd * sn) / 1.1f;
  const float thacc =
      (9.8f * sn - cs * temp) / (0.5f * (4.0f / 3.0f - 0.1f * cs * cs / 1.1f));
  const float xacc = temp - 0.05f * thacc * cs / 1.1f;
  s[0] = x + 0.02f * xd;
  s[1] = xd + 0.02f * xacc;
  s[2] = th + 0.02f * thd;
  s[3] = thd + 0.02f * thacc;
  reward = 1.0f;
  return (fabsf(s[0]) > 2.4f || fabsf(s[2]) > 0.20943951f) ? 1 : 0;
}

// One step (dt = 0.05) under the UNCLIPPED action a: the torque is
// 2 clip(a, -1, 1), the reward uses the old theta, theta' is wrapped into
// [-pi, pi).  Never terminates.
DEV_INLINE int pendulum_step(float* s, float a, float& reward) {
  const float th = s[0], thd = s[1];
  const float u = 2.0f * fminf(fmaxf(a, -1.0f), 1.0f);
  reward = -(th * th + 0.1f * thd * thd + 0.001f * u * u);
  const float thd2 =
      fminf(fmaxf(thd + (15.0f * sinf(th) + 3.0f * u) * 0.05f, -8.0f), 8.0f);
  const float z = th + 0.05f * thd2;
  s[0] = z - 6.2831853071795865f *
                 floorf((z + 3.1415926535897932f) / 6.2831853071795865f);
  s[1] = thd2;
  return 0;
}

// fresh state of a finished env: dim d uniform in (-half_d, half_d] from the
// RNG_SLOT_RESET + d draw of (env, step)
template <int ENV>
DEV_INLINE void classic_reset(float* s, unsigned seed, int env, int step) {
#pragma unroll
  for (int d = 0; d < ClassicEnv<ENV>::S; ++d) {
    const float half = (ENV == ENV_CARTPOLE) ? 0.05f
                       : (d == 0)            ? 3.1415926535897932f
                                             : 1.0f;
    const float u = rng_uniform(seed, env, step, RNG_SLOT_RESET + d);
    s[d] = (2.0f * u - 1.0f) * half;
  }
}

// observation of state s
template <int ENV>
DEV_INLINE void classic_obs(const float* s, float* x) {
  if constexpr (ENV == ENV_CARTPOLE) {
#pragma unroll
    for (int d = 0; d < 4; ++d) x[d] = s[d];
  } else {
    x[0] = cosf(s[0]);
    x[1] = sinf(s[0]);
    x[2] = s[1];
  }
}
