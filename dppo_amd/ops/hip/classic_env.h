// Classic-control device math: the CartPole-v0, Pendulum-v1, Acrobot-v1,
// MountainCar-v0 and MountainCarContinuous-v0 transitions, their reset draws
// and observations, as functions of scalars.
// The float32 expressions are those of envs/classic.py (cartpole_step,
// pendulum_step, acrobot_step, mountaincar_step, mountaincar_cont_step),
// which the tests hold the kernel to.  sinf / cosf / floorf are the accurate
// forms on purpose: the state is integrated over hundreds of steps.
// RNG, slot scheme and samplers are rollout_math.h's.
#pragma once

#include "rollout_math.h"

constexpr int ENV_CARTPOLE = 0;
constexpr int ENV_PENDULUM = 1;
constexpr int ENV_ACROBOT = 2;
constexpr int ENV_MOUNTAINCAR = 3;
constexpr int ENV_MOUNTAINCAR_CONT = 4;

// Per-env traits.  Shapes: S state scalars, D observation scalars, P
// policy-head columns (Categorical: the logits; DiagGaussian with A = 1:
// mean, logstd).  BOX: the policy is the DiagGaussian (else Categorical).
// Reset: state dim d is drawn uniform in (center(d) - half(d), center(d) +
// half(d)]; a dim with half 0 starts at its centre.
template <int ENV>
struct ClassicEnv;

template <>
struct ClassicEnv<ENV_CARTPOLE> {
  static constexpr int S = 4;  // x, x_dot, theta, theta_dot
  static constexpr int D = 4;  // the state itself
  static constexpr int P = 2;
  static constexpr bool BOX = false;
  static constexpr float reset_half(int) { return 0.05f; }
  static constexpr float reset_center(int) { return 0.0f; }
};

template <>
struct ClassicEnv<ENV_PENDULUM> {
  static constexpr int S = 2;  // theta, theta_dot
  static constexpr int D = 3;  // cos theta, sin theta, theta_dot
  static constexpr int P = 2;
  static constexpr bool BOX = true;
  static constexpr float reset_half(int d) {
    return d == 0 ? 3.1415926535897932f : 1.0f;
  }
  static constexpr float reset_center(int) { return 0.0f; }
};

template <>
struct ClassicEnv<ENV_ACROBOT> {
  static constexpr int S = 4;  // theta1, theta2, omega1, omega2
  static constexpr int D = 6;  // cos, sin of theta1; cos, sin of theta2; omegas
  static constexpr int P = 3;
  static constexpr bool BOX = false;
  static constexpr float reset_half(int) { return 0.1f; }
  static constexpr float reset_center(int) { return 0.0f; }
};

// both MountainCars: the car starts at rest, position in (-0.6, -0.4]
struct MountainCarReset {
  static constexpr float reset_half(int d) { return d == 0 ? 0.1f : 0.0f; }
  static constexpr float reset_center(int d) { return d == 0 ? -0.5f : 0.0f; }
};

template <>
struct ClassicEnv<ENV_MOUNTAINCAR> : MountainCarReset {
  static constexpr int S = 2;  // position, velocity
  static constexpr int D = 2;  // the state itself
  static constexpr int P = 3;
  static constexpr bool BOX = false;
};

template <>
struct ClassicEnv<ENV_MOUNTAINCAR_CONT> : MountainCarReset {
  static constexpr int S = 2;
  static constexpr int D = 2;
  static constexpr int P = 2;  // mean, logstd
  static constexpr bool BOX = true;
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

// wrap an angle into [-pi, pi) (the floor form of pendulum_step)
DEV_INLINE float wrap_pi(float z) {
  return z - 6.2831853071795865f *
                 floorf((z + 3.1415926535897932f) / 6.2831853071795865f);
}

// Angular accelerations of gym's "book" Acrobot, every link constant 1,
// lc = 0.5, I = 1, g = 9.8, constants folded and cos(x - pi/2) as sin x.
// sin / cos of theta2 are recomputed per evaluation: nothing but the stage
// state lives across the four RK4 stages.
DEV_INLINE void acrobot_accel(float th1, float th2, float w1, float w2,
                              float tau, float& a1, float& a2) {
  float s2, c2;
  sincosf(th2, &s2, &c2);
  const float s1 = sinf(th1);
  const float d1 = 3.5f + c2;
  const float d2 = 1.25f + 0.5f * c2;
  const float phi2 = 4.9f * sinf(th1 + th2);
  const float phi1 = -0.5f * w2 * w2 * s2 - w2 * w1 * s2 + 14.7f * s1 + phi2;
  a2 = (tau + d2 / d1 * phi1 - 0.5f * w1 * w1 * s2 - phi2) /
       (1.25f - d2 * d2 / d1);
  a1 = -(d2 * a2 + phi1) / d1;
}

// One classical RK4 step (dt = 0.2) under action a in {0, 1, 2}: torque
// a - 1 on the second joint, held over the step.  Stage q evaluates f at
// y + c_q k_{q-1} with c = (0, 0.1, 0.1, 0.2) and adds w_q k_q, w = (1, 2, 2,
// 1), to the running sum, in that order (acrobot_step of envs/classic.py;
// 0 + 1 k1, acc + 2 k and acc + 1 k4 round as k1, acc + 2 k and acc + k4 do,
// fused or not).  The stage loop stays rolled: one copy of the four sine
// expansions instead of four.  Angles are wrapped into [-pi, pi), omega1
// clamped to +-4 pi, omega2 to +-9 pi.  Reward -1, or 0 on the terminating
// step; returns the termination flag of the new state.
DEV_INLINE int acrobot_step(float* s, int a, float& reward) {
  const float tau = (float)a - 1.0f;
  float k0 = 0.f, k1 = 0.f, k2 = 0.f, k3 = 0.f;
  float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f, acc3 = 0.f;
#pragma unroll 1
  for (int q = 0; q < 4; ++q) {
    const float c = (q == 0) ? 0.0f : (q == 3) ? 0.2f : 0.1f;
    const float w = (q == 0 || q == 3) ? 1.0f : 2.0f;
    const float th1 = s[0] + c * k0, th2 = s[1] + c * k1;
    const float w1 = s[2] + c * k2, w2 = s[3] + c * k3;
    k0 = w1;
    k1 = w2;
    acrobot_accel(th1, th2, w1, w2, tau, k2, k3);
    acc0 += w * k0;
    acc1 += w * k1;
    acc2 += w * k2;
    acc3 += w * k3;
  }
  const float h6 = 0.2f / 6.0f;
  s[0] = wrap_pi(s[0] + h6 * acc0);
  s[1] = wrap_pi(s[1] + h6 * acc1);
  s[2] = fminf(fmaxf(s[2] + h6 * acc2, -12.566370614359172f),
               12.566370614359172f);
  s[3] = fminf(fmaxf(s[3] + h6 * acc3, -28.274333882308138f),
               28.274333882308138f);
  const int term = (-cosf(s[0]) - cosf(s[0] + s[1]) > 1.0f) ? 1 : 0;
  reward = term ? 0.0f : -1.0f;
  return term;
}

// The end of both MountainCar steps, from the old position p and the new,
// clamped velocity v2 (_shared_tail of envs/classic.py): the position is
// clamped to [-1.2, 0.6]; on the left wall a leftward velocity becomes 0;
// returns the termination flag (position >= goal with a velocity >= 0).
DEV_INLINE int mountaincar_tail(float* s, float p, float v2, float goal) {
  const float p2 = fminf(fmaxf(p + v2, -1.2f), 0.6f);
  const float v3 = (p2 == -1.2f && v2 < 0.0f) ? 0.0f : v2;
  s[0] = p2;
  s[1] = v3;
  return (p2 >= goal && v3 >= 0.0f) ? 1 : 0;
}

// One step of MountainCar-v0 under action a in {0, 1, 2}: push left, not at
// all, right.  Reward -1 on every step, the terminating one included;
// returns the termination flag (position >= 0.5).
DEV_INLINE int mountaincar_step(float* s, int a, float& reward) {
  const float p = s[0], v = s[1];
  const float push = (float)a - 1.0f;
  const float v2 = fminf(
      fmaxf(v + push * 0.001f + cosf(3.0f * p) * (-0.0025f), -0.07f), 0.07f);
  reward = -1.0f;
  return mountaincar_tail(s, p, v2, 0.5f);
}

// One step of MountainCarContinuous-v0 under the UNCLIPPED action a: the
// force is clip(a, -1, 1), but the reward's 0.1 a^2 penalty takes the raw a,
// as gym has it; 100 is added on the terminating step.  Returns the
// termination flag (position >= 0.45).
DEV_INLINE int mountaincar_cont_step(float* s, float a, float& reward) {
  const float p = s[0], v = s[1];
  const float f = fminf(fmaxf(a, -1.0f), 1.0f);
  const float v2 = fminf(
      fmaxf(v + f * 0.0015f - 0.0025f * cosf(3.0f * p), -0.07f), 0.07f);
  const int term = mountaincar_tail(s, p, v2, 0.45f);
  reward = (term ? 100.0f : 0.0f) - 0.1f * a * a;
  return term;
}

// fresh state of a finished env: dim d uniform in (center_d - half_d,
// center_d + half_d] from the RNG_SLOT_RESET + d draw of (env, step); a dim
// of half-width 0 is its centre and draws nothing
template <int ENV>
DEV_INLINE void classic_reset(float* s, unsigned seed, int env, int step) {
  using Env = ClassicEnv<ENV>;
#pragma unroll
  for (int d = 0; d < Env::S; ++d) {
    if (Env::reset_half(d) == 0.0f) {
      s[d] = Env::reset_center(d);
      continue;
    }
    const float u = rng_uniform(seed, env, step, RNG_SLOT_RESET + d);
    const float z = (2.0f * u - 1.0f) * Env::reset_half(d);
    // a zero centre is not added: the symmetric envs keep their expression
    s[d] = (Env::reset_center(d) == 0.0f) ? z : Env::reset_center(d) + z;
  }
}

// observation of state s
template <int ENV>
DEV_INLINE void classic_obs(const float* s, float* x) {
  if constexpr (ClassicEnv<ENV>::D == ClassicEnv<ENV>::S) {
#pragma unroll
    for (int d = 0; d < ClassicEnv<ENV>::S; ++d) x[d] = s[d];
  } else if constexpr (ENV == ENV_ACROBOT) {
    sincosf(s[0], &x[1], &x[0]);
    sincosf(s[1], &x[3], &x[2]);
    x[4] = s[2];
    x[5] = s[3];
  } else {
    x[0] = cosf(s[0]);
    x[1] = sinf(s[0]);
    x[2] = s[1];
  }
}
