// Shared rollout device math: the counter RNG, its slot scheme, Box,
// MultiCategorical and Bernoulli action sampling, the synthetic env
// transition and the per-env episode step.
// rollout.hip (whole-rollout kernel, sample_kernel, env_finish_kernel),
// mfma_gemm.hip (fused env-step epilogue, fused policy forward,
// env_finish2_kernel), cat_loss.hip (Gumbel-max sampler) and multi_loss.hip
// (mcat_sample, bern_sample) all take them from here, so the paths that must
// agree bitwise run the same expressions.
#pragma once

#include "common.h"

// ---- counter-based 32-bit RNG ---------------------------------------------
// Stateless: a draw is a hash of (seed, env, step, slot).  Slot scheme, per
// (env, step):
//   j                 action draw of dim / class j (Box: normal, .x of the
//                     pair; Categorical: the Gumbel uniform;
//                     MultiCategorical: the Gumbel uniform of GLOBAL logit
//                     column j = off_c + class, so components never share
//                     a draw; Bernoulli: the uniform compared to sigmoid)
//   RNG_SLOT_ENV + s  env transition noise, one Box-Muller PAIR per slot:
//                     - whole-rollout kernel: s = d, the pair drawn for the
//                       EVEN env of a pair feeds dim d of envs 2q and 2q+1;
//                     - per-step path (env_finish_kernel and the fused
//                       env-step epilogue): s = 2c and 2c+1 feed dims
//                       4c..4c+3 of ONE env (c = float4 chunk index).
//                     The two layouts differ on purpose: each path is
//                     deterministic per seed on its own, nothing requires
//                     them to share trajectories.
//   RNG_SLOT_RESET + d   reset state of dim d (0.1 * normal, .x of the pair)
//   RNG_SLOT_EPS         epsilon-greedy decision (uniform < eps)
//   RNG_SLOT_EPS_ACT + j epsilon-greedy action draw (Categorical: j = 0;
//                        MultiCategorical: j = component; Bernoulli: j = dim)
// The stand-alone samplers (cat_sample, mcat_sample, bern_sample) use the
// action slots with env = batch row and step = the caller's counter.
// Within the per-step path every kernel uses the same slots, so the split
// launches (sample_kernel, env_finish_kernel) and the fused ones
// (mlp_fwd_fused_kernel, gemm_fwd_glds_kernel<*, true>) sample the same
// actions, noise and resets for a given seed.
constexpr int RNG_SLOT_ENV = 1000;
constexpr int RNG_SLOT_RESET = 5000;
constexpr int RNG_SLOT_EPS = 90001;
constexpr int RNG_SLOT_EPS_ACT = 90010;

DEV_INLINE unsigned lowbias32(unsigned x) {
  x ^= x >> 16;
  x *= 0x7feb352dU;
  x ^= x >> 15;
  x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}

// uniform in (0, 1]
DEV_INLINE float rng_uniform(unsigned seed, int env, int step, int slot) {
  unsigned h = lowbias32(seed ^ (unsigned)env * 0x9E3779B9U ^
                         (unsigned)step * 0x85EBCA6BU ^
                         (unsigned)slot * 0xC2B2AE35U);
  return ((h >> 8) + 1) * (1.0f / 16777217.0f);
}

// One hash -> two 16-bit uniforms -> one Box-Muller pair.  The rollout
// draws ~1500 normals per block-step (env noise dominates); the naive
// 2-hash + log + cos per normal made the whole kernel transcendental-
// bound.  16-bit resolution truncates the tails at ~4.7 sigma, which is
// statistically invisible for synthetic-env noise and recorded actions.
DEV_INLINE float2 rng_normal2(unsigned seed, int env, int step, int slot) {
  const unsigned h = lowbias32(seed ^ (unsigned)env * 0x9E3779B9U ^
                               (unsigned)step * 0x85EBCA6BU ^
                               (unsigned)slot * 0xC2B2AE35U);
  const float u1 = ((h >> 16) + 1) * (1.0f / 65537.0f);
  const float u2 = (h & 0xFFFFu) * (1.0f / 65536.0f);
  const float r = sqrtf(-2.0f * __logf(u1));
  float sn, cs;
  __sincosf(6.2831853071795865f * u2, &sn, &cs);
  return make_float2(r * cs, r * sn);
}

DEV_INLINE float rng_normal(unsigned seed, int env, int step, int slot) {
  return rng_normal2(seed, env, step, slot).x;
}

// ---- Box action: DiagGaussian sample + epsilon-greedy overlay -------------
// (reference Worker.py:149-152: with probability eps the action is uniform
// in [low, high]).  The per-step kernels call this; rollout_kernel spells
// the same expression out (see there).
DEV_INLINE float box_sample(float mean, float logstd, unsigned seed,
                            int64_t env, int step, int j, float eps,
                            float low, float high) {
  float act = mean + __expf(logstd) * rng_normal(seed, (int)env, step, j);
  const float u_dec = rng_uniform(seed, (int)env, step, RNG_SLOT_EPS);
  if (u_dec < eps) {
    const float u =
        rng_uniform(seed, (int)env, step, RNG_SLOT_EPS_ACT + j);
    act = low + (high - low) * u;
  }
  return act;
}

// ---- MultiCategorical action: Gumbel-max per component --------------------
// argmax_j(logit_j - log(-log u_j)) over the n logits of one component that
// starts at global column `off`; logit_at(col) reads a logit (LDS in the
// rollout kernel, global memory in mcat_sample_kernel).  Ties and non-finite
// scores go to the lowest index; -log u is floored at 2^-24 as in the
// Categorical rollout, so the draw is finite for u == 1.
template <class LogitAt>
DEV_INLINE int mcat_draw(LogitAt logit_at, int off, int n, unsigned seed,
                         int env, int step) {
  float best = -3.0e38f;
  int arg = 0;
  for (int j = 0; j < n; ++j) {
    const float nl = fmaxf(-__logf(rng_uniform(seed, env, step, off + j)),
                           5.9604645e-8f);
    const float gv = logit_at(off + j) - __logf(nl);
    if (gv > best) {
      best = gv;
      arg = j;
    }
  }
  return arg;
}

// epsilon-greedy overlay of component c (n classes): ONE decision per
// (env, step); an explored env redraws every component uniformly.  The
// result is clamped into [0, n-1] (u == 1 gives n).
DEV_INLINE int mcat_explore(int arg, int n, int c, unsigned seed, int env,
                            int step, float eps) {
  if (rng_uniform(seed, env, step, RNG_SLOT_EPS) < eps)
    arg = (int)(rng_uniform(seed, env, step, RNG_SLOT_EPS_ACT + c) * n);
  return max(0, min(n - 1, arg));
}

// ---- Bernoulli action ------------------------------------------------------
// a_j = (u_j <= sigmoid(l_j)): u is in (0, 1], so `<=` makes a saturated head
// (p rounds to 1) always give 1, and p == 0 never does.
DEV_INLINE float bern_draw(float logit, unsigned seed, int env, int step,
                           int j) {
  const float p = 1.f / (1.f + __expf(-logit));
  return (rng_uniform(seed, env, step, j) <= p) ? 1.f : 0.f;
}

// epsilon-greedy overlay of dim j: one decision per (env, step), explored
// dims are Bernoulli(0.5)
DEV_INLINE float bern_explore(float act, int j, unsigned seed, int env,
                              int step, float eps) {
  if (rng_uniform(seed, env, step, RNG_SLOT_EPS) < eps)
    act = (rng_uniform(seed, env, step, RNG_SLOT_EPS_ACT + j) < 0.5f) ? 1.f
                                                                     : 0.f;
  return act;
}

// ---- per-step env transition ----------------------------------------------
// env_finish_kernel and the fused env-step epilogue work on one float4 =
// dims 4c..4c+3 of one env per lane, and must agree bitwise.  They share
// the three expressions below (deliberately one-level wrappers: a single
// float4 transition function, and the xor tree as a function, changed the
// generated code of the kernels that call them) and this reward sum order:
// per float4 chunk sq4(), the 16 chunks of one 64-column panel by an xor
// tree over 16 adjacent lanes, then the panels in ascending order.

// noise pair k (0, 1) of float4 chunk c: dims 4c+2k, 4c+2k+1
DEV_INLINE float2 env_noise_pair(unsigned seed, int env, int step, int c,
                                 int k) {
  return rng_normal2(seed, env, step, RNG_SLOT_ENV + 2 * c + k);
}

// next state of one dim: G = [x@V | act] @ [U; B], n = its noise draw
DEV_INLINE float env_pred(float x, float d, float g, float sigma, float n) {
  return fast_tanhf(x * d + g + sigma * n);
}

// fresh state of dim d of a finished env (every rollout path)
DEV_INLINE float env_reset(unsigned seed, int env, int step, int d) {
  return 0.1f * rng_normal(seed, env, step, RNG_SLOT_RESET + d);
}

// ---- per-env episode step (reference Worker.py:57-65) ---------------------
// reward from the env's pred^2 sum, return / step-count update, done at the
// horizon (both reset).
DEV_INLINE void episode_step(float ss, int D, int64_t e, int& done,
                            const int* __restrict__ horizons,
                            int* __restrict__ t, float* __restrict__ epr,
                            float* __restrict__ rewards,
                            float* __restrict__ dones) {
  const float r = 1.0f - ss / D;
  rewards[e] = r;
  float ep = epr[e] + r;
  int tc = t[e] + 1;
  done = (tc >= horizons[e]) ? 1 : 0;
  dones[e] = (float)done;
  if (done) {
    ep = 0.f;
    tc = 0;
  }
  epr[e] = ep;
  t[e] = tc;
}
