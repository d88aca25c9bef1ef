// Serial per-row math of the discrete policy families, for kernels where
// ONE lane owns a whole row held in LDS (disc_gh.hip): the Categorical
// segment (reference distributions.py:131-153), used once per row by
// Categorical and once per component by MultiCategorical (:161-182), and the
// Bernoulli dim (:210-229).  Two passes per row, because the policy
// coefficient g_logp needs the whole row's log-probs first:
//   *_stats : logp_pi(a), logp_old(a) and the entropy, accumulated;
//   *_grads : d total_loss / d logits, written over the row's gh slot.
// Nothing is carried between the passes but scalars; the second pass
// recomputes max / exp-sum from LDS, so no lane keeps a runtime-indexed
// register array (those go to scratch).
//
// Same formulas as the wave-per-row kernels of cat_loss.hip / multi_loss.hip:
//   d logp/d l_j = 1[j == a] - p_j,  d H/d l_j = -p_j (log p_j + H)
//   Bernoulli: d logp/d l_j = a_j - p_j,  d H/d l_j = -l_j p_j (1 - p_j)
#pragma once

#include "common.h"

namespace {

struct RowSums {
  float lp, lo, ent;  // logp_pi(a), logp_old(a), H(pi)
};

// max, sum exp(l - max) and sum exp(l - max) (l - max) of l[0..K)
struct SegStats {
  float m, z, sa;
};

DEV_INLINE SegStats seg_stats(const float* __restrict__ l, int K) {
  SegStats s;
  s.m = l[0];
  for (int j = 1; j < K; ++j) s.m = fmaxf(s.m, l[j]);
  s.z = 0.f;
  s.sa = 0.f;
  for (int j = 0; j < K; ++j) {
    const float a0 = l[j] - s.m;
    const float e = __expf(a0);
    s.z += e;
    s.sa += e * a0;
  }
  return s;
}

// One categorical segment pd[0..K) / og[0..K) with taken class a.
DEV_INLINE void cat_seg_stats(const float* __restrict__ pd,
                              const float* __restrict__ og, int K, int a,
                              RowSums& r) {
  const SegStats s = seg_stats(pd, K);
  float mo = og[0];
  for (int j = 1; j < K; ++j) mo = fmaxf(mo, og[j]);
  float zo = 0.f;
  for (int j = 0; j < K; ++j) zo += __expf(og[j] - mo);
  const float logz = __logf(s.z);
  // H = log z - sum p (l - max)  (shifted-logit form)
  r.ent += logz - s.sa / s.z;
  r.lp += (pd[a] - s.m) - logz;
  r.lo += (og[a] - mo) - __logf(zo);
}

DEV_INLINE void cat_seg_grads(const float* __restrict__ pd,
                              float* __restrict__ gh, int K, int a,
                              float g_logp, float g_ent) {
  const SegStats s = seg_stats(pd, K);
  const float logz = __logf(s.z);
  const float ent = logz - s.sa / s.z;
  const float iz = 1.f / s.z;
  for (int j = 0; j < K; ++j) {
    const float a0 = pd[j] - s.m;
    const float p = __expf(a0) * iz;
    const float d_lp = (j == a ? 1.f : 0.f) - p;
    const float d_ent = -p * ((a0 - logz) + ent);
    gh[j] = g_logp * d_lp + g_ent * d_ent;
  }
}

struct BernTerms {
  float nlp;  // -log p(a) of this dim
  float ent;  // entropy of this dim
  float p;    // sigmoid(l)
  float pq;   // p (1 - p)
};

// The stable-softplus forms of multi_loss.hip's bern_terms: with
// e = exp(-|l|), softplus(l) = max(l, 0) + log1p(e), so
//   softplus(l) - a l = log1p(e) + (l >= 0 ? (1 - a) l : -a l)
//   softplus(l) - p l = log1p(e) + |l| e / (1 + e)
// without subtracting two numbers of size |l|, and p (1 - p) = e / (1 + e)^2.
DEV_INLINE BernTerms bern_dim(float l, float a) {
  const float al = fabsf(l);
  const float e = __expf(-al);
  const float l1p = log1pf(e);
  const float inv = 1.f / (1.f + e);
  BernTerms t;
  t.nlp = l1p + (l >= 0.f ? (1.f - a) * l : -a * l);
  t.ent = l1p + al * e * inv;
  t.p = l >= 0.f ? inv : e * inv;
  t.pq = e * inv * inv;
  return t;
}

DEV_INLINE void bern_row_stats(const float* __restrict__ pd,
                               const float* __restrict__ og,
                               const float* __restrict__ ac, int n,
                               RowSums& r) {
  for (int j = 0; j < n; ++j) {
    const float a = ac[j];
    const BernTerms t = bern_dim(pd[j], a);
    r.lp -= t.nlp;
    r.ent += t.ent;
    r.lo -= bern_dim(og[j], a).nlp;
  }
}

DEV_INLINE void bern_row_grads(const float* __restrict__ pd,
                               const float* __restrict__ ac,
                               float* __restrict__ gh, int n, float g_logp,
                               float g_ent) {
  for (int j = 0; j < n; ++j) {
    const float l = pd[j], a = ac[j];
    const BernTerms t = bern_dim(l, a);
    gh[j] = g_logp * (a - t.p) + g_ent * (-l * t.pq);
  }
}

}  // namespace
