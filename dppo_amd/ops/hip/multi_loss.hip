// Fused PPO clipped-surrogate loss + sampling for MultiCategorical
// (MultiDiscrete) and Bernoulli (MultiBinary) policies (gfx950).
//
// Same per-row math as cat_loss.hip, fed through ppo_row_grads, with
// double-precision block-reduced means and the shared finalize kernel:
//   MultiCategorical (reference distributions.py:161-182): per component the
//     logsumexp log-prob of pi and oldpi and the shifted-logit entropy;
//     logp = sum_c logp_c, H = sum_c H_c.
//   Bernoulli (:210-229): neglogp = sum_j softplus(l_j) - a_j l_j and
//     H = sum_j softplus(l_j) - p_j l_j, both written without the
//     l - l cancellation (see bern_terms).
//
// Layout: wave-per-row for MultiCategorical — lane j owns logit column j,
// P <= 64, and the per-component max/sum are SEGMENTED scans (components are
// not power-of-two aligned, so an xor butterfly cannot carry them): an
// inclusive shfl_up scan that stops at the component's first column, then a
// broadcast from its last column.  Bernoulli packs 64/G rows per wave,
// G = the power of two >= n, so narrow heads do not idle the wave; its row
// sums are xor butterflies inside the aligned G-lane groups.  The samplers
// are thread per (row, component) and per (row, dim), on rollout_math.h's
// draw functions and slot scheme.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "common.h"
#include "loss_rows.h"
#include "ppo_math.h"
#include "rollout_math.h"

namespace {

constexpr int MAX_COMP = 32;  // nvec[c] >= 2 and P <= 64

// Per logit column j < P: first and last column of its component and the
// component's index; columns >= P are one-lane segments of their own.
struct McatMap {
  unsigned char s0[WAVE], s1[WAVE], comp[WAVE];
};

// component offsets for the sampler: off[c], off[C] = P
struct McatOffsets {
  int off[MAX_COMP + 1];
};

template <bool IS_MAX>
DEV_INLINE float seg_allreduce(float x, int lane, int s0, int s1) {
  #pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    const float y = __shfl_up(x, off, WAVE);
    if (lane - off >= s0) x = IS_MAX ? fmaxf(x, y) : x + y;
  }
  return __shfl(x, s1, WAVE);
}

struct McatRow {
  float lp, lo, ent;  // row totals, in every lane
  float p;            // this lane's softmax prob within its component
  float logp_j;       // this lane's log p_j
  float ent_c;        // entropy of this lane's component
  bool picked;        // this lane is the taken class of its component
};

DEV_INLINE McatRow mcat_row(const float* __restrict__ lpi,
                            const float* __restrict__ lold,
                            const int64_t* __restrict__ act, int lane, int P,
                            int s0, int s1, int comp) {
  const bool on = lane < P;
  const float lg = on ? lpi[lane] : NEG_INF;
  const float lgo = on ? lold[lane] : NEG_INF;
  const float m = seg_allreduce<true>(lg, lane, s0, s1);
  const float mo = seg_allreduce<true>(lgo, lane, s0, s1);
  const float a0 = on ? lg - m : 0.f;
  const float e = on ? __expf(a0) : 1.f;  // off lanes: z = 1, no inf/NaN
  const float eo = on ? __expf(lgo - mo) : 1.f;
  const float z = seg_allreduce<false>(e, lane, s0, s1);
  const float zo = seg_allreduce<false>(eo, lane, s0, s1);
  // H_c = log z - sum p * a0  (reference distributions.py:148-153)
  const float sa = seg_allreduce<false>(e * a0, lane, s0, s1);
  const float logz = __logf(z);
  McatRow r;
  r.ent_c = logz - sa / z;
  r.p = e / z;
  r.logp_j = a0 - logz;
  r.picked = on && (int64_t)(lane - s0) == act[comp];
  r.lp = wave_allreduce_sum(r.picked ? r.logp_j : 0.f);
  r.lo = wave_allreduce_sum(r.picked ? (lgo - mo) - __logf(zo) : 0.f);
  r.ent = wave_allreduce_sum((on && lane == s0) ? r.ent_c : 0.f);
  return r;
}

// the three per-row loss terms (reference PPO.py:29-40), as in cat_loss.hip
DEV_INLINE void ppo_row_terms(float lp, float lo, float ent_row, int64_t b,
                              const float* __restrict__ vpred,
                              const float* __restrict__ oldv,
                              const float* __restrict__ adv,
                              const float* __restrict__ etr, float clip,
                              float& pol, float& ent, float& val) {
  const float ratio = __expf(lp - lo);
  const float ab = adv[b];
  const float surr1 = ratio * ab;
  const float rc = fminf(fmaxf(ratio, 1.f - clip), 1.f + clip);
  pol += fminf(surr1, rc * ab);
  ent += ent_row;
  const float vb = vpred[b], ob = oldv[b], eb = etr[b];
  const float d1 = vb - eb;
  const float dc = fminf(fmaxf(vb - ob, -clip), clip);
  const float d2 = ob + dc - eb;
  val += fmaxf(d1 * d1, d2 * d2);
}

// rows [rb0, rb1) of this wave: B rows split evenly over the grid's waves
DEV_INLINE void wave_rows(int64_t B, int64_t& rb0, int64_t& rb1) {
  const int64_t waves_total = (int64_t)gridDim.x * 4;
  const int64_t wid = (int64_t)blockIdx.x * 4 + threadIdx.x / WAVE;
  const int64_t per = (B + waves_total - 1) / waves_total;
  rb0 = wid * per < B ? wid * per : B;
  rb1 = rb0 + per < B ? rb0 + per : B;
}

__launch_bounds__(256)
__global__ void ppo_mcat_fwd_kernel(
    const float* __restrict__ lpi, const float* __restrict__ lold,
    const float* __restrict__ vpred, const float* __restrict__ oldv,
    const int64_t* __restrict__ act, const float* __restrict__ adv,
    const float* __restrict__ etr,
    double* __restrict__ acc,  // [3] {policy_min_sum, ent_sum, value_max_sum}
    McatMap map, int64_t B, int P, int C, float clip) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int s0 = map.s0[lane], s1 = map.s1[lane], comp = map.comp[lane];
  int64_t rb0, rb1;
  wave_rows(B, rb0, rb1);

  float pol = 0.f, ent = 0.f, val = 0.f;  // lane 0 accumulates rows
  for (int64_t b = rb0; b < rb1; ++b) {
    const McatRow r = mcat_row(lpi + b * P, lold + b * P, act + b * C, lane,
                               P, s0, s1, comp);
    if (lane == 0)
      ppo_row_terms(r.lp, r.lo, r.ent, b, vpred, oldv, adv, etr, clip, pol,
                    ent, val);
  }
  if (lane == 0) {
    atomicAdd(&acc[0], static_cast<double>(pol));
    atomicAdd(&acc[1], static_cast<double>(ent));
    atomicAdd(&acc[2], static_cast<double>(val));
  }
}

__launch_bounds__(256)
__global__ void ppo_mcat_bwd_kernel(
    const float* __restrict__ lpi, const float* __restrict__ lold,
    const float* __restrict__ vpred, const float* __restrict__ oldv,
    const int64_t* __restrict__ act, const float* __restrict__ adv,
    const float* __restrict__ etr,
    const float* __restrict__ gtotal,   // [1] upstream d(total_loss)
    float* __restrict__ g_logits,       // [B, P]
    float* __restrict__ g_v,            // [B]
    McatMap map, int64_t B, int P, int C, float clip, float entcoeff,
    float vcoeff) {
  const float g = gtotal[0];
  const int lane = threadIdx.x & (WAVE - 1);
  const int s0 = map.s0[lane], s1 = map.s1[lane], comp = map.comp[lane];
  int64_t rb0, rb1;
  wave_rows(B, rb0, rb1);

  for (int64_t b = rb0; b < rb1; ++b) {
    const McatRow r = mcat_row(lpi + b * P, lold + b * P, act + b * C, lane,
                               P, s0, s1, comp);
    GaussRow rr;  // ppo_row_grads only reads logp_pi / logp_old
    rr.logp_pi = r.lp;
    rr.logp_old = r.lo;
    rr.ent = r.ent;
    const PPORowGrads gr = ppo_row_grads(rr, vpred[b], oldv[b], adv[b],
                                         etr[b], B, clip, entcoeff, vcoeff, g);
    if (lane < P) {
      // with c the component of column j:
      // d logp/d l_j = 1[j == off_c + a_c] - p_j;
      // d H/d l_j = -p_j (log p_j + H_c)
      const float d_lp = (r.picked ? 1.f : 0.f) - r.p;
      const float d_ent = -r.p * (r.logp_j + r.ent_c);
      g_logits[b * P + lane] = gr.g_logp * d_lp + gr.g_ent * d_ent;
    }
    if (lane == 0) g_v[b] = gr.g_v;
  }
}

// ---- Bernoulli -------------------------------------------------------------

struct BernTerms {
  float nlp;  // -log p(a) of this dim
  float ent;  // entropy of this dim
  float p;    // sigmoid(l)
  float pq;   // p (1 - p)
};

// With e = exp(-|l|): softplus(l) = max(l, 0) + log1p(e), so
//   softplus(l) - a l = log1p(e) + (l >= 0 ? (1 - a) l : -a l)
//   softplus(l) - p l = log1p(e) + |l| e / (1 + e)
// which are the reference's expressions without subtracting two numbers of
// size |l| (exact at saturated heads), and p (1 - p) = e / (1 + e)^2.
DEV_INLINE BernTerms bern_terms(float l, float a) {
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

// sum over the aligned G-lane group of this lane (G a power of two)
DEV_INLINE float group_allreduce_sum(float x, int G) {
  for (int off = G >> 1; off > 0; off >>= 1) x += __shfl_xor(x, off, WAVE);
  return x;
}

struct BernRow {
  float lp, lo, ent;  // row totals, in every lane of the row's group
  BernTerms t;        // this lane's dim under pi
  float a;
};

// lane (row slot lane >> sh, dim lane & (G-1)) of a wave holding 64/G rows
DEV_INLINE BernRow bern_row(const float* __restrict__ lpi,
                            const float* __restrict__ lold,
                            const float* __restrict__ act, int64_t row,
                            bool on, int sub, int n, int G) {
  BernRow r;
  float l = 0.f, lo = 0.f;
  r.a = 0.f;
  if (on) {
    l = lpi[row * n + sub];
    lo = lold[row * n + sub];
    r.a = act[row * n + sub];
  }
  r.t = bern_terms(l, r.a);
  const BernTerms to = bern_terms(lo, r.a);
  r.lp = -group_allreduce_sum(on ? r.t.nlp : 0.f, G);
  r.lo = -group_allreduce_sum(on ? to.nlp : 0.f, G);
  r.ent = group_allreduce_sum(on ? r.t.ent : 0.f, G);
  return r;
}

__launch_bounds__(256)
__global__ void ppo_bern_fwd_kernel(
    const float* __restrict__ lpi, const float* __restrict__ lold,
    const float* __restrict__ vpred, const float* __restrict__ oldv,
    const float* __restrict__ act, const float* __restrict__ adv,
    const float* __restrict__ etr, double* __restrict__ acc, int64_t B, int n,
    int sh, float clip) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int G = 1 << sh, sub = lane & (G - 1), slot = lane >> sh;
  const int rows_per_wave = WAVE >> sh;
  int64_t rb0, rb1;
  wave_rows(B, rb0, rb1);

  float pol = 0.f, ent = 0.f, val = 0.f;  // each group's lane 0 accumulates
  for (int64_t b = rb0; b < rb1; b += rows_per_wave) {
    const int64_t row = b + slot;
    const bool live = row < rb1;
    const BernRow r = bern_row(lpi, lold, act, row, live && sub < n, sub, n, G);
    if (live && sub == 0)
      ppo_row_terms(r.lp, r.lo, r.ent, row, vpred, oldv, adv, etr, clip, pol,
                    ent, val);
  }
  pol = wave_reduce_sum(pol);
  ent = wave_reduce_sum(ent);
  val = wave_reduce_sum(val);
  if (lane == 0) {
    atomicAdd(&acc[0], static_cast<double>(pol));
    atomicAdd(&acc[1], static_cast<double>(ent));
    atomicAdd(&acc[2], static_cast<double>(val));
  }
}

__launch_bounds__(256)
__global__ void ppo_bern_bwd_kernel(
    const float* __restrict__ lpi, const float* __restrict__ lold,
    const float* __restrict__ vpred, const float* __restrict__ oldv,
    const float* __restrict__ act, const float* __restrict__ adv,
    const float* __restrict__ etr, const float* __restrict__ gtotal,
    float* __restrict__ g_logits,  // [B, n]
    float* __restrict__ g_v,       // [B]
    int64_t B, int n, int sh, float clip, float entcoeff, float vcoeff) {
  const float g = gtotal[0];
  const int lane = threadIdx.x & (WAVE - 1);
  const int G = 1 << sh, sub = lane & (G - 1), slot = lane >> sh;
  const int rows_per_wave = WAVE >> sh;
  int64_t rb0, rb1;
  wave_rows(B, rb0, rb1);

  for (int64_t b = rb0; b < rb1; b += rows_per_wave) {
    const int64_t row = b + slot;
    const bool live = row < rb1;
    const bool on = live && sub < n;
    const BernRow r = bern_row(lpi, lold, act, row, on, sub, n, G);
    if (!live) continue;  // after the group shuffles: no lane skips those
    GaussRow rr;  // ppo_row_grads only reads logp_pi / logp_old
    rr.logp_pi = r.lp;
    rr.logp_old = r.lo;
    rr.ent = r.ent;
    const PPORowGrads gr =
        ppo_row_grads(rr, vpred[row], oldv[row], adv[row], etr[row], B, clip,
                      entcoeff, vcoeff, g);
    if (on) {
      // d logp/d l_j = a_j - p_j;  d H/d l_j = -l_j p_j (1 - p_j)
      const float d_lp = r.a - r.t.p;
      const float d_ent = -lpi[row * n + sub] * r.t.pq;
      g_logits[row * n + sub] = gr.g_logp * d_lp + gr.g_ent * d_ent;
    }
    if (sub == 0) g_v[row] = gr.g_v;
  }
}

// ---- samplers --------------------------------------------------------------

__global__ void mcat_sample_kernel(const float* __restrict__ logits,
                                   int64_t* __restrict__ out,  // [B, C]
                                   McatOffsets mo, int64_t B, int P, int C,
                                   unsigned seed, unsigned ctr) {
  for (int64_t i = gidx(); i < B * C; i += gstride()) {
    const int64_t b = i / C;
    const int c = (int)(i % C);
    const float* row = logits + b * P;
    const int off = mo.off[c];
    out[i] = mcat_draw([&](int col) { return row[col]; }, off,
                       mo.off[c + 1] - off, seed, (int)b, (int)ctr);
  }
}

__global__ void bern_sample_kernel(const float* __restrict__ logits,
                                   float* __restrict__ out,  // [B, n]
                                   int64_t B, int n, unsigned seed,
                                   unsigned ctr) {
  for (int64_t i = gidx(); i < B * n; i += gstride())
    out[i] = bern_draw(logits[i], seed, (int)(i / n), (int)ctr, (int)(i % n));
}

// nvec -> component offsets (off[C] = P), with the limits the kernels need
McatOffsets mcat_offsets(const std::vector<int64_t>& nvec, int64_t P) {
  TORCH_CHECK(!nvec.empty() && nvec.size() <= (size_t)MAX_COMP,
              "multi-categorical kernels support 1..32 components");
  McatOffsets mo{};
  int off = 0;
  for (size_t c = 0; c < nvec.size(); ++c) {
    TORCH_CHECK(nvec[c] >= 1 && off + nvec[c] <= WAVE,
                "multi-categorical kernels support sum(nvec) <= 64");
    mo.off[c] = off;
    off += static_cast<int>(nvec[c]);
  }
  mo.off[nvec.size()] = off;
  TORCH_CHECK(off == P, "logits width must equal sum(nvec)");
  return mo;
}

McatMap mcat_map(const McatOffsets& mo, int C) {
  McatMap map;
  for (int j = 0; j < WAVE; ++j) {
    map.s0[j] = map.s1[j] = static_cast<unsigned char>(j);
    map.comp[j] = 0;
  }
  for (int c = 0; c < C; ++c)
    for (int j = mo.off[c]; j < mo.off[c + 1]; ++j) {
      map.s0[j] = static_cast<unsigned char>(mo.off[c]);
      map.s1[j] = static_cast<unsigned char>(mo.off[c + 1] - 1);
      map.comp[j] = static_cast<unsigned char>(c);
    }
  return map;
}

void check_loss_args(const torch::Tensor& lpi, const torch::Tensor& lold,
                     const torch::Tensor& vpred, const torch::Tensor& oldv,
                     const torch::Tensor& act, int64_t act_w,
                     torch::ScalarType act_dtype, const torch::Tensor& adv,
                     const torch::Tensor& etr) {
  TORCH_CHECK(lpi.is_cuda() && lpi.dtype() == torch::kFloat32 &&
              lpi.is_contiguous() && lpi.dim() == 2);
  TORCH_CHECK(lpi.size(1) >= 1 && lpi.size(1) <= WAVE,
              "fused loss supports 1..64 logit columns");
  const int64_t B = lpi.size(0);
  TORCH_CHECK(lold.is_cuda() && lold.dtype() == torch::kFloat32 &&
              lold.is_contiguous() && lold.sizes() == lpi.sizes());
  TORCH_CHECK(act.is_cuda() && act.dtype() == act_dtype &&
              act.is_contiguous() && act.numel() == B * act_w);
  for (const torch::Tensor* t : {&vpred, &oldv, &adv, &etr})
    TORCH_CHECK(t->is_cuda() && t->dtype() == torch::kFloat32 &&
                t->is_contiguous() && t->numel() == B);
}

int log2_group(int n) {  // sh with 2^sh the power of two >= n
  int sh = 0;
  while ((1 << sh) < n) ++sh;
  return sh;
}

}  // namespace

torch::Tensor ppo_loss_mcat_fwd(torch::Tensor lpi, torch::Tensor lold,
                                torch::Tensor vpred, torch::Tensor oldv,
                                torch::Tensor act, torch::Tensor adv,
                                torch::Tensor etr, std::vector<int64_t> nvec,
                                double clip, double entcoeff, double vcoeff) {
  const int C = static_cast<int>(nvec.size());
  check_loss_args(lpi, lold, vpred, oldv, act, C, torch::kInt64, adv, etr);
  const int64_t B = lpi.size(0);
  const int P = static_cast<int>(lpi.size(1));
  const McatMap map = mcat_map(mcat_offsets(nvec, P), C);

  auto acc = torch::zeros({3}, lpi.options().dtype(torch::kFloat64));
  auto losses = torch::empty({4}, lpi.options());
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(ppo_mcat_fwd_kernel, dim3(2048), dim3(256), 0, stream,
                     lpi.data_ptr<float>(), lold.data_ptr<float>(),
                     vpred.data_ptr<float>(), oldv.data_ptr<float>(),
                     act.data_ptr<int64_t>(), adv.data_ptr<float>(),
                     etr.data_ptr<float>(), acc.data_ptr<double>(), map, B, P,
                     C, (float)clip);
  hipLaunchKernelGGL(ppo_rows_finalize_kernel, dim3(1), dim3(1), 0, stream,
                     acc.data_ptr<double>(), losses.data_ptr<float>(), B,
                     (float)entcoeff, (float)vcoeff);
  return losses;
}

std::vector<torch::Tensor> ppo_loss_mcat_bwd(
    torch::Tensor lpi, torch::Tensor lold, torch::Tensor vpred,
    torch::Tensor oldv, torch::Tensor act, torch::Tensor adv,
    torch::Tensor etr, std::vector<int64_t> nvec, double clip,
    double entcoeff, double vcoeff, torch::Tensor gtotal) {
  const int C = static_cast<int>(nvec.size());
  check_loss_args(lpi, lold, vpred, oldv, act, C, torch::kInt64, adv, etr);
  const int64_t B = lpi.size(0);
  const int P = static_cast<int>(lpi.size(1));
  const McatMap map = mcat_map(mcat_offsets(nvec, P), C);
  auto g_logits = torch::empty_like(lpi);
  auto g_v = torch::empty_like(vpred);
  auto gt = gtotal.to(lpi.options()).contiguous();
  TORCH_CHECK(gt.numel() == 1);
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(ppo_mcat_bwd_kernel, dim3(2048), dim3(256), 0, stream,
                     lpi.data_ptr<float>(), lold.data_ptr<float>(),
                     vpred.data_ptr<float>(), oldv.data_ptr<float>(),
                     act.data_ptr<int64_t>(), adv.data_ptr<float>(),
                     etr.data_ptr<float>(), gt.data_ptr<float>(),
                     g_logits.data_ptr<float>(), g_v.data_ptr<float>(), map, B,
                     P, C, (float)clip, (float)entcoeff, (float)vcoeff);
  return {g_logits, g_v};
}

torch::Tensor ppo_loss_bern_fwd(torch::Tensor lpi, torch::Tensor lold,
                                torch::Tensor vpred, torch::Tensor oldv,
                                torch::Tensor act, torch::Tensor adv,
                                torch::Tensor etr, double clip,
                                double entcoeff, double vcoeff) {
  check_loss_args(lpi, lold, vpred, oldv, act, lpi.dim() == 2 ? lpi.size(1) : 0,
                  torch::kFloat32, adv, etr);
  const int64_t B = lpi.size(0);
  const int n = static_cast<int>(lpi.size(1));
  auto acc = torch::zeros({3}, lpi.options().dtype(torch::kFloat64));
  auto losses = torch::empty({4}, lpi.options());
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(ppo_bern_fwd_kernel, dim3(2048), dim3(256), 0, stream,
                     lpi.data_ptr<float>(), lold.data_ptr<float>(),
                     vpred.data_ptr<float>(), oldv.data_ptr<float>(),
                     act.data_ptr<float>(), adv.data_ptr<float>(),
                     etr.data_ptr<float>(), acc.data_ptr<double>(), B, n,
                     log2_group(n), (float)clip);
  hipLaunchKernelGGL(ppo_rows_finalize_kernel, dim3(1), dim3(1), 0, stream,
                     acc.data_ptr<double>(), losses.data_ptr<float>(), B,
                     (float)entcoeff, (float)vcoeff);
  return losses;
}

std::vector<torch::Tensor> ppo_loss_bern_bwd(
    torch::Tensor lpi, torch::Tensor lold, torch::Tensor vpred,
    torch::Tensor oldv, torch::Tensor act, torch::Tensor adv,
    torch::Tensor etr, double clip, double entcoeff, double vcoeff,
    torch::Tensor gtotal) {
  check_loss_args(lpi, lold, vpred, oldv, act, lpi.dim() == 2 ? lpi.size(1) : 0,
                  torch::kFloat32, adv, etr);
  const int64_t B = lpi.size(0);
  const int n = static_cast<int>(lpi.size(1));
  auto g_logits = torch::empty_like(lpi);
  auto g_v = torch::empty_like(vpred);
  auto gt = gtotal.to(lpi.options()).contiguous();
  TORCH_CHECK(gt.numel() == 1);
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(ppo_bern_bwd_kernel, dim3(2048), dim3(256), 0, stream,
                     lpi.data_ptr<float>(), lold.data_ptr<float>(),
                     vpred.data_ptr<float>(), oldv.data_ptr<float>(),
                     act.data_ptr<float>(), adv.data_ptr<float>(),
                     etr.data_ptr<float>(), gt.data_ptr<float>(),
                     g_logits.data_ptr<float>(), g_v.data_ptr<float>(), B, n,
                     log2_group(n), (float)clip, (float)entcoeff,
                     (float)vcoeff);
  return {g_logits, g_v};
}

torch::Tensor mcat_sample(torch::Tensor logits, std::vector<int64_t> nvec,
                          int64_t seed, int64_t ctr) {
  TORCH_CHECK(logits.is_cuda() && logits.dtype() == torch::kFloat32);
  TORCH_CHECK(logits.dim() == 2);
  const int64_t B = logits.size(0);
  const int P = static_cast<int>(logits.size(1));
  const int C = static_cast<int>(nvec.size());
  const McatOffsets mo = mcat_offsets(nvec, P);
  auto lg = logits.contiguous();
  auto out = torch::empty({B, (int64_t)C},
                          logits.options().dtype(torch::kInt64));
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  const int block = 256;
  hipLaunchKernelGGL(mcat_sample_kernel,
                     dim3(elementwise_grid(B * C, block)), dim3(block), 0,
                     stream, lg.data_ptr<float>(), out.data_ptr<int64_t>(), mo,
                     B, P, C, (unsigned)(seed & 0xFFFFFFFF),
                     (unsigned)(ctr & 0xFFFFFFFF));
  return out;
}

torch::Tensor bern_sample(torch::Tensor logits, int64_t seed, int64_t ctr) {
  TORCH_CHECK(logits.is_cuda() && logits.dtype() == torch::kFloat32);
  TORCH_CHECK(logits.dim() == 2 && logits.size(1) >= 1);
  const int64_t B = logits.size(0);
  const int n = static_cast<int>(logits.size(1));
  auto lg = logits.contiguous();
  auto out = torch::empty_like(lg);
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  const int block = 256;
  hipLaunchKernelGGL(bern_sample_kernel,
                     dim3(elementwise_grid(B * n, block)), dim3(block), 0,
                     stream, lg.data_ptr<float>(), out.data_ptr<float>(), B, n,
                     (unsigned)(seed & 0xFFFFFFFF),
                     (unsigned)(ctr & 0xFFFFFFFF));
  return out;
}
