// PPO loss gradient gh = [dL/d logits | dL/d vpred | 0-pad] for the discrete
// policy families (gfx950): Categorical, MultiCategorical and Bernoulli.
//
// The contract is ppo_loss_gauss_gh's (ppo_loss.hip; eager definition:
// ops/ppo_loss.py ppo_gh_ref): gh is [B][ldgh], ldgh = (P + 1 + 3) & ~3,
// columns 0..P-1 hold d total_loss / d logits with the upstream gradient 1
// and the 1/B of the means folded in, column P holds d total_loss / d vpred,
// columns P+1..ldgh-1 are written as zero.  That is the operand the update's
// dgrad GEMM chain and the combined-heads dW consume (trainer
// _fused_backward), so the three families share the Box policy's MFMA chain.
//
// Layout: the LDS-tiled row-per-lane design of ppo_gh_tile_kernel, not the
// wave-per-row design of the cat/mcat/bern backward kernels, which at K = 2
// (CartPole) keeps 2 of 64 lanes busy.  A 256-thread block stages a tile of
// rows of every operand with full-width coalesced loads into odd-stride LDS
// rows (int64 actions narrowed to int32), each lane computes one row serially
// (disc_rows.h), writes its gh row over its own oldpi-logits row, and the
// block stores the tile as float4.
//
// Tile height, by the LDS floats one row takes,
//   rowf = (P|1) + (ldgh|1) + (W|1) + 4,  W = 1 | C | n action columns:
//   rowf <= 128 -> 128 rows, at most 64 KB;  else 64 rows, at most 51 KB
//   (rowf <= 203 at P = 64).  No opt-in LDS attribute is needed.
//   Categorical:  K <= 59 -> 128 rows, K = 60..64 -> 64 rows
//   Bernoulli:    n <= 39 -> 128 rows, n = 40..64 -> 64 rows
//   MultiCat:     by P and C; (2,)*32 (P 64, C 32) -> 64 rows
// Blocks per CU (160 KB LDS, 8 blocks of 4 waves at most): 8 up to rowf 40
// (CartPole rowf 13, LunarLander 19, MultiLever 31, BitFlipper 35), 2 at
// rowf 128, 3..4 in the 64-row range.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "common.h"
#include "disc_rows.h"
#include "gh_tile.h"
#include "ppo_math.h"

namespace {

constexpr int DISC_MAX_COMP = 32;  // nvec[c] >= 2 and P <= 64

enum DiscFamily { FAM_CAT = 0, FAM_MCAT = 1, FAM_BERN = 2 };

// component offsets, passed by value: off[c], off[C] = P
struct DiscOffsets {
  int off[DISC_MAX_COMP + 1];
};

int disc_row_floats(int P, int W) {
  const int ldgh = (P + 1 + 3) & ~3;
  return (P | 1) + (ldgh | 1) + (W | 1) + 4;
}

int disc_tile_rows(int P, int W) {
  return disc_row_floats(P, W) <= 128 ? 128 : 64;
}

template <int FAM>
__launch_bounds__(256)
__global__ void disc_gh_tile_kernel(
    const float* __restrict__ lpi, const float* __restrict__ lold,
    const float* __restrict__ vpred, const float* __restrict__ oldv,
    const void* __restrict__ act,  // int64 [B][W], Bernoulli: float [B][W]
    const float* __restrict__ adv, const float* __restrict__ etr,
    float* __restrict__ gh,              // [B][ldgh]
    const float* __restrict__ clip_dev,  // nullptr -> use `clip` arg
    DiscOffsets mo, int64_t B, int P, int W, int ldgh, int tile, float clip,
    float entcoeff, float vcoeff) {
  if (clip_dev != nullptr) clip = clip_dev[0];
  extern __shared__ float lds[];
  const int sp = P | 1;     // pi logits row stride (odd)
  const int sg = ldgh | 1;  // oldpi logits / gh shared row stride (> P, odd)
  const int sa = W | 1;     // action row stride (odd)
  float* l_pd = lds;
  float* l_og = l_pd + tile * sp;  // oldpi logits, later this tile's gh
  float* l_ac = l_og + tile * sg;  // int32 (Bernoulli: float) actions
  float* l_sc = l_ac + tile * sa;  // [4][tile]: vpred|oldv|adv|etr
  const int tid = threadIdx.x;
  const int64_t tb = (int64_t)blockIdx.x * tile;
  const int rows = (int)min((int64_t)tile, B - tb);

  stage_tile(lpi + tb * P, l_pd, P, sp, rows, tid);
  stage_tile(lold + tb * P, l_og, P, sg, rows, tid);
  if (FAM == FAM_BERN)
    stage_tile(static_cast<const float*>(act) + tb * W, l_ac, W, sa, rows,
               tid);
  else
    stage_tile_i64(static_cast<const int64_t*>(act) + tb * W,
                   reinterpret_cast<int*>(l_ac), W, sa, rows, tid);
  for (int idx = tid; idx < 4 * tile; idx += 256) {
    const int s = idx / tile, t = idx % tile;
    if (t < rows) {
      const float* src = s == 0 ? vpred : s == 1 ? oldv : s == 2 ? adv : etr;
      l_sc[s * tile + t] = src[tb + t];
    }
  }
  __syncthreads();

  // compute: one row per lane (rows <= tile of the 256 threads — the kernel
  // is memory-bound, the idle compute lanes cost nothing)
  if (tid < rows) {
    const float* pd = l_pd + tid * sp;
    const float* og = l_og + tid * sg;
    const float* ac = l_ac + tid * sa;
    const int* ai = reinterpret_cast<const int*>(ac);
    RowSums r{0.f, 0.f, 0.f};
    if (FAM == FAM_CAT) {
      cat_seg_stats(pd, og, P, ai[0], r);
    } else if (FAM == FAM_MCAT) {
      for (int c = 0; c < W; ++c) {
        const int o = mo.off[c];
        cat_seg_stats(pd + o, og + o, mo.off[c + 1] - o, ai[c], r);
      }
    } else {
      bern_row_stats(pd, og, ac, P, r);
    }
    GaussRow row;  // ppo_row_grads only reads logp_pi / logp_old
    row.logp_pi = r.lp;
    row.logp_old = r.lo;
    row.ent = r.ent;
    const PPORowGrads g =
        ppo_row_grads(row, l_sc[tid], l_sc[tile + tid], l_sc[2 * tile + tid],
                      l_sc[3 * tile + tid], B, clip, entcoeff, vcoeff, 1.f);
    // overwrite this lane's own oldpi row: it is read in the pass above
    // only, and only by this lane
    float* ghr = l_og + tid * sg;
    if (FAM == FAM_CAT) {
      cat_seg_grads(pd, ghr, P, ai[0], g.g_logp, g.g_ent);
    } else if (FAM == FAM_MCAT) {
      for (int c = 0; c < W; ++c) {
        const int o = mo.off[c];
        cat_seg_grads(pd + o, ghr + o, mo.off[c + 1] - o, ai[c], g.g_logp,
                      g.g_ent);
      }
    } else {
      bern_row_grads(pd, ac, ghr, P, g.g_logp, g.g_ent);
    }
    ghr[P] = g.g_v;
    for (int j = P + 1; j < ldgh; ++j) ghr[j] = 0.f;
  }
  __syncthreads();

  store_tile(l_og, gh + tb * ldgh, ldgh, sg, rows, tid);
}

// operand checks shared by the three entry points; `what` names the binding
void check_gh_args(const char* what, const torch::Tensor& lpi,
                   const torch::Tensor& lold, const torch::Tensor& vpred,
                   const torch::Tensor& oldv, const torch::Tensor& act,
                   int64_t W, torch::ScalarType act_dtype,
                   const torch::Tensor& adv, const torch::Tensor& etr,
                   const torch::Tensor& clip_dev) {
  TORCH_CHECK(lpi.is_cuda() && lpi.dtype() == torch::kFloat32 &&
                  lpi.is_contiguous() && lpi.dim() == 2 && lpi.size(0) >= 1,
              what, " needs contiguous fp32 logits [B][P], B >= 1");
  const int64_t B = lpi.size(0);
  TORCH_CHECK(lold.is_cuda() && lold.dtype() == torch::kFloat32 &&
                  lold.is_contiguous() && lold.sizes() == lpi.sizes(),
              what, " needs oldpi logits of the logits' shape and dtype");
  TORCH_CHECK(act.is_cuda() && act.dtype() == act_dtype &&
                  act.is_contiguous() && act.numel() == B * W,
              what, " needs contiguous actions [B][", W, "] of dtype ",
              act_dtype);
  for (const torch::Tensor* t : {&vpred, &oldv, &adv, &etr})
    TORCH_CHECK(t->is_cuda() && t->dtype() == torch::kFloat32 &&
                    t->is_contiguous() && t->numel() == B,
                what, " needs contiguous fp32 vpred/oldv/adv/etr of B rows");
  TORCH_CHECK(clip_dev.numel() == 0 ||
                  (clip_dev.is_cuda() && clip_dev.dtype() == torch::kFloat32),
              what, " needs an empty or fp32 device clip_dev");
}

template <int FAM>
torch::Tensor launch_disc_gh(const torch::Tensor& lpi,
                             const torch::Tensor& lold,
                             const torch::Tensor& vpred,
                             const torch::Tensor& oldv,
                             const torch::Tensor& act, int W,
                             const DiscOffsets& mo, const torch::Tensor& adv,
                             const torch::Tensor& etr, double clip,
                             double entcoeff, double vcoeff,
                             const torch::Tensor& clip_dev) {
  const int64_t B = lpi.size(0);
  const int P = static_cast<int>(lpi.size(1));
  // row stride padded to a float4 multiple, as ppo_loss_gauss_gh's
  const int ldgh = (P + 1 + 3) & ~3;
  auto gh = torch::empty({B, (int64_t)ldgh}, lpi.options());
  const int tile = disc_tile_rows(P, W);
  const int lds_bytes = tile * disc_row_floats(P, W) * (int)sizeof(float);
  TORCH_CHECK(lds_bytes <= 65536);  // holds for every P, W <= 64
  const int64_t grid = (B + tile - 1) / tile;
  TORCH_CHECK(grid <= INT32_MAX);
  const float* cd =
      (clip_dev.numel() > 0) ? clip_dev.data_ptr<float>() : nullptr;
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  hipLaunchKernelGGL(disc_gh_tile_kernel<FAM>, dim3((unsigned)grid), dim3(256),
                     lds_bytes, stream, lpi.data_ptr<float>(),
                     lold.data_ptr<float>(), vpred.data_ptr<float>(),
                     oldv.data_ptr<float>(), act.data_ptr(),
                     adv.data_ptr<float>(), etr.data_ptr<float>(),
                     gh.data_ptr<float>(), cd, mo, B, P, W, ldgh, tile,
                     (float)clip, (float)entcoeff, (float)vcoeff);
  return gh;
}

}  // namespace

int64_t ppo_gh_disc_tile(int64_t P, int64_t act_width) {
  TORCH_CHECK(P >= 1 && P <= WAVE && act_width >= 1 && act_width <= WAVE,
              "ppo_gh_disc_tile supports 1..64 logit and action columns");
  return disc_tile_rows(static_cast<int>(P), static_cast<int>(act_width));
}

torch::Tensor ppo_loss_cat_gh(torch::Tensor lpi, torch::Tensor lold,
                              torch::Tensor vpred, torch::Tensor oldv,
                              torch::Tensor act, torch::Tensor adv,
                              torch::Tensor etr, double clip, double entcoeff,
                              double vcoeff, torch::Tensor clip_dev) {
  check_gh_args("ppo_loss_cat_gh", lpi, lold, vpred, oldv, act, 1,
                torch::kInt64, adv, etr, clip_dev);
  TORCH_CHECK(lpi.size(1) >= 2 && lpi.size(1) <= WAVE,
              "ppo_loss_cat_gh supports 2 <= K <= 64");
  return launch_disc_gh<FAM_CAT>(lpi, lold, vpred, oldv, act, 1, DiscOffsets{},
                                 adv, etr, clip, entcoeff, vcoeff, clip_dev);
}

torch::Tensor ppo_loss_mcat_gh(torch::Tensor lpi, torch::Tensor lold,
                               torch::Tensor vpred, torch::Tensor oldv,
                               torch::Tensor act, torch::Tensor adv,
                               torch::Tensor etr, std::vector<int64_t> nvec,
                               double clip, double entcoeff, double vcoeff,
                               torch::Tensor clip_dev) {
  TORCH_CHECK(!nvec.empty() && nvec.size() <= (size_t)DISC_MAX_COMP,
              "ppo_loss_mcat_gh supports 1..32 components");
  DiscOffsets mo{};
  int64_t off = 0;
  for (size_t c = 0; c < nvec.size(); ++c) {
    TORCH_CHECK(nvec[c] >= 2 && off + nvec[c] <= WAVE,
                "ppo_loss_mcat_gh supports nvec[c] >= 2 and sum(nvec) <= 64");
    mo.off[c] = static_cast<int>(off);
    off += nvec[c];
  }
  mo.off[nvec.size()] = static_cast<int>(off);
  const int C = static_cast<int>(nvec.size());
  check_gh_args("ppo_loss_mcat_gh", lpi, lold, vpred, oldv, act, C,
                torch::kInt64, adv, etr, clip_dev);
  TORCH_CHECK(lpi.size(1) == off,
              "ppo_loss_mcat_gh needs logits width == sum(nvec)");
  return launch_disc_gh<FAM_MCAT>(lpi, lold, vpred, oldv, act, C, mo, adv, etr,
                                  clip, entcoeff, vcoeff, clip_dev);
}

torch::Tensor ppo_loss_bern_gh(torch::Tensor lpi, torch::Tensor lold,
                               torch::Tensor vpred, torch::Tensor oldv,
                               torch::Tensor act, torch::Tensor adv,
                               torch::Tensor etr, double clip, double entcoeff,
                               double vcoeff, torch::Tensor clip_dev) {
  TORCH_CHECK(lpi.dim() == 2 && lpi.size(1) >= 1 && lpi.size(1) <= WAVE,
              "ppo_loss_bern_gh supports 1 <= n <= 64");
  check_gh_args("ppo_loss_bern_gh", lpi, lold, vpred, oldv, act, lpi.size(1),
                torch::kFloat32, adv, etr, clip_dev);
  return launch_disc_gh<FAM_BERN>(lpi, lold, vpred, oldv, act,
                                  static_cast<int>(lpi.size(1)), DiscOffsets{},
                                  adv, etr, clip, entcoeff, vcoeff, clip_dev);
}
