// Python bindings for the dppo_amd gfx950 kernel library.
#include <torch/extension.h>

#include <vector>

std::vector<torch::Tensor> gae_scan(torch::Tensor rewards, torch::Tensor values,
                                    torch::Tensor dones, torch::Tensor boot,
                                    double gamma, double lam, bool whiten,
                                    double eps, torch::Tensor adv_out,
                                    torch::Tensor etr_out);

torch::Tensor ppo_loss_gauss_fwd(torch::Tensor pdpi, torch::Tensor pdold,
                                 torch::Tensor vpred, torch::Tensor oldv,
                                 torch::Tensor act, torch::Tensor adv,
                                 torch::Tensor etr, double clip,
                                 double entcoeff, double vcoeff);

torch::Tensor ppo_loss_gauss_gh(torch::Tensor pdflat, torch::Tensor oldflat,
                                torch::Tensor vpred, torch::Tensor oldv,
                                torch::Tensor act, torch::Tensor adv,
                                torch::Tensor etr, double clip,
                                double entcoeff, double vcoeff,
                                torch::Tensor clip_dev);

std::vector<torch::Tensor> ppo_loss_gauss_bwd(
    torch::Tensor pdpi, torch::Tensor pdold, torch::Tensor vpred,
    torch::Tensor oldv, torch::Tensor act, torch::Tensor adv,
    torch::Tensor etr, double clip, double entcoeff, double vcoeff,
    torch::Tensor gtotal);

torch::Tensor ppo_loss_cat_fwd(torch::Tensor lpi, torch::Tensor lold,
                               torch::Tensor vpred, torch::Tensor oldv,
                               torch::Tensor act, torch::Tensor adv,
                               torch::Tensor etr, double clip,
                               double entcoeff, double vcoeff);

std::vector<torch::Tensor> ppo_loss_cat_bwd(
    torch::Tensor lpi, torch::Tensor lold, torch::Tensor vpred,
    torch::Tensor oldv, torch::Tensor act, torch::Tensor adv,
    torch::Tensor etr, double clip, double entcoeff, double vcoeff,
    torch::Tensor gtotal);

torch::Tensor cat_sample(torch::Tensor logits, int64_t seed, int64_t ctr);

void bf16_mm256(torch::Tensor A, torch::Tensor B, torch::Tensor C,
                int64_t epi, torch::Tensor bias, torch::Tensor aux,
                torch::Tensor grad, int64_t grad_off, torch::Tensor CT,
                int64_t ldt, torch::Tensor sums, int64_t sums_off);

void bf16_mm_small(torch::Tensor A, torch::Tensor B, torch::Tensor C,
                   torch::Tensor C2, torch::Tensor aux, torch::Tensor grad,
                   int64_t g1_off, int64_t g2_off, int64_t srow, int64_t epi,
                   int64_t m_real, int64_t n_real, int64_t ldc,
                   torch::Tensor bias);

void bf16_transpose(torch::Tensor in, torch::Tensor out, torch::Tensor sums,
                    int64_t sums_off, int64_t R, int64_t C, int64_t ld_in,
                    int64_t ld_out);

void gauss_gh_wide(torch::Tensor pdflat_bf, torch::Tensor oldflat,
                   torch::Tensor v_bf, torch::Tensor oldv, torch::Tensor act,
                   torch::Tensor adv, torch::Tensor etr, torch::Tensor gh,
                   torch::Tensor clip_dev, double clip, double entcoeff,
                   double vcoeff);

void adam_step(torch::Tensor p, torch::Tensor g, torch::Tensor m,
               torch::Tensor v, int64_t step, double lr, double beta1,
               double beta2, double eps);

void adam_step_dev(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                   torch::Tensor v, torch::Tensor step_dev,
                   torch::Tensor lr_dev, torch::Tensor coef, double beta1,
                   double beta2, double eps);

void gemm_fwd(torch::Tensor X, torch::Tensor Wt, torch::Tensor bias,
              int64_t activation, int64_t heads, torch::Tensor C,
              torch::Tensor v, torch::Tensor aux, int64_t wt_layout,
              int64_t ablate, int64_t ldc);

bool mlp_fwd_fused_supported(int64_t D, int64_t H1, int64_t H2, int64_t A);

void mlp_fwd_fused(torch::Tensor X, torch::Tensor W1t, torch::Tensor b1,
                   torch::Tensor W2t, torch::Tensor b2, torch::Tensor WhT_pad,
                   torch::Tensor bh_pad, int64_t act_code, torch::Tensor h1,
                   torch::Tensor h2, torch::Tensor pdflat, torch::Tensor v,
                   torch::Tensor actions, torch::Tensor xva,
                   torch::Tensor seed_dev, torch::Tensor eps_dev, int64_t step,
                   int64_t va_off, double act_low, double act_high);

void dw_mfma(torch::Tensor delta, torch::Tensor acts, torch::Tensor grad_buf,
             int64_t w_off, int64_t b_off, int64_t split_row, int64_t w_off2,
             int64_t b_off2, int64_t ablate);

void rollout_sample(torch::Tensor pdflat, torch::Tensor actions,
                    torch::Tensor xva, torch::Tensor seed_dev,
                    torch::Tensor eps_dev, int64_t step, int64_t va_off,
                    double act_low, double act_high);

void gemm_env_step(torch::Tensor xva, torch::Tensor M, torch::Tensor xin,
                   torch::Tensor xout, torch::Tensor envd,
                   torch::Tensor horizons, torch::Tensor t,
                   torch::Tensor epr,
                   torch::Tensor rewards, torch::Tensor dones,
                   torch::Tensor rsum, torch::Tensor seed_dev, double sigma,
                   int64_t step, torch::Tensor V, torch::Tensor xvp);

void env_step_rows(torch::Tensor xva, torch::Tensor M, torch::Tensor xin,
                   torch::Tensor xout, torch::Tensor envd,
                   torch::Tensor horizons, torch::Tensor t,
                   torch::Tensor epr, torch::Tensor rewards,
                   torch::Tensor dones, torch::Tensor seed_dev, double sigma,
                   int64_t step, torch::Tensor V);

void rollout_env_step(torch::Tensor xin, torch::Tensor xout, torch::Tensor G,
                      torch::Tensor envd, torch::Tensor horizons,
                      torch::Tensor t, torch::Tensor epr,
                      torch::Tensor rewards, torch::Tensor dones,
                      torch::Tensor seed_dev, double sigma, int64_t step);

torch::Tensor rollout_moments(torch::Tensor rewards, torch::Tensor dones,
                              torch::Tensor epr_in, int64_t T, int64_t E);

bool mlp_chunk_supported(int64_t D, int64_t H, int64_t A, int64_t n_hidden);

void mlp_chunk_train(
    torch::Tensor params, torch::Tensor states, torch::Tensor actions,
    torch::Tensor adv, torch::Tensor etr, torch::Tensor oldflat,
    torch::Tensor oldv, std::vector<int64_t> offsets,
    std::vector<int64_t> dims, int64_t activation, torch::Tensor clip_dev,
    double clip, double entcoeff, double vcoeff, torch::Tensor slabs,
    torch::Tensor mom, torch::Tensor vel, torch::Tensor step_dev,
    torch::Tensor lr_dev, torch::Tensor coef, torch::Tensor flat_grad,
    bool fuse_adam, double beta1, double beta2, double eps);

bool mlp_mid_supported(int64_t H1, int64_t H2, int64_t A, int64_t n_hidden);

void mlp_mid_bwd(torch::Tensor params, std::vector<int64_t> offsets,
                 torch::Tensor h1, torch::Tensor h2, torch::Tensor pdflat,
                 torch::Tensor v, torch::Tensor oldflat, torch::Tensor oldv,
                 torch::Tensor act, torch::Tensor adv, torch::Tensor etr,
                 int64_t activation, torch::Tensor clip_dev, double clip,
                 double entcoeff, double vcoeff, torch::Tensor dz1,
                 torch::Tensor grad);

std::vector<torch::Tensor> rollout_run(
    torch::Tensor params, std::vector<int64_t> offsets,
    std::vector<int64_t> dims, int64_t activation,
    torch::Tensor envblob, int64_t rank, torch::Tensor horizons,
    double noise, double act_low, double act_high, double eps_explore,
    torch::Tensor x, torch::Tensor t, torch::Tensor epr,
    int64_t T, int64_t act_dim, int64_t seed, torch::Tensor out_buf,
    int64_t ablate);

std::vector<torch::Tensor> rollout_run_cat(
    torch::Tensor params, std::vector<int64_t> offsets,
    std::vector<int64_t> dims, int64_t activation,
    torch::Tensor envblob, int64_t rank, torch::Tensor horizons,
    double noise, double eps_explore,
    torch::Tensor x, torch::Tensor t, torch::Tensor epr,
    int64_t T, int64_t n_actions, int64_t seed, torch::Tensor out_buf,
    int64_t ablate);

std::vector<torch::Tensor> rollout_run_mcat(
    torch::Tensor params, std::vector<int64_t> offsets,
    std::vector<int64_t> dims, int64_t activation,
    torch::Tensor envblob, int64_t rank, torch::Tensor horizons,
    double noise, double eps_explore,
    torch::Tensor x, torch::Tensor t, torch::Tensor epr,
    int64_t T, std::vector<int64_t> nvec, int64_t seed, torch::Tensor out_buf,
    int64_t ablate);

std::vector<torch::Tensor> rollout_run_bern(
    torch::Tensor params, std::vector<int64_t> offsets,
    std::vector<int64_t> dims, int64_t activation,
    torch::Tensor envblob, int64_t rank, torch::Tensor horizons,
    double noise, double eps_explore,
    torch::Tensor x, torch::Tensor t, torch::Tensor epr,
    int64_t T, int64_t n, int64_t seed, torch::Tensor out_buf,
    int64_t ablate);

torch::Tensor ppo_loss_mcat_fwd(torch::Tensor lpi, torch::Tensor lold,
                                torch::Tensor vpred, torch::Tensor oldv,
                                torch::Tensor act, torch::Tensor adv,
                                torch::Tensor etr, std::vector<int64_t> nvec,
                                double clip, double entcoeff, double vcoeff);

std::vector<torch::Tensor> ppo_loss_mcat_bwd(
    torch::Tensor lpi, torch::Tensor lold, torch::Tensor vpred,
    torch::Tensor oldv, torch::Tensor act, torch::Tensor adv,
    torch::Tensor etr, std::vector<int64_t> nvec, double clip,
    double entcoeff, double vcoeff, torch::Tensor gtotal);

torch::Tensor ppo_loss_bern_fwd(torch::Tensor lpi, torch::Tensor lold,
                                torch::Tensor vpred, torch::Tensor oldv,
                                torch::Tensor act, torch::Tensor adv,
                                torch::Tensor etr, double clip,
                                double entcoeff, double vcoeff);

std::vector<torch::Tensor> ppo_loss_bern_bwd(
    torch::Tensor lpi, torch::Tensor lold, torch::Tensor vpred,
    torch::Tensor oldv, torch::Tensor act, torch::Tensor adv,
    torch::Tensor etr, double clip, double entcoeff, double vcoeff,
    torch::Tensor gtotal);

torch::Tensor mcat_sample(torch::Tensor logits, std::vector<int64_t> nvec,
                          int64_t seed, int64_t ctr);

torch::Tensor bern_sample(torch::Tensor logits, int64_t seed, int64_t ctr);

torch::Tensor ppo_loss_cat_gh(torch::Tensor lpi, torch::Tensor lold,
                              torch::Tensor vpred, torch::Tensor oldv,
                              torch::Tensor act, torch::Tensor adv,
                              torch::Tensor etr, double clip, double entcoeff,
                              double vcoeff, torch::Tensor clip_dev);

torch::Tensor ppo_loss_mcat_gh(torch::Tensor lpi, torch::Tensor lold,
                               torch::Tensor vpred, torch::Tensor oldv,
                               torch::Tensor act, torch::Tensor adv,
                               torch::Tensor etr, std::vector<int64_t> nvec,
                               double clip, double entcoeff, double vcoeff,
                               torch::Tensor clip_dev);

torch::Tensor ppo_loss_bern_gh(torch::Tensor lpi, torch::Tensor lold,
                               torch::Tensor vpred, torch::Tensor oldv,
                               torch::Tensor act, torch::Tensor adv,
                               torch::Tensor etr, double clip, double entcoeff,
                               double vcoeff, torch::Tensor clip_dev);

int64_t ppo_gh_disc_tile(int64_t P, int64_t act_width);

std::vector<torch::Tensor> classic_rollout_cat(
    torch::Tensor params, std::vector<int64_t> offsets,
    std::vector<int64_t> dims, int64_t activation, int64_t env_id,
    torch::Tensor s, int64_t time_limit, double eps_explore, torch::Tensor x,
    torch::Tensor t, torch::Tensor epr, int64_t T, int64_t n_actions,
    int64_t seed, torch::Tensor out_buf);

std::vector<torch::Tensor> classic_rollout_box(
    torch::Tensor params, std::vector<int64_t> offsets,
    std::vector<int64_t> dims, int64_t activation, int64_t env_id,
    torch::Tensor s, int64_t time_limit, double act_low, double act_high,
    double eps_explore, torch::Tensor x, torch::Tensor t, torch::Tensor epr,
    int64_t T, int64_t act_dim, int64_t seed, torch::Tensor out_buf);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, mod) {
  mod.def("classic_rollout_cat", &classic_rollout_cat,
          "lane-per-env T-step CartPole (env_id 0, Discrete(2)), Acrobot "
          "(env_id 2, Discrete(3), RK4) or MountainCar (env_id 3, Discrete(3)) "
          "rollout, Categorical policy: MLP fwd + "
          "Gumbel-max sample + physics step, int64 actions; rollout_run_cat's "
          "out blob with K = n_actions (gfx950)");
  mod.def("classic_rollout_box", &classic_rollout_box,
          "lane-per-env T-step Pendulum (env_id 1) or MountainCarContinuous "
          "(env_id 4) rollout, Box(1)/DiagGaussian policy: "
          "MLP fwd + sample + physics step; rollout_run's out blob (gfx950)");
  mod.def("ppo_loss_cat_gh", &ppo_loss_cat_gh,
          "Categorical PPO loss gradient -> gh [B][ldgh] = [g_logits | g_v | "
          "0], int64 actions [B]; layout: ops.ppo_loss.ppo_gh_ref (gfx950)");
  mod.def("ppo_loss_mcat_gh", &ppo_loss_mcat_gh,
          "MultiCategorical PPO loss gradient -> gh [B][ldgh] = [g_logits | "
          "g_v | 0], int64 actions [B][C]; layout: ops.ppo_loss.ppo_gh_ref "
          "(gfx950)");
  mod.def("ppo_loss_bern_gh", &ppo_loss_bern_gh,
          "Bernoulli PPO loss gradient -> gh [B][ldgh] = [g_logits | g_v | "
          "0], float 0/1 actions [B][n]; layout: ops.ppo_loss.ppo_gh_ref "
          "(gfx950)");
  mod.def("ppo_gh_disc_tile", &ppo_gh_disc_tile,
          "rows per block of the ppo_loss_{cat,mcat,bern}_gh kernels for P "
          "logit and act_width action columns");
  mod.def("rollout_run_mcat", &rollout_run_mcat,
          "fused T-step rollout, MultiDiscrete/MultiCategorical policy: MLP "
          "fwd + per-component Gumbel-max + synthetic env, int64 actions "
          "(gfx950)");
  mod.def("rollout_run_bern", &rollout_run_bern,
          "fused T-step rollout, MultiBinary/Bernoulli policy: MLP fwd + "
          "Bernoulli sample + synthetic env, float 0/1 actions (gfx950)");
  mod.def("ppo_loss_mcat_fwd", &ppo_loss_mcat_fwd,
          "fused MultiCategorical PPO loss forward (gfx950)");
  mod.def("ppo_loss_mcat_bwd", &ppo_loss_mcat_bwd,
          "fused MultiCategorical PPO loss backward (gfx950)");
  mod.def("ppo_loss_bern_fwd", &ppo_loss_bern_fwd,
          "fused Bernoulli PPO loss forward (gfx950)");
  mod.def("ppo_loss_bern_bwd", &ppo_loss_bern_bwd,
          "fused Bernoulli PPO loss backward (gfx950)");
  mod.def("mcat_sample", &mcat_sample,
          "per-component Gumbel-max sampling, counter-based RNG (gfx950)");
  mod.def("bern_sample", &bern_sample,
          "Bernoulli sampling, counter-based RNG (gfx950)");
  mod.def("gae_scan", &gae_scan,
          "segmented GAE reverse scan + whitening (gfx950)");
  mod.def("ppo_loss_gauss_fwd", &ppo_loss_gauss_fwd,
          "fused DiagGaussian PPO loss forward (gfx950)");
  mod.def("ppo_loss_gauss_bwd", &ppo_loss_gauss_bwd,
          "fused DiagGaussian PPO loss backward (gfx950)");
  mod.def("ppo_loss_cat_fwd", &ppo_loss_cat_fwd,
          "fused Categorical PPO loss forward (gfx950)");
  mod.def("ppo_loss_cat_bwd", &ppo_loss_cat_bwd,
          "fused Categorical PPO loss backward (gfx950)");
  mod.def("cat_sample", &cat_sample,
          "Gumbel-max categorical sampling, counter-based RNG (gfx950)");
  mod.def("bf16_mm256", &bf16_mm256,
          "bf16 MFMA GEMM, 256^2 tile, pipelined glds, fused epilogues "
          "(gfx950)");
  mod.def("bf16_mm_small", &bf16_mm_small,
          "guarded bf16 MFMA GEMM for ragged heads shapes (gfx950)");
  mod.def("bf16_transpose", &bf16_transpose,
          "bf16 2D transpose with fused column sums (gfx950)");
  mod.def("gauss_gh_wide", &gauss_gh_wide,
          "wide-policy PPO loss gradient -> bf16 [g_pd | g_v] (gfx950)");
  mod.def("adam_step", &adam_step, "fused flat Adam step (gfx950)");
  mod.def("adam_step_dev", &adam_step_dev,
          "graph-replayable fused Adam (device step/lr) (gfx950)");
  mod.def("rollout_run", &rollout_run,
          "fused T-step rollout: MLP fwd + sample + synthetic env (gfx950)");
  mod.def("rollout_run_cat", &rollout_run_cat,
          "fused T-step rollout, Discrete/Categorical policy: MLP fwd + "
          "Gumbel-max sample + synthetic env, int64 actions (gfx950)");
  mod.def("rollout_sample", &rollout_sample,
          "per-step action sampling + eps-greedy (v3 rollout) (gfx950)");
  mod.def("gemm_env_step", &gemm_env_step,
          "fused G-GEMM + env transition epilogue + per-env finish, "
          "optionally folding the next step's x@V (v3 rollout; gfx950)");
  mod.def("env_step_rows", &env_step_rows,
          "row-owning env step: G-GEMM + env transition + per-env finish + "
          "the next step's x@V in one launch, bitwise gemm_env_step + "
          "gemm_fwd (v3 rollout; gfx950)");
  mod.def("rollout_env_step", &rollout_env_step,
          "per-step synthetic env finish: tanh/reward/done/reset (gfx950)");
  mod.def("rollout_moments", &rollout_moments,
          "episode-reward moments from reward/done streams (gfx950)");
  mod.def("ppo_loss_gauss_gh", &ppo_loss_gauss_gh,
          "wave-per-row PPO loss gradient -> [g_pd | g_v] (gfx950)");
  mod.def("gemm_fwd", &gemm_fwd,
          "MFMA f32 layer forward C=act(X@Wt+b), fused tanh (gfx950)");
  mod.def("mlp_fwd_fused_supported", &mlp_fwd_fused_supported,
          "shape eligibility for the fused policy forward (gfx950)");
  mod.def("mlp_fwd_fused", &mlp_fwd_fused,
          "fused policy forward: L1 + L2 + heads (+ action sampling) in one "
          "launch, h1/h2 written once and never re-read (gfx950)");
  mod.def("dw_mfma", &dw_mfma,
          "MFMA f32 split-K dW += delta^T@acts into flat grad (gfx950)");
  mod.def("mlp_chunk_supported", &mlp_chunk_supported,
          "shape eligibility for the fused chunk-step kernel (gfx950)");
  mod.def("mlp_chunk_train", &mlp_chunk_train,
          "fused small-MLP training chunk step: fwd+PPO grad+bwd+dW "
          "partials + slab-reduce Adam (gfx950)");
  mod.def("mlp_mid_supported", &mlp_mid_supported,
          "shape eligibility for the fused update-middle kernel (gfx950)");
  mod.def("mlp_mid_bwd", &mlp_mid_bwd,
          "fused update middle: PPO grad + heads/L2 dgrad + dW2/heads dW "
          "partials -> dz1 and flat grad, no gh/dz2 in HBM (gfx950)");
}
