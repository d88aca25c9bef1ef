// Classic-control rollout (gfx950): the whole T-step rollout of CartPole-v0,
// Pendulum-v1, Acrobot-v1, MountainCar-v0 or MountainCarContinuous-v0 in one
// launch, ONE LANE PER ENV.
//
// A classic-control env is a handful of scalars, so rollout.hip's
// decomposition (8 envs per 256-thread block, lanes split over the
// observation dimension) would leave 4 lanes busy in its env phase.  Here a
// lane owns one env for the whole loop: its state, step counter and episode
// return stay in registers, and per step it runs the policy forward, samples
// with the epsilon overlay, steps the physics (classic_env.h), books the
// episode and resets.  After the T steps it computes the bootstrap value and
// persists s, x, t and epr.  The episode moments (count, sum, sum of
// squares, min, max of the finished episodes' returns) are kept per lane and
// folded in fixed order, per block and then by classic_moments_kernel, so
// every output of a launch is bitwise reproducible.
//
// Block = one wave.  The policy weights are wave-uniform: they are staged
// once into LDS (rows padded to 4 floats, pads zero, so every loop runs on
// the padded width and padded units contribute act(0) * 0) and read as
// same-address float4 broadcasts.  There is no inter-lane communication and
// no barrier between the staging and the moments butterfly that ends the
// kernel.
//   - Layer 1 reads the observation from registers (D is a template
//     constant) and produces units four at a time.
//   - With two hidden layers, layer 1's activations go to a per-lane LDS
//     image laid out [unit][lane] (bank = lane: conflict-free), because a
//     per-lane array indexed by a runtime unit would go to scratch; layer 2
//     reads one image dword + four weight float4s per 16 FMAs (units 16 at
//     a time, a 4-unit tile for the rest).
//   - The LAST hidden layer is never stored: each unit is folded into the
//     1 + P head accumulators (v, p0, p1 and, for P = 3, p2) as it is
//     produced.  P, the number of policy-head columns, is a compile-time
//     property of the env (ClassicEnv<ENV>::P): 2 for CartPole (2 logits),
//     Pendulum and MountainCarContinuous (mean, logstd), 3 for Acrobot and
//     MountainCar (3 logits).  Heads are staged as
//     one float4 (Wv, Wp0, Wp1, Wp2 or 0) per unit, so P = 3 fills the lane
//     that P = 2 pads and the LDS layout is the same for both.
//   - The env step runs in scalar registers.  Acrobot's is one RK4 step: four
//     derivative evaluations with their own sines and cosines
//     (classic_env.h), about the cost of a (16,) trunk.
// Per-step global writes have lane == env ([T][E] and [T][E][D] rows), so
// they are coalesced by construction; 16-byte CartPole state rows, 8-byte
// MountainCar state rows and 8-byte pd rows go out as one vector store,
// 24-byte Acrobot state rows as three float2 stores, where the row base is
// aligned; 12-byte K = 3 pd rows go out as scalars (lane stride 12 B is
// still a dense wave write).
//
// Limits (checked in the bindings, mirrored by the engine's
// _can_rollout_classic): 1-2 hidden layers of width <= 64; Categorical with
// K = 2 on CartPole and K = 3 on Acrobot and MountainCar, DiagGaussian with
// A = 1 on Pendulum and MountainCarContinuous.  The family is a property of
// the env (ClassicEnv<ENV>::BOX); the step inside the T loop is chosen by ENV.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "classic_env.h"
#include "common.h"
#include "rollout_blob.h"

namespace {

constexpr int CL_MAX_H = 64;
constexpr int CL_FAM_BOX = 0;  // DiagGaussian, A = 1: pd = (mean, logstd)
constexpr int CL_FAM_CAT = 1;  // Categorical, K = 2 or 3: pd = K logits

struct ClassicArgs {
  const float* params;  // _rollout_weight_blob(): Wt[in][out], b per hidden
                        // layer, Wv[H], bv, Wpt[H][P], bp
  int off_w[2], off_b[2], off_wv, off_bv, off_wp, off_bp;
  int H[2];             // hidden widths (H[1] unused with one layer)
  int activation;       // 1 tanh, 0 relu
  float* s;             // [E][S] env state, in/out
  float* x;             // [E][D] observation, out
  int* t;               // [E] step counters, in/out
  float* epr;           // [E] running episode returns, in/out
  float* out;           // output blob (layouts: the bindings)
  float* part;          // [grid][5] per-block episode moments
  int E, T, time_limit;
  unsigned seed;
  float eps, act_low, act_high;
};

// float offsets of the staged weights (and the h1 image) in LDS
struct ClassicLds {
  int w1, b1, w2, b2, heads, hb, img, total;
  int h0p, h1p;  // padded widths
};

template <int NH>
__host__ __device__ inline ClassicLds classic_lds(int D, int H0, int H1) {
  ClassicLds m;
  m.h0p = (H0 + 3) & ~3;
  m.h1p = (H1 + 3) & ~3;
  int o = 0;
  m.w1 = o; o += D * m.h0p;
  m.b1 = o; o += m.h0p;
  m.w2 = o; o += (NH == 2) ? m.h0p * m.h1p : 0;
  m.b2 = o; o += (NH == 2) ? m.h1p : 0;
  m.heads = o; o += 4 * ((NH == 2) ? m.h1p : m.h0p);
  m.hb = o; o += 4;
  m.img = o; o += (NH == 2) ? m.h0p * WAVE : 0;
  m.total = o;
  return m;
}

DEV_INLINE float4 activate4(float4 z, int activation) {
  if (activation) {
    z.x = fast_tanhf(z.x); z.y = fast_tanhf(z.y);
    z.z = fast_tanhf(z.z); z.w = fast_tanhf(z.w);
  } else {
    z.x = fmaxf(z.x, 0.f); z.y = fmaxf(z.y, 0.f);
    z.z = fmaxf(z.z, 0.f); z.w = fmaxf(z.w, 0.f);
  }
  return z;
}

// fold last-layer units j..j+3 (activations h) into the head accumulators
// (p2 is touched only with P = 3)
template <int P>
DEV_INLINE void heads4(const float* lds, const ClassicLds& m, int j, float4 h,
                       float& v, float& p0, float& p1, float& p2) {
  const float4* hw = reinterpret_cast<const float4*>(lds + m.heads) + j;
  const float hh[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float4 w = hw[i];
    v = fmaf(w.x, hh[i], v);
    p0 = fmaf(w.y, hh[i], p0);
    p1 = fmaf(w.z, hh[i], p1);
    if constexpr (P == 3) p2 = fmaf(w.w, hh[i], p2);
  }
}

// Units j..j+JT-1 of the second hidden layer from this lane's image column,
// folded into the heads.  One image dword and JT/4 weight float4s feed JT
// FMAs per k; each unit still sums over k in ascending order, so the tile
// width does not change a result.  With the image (35 KB per block at
// 64x64) LDS holds the CU to four blocks, one wave per SIMD, so the wide
// tile's independent chains are what hides the LDS latency: CartPole (64,64)
// at E=65536 took 3.63 ms per rollout with 4-unit tiles only, 1.97 ms with
// the 16-unit tile (profiles/r12_rollout_classic.txt).
template <int JT, int P>
DEV_INLINE void hidden2_tile(const float* lds, const ClassicLds& m,
                             const float* img, int j, int activation,
                             float& v, float& p0, float& p1, float& p2) {
  constexpr int Q = JT / 4;
  float4 z[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q)
    z[q] = *reinterpret_cast<const float4*>(lds + m.b2 + j + 4 * q);
#pragma unroll 4
  for (int k = 0; k < m.h0p; ++k) {
    const float h = img[k * WAVE];
    const float4* w =
        reinterpret_cast<const float4*>(lds + m.w2 + k * m.h1p + j);
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const float4 wq = w[q];
      z[q].x = fmaf(wq.x, h, z[q].x);
      z[q].y = fmaf(wq.y, h, z[q].y);
      z[q].z = fmaf(wq.z, h, z[q].z);
      z[q].w = fmaf(wq.w, h, z[q].w);
    }
  }
#pragma unroll
  for (int q = 0; q < Q; ++q)
    heads4<P>(lds, m, j + 4 * q, activate4(z[q], activation), v, p0, p1, p2);
}

// policy forward of one lane's observation x[D]: value and the P pd params
template <int D, int NH, int P>
DEV_INLINE void classic_forward(float* lds, const ClassicLds& m,
                                const float* x, int activation, float& v,
                                float& p0, float& p1, float& p2) {
  const float4 hb = *reinterpret_cast<const float4*>(lds + m.hb);
  v = hb.x;
  p0 = hb.y;
  p1 = hb.z;
  if constexpr (P == 3) p2 = hb.w;
  float* img = lds + m.img + threadIdx.x;  // this lane's column
  for (int j = 0; j < m.h0p; j += 4) {
    float4 z = *reinterpret_cast<const float4*>(lds + m.b1 + j);
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const float4 w =
          *reinterpret_cast<const float4*>(lds + m.w1 + d * m.h0p + j);
      z.x = fmaf(w.x, x[d], z.x);
      z.y = fmaf(w.y, x[d], z.y);
      z.z = fmaf(w.z, x[d], z.z);
      z.w = fmaf(w.w, x[d], z.w);
    }
    z = activate4(z, activation);
    if constexpr (NH == 1) {
      heads4<P>(lds, m, j, z, v, p0, p1, p2);
    } else {
      img[(j + 0) * WAVE] = z.x;
      img[(j + 1) * WAVE] = z.y;
      img[(j + 2) * WAVE] = z.z;
      img[(j + 3) * WAVE] = z.w;
    }
  }
  if constexpr (NH == 2) {
    // the image column is this lane's own: written and read by the same
    // lane in program order, no barrier
    int j = 0;
    for (; j + 16 <= m.h1p; j += 16)
      hidden2_tile<16, P>(lds, m, img, j, activation, v, p0, p1, p2);
    for (; j < m.h1p; j += 4)
      hidden2_tile<4, P>(lds, m, img, j, activation, v, p0, p1, p2);
  }
}

// rows x cols block of the blob (row stride cols) -> LDS (row stride colsp,
// rows .. rowsp and cols .. colsp zero)
DEV_INLINE void stage_padded(float* dst, const float* __restrict__ src,
                             int rows, int cols, int rowsp, int colsp) {
  for (int i = threadIdx.x; i < rowsp * colsp; i += blockDim.x) {
    const int r = i / colsp, c = i - r * colsp;
    dst[i] = (r < rows && c < cols) ? src[r * cols + c] : 0.f;
  }
}

// Episode moments, in two fixed-order stages so that a launch is bitwise
// reproducible (ep_moments_kernel's float atomics are not): an xor butterfly
// over the wave, one [5] partial per block; classic_moments_kernel below
// folds the partials.
DEV_INLINE void wave_moments(float& c, float& s, float& ss, float& mn,
                             float& mx) {
#pragma unroll
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    c += __shfl_xor(c, off, WAVE);
    s += __shfl_xor(s, off, WAVE);
    ss += __shfl_xor(ss, off, WAVE);
    mn = fminf(mn, __shfl_xor(mn, off, WAVE));
    mx = fmaxf(mx, __shfl_xor(mx, off, WAVE));
  }
}

DEV_INLINE void classic_block_moments(float* __restrict__ part, float c,
                                      float s, float ss, float mn, float mx) {
  wave_moments(c, s, ss, mn, mx);
  if (threadIdx.x == 0) {
    float* p = part + 5 * (int64_t)blockIdx.x;
    p[0] = c; p[1] = s; p[2] = ss; p[3] = mn; p[4] = mx;
  }
}

// One wave: lane l folds partials l, l + 64, ... in ascending order, then the
// butterfly; min and max are 0 when no episode finished, as
// ep_moments_decode_kernel has them.
__global__ __launch_bounds__(WAVE) void classic_moments_kernel(
    const float* __restrict__ part, int nblocks, float* __restrict__ out) {
  float c = 0.f, s = 0.f, ss = 0.f, mn = 3.0e38f, mx = -3.0e38f;
  for (int b = threadIdx.x; b < nblocks; b += WAVE) {
    const float* p = part + 5 * (int64_t)b;
    c += p[0];
    s += p[1];
    ss += p[2];
    mn = fminf(mn, p[3]);
    mx = fmaxf(mx, p[4]);
  }
  wave_moments(c, s, ss, mn, mx);
  if (threadIdx.x == 0) {
    out[0] = c; out[1] = s; out[2] = ss;
    out[3] = (c > 0.f) ? mn : 0.f;
    out[4] = (c > 0.f) ? mx : 0.f;
  }
}

template <int FAM, int ENV, int NH>
__global__ __launch_bounds__(WAVE) void classic_rollout_kernel(ClassicArgs a) {
  constexpr int S = ClassicEnv<ENV>::S;
  constexpr int D = ClassicEnv<ENV>::D;
  constexpr int P = ClassicEnv<ENV>::P;
  static_assert((FAM == CL_FAM_BOX) == ClassicEnv<ENV>::BOX,
                "policy family and env do not go together");
  extern __shared__ __align__(16) float lds[];
  const ClassicLds m = classic_lds<NH>(D, a.H[0], a.H[1]);

  // ---- stage the weights -------------------------------------------------
  const int HL = (NH == 2) ? a.H[1] : a.H[0];  // last hidden width
  const int hlp = (NH == 2) ? m.h1p : m.h0p;
  stage_padded(lds + m.w1, a.params + a.off_w[0], D, a.H[0], D, m.h0p);
  stage_padded(lds + m.b1, a.params + a.off_b[0], 1, a.H[0], 1, m.h0p);
  if constexpr (NH == 2) {
    stage_padded(lds + m.w2, a.params + a.off_w[1], a.H[0], a.H[1], m.h0p,
                 m.h1p);
    stage_padded(lds + m.b2, a.params + a.off_b[1], 1, a.H[1], 1, m.h1p);
  }
  for (int j = threadIdx.x; j < hlp; j += blockDim.x) {
    const bool in = j < HL;
    lds[m.heads + 4 * j + 0] = in ? a.params[a.off_wv + j] : 0.f;
    lds[m.heads + 4 * j + 1] = in ? a.params[a.off_wp + P * j] : 0.f;
    lds[m.heads + 4 * j + 2] = in ? a.params[a.off_wp + P * j + 1] : 0.f;
    lds[m.heads + 4 * j + 3] =
        (P == 3 && in) ? a.params[a.off_wp + P * j + P - 1] : 0.f;
  }
  if (threadIdx.x == 0) {
    lds[m.hb + 0] = a.params[a.off_bv];
    lds[m.hb + 1] = a.params[a.off_bp];
    lds[m.hb + 2] = a.params[a.off_bp + 1];
    lds[m.hb + 3] = (P == 3) ? a.params[a.off_bp + P - 1] : 0.f;
  }
  __syncthreads();

  // finished-episode moments of this lane's env: count, sum, sum of squares,
  // min, max of the episode returns
  float mc = 0.f, ms = 0.f, mss = 0.f, mn = 3.0e38f, mx = -3.0e38f;
  const int e = blockIdx.x * WAVE + threadIdx.x;
  if (e < a.E) {  // no barrier below; tail lanes only join the reduction
    // ---- carve the output blob --------------------------------------------
    // the layout rollout_blob.h defines (rollout_blob(T, E, D, P, 1, FAM ==
    // CL_FAM_CAT)), spelled out here because taking the offsets from the
    // struct changed the instructions of four of the ten instantiations
    // (<0,4,2>, <1,0,2>, <1,3,1>, <1,3,2>: 2 to 42 lines each, same counts)
    const int64_t TE = (int64_t)a.T * a.E;
    float* o = a.out;
    int64_t* act_i64 = nullptr;
    float* act_f = nullptr;
    if constexpr (FAM == CL_FAM_CAT) {
      act_i64 = reinterpret_cast<int64_t*>(o);
      o += 2 * TE;
    }
    float* states = o; o += TE * D;
    float* pd = o; o += TE * P;
    if constexpr (FAM == CL_FAM_BOX) {
      act_f = o;
      o += TE;
    }
    float* values = o; o += TE;
    float* rewards = o; o += TE;
    float* dones = o; o += TE;
    float* boot = o;
    const bool states_vec =
        D == 4 && (reinterpret_cast<uintptr_t>(states) & 15) == 0;
    const bool states_vec2 =
        (D == 6 || D == 2) && (reinterpret_cast<uintptr_t>(states) & 7) == 0;
    const bool pd_vec = (reinterpret_cast<uintptr_t>(pd) & 7) == 0;

    // ---- this lane's env --------------------------------------------------
    float s[S], x[D];
#pragma unroll
    for (int d = 0; d < S; ++d) s[d] = a.s[(int64_t)e * S + d];
    classic_obs<ENV>(s, x);
    int tc = a.t[e];
    float ep = a.epr[e];

    for (int step = 0; step < a.T; ++step) {
      const int64_t i = (int64_t)step * a.E + e;
      bool row_stored = false;
      if constexpr (D == 4) {
        if (states_vec) {
          *reinterpret_cast<float4*>(states + i * 4) =
              make_float4(x[0], x[1], x[2], x[3]);
          row_stored = true;
        }
      }
      if constexpr (D == 6) {
        if (states_vec2) {
          float2* row = reinterpret_cast<float2*>(states + i * 6);
          row[0] = make_float2(x[0], x[1]);
          row[1] = make_float2(x[2], x[3]);
          row[2] = make_float2(x[4], x[5]);
          row_stored = true;
        }
      }
      if constexpr (D == 2) {
        if (states_vec2) {
          *reinterpret_cast<float2*>(states + i * 2) = make_float2(x[0], x[1]);
          row_stored = true;
        }
      }
      if (!row_stored) {
#pragma unroll
        for (int d = 0; d < D; ++d) states[i * D + d] = x[d];
      }
      float v, p0, p1, p2;
      classic_forward<D, NH, P>(lds, m, x, a.activation, v, p0, p1, p2);
      if constexpr (P == 3) {
        pd[i * 3] = p0;
        pd[i * 3 + 1] = p1;
        pd[i * 3 + 2] = p2;
      } else if (pd_vec) {
        *reinterpret_cast<float2*>(pd + i * 2) = make_float2(p0, p1);
      } else {
        pd[i * 2] = p0;
        pd[i * 2 + 1] = p1;
      }
      values[i] = v;

      float r;
      int done;
      if constexpr (FAM == CL_FAM_CAT) {
        int arg;
        if constexpr (P == 3) {
          arg = mcat_draw(
              [&](int c) { return c == 0 ? p0 : (c == 1 ? p1 : p2); }, 0, 3,
              a.seed, e, step);
        } else {
          arg = mcat_draw([&](int c) { return c == 0 ? p0 : p1; }, 0, 2,
                          a.seed, e, step);
        }
        arg = mcat_explore(arg, P, 0, a.seed, e, step, a.eps);
        act_i64[i] = arg;
        if constexpr (ENV == ENV_CARTPOLE) {
          done = cartpole_step(s, arg, r);
        } else if constexpr (ENV == ENV_ACROBOT) {
          done = acrobot_step(s, arg, r);
        } else {
          static_assert(ENV == ENV_MOUNTAINCAR, "no step for this env");
          done = mountaincar_step(s, arg, r);
        }
      } else {
        const float act = box_sample(p0, p1, a.seed, e, step, 0, a.eps,
                                     a.act_low, a.act_high);
        act_f[i] = act;
        if constexpr (ENV == ENV_PENDULUM) {
          done = pendulum_step(s, act, r);
        } else {
          static_assert(ENV == ENV_MOUNTAINCAR_CONT, "no step for this env");
          done = mountaincar_cont_step(s, act, r);
        }
      }
      rewards[i] = r;
      ep += r;
      tc += 1;
      done |= (tc >= a.time_limit) ? 1 : 0;
      dones[i] = (float)done;
      if (done) {
        mc += 1.f;
        ms += ep;
        mss += ep * ep;
        mn = fminf(mn, ep);
        mx = fmaxf(mx, ep);
        ep = 0.f;
        tc = 0;
        classic_reset<ENV>(s, a.seed, e, step);
      }
      classic_obs<ENV>(s, x);
    }

    // ---- bootstrap value, persisted env state ------------------------------
    float v, p0, p1, p2;
    classic_forward<D, NH, P>(lds, m, x, a.activation, v, p0, p1, p2);
    boot[e] = v;
#pragma unroll
    for (int d = 0; d < S; ++d) a.s[(int64_t)e * S + d] = s[d];
#pragma unroll
    for (int d = 0; d < D; ++d) a.x[(int64_t)e * D + d] = x[d];
    a.t[e] = tc;
    a.epr[e] = ep;
  }
  classic_block_moments(a.part, mc, ms, mss, mn, mx);
}

bool f32_cuda(const torch::Tensor& t) {
  return t.is_cuda() && t.is_contiguous() && t.dtype() == torch::kFloat32;
}

// Shared body of the bindings: checks, launch, blob views, moments.
template <int FAM, int ENV>
std::vector<torch::Tensor> classic_run(
    torch::Tensor params, std::vector<int64_t> offsets,
    std::vector<int64_t> dims, int64_t activation, int64_t env_id,
    torch::Tensor s, int64_t time_limit, double act_low, double act_high,
    double eps_explore, torch::Tensor x, torch::Tensor t, torch::Tensor epr,
    int64_t T, int64_t seed, torch::Tensor out_buf) {
  constexpr int S = ClassicEnv<ENV>::S;
  constexpr int D = ClassicEnv<ENV>::D;
  constexpr int P = ClassicEnv<ENV>::P;
  TORCH_CHECK(env_id == ENV,
              FAM == CL_FAM_CAT
                  ? "classic_rollout_cat runs CartPole (env 0), Acrobot "
                    "(env 2) and MountainCar (env 3)"
                  : "classic_rollout_box runs Pendulum (env 1) and "
                    "MountainCarContinuous (env 4)");
  const int nh = static_cast<int>(dims.size()) - 1;
  TORCH_CHECK(nh == 1 || nh == 2,
              "classic rollout supports 1 or 2 hidden layers");
  TORCH_CHECK(dims[0] == D, "dims[0] must be the env's observation width");
  for (int l = 1; l <= nh; ++l)
    TORCH_CHECK(dims[l] >= 1 && dims[l] <= CL_MAX_H,
                "classic rollout supports hidden widths 1..64");
  TORCH_CHECK((int)offsets.size() == 2 * nh + 4,
              "offsets: W, b per hidden layer, then Wv, bv, Wp, bp");
  TORCH_CHECK(f32_cuda(params), "params must be a contiguous f32 GPU tensor");
  const int64_t E = x.size(0);
  TORCH_CHECK(f32_cuda(s) && s.dim() == 2 && s.size(0) == E && s.size(1) == S,
              "s must be [E][S] f32");
  TORCH_CHECK(f32_cuda(x) && x.dim() == 2 && x.size(1) == D,
              "x must be [E][D] f32");
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                  t.dtype() == torch::kInt32 && t.numel() == E,
              "t must be [E] int32");
  TORCH_CHECK(f32_cuda(epr) && epr.numel() == E, "epr must be [E] f32");
  TORCH_CHECK(E >= 1 && E <= (1 << 30) && T >= 1 && T <= (1 << 30) &&
                  time_limit >= 1 && time_limit <= (1 << 30),
              "E, T and time_limit must be in 1..2^30");

  ClassicArgs a;
  a.params = params.data_ptr<float>();
  // every block the kernel reads must lie inside the blob
  const int64_t HL = dims[nh];
  int64_t in = D;
  for (int l = 0; l < nh; ++l) {
    TORCH_CHECK(offsets[2 * l] >= 0 && offsets[2 * l + 1] >= 0 &&
                    offsets[2 * l] + in * dims[l + 1] <= params.numel() &&
                    offsets[2 * l + 1] + dims[l + 1] <= params.numel(),
                "weight blob too small for a hidden layer");
    a.off_w[l] = static_cast<int>(offsets[2 * l]);
    a.off_b[l] = static_cast<int>(offsets[2 * l + 1]);
    a.H[l] = static_cast<int>(dims[l + 1]);
    in = dims[l + 1];
  }
  if (nh == 1) {
    a.off_w[1] = a.off_b[1] = 0;
    a.H[1] = 0;
  }
  const int64_t* ho = offsets.data() + 2 * nh;
  TORCH_CHECK(ho[0] >= 0 && ho[1] >= 0 && ho[2] >= 0 && ho[3] >= 0 &&
                  ho[0] + HL <= params.numel() && ho[1] + 1 <= params.numel() &&
                  ho[2] + P * HL <= params.numel() &&
                  ho[3] + P <= params.numel(),
              "weight blob too small for the value and policy heads");
  a.off_wv = static_cast<int>(ho[0]);
  a.off_bv = static_cast<int>(ho[1]);
  a.off_wp = static_cast<int>(ho[2]);
  a.off_bp = static_cast<int>(ho[3]);
  a.activation = static_cast<int>(activation);
  a.s = s.data_ptr<float>();
  a.x = x.data_ptr<float>();
  a.t = t.data_ptr<int>();
  a.epr = epr.data_ptr<float>();
  a.E = static_cast<int>(E);
  a.T = static_cast<int>(T);
  a.time_limit = static_cast<int>(time_limit);
  a.seed = static_cast<unsigned>(seed);
  a.eps = static_cast<float>(eps_explore);
  a.act_low = static_cast<float>(act_low);
  a.act_high = static_cast<float>(act_high);

  // the out blob layouts of rollout_run_cat (K = P) / rollout_run (A = 1)
  const RolloutBlob blob = rollout_blob(T, E, D, P, 1, FAM == CL_FAM_CAT);
  torch::Tensor out = rollout_blob_tensor(blob, out_buf, x);
  a.out = out.data_ptr<float>();
  const int nblocks = static_cast<int>((E + WAVE - 1) / WAVE);
  auto part = torch::empty({nblocks, 5}, x.options());
  a.part = part.data_ptr<float>();

  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  const dim3 grid(nblocks), block(WAVE);
  if (nh == 1) {
    const size_t lds_bytes =
        classic_lds<1>(D, a.H[0], a.H[1]).total * sizeof(float);
    hipLaunchKernelGGL((classic_rollout_kernel<FAM, ENV, 1>), grid, block,
                       lds_bytes, stream, a);
  } else {
    const size_t lds_bytes =
        classic_lds<2>(D, a.H[0], a.H[1]).total * sizeof(float);
    hipLaunchKernelGGL((classic_rollout_kernel<FAM, ENV, 2>), grid, block,
                       lds_bytes, stream, a);
  }

  auto views = rollout_blob_views(blob, out, FAM == CL_FAM_CAT);
  hipLaunchKernelGGL(classic_moments_kernel, dim3(1), block, 0, stream,
                     a.part, nblocks, views[7].data_ptr<float>());
  return views;
}

}  // namespace

// CartPole under a Discrete(2), or Acrobot or MountainCar under a
// Discrete(3), Categorical policy, chosen by env_id.  Argument order follows rollout_run_cat, with the
// synthetic env's (blob, rank, horizons, noise) replaced by (env_id, s,
// time_limit).
std::vector<torch::Tensor> classic_rollout_cat(
    torch::Tensor params, std::vector<int64_t> offsets,
    std::vector<int64_t> dims, int64_t activation, int64_t env_id,
    torch::Tensor s, int64_t time_limit, double eps_explore, torch::Tensor x,
    torch::Tensor t, torch::Tensor epr, int64_t T, int64_t n_actions,
    int64_t seed, torch::Tensor out_buf) {
  const bool cartpole = env_id == ENV_CARTPOLE && n_actions == 2;
  const bool acrobot = env_id == ENV_ACROBOT && n_actions == 3;
  const bool mountaincar = env_id == ENV_MOUNTAINCAR && n_actions == 3;
  TORCH_CHECK(cartpole || acrobot || mountaincar,
              "classic_rollout_cat supports (env_id, n_actions) = (0, 2) "
              "CartPole, (2, 3) Acrobot and (3, 3) MountainCar; got (", env_id,
              ", ", n_actions, ")");
  if (mountaincar)
    return classic_run<CL_FAM_CAT, ENV_MOUNTAINCAR>(
        params, offsets, dims, activation, env_id, s, time_limit, 0.0, 0.0,
        eps_explore, x, t, epr, T, seed, out_buf);
  if (acrobot)
    return classic_run<CL_FAM_CAT, ENV_ACROBOT>(
        params, offsets, dims, activation, env_id, s, time_limit, 0.0, 0.0,
        eps_explore, x, t, epr, T, seed, out_buf);
  return classic_run<CL_FAM_CAT, ENV_CARTPOLE>(
      params, offsets, dims, activation, env_id, s, time_limit, 0.0, 0.0,
      eps_explore, x, t, epr, T, seed, out_buf);
}

// Pendulum or MountainCarContinuous under a Box(1) / DiagGaussian policy,
// chosen by env_id, after rollout_run.
std::vector<torch::Tensor> classic_rollout_box(
    torch::Tensor params, std::vector<int64_t> offsets,
    std::vector<int64_t> dims, int64_t activation, int64_t env_id,
    torch::Tensor s, int64_t time_limit, double act_low, double act_high,
    double eps_explore, torch::Tensor x, torch::Tensor t, torch::Tensor epr,
    int64_t T, int64_t act_dim, int64_t seed, torch::Tensor out_buf) {
  TORCH_CHECK(act_dim == 1, "classic_rollout_box supports A = 1");
  TORCH_CHECK(env_id == ENV_PENDULUM || env_id == ENV_MOUNTAINCAR_CONT,
              "classic_rollout_box supports env_id 1 Pendulum and 4 "
              "MountainCarContinuous; got ", env_id);
  if (env_id == ENV_MOUNTAINCAR_CONT)
    return classic_run<CL_FAM_BOX, ENV_MOUNTAINCAR_CONT>(
        params, offsets, dims, activation, env_id, s, time_limit, act_low,
        act_high, eps_explore, x, t, epr, T, seed, out_buf);
  return classic_run<CL_FAM_BOX, ENV_PENDULUM>(
      params, offsets, dims, activation, env_id, s, time_limit, act_low,
      act_high, eps_explore, x, t, epr, T, seed, out_buf);
}
