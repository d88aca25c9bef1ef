// MFMA f32 GEMM kernels for the MLP forward / update path and the v3
// rollout's fused env step (gfx950).
//
// gfx950 has exact fp32-input MFMA (v_mfma_f32_32x32x2_f32: bitwise a
// k-ordered fmaf chain, 157 TF chip peak = the f32 vector peak — cdna
// guide §3 "FP32-input MFMA") — ~2.4x a VALU f32 GEMM at identical
// numerics, and an order of magnitude over rocBLAS/Tensile's fp32
// tall-skinny picks on these shapes (<1 TB/s effective measured).
//
//   gemm_fwd:   C[B,N] = act(X[B,K] @ Wt[K,N] + bias) — one hidden layer,
//               fused activation (tanh/relu), activations ARE the saved
//               forward outputs.  X tiles are LDS-staged (the MFMA A
//               fragment is a column read, lane = row); Wt streams from
//               L2 coalesced (reused by every row block).
//   heads mode: same, N = 2A+1, no activation; epilogue splits columns
//               into pdflat[B,2A] and v[B].
//   mlp_fwd_fused: L1 -> L2 -> heads (-> action sampling) of a 64-64
//               policy for one 128-row tile in one launch, on gemm_fwd's
//               glds K loop and epilogue helpers: bitwise the three
//               gemm_fwd calls, without reading h1 / h2 / pdflat back.
//   gemm_env_step: the rollout's G = [XV|a] @ [U;B] GEMM with the env
//               transition as its epilogue (gemm_fwd_glds_kernel<*, true>)
//               + env_finish2_kernel; the per-element math is
//               rollout_math.h's, shared with rollout.hip's split kernels.
//   env_step_rows: the same env step with one block owning all column
//               panels of its rows (env_step_rows_kernel): no reward
//               partials or finish launch, and the next step's x@V comes
//               out of the same launch in gemm_fwd's k order — bitwise
//               gemm_env_step + gemm_fwd.
//   dgrad modes (activation 3/4): C = act'(aux) * (X @ Wt) — the
//               backward chain reuses torch weight layouts directly.
//   dw_mfma:    dW[out,in] += delta^T @ acts, split-K over row blocks
//               into per-split slabs (atomics measured 8.4M adds/launch
//               and dominated), reduced by dw_reduce/db_reduce; fused
//               db += sum(delta); optional row split routes combined
//               [g_pd | g_v] head deltas to Wp/bp and Wv/bv.
//
// Tile-size experiments are in the commit history with measurements:
// MT=2 row fragments and NT>2 column tiles LOSE on these shapes (64-128
// AGPR accumulators drop waves/SIMD; occupancy beats per-wave tile size
// every time it was tried), as did T14 register staging and dual-buffer
// staging — BK=16 single-buffer with 5-6 blocks/CU is the measured
// optimum.
//
// Fragment layout of v_mfma_f32_32x32x2_f32: mfma_frag.h.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "common.h"
#include "mfma_frag.h"
#include "rollout_math.h"

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int BK = 16;        // K-step per stage
constexpr int M_WAVE = 32;    // rows per wave tile
constexpr int FWD_WAVES = 4;  // waves per block (each owns 32 rows)
constexpr int FWD_M = FWD_WAVES * M_WAVE;  // 128 rows per block
constexpr int MAX_NT = 4;     // 32-col accumulator tiles per wave

// ---------------------------------------------------------------------------
// Forward layer: C = act(X @ Wt + b).  heads_mode splits the epilogue.
// ---------------------------------------------------------------------------

struct FwdArgs {
  const float* X;     // [B][K]
  const float* Wt;    // [K][N] (wt_layout 0) or [N][K] torch layout (1)
  const float* bias;  // [N]
  const float* aux;   // [B][N] forward activations (dgrad modes)
  float* C;           // [B][N]      (heads: pdflat [B][N-1])
  float* v;           // [B] heads only
  int64_t B;
  int K, N;
  int activation;     // 0 relu, 1 tanh, 2 none;
                      // 3 tanh-grad: C = (1-aux^2)*acc (no bias)
                      // 4 relu-grad: C = (aux>0)*acc   (no bias)
  int heads;          // if 1: last column -> v, rest -> C (pdflat)
  int wt_layout;      // 0: Wt[K][N]; 1: torch W[N][K] (staged transposed)
  int ldc;            // C row stride (>= N; heads: >= N-1) — lets C land
                      // in a column block of a wider buffer
  int ablate;         // perf diagnosis only (wrong results when nonzero):
                      // 1 skip X stage, 2 skip W stage, 4 skip MFMA,
                      // 8 skip epilogue stores
  // activation 5 (fused env step, v3 rollout; gemm_fwd_glds_kernel's ENV
  // instantiation): the G = [XV|a] @ [U;B] GEMM's epilogue computes the
  // env transition directly — pred = tanh(x*d + acc + sigma*noise),
  // out = done ? fresh : pred — writing the next recorded state and
  // per-(panel, env) pred^2 partials for the reward.  The accumulators
  // are repacked through LDS into env_finish_kernel's float4-per-lane
  // layout, so the per-element work, RNG slots and results are that
  // kernel's; the [E][D] G write + read never happen.  With env_xvp set
  // the block also multiplies its finished next-state tile by its rows
  // of V (the next step's x@V, per-panel partials).
  const float* env_xin;     // [E][D] state at `step`
  float* env_x;             // [E][D] out: state at `step`+1 (the v3 loop
                            // passes the states-blob slot directly; may
                            // alias env_xin)
  const float* envd;        // [D]
  const int* horizons;      // [E]
  const int* tcount;        // [E] (read; env_finish2 increments)
  const long long* seed_dev;
  float* env_rsum;          // [npanels][E] per-panel pred^2 partials
                            // (plain stores — deterministic, no zeroing)
  const float* env_V;       // [D][16] x@V fold operand (null: no fold)
  float* env_xvp;           // [npanels][E][16] next-state @ V partials
  float sigma;
  int step;
};

// bias + activation of one accumulator element (layer modes 0 relu,
// 1 tanh, 2 none)
DEV_INLINE float fwd_bias_act(float acc, float bv, int activation) {
  float x = acc + bv;
  if (activation == 0) x = fmaxf(x, 0.f);
  else if (activation == 1) x = fast_tanhf(x);
  return x;
}

// one output element by heads mode: 2 = padded heads (N includes pad
// columns so N%4==0 shapes can take the glds kernel; v at column N-2,
// columns >= N-1 are the zero-weight pad, discarded), 1 = v at N-1
DEV_INLINE void fwd_store(float* C, float* v, int heads, int N, int ldc,
                          int64_t row, int col, float x) {
  if (heads == 2) {
    if (col == N - 2) v[row] = x;
    else if (col < N - 2) C[row * ldc + col] = x;
  } else if (heads) {
    if (col == N - 1) v[row] = x;
    else C[row * ldc + col] = x;
  } else {
    C[row * ldc + col] = x;
  }
}

// Layer epilogue of one wave's [32 rows][NT*32 cols] accumulator tile at
// (b0 + 32*wave, n0): bias + activation, or act'(aux) * acc in the dgrad
// modes, then the heads-mode store.  Shared by the plain and glds kernels;
// the pipe kernel keeps the same code written out (see there).
template <int NT>
DEV_INLINE void fwd_epilogue(const FwdArgs& a, const f32x16 (&acc)[NT],
                             int64_t b0, int n0, int wave, int lane) {
  #pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = n0 + t * M_WAVE + (lane & 31);
    if (col < a.N) {
      const float bv = (a.activation >= 3) ? 0.f : a.bias[col];
      #pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int64_t row = b0 + wave * M_WAVE + cd_row(r, lane);
        if (row < a.B) {
          float x;
          if (a.activation >= 3) {
            const float h = a.aux[row * a.N + col];
            x = acc[t][r] * act_grad(h, a.activation == 3);
          } else {
            x = fwd_bias_act(acc[t][r], bv, a.activation);
          }
          fwd_store(a.C, a.v, a.heads, a.N, a.ldc, row, col, x);
        }
      }
    }
  }
}

template <int NT>
__launch_bounds__(FWD_WAVES * 64)
__global__ void gemm_fwd_kernel(FwdArgs a) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;

  // X tile [FWD_M][BK] (+1 pad: the A-fragment read is a column read);
  // Wt tile [BK][NT*32] staged coalesced so the MFMA B-operand comes
  // from LDS instead of a fresh L2 round trip per k-step.
  __shared__ float xs[FWD_M][BK + 1];
  __shared__ float ws[BK][NT * M_WAVE];

  const int i_l = lane & 31;   // A row within wave tile
  const int k_l = lane >> 5;   // A k within pair
  const int NW = NT * M_WAVE;

  for (int64_t tile = blockIdx.x; tile * FWD_M < a.B; tile += gridDim.x) {
    const int64_t b0 = tile * FWD_M;
    f32x16 acc[NT];
    #pragma unroll
    for (int t = 0; t < NT; ++t)
      #pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    for (int kb = 0; kb < a.K; kb += BK) {
      __syncthreads();
      // float4 staging (scalar element staging measured as the dominant
      // per-call cost: 32 scalar dword loads per thread per stage)
      constexpr int BK4 = BK / 4;
      if (!(a.ablate & 1))
      for (int idx = threadIdx.x; idx < FWD_M * BK4; idx += FWD_WAVES * 64) {
        const int r = idx / BK4, c4 = (idx % BK4) * 4;
        const int64_t row = b0 + r;
        const int col = kb + c4;
        float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < a.B) {
          if (col + 3 < a.K) {
            val = *reinterpret_cast<const float4*>(&a.X[row * a.K + col]);
          } else {
            float tmp[4] = {0.f, 0.f, 0.f, 0.f};
            for (int q = 0; q < 4; ++q)
              if (col + q < a.K) tmp[q] = a.X[row * a.K + col + q];
            val = make_float4(tmp[0], tmp[1], tmp[2], tmp[3]);
          }
        }
        xs[r][c4] = val.x;
        xs[r][c4 + 1] = val.y;
        xs[r][c4 + 2] = val.z;
        xs[r][c4 + 3] = val.w;
      }
      if (a.ablate & 2) {
        // skip W stage
      } else if (a.wt_layout == 0) {
        const int NW4 = NW / 4;
        for (int idx = threadIdx.x; idx < BK * NW4; idx += FWD_WAVES * 64) {
          const int r = idx / NW4, c4 = (idx % NW4) * 4;
          const int krow = kb + r;
          float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
          if (krow < a.K) {
            if (c4 + 3 < a.N) {
              val = *reinterpret_cast<const float4*>(
                  &a.Wt[(int64_t)krow * a.N + c4]);
            } else {
              float tmp[4] = {0.f, 0.f, 0.f, 0.f};
              for (int q = 0; q < 4; ++q)
                if (c4 + q < a.N) tmp[q] = a.Wt[(int64_t)krow * a.N + c4 + q];
              val = make_float4(tmp[0], tmp[1], tmp[2], tmp[3]);
            }
          }
          *reinterpret_cast<float4*>(&ws[r][c4]) = val;
        }
      } else {
        // torch W[N][K]: c-major mapping keeps the row-segment reads
        // coalesced and transposes into ws on the fly — no host-side
        // W.t().contiguous() per update step
        constexpr int BK4 = BK / 4;
        for (int idx = threadIdx.x; idx < NW * BK4; idx += FWD_WAVES * 64) {
          const int c = idx / BK4, r4 = (idx % BK4) * 4;
          const int krow = kb + r4;
          float4 val = make_float4(0.f, 0.f, 0.f, 0.f);
          if (c < a.N) {
            if (krow + 3 < a.K) {
              val = *reinterpret_cast<const float4*>(
                  &a.Wt[(int64_t)c * a.K + krow]);
            } else {
              float tmp[4] = {0.f, 0.f, 0.f, 0.f};
              for (int q = 0; q < 4; ++q)
                if (krow + q < a.K) tmp[q] = a.Wt[(int64_t)c * a.K + krow + q];
              val = make_float4(tmp[0], tmp[1], tmp[2], tmp[3]);
            }
          }
          ws[r4][c] = val.x;
          ws[r4 + 1][c] = val.y;
          ws[r4 + 2][c] = val.z;
          ws[r4 + 3][c] = val.w;
        }
      }
      __syncthreads();

      const int ksteps = (a.ablate & 4) ? 0 : min(BK, a.K - kb);
      #pragma unroll 4
      for (int k2 = 0; k2 < ksteps; k2 += 2) {
        const float av = xs[wave * M_WAVE + i_l][k2 + k_l];
        #pragma unroll
        for (int t = 0; t < NT; ++t) {
          const float bv = ws[k2 + k_l][t * M_WAVE + i_l];
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
        }
      }
    }

    if (!(a.ablate & 8)) fwd_epilogue<NT>(a, acc, b0, 0, wave, lane);
  }
}

// ---------------------------------------------------------------------------
// Pipelined forward (T14 register staging, cdna guide "write tile t+1 AFTER
// the barrier"): the runtime-ablation split measured the plain kernel's
// stage / MFMA / epilogue phases strictly ADDITIVE (L1 886 us = 420 + 321
// + 145; profiles/r01_gemm_ablation.txt) — no cross-phase overlap at 4
// waves/SIMD.  Here each stage issues the NEXT tile's global loads into
// registers before the barrier (plain loads survive s_barrier; guide §5),
// so HBM latency hides under the current stage's MFMAs.
//
// Loads are BRANCHLESS (clamped addresses, whole-float4 validity, zero-fix
// by select at LDS-write time — NO global access in the write phase): a
// per-element guard branch or a write-time refetch makes hipcc emit
// load;s_waitcnt vmcnt(0);ds_write per ELEMENT and serializes the whole
// pipeline (first attempt measured 1.7x SLOWER than the plain kernel).
// Whole-float4 validity requires K%4==0 (and N%4==0 for wt_layout 0);
// other shapes take the plain kernel (host dispatch).
// ---------------------------------------------------------------------------

// NT<=2 (every shape this model family hits): force the allocation to 128
// VGPRs = 4 waves/SIMD — the un-hinted build lands at 132 and loses a
// whole wave to 4 registers.  NT>=3 would spill catastrophically; leave it.
template <int NT, int PBK>
__launch_bounds__(FWD_WAVES * 64, (NT <= 2 && PBK == 16) ? 4 : 1)
__global__ void gemm_fwd_pipe_kernel(FwdArgs a) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;

  // PBK: K-step per stage.  32 gives the prefetch twice the MFMA cycles
  // to hide under but costs 177 VGPR (2 waves/SIMD); 16 keeps 4
  // waves/SIMD.  Both instantiated; dispatch measures/chooses per shape.
  // X rows padded +4 (not +1): a 17-float row stride leaves the float4
  // staging writes 16B-MISALIGNED, so hipcc splits them into scalar
  // ds_writes (PMC: 5.7e8 bank-conflict cycles on 3.2e8 LDS ops).  +4
  // keeps b128 writes; the A-fragment column reads pick up a 4-way bank
  // conflict but there are only 8 of them per wave-stage.
  __shared__ float xs[FWD_M][PBK + 4];
  __shared__ float ws[PBK][NT * M_WAVE];

  const int i_l = lane & 31;
  const int k_l = lane >> 5;
  constexpr int NW = NT * M_WAVE;
  constexpr int PBK4 = PBK / 4;
  constexpr int XIT = (FWD_M * PBK4 + FWD_WAVES * 64 - 1) / (FWD_WAVES * 64);
  constexpr int WIT = (PBK * NW / 4 + FWD_WAVES * 64 - 1) / (FWD_WAVES * 64);
  constexpr int W_ITEMS = PBK * NW / 4;  // float4 slots in the W tile
  // column panel (grid.y): this block computes columns [n0, n0+NW) of N —
  // wide-N GEMMs (the env-dynamics [E][36] @ [36][D] call) run as panels
  const int n0 = blockIdx.y * NW;

  float4 xreg[XIT];
  float4 wreg[WIT];

  // ---- branchless load issue for one k-stage (clamped addresses) ----
  auto issue_x = [&](int64_t b0, int kb) {
    #pragma unroll
    for (int it = 0; it < XIT; ++it) {
      const int idx = threadIdx.x + it * FWD_WAVES * 64;
      const int r = idx / PBK4, c4 = (idx % PBK4) * 4;
      int64_t row = b0 + r;
      row = row < a.B ? row : a.B - 1;
      int col = kb + c4;
      col = col < a.K ? col : a.K - 4;   // K%4==0: col<K => col+3<K
      xreg[it] = *reinterpret_cast<const float4*>(&a.X[row * a.K + col]);
    }
  };
  auto issue_w = [&](int kb) {
    if (a.wt_layout == 0) {
      constexpr int NW4 = NW / 4;
      #pragma unroll
      for (int it = 0; it < WIT; ++it) {
        const int idx = threadIdx.x + it * FWD_WAVES * 64;
        if (idx >= W_ITEMS) break;
        const int r = idx / NW4, c4 = (idx % NW4) * 4;
        int krow = kb + r;
        krow = krow < a.K ? krow : a.K - 1;
        const int c = n0 + c4 < a.N ? n0 + c4 : a.N - 4;  // N%4==0
        wreg[it] = *reinterpret_cast<const float4*>(&a.Wt[(int64_t)krow * a.N + c]);
      }
    } else {
      #pragma unroll
      for (int it = 0; it < WIT; ++it) {
        const int idx = threadIdx.x + it * FWD_WAVES * 64;
        if (idx >= W_ITEMS) break;
        const int c0 = idx / PBK4, r4 = (idx % PBK4) * 4;
        const int c = n0 + c0 < a.N ? n0 + c0 : a.N - 1;
        int krow = kb + r4;
        krow = krow < a.K ? krow : a.K - 4;  // K%4==0
        wreg[it] = *reinterpret_cast<const float4*>(&a.Wt[(int64_t)c * a.K + krow]);
      }
    }
  };
  // ---- LDS write of the staged registers (selects only, no loads) ----
  auto write_x = [&](int64_t b0, int kb) {
    #pragma unroll
    for (int it = 0; it < XIT; ++it) {
      const int idx = threadIdx.x + it * FWD_WAVES * 64;
      const int r = idx / PBK4, c4 = (idx % PBK4) * 4;
      const bool ok = (b0 + r < a.B) & (kb + c4 < a.K);
      const float* v = reinterpret_cast<const float*>(&xreg[it]);
      #pragma unroll
      for (int q = 0; q < 4; ++q) xs[r][c4 + q] = ok ? v[q] : 0.f;
    }
  };
  auto write_w = [&](int kb) {
    if (a.wt_layout == 0) {
      constexpr int NW4 = NW / 4;
      #pragma unroll
      for (int it = 0; it < WIT; ++it) {
        const int idx = threadIdx.x + it * FWD_WAVES * 64;
        if (idx >= W_ITEMS) break;
        const int r = idx / NW4, c4 = (idx % NW4) * 4;
        const bool ok = (kb + r < a.K) & (n0 + c4 < a.N);
        const float* v = reinterpret_cast<const float*>(&wreg[it]);
        #pragma unroll
        for (int q = 0; q < 4; ++q) ws[r][c4 + q] = ok ? v[q] : 0.f;
      }
    } else {
      #pragma unroll
      for (int it = 0; it < WIT; ++it) {
        const int idx = threadIdx.x + it * FWD_WAVES * 64;
        if (idx >= W_ITEMS) break;
        const int c0 = idx / PBK4, r4 = (idx % PBK4) * 4;  // c0 < NW always
        const bool cok = n0 + c0 < a.N;
        const bool kok = kb + r4 < a.K;  // K%4==0: whole-float4 validity
        const float* v = reinterpret_cast<const float*>(&wreg[it]);
        #pragma unroll
        for (int q = 0; q < 4; ++q)
          ws[r4 + q][c0] = (cok & kok) ? v[q] : 0.f;
      }
    }
  };

  // One TILE per block (host launches grid == tile count): tile-boundary
  // cold starts are hidden by BLOCK scheduling — a freshly placed block's
  // prologue loads overlap the other resident blocks' MFMA phases — which
  // costs zero registers, where an explicit cross-tile prefetch kept
  // xreg/wreg live across the epilogue and measured +29 VGPR (137: 3
  // waves/SIMD) and gave the occupancy back.
  for (int64_t tile = blockIdx.x; tile * FWD_M < a.B; tile += gridDim.x) {
    const int64_t b0 = tile * FWD_M;
    f32x16 acc[NT];
    #pragma unroll
    for (int t = 0; t < NT; ++t)
      #pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    issue_x(b0, 0);
    issue_w(0);
    for (int kb = 0; kb < a.K; kb += PBK) {
      write_x(b0, kb);
      write_w(kb);
      if (kb + PBK < a.K) {  // prefetch the NEXT stage before the barrier
        issue_x(b0, kb + PBK);
        issue_w(kb + PBK);
      }
      __syncthreads();

      const int ksteps = min(PBK, a.K - kb);
      #pragma unroll 4
      for (int k2 = 0; k2 < ksteps; k2 += 2) {
        const float av = xs[wave * M_WAVE + i_l][k2 + k_l];
        #pragma unroll
        for (int t = 0; t < NT; ++t) {
          const float bv = ws[k2 + k_l][t * M_WAVE + i_l];
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
        }
      }
      __syncthreads();
    }

    // fwd_epilogue<NT>, kept written out: folded in, <2,16> measured slower
    // on the L1 shape (profiles/r08_device_dedup.txt)
    #pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int col = n0 + t * M_WAVE + i_l;
      if (col < a.N) {
        const float bv = (a.activation >= 3) ? 0.f : a.bias[col];
        #pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int64_t row = b0 + wave * M_WAVE + cd_row(r, lane);
          if (row < a.B) {
            float x;
            if (a.activation >= 3) {
              const float h = a.aux[row * a.N + col];
              x = acc[t][r] * ((a.activation == 3) ? (1.f - h * h)
                                                   : (h > 0.f ? 1.f : 0.f));
            } else {
              x = acc[t][r] + bv;
              if (a.activation == 0) x = fmaxf(x, 0.f);
              else if (a.activation == 1) x = fast_tanhf(x);
            }
            if (a.heads == 2) {
              if (col == a.N - 2) a.v[row] = x;
              else if (col < a.N - 2) a.C[row * a.ldc + col] = x;
            } else if (a.heads) {
              if (col == a.N - 1) a.v[row] = x;
              else a.C[row * a.ldc + col] = x;
            } else {
              a.C[row * a.ldc + col] = x;
            }
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// glds 3-buffer streaming forward (round-2 lever #1, profiles/
// r01_final_v3_69M.txt): the register-staged pipe kernel measured 2.5
// TB/s effective on the tall-skinny update GEMMs vs ~6 TB/s streaming
// capability — its per-stage issue->vmcnt(0)-at-write->ds_write chain
// plus two __syncthreads serialize the stream.  Here the X/W tiles go
// straight to LDS by global_load_lds into a 3-deep ring with COUNTED
// vmcnt across raw barriers (guide §5 "3-buf span +83%"), so two stages
// stay in flight while one computes and the wave stream carries only
// MFMAs + fragment reads.
//
// Shape contract: NT==2 (one W piece per thread keeps the vmcnt count
// wave-uniform), wt_layout 0.  K tails (K % 16 != 0) are handled by
// clamped sources + zeroing the ws rows >= K before the last stage's
// MFMAs (garbage X columns then multiply zero W rows).  The xs image is
// UNPADDED [128][16] (glds needs a lane-linear dest); the 4-way
// A-column bank spread that the pipe kernel's +4 row pad bought is kept
// by XOR-swizzling the float4 piece index with row bits on the SOURCE
// address (guide rule 21) — same 64 B cacheline, zero coalescing cost.
// ---------------------------------------------------------------------------

constexpr int GLDS_NT = 2;
constexpr int GLDS_BK = 16;
constexpr int GLDS_NW = GLDS_NT * M_WAVE;        // 64
constexpr int GLDS_XB = FWD_M * GLDS_BK * 4;     // 8192 B
constexpr int GLDS_WB = GLDS_BK * GLDS_NW * 4;   // 4096 B
constexpr int GLDS_SLOT = GLDS_XB + GLDS_WB;

// The streaming K loop of one [128 rows][64 cols] tile: stage ring, K tail
// and per-block K-phase rotation.  Shared by gemm_fwd_glds_kernel and the
// fused policy forward, so both run the same MFMA chain.  Returns with
// every glds landed and the block past a barrier: acc is live and the ring
// (smem, RING * GLDS_SLOT bytes) is dead.
template <int RING>
DEV_INLINE void glds_fwd_mainloop(const FwdArgs& a, char* smem, int64_t b0,
                                  int n0, f32x16 (&acc)[GLDS_NT]) {
  constexpr int NT = GLDS_NT;
  constexpr int PBK = GLDS_BK;
  constexpr int NW = GLDS_NW;
  constexpr int XB = GLDS_XB;
  constexpr int SLOT = GLDS_SLOT;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = tid / WAVE;
  const int i_l = lane & 31;
  const int k_l = lane >> 5;

  // per-thread glds sources (constant; advance by kb each stage)
  // X: two 16-B pieces per thread; dest piece q = tid + p*256 ->
  // row = q/4, c4 = (q%4) with the source float4 swizzled by row bits
  const float* srcX[2];
  int xcol[2];
  int64_t xrow[2];
  #pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int q = tid + p * FWD_WAVES * 64;
    const int r = q >> 2;
    const int c4 = (q & 3) ^ (r & 3);  // source-side st swizzle
    int64_t row = b0 + r;
    row = row < a.B ? row : a.B - 1;
    xrow[p] = row;
    xcol[p] = c4 * 4;
    srcX[p] = a.X + row * a.K;
  }
  // W: one 16-B piece per thread; dest q = tid -> k = q/(NW/4), c4 = q%(NW/4)
  const int wk = tid / (NW / 4);
  int wc4 = (tid % (NW / 4)) * 4;
  {
    int c = n0 + wc4;
    c = c + 3 < a.N ? c : a.N - 4;  // clamped (garbage cols discarded)
    wc4 = c;
  }

  // per-block K-phase rotation: co-resident blocks otherwise hit their
  // stage barriers in lockstep (PMC: MFMA pipe 51% busy, 34% of wave
  // time parked on vmcnt/barrier) — rotating the stage order by
  // blockIdx desynchronizes the convoy at unchanged traffic.  fp32
  // accumulation order changes per block (still deterministic per
  // shape; numerics tests compare against eager to tolerance).
  const int S_ = (a.K + PBK - 1) / PBK;
  const int phase = (int)(blockIdx.x % (unsigned)S_);
  auto smap = [&](int s) {
    const int t = s + phase;
    return t >= S_ ? t - S_ : t;
  };
  auto issue = [&](int s) {
    const int kb = smap(s) * PBK;
    char* slot = smem + (s % RING) * SLOT;
    #pragma unroll
    for (int p = 0; p < 2; ++p) {
      int col = kb + xcol[p];
      col = col + 3 < a.K ? col : a.K - 4;  // clamp; tail fixed via ws zeros
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned*)(srcX[p] + col),
          (unsigned*)(slot + p * 4096 + wave * 1024), 16, 0, 0);
    }
    int krow = kb + wk;
    krow = krow < a.K ? krow : a.K - 1;
    __builtin_amdgcn_global_load_lds(
        (const __attribute__((address_space(1))) unsigned*)(
            a.Wt + (int64_t)krow * a.N + wc4),
        (unsigned*)(slot + XB + wave * 1024), 16, 0, 0);
  };

  const int S = (a.K + PBK - 1) / PBK;
  #pragma unroll
  for (int p = 0; p < RING - 1; ++p)
    if (p < S) issue(p);

  #pragma unroll
  for (int t = 0; t < NT; ++t)
    #pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  for (int s = 0; s < S; ++s) {
    // stage s landed when only the later in-flight stages' glds (3 each)
    // remain outstanding: rem = how many stages beyond s are in flight
    const int rem = min(S - 1 - s, RING - 2);
    if (rem >= RING - 2)
      asm volatile("s_waitcnt vmcnt(%0)" ::"i"(3 * (RING - 2)) : "memory");
    else if (RING == 4 && rem == 1)
      asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    char* slot = smem + (s % RING) * SLOT;
    float* xs = (float*)slot;
    float* ws = (float*)(slot + XB);
    const int kb = smap(s) * PBK;
    if (kb + PBK > a.K) {
      // zero the W rows past K so the clamped/garbage X columns of the
      // tail stage contribute nothing
      for (int idx = tid; idx < (kb + PBK - a.K) * NW; idx += FWD_WAVES * 64)
        ws[(a.K - kb) * NW + idx] = 0.f;
      __builtin_amdgcn_s_barrier();
    }
    // buf (s+RING-1)%RING == (s-1)%RING, freed by the barrier above
    if (s + RING - 1 < S) issue(s + RING - 1);
    #pragma unroll 4
    for (int k2 = 0; k2 < PBK; k2 += 2) {
      const int k = k2 + k_l;
      const int row = wave * M_WAVE + i_l;
      const float av = xs[row * PBK + (((k >> 2) ^ (row & 3)) << 2) + (k & 3)];
      #pragma unroll
      for (int t = 0; t < NT; ++t) {
        const float bv = ws[k * NW + t * M_WAVE + i_l];
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
}

// ---- fused env-step epilogue pieces ---------------------------------------
// Shared by gemm_fwd_glds_kernel<*, true> (one block per panel) and
// env_step_rows_kernel (one block per row tile, all panels); the image
// layout and its bank arithmetic are described in the former.
constexpr int ENV_HR = 16;  // rows per wave per repack pass

// pass h of a wave's accumulators (registers 8h..8h+7 of both column tiles
// = rows 16h..16h+15) -> its [16][64] XOR-swizzled LDS image
DEV_INLINE void env_tile_dump(float* tile, const f32x16 (&acc)[GLDS_NT],
                              int h, int lane) {
  // opaque copy of the lane id: without it the 16 dump addresses of
  // pass 0 are kept live for pass 1 and the allocator spills them
  // (80-VGPR budget at 6 blocks/CU); recomputing costs one XOR each
  int ln = lane;
  asm volatile("" : "+v"(ln));
  #pragma unroll
  for (int t = 0; t < GLDS_NT; ++t) {
    #pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int lr = cd_row(8 * h + q, ln) - ENV_HR * h;
      const int cc = t * M_WAVE + (ln & 31);
      tile[lr * GLDS_NW + ((((cc >> 2) ^ lr) << 2) | (cc & 3))] =
          acc[t][8 * h + q];
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// One float4 (dims d..d+3 of env e, G in *slot) of the env transition:
// v = the state written to env_x (fresh if the env is done; zeros where
// !ok), ss = the whole 64-column panel's pred^2 of that row, summed over
// its 16 lanes in the shared order (rollout_math.h).  PRE_DONE: the caller
// read the row's done flag once; otherwise it is read here.
template <bool PRE_DONE>
DEV_INLINE void env_tile_f4(const FwdArgs& a, const float4* slot, int64_t e,
                            int d, int c, bool ok, unsigned seed, float sigma,
                            int step, const float4& dv, int pre_done,
                            float4& v, float& ss) {
  v = make_float4(0.f, 0.f, 0.f, 0.f);
  ss = 0.f;
  if (ok) {
    const float4 gv = *slot;
    const float4 xv =
        *reinterpret_cast<const float4*>(&a.env_xin[e * a.N + d]);
    float nz[4] = {0.f, 0.f, 0.f, 0.f};
    if (sigma != 0.f) {
      const float2 p0 = env_noise_pair(seed, (int)e, step, c, 0);
      const float2 p1 = env_noise_pair(seed, (int)e, step, c, 1);
      nz[0] = p0.x; nz[1] = p0.y; nz[2] = p1.x; nz[3] = p1.y;
    }
    v.x = env_pred(xv.x, dv.x, gv.x, sigma, nz[0]);
    v.y = env_pred(xv.y, dv.y, gv.y, sigma, nz[1]);
    v.z = env_pred(xv.z, dv.z, gv.z, sigma, nz[2]);
    v.w = env_pred(xv.w, dv.w, gv.w, sigma, nz[3]);
    ss = sq4(v);
    int done;
    if constexpr (PRE_DONE) done = pre_done;
    else done = a.tcount[e] + 1 >= a.horizons[e] ? 1 : 0;
    if (done) {
      v.x = env_reset(seed, (int)e, step, d);
      v.y = env_reset(seed, (int)e, step, d + 1);
      v.z = env_reset(seed, (int)e, step, d + 2);
      v.w = env_reset(seed, (int)e, step, d + 3);
    }
    *reinterpret_cast<float4*>(&a.env_x[e * a.N + d]) = v;
  }
  // the 16 lanes of a row hold the whole panel's pred^2
  #pragma unroll
  for (int off = 8; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 16);
}

template <int RING,   // ring depth: 2 (24 KB, 6 blocks/CU — overlap via
                      // MORE co-resident blocks), 3 (36 KB, 4 blocks/CU,
                      // default), 4 (48 KB, 3 blocks/CU — deeper
                      // in-flight staging; measured slower)
          bool ENV = false>  // fused env-step epilogue (activation 5) — its
                             // own instantiation, so the layer GEMMs'
                             // registers and occupancy do not see it
__launch_bounds__(FWD_WAVES * 64, RING == 2 ? 6 : RING == 3 ? 4 : 3)
__global__ void gemm_fwd_glds_kernel(FwdArgs a) {
  constexpr int NT = GLDS_NT;
  constexpr int NW = GLDS_NW;
  constexpr int SLOT = GLDS_SLOT;
  __shared__ __attribute__((aligned(16))) char smem[RING * SLOT];
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = tid / WAVE;
  const int i_l = lane & 31;
  const int n0 = blockIdx.y * NW;

  const int64_t b0 = (int64_t)blockIdx.x * FWD_M;
  if (b0 >= a.B) return;

  f32x16 acc[NT];
  glds_fwd_mainloop<RING>(a, smem, b0, n0, acc);

  if constexpr (ENV) {
    // Fused env step.  The accumulator layout (lane = column) would make
    // every element pay a whole Box-Muller pair and move x/d/x' as 4-B
    // scalars, so the tile is repacked through the (now dead) ring LDS
    // into env_finish_kernel's layout: one float4 = 4 consecutive dims of
    // one row per lane, two noise pairs per float4, b128 global traffic.
    //
    // Each wave repacks its own 32 rows in two passes of 16 rows x 64
    // cols (accumulator registers 8h..8h+7 of both column tiles are rows
    // 16h..16h+15), 4 KB per wave and 16 KB per block — inside the 24 KB
    // of the 2-deep ring, and no block barrier: a wave only ever touches
    // its own image, and its LDS operations complete in order.
    //
    // Image: row stride 64 floats (one 256-B bank row), float4 slot s of
    // row i stored at slot s ^ i.
    //   - ds_write_b32 of one accumulator register: a 32-lane half writes
    //     32 consecutive columns of one row; the XOR permutes whole
    //     16-B slots inside the row, so the 32 dwords stay on 32 distinct
    //     banks (mod 32).
    //   - ds_read_b128, lane l -> (row 4j + l/16, slot l%16): each of the
    //     instruction's 16-lane groups ({0-3,12-15,20-27}, ...) takes 8
    //     slots of one row and the complementary 8 of the next; rows i
    //     and i^1 XOR them with values that differ in bit 0 only, which
    //     maps the two 8-slot sets onto disjoint slots — all 64 banks
    //     once.
    //   - the fold's A fragments (below) read b128 at (row l%16, slot
    //     (4q + l/16) ^ row): per 16-lane group the 16 (row, slot) pairs
    //     land on 16 distinct slots, again conflict-free.  An unswizzled
    //     image would put all 16 rows of a column on one bank.
    constexpr int HR = ENV_HR;
    static_assert(RING * SLOT >= FWD_WAVES * HR * NW * 4 + NW * 16 * 4,
                  "env epilogue image + V panel must fit the ring");
    float* tile = reinterpret_cast<float*>(smem) + wave * (HR * NW);
    float* vs = reinterpret_cast<float*>(smem) + FWD_WAVES * HR * NW;
    const bool fold = a.env_xvp != nullptr;
    if (fold) {
      // this panel's rows of V ([64][16], pad rows zero) -> LDS, one
      // float4 per thread.  Rows 4..7 of every 8 swap with their odd/even
      // neighbour: the B fragment's two lane groups of a 32-lane half
      // read rows k and k+4, 64 floats apart = the same 32-bank window.
      const int kl = tid >> 2;
      const int kr = n0 + kl;
      float4 vv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (kr < a.N)
        vv = *reinterpret_cast<const float4*>(
            &a.env_V[(int64_t)kr * 16 + 4 * (tid & 3)]);
      *reinterpret_cast<float4*>(
          &vs[(kl ^ ((kl >> 2) & 1)) * 16 + 4 * (tid & 3)]) = vv;
      __syncthreads();
    }
    const unsigned seed = (unsigned)(*a.seed_dev);
    const float sigma = a.sigma;
    const int step = a.step;
    const int c4 = lane & 15;   // float4 slot inside the 64-col panel
    const int rsub = lane >> 4;
    const int d = n0 + 4 * c4;  // first of this lane's 4 dims
    const int c = d >> 2;       // env_finish_kernel's float4 chunk index
    const bool cok = d < a.N;   // N%4==0: a float4 is all in or all out
    float4 dv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cok) dv = *reinterpret_cast<const float4*>(&a.envd[d]);
    #pragma unroll
    for (int h = 0; h < 2; ++h) {
      env_tile_dump(tile, acc, h, lane);
      #pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int lr = 4 * j + rsub;
        const int64_t e = b0 + wave * M_WAVE + HR * h + lr;
        const bool rok = e < a.B;
        float4* slot =
            reinterpret_cast<float4*>(&tile[lr * NW + ((c4 ^ lr) << 2)]);
        float4 v;
        float ss;
        env_tile_f4<false>(a, slot, e, d, c, rok && cok, seed, sigma, step, dv,
                           0, v, ss);
        // one plain store per (panel, row) keeps the reward deterministic,
        // in the shared sum order (rollout_math.h)
        if (c4 == 0 && rok) a.env_rsum[(int64_t)blockIdx.y * a.B + e] = ss;
        // fold operand: the state actually written (reset rows included),
        // zeros in pad columns and rows
        if (fold) *slot = v;
      }
      if (fold) {
        // x@V fold: [16 rows][64 cols] (LDS) @ V[64][16] on the exact-f32
        // 16x16x4 MFMA.  The k order inside the sum is free as long as A
        // and B agree: lane group g = l/16 reads the float4 slot 4q+g and
        // MFMA (q, m) takes component m of it, i.e. column 4*(4q+g)+m.
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        const int fi = lane & 15;
        f32x4 xa = {0.f, 0.f, 0.f, 0.f};
        #pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 av = *reinterpret_cast<const float4*>(
              &tile[fi * NW + (((4 * q + rsub) ^ fi) << 2)]);
          const float am[4] = {av.x, av.y, av.z, av.w};
          #pragma unroll
          for (int m = 0; m < 4; ++m) {
            const int k = 4 * (4 * q + rsub) + m;
            const float bv = vs[(k ^ ((k >> 2) & 1)) * 16 + fi];
            xa = __builtin_amdgcn_mfma_f32_16x16x4f32(am[m], bv, xa, 0, 0, 0);
          }
        }
        // D reg r: row 4*(l/16) + r, col l%16
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t e = b0 + wave * M_WAVE + HR * h + 4 * rsub + r;
          if (e < a.B)
            a.env_xvp[((int64_t)blockIdx.y * a.B + e) * 16 + fi] = xa[r];
        }
      }
    }
    return;
  }

  fwd_epilogue<NT>(a, acc, b0, n0, wave, lane);
}

// ---------------------------------------------------------------------------
// Row-owning env step: one block per 128-row tile runs ALL column panels of
// the G = [XV|a] @ [U;B] GEMM in ascending order, each with
// gemm_fwd_glds_kernel<2, true>'s K loop (same phase: the row-tile index)
// and env epilogue pieces, so states are bitwise that kernel's.  Owning
// every panel of its rows, the block needs no cross-block partials:
//   - reward: instead of storing the per-(panel, row) pred^2 sum to rsum, a
//     lane of the row keeps a running sum, ss = 0; ss += partial_p, p ascending
//     — env_finish2_kernel's order — and calls episode_step() for its row
//     after the last panel.  No rsum buffer, no finish launch.
//   - next step's x@V: the finished x' float4s go back into the wave's
//     image and extend ONE accumulator per 16-row pass on the exact-f32
//     16x16x4 MFMA.  MFMA j of a panel takes panel columns 4j..4j+3 (lane
//     group g = lane/16 supplies column 4j+g), so global k ascends strictly
//     through the panel and from panel to panel: bitwise the k-ordered fmaf
//     chain of gemm_fwd_pipe_kernel<1,16> on the written states.  Exactly
//     D/4 MFMAs per row — the last panel's j beyond D are skipped, not
//     zero-padded (a padded fma would turn a -0 accumulator into +0).  No
//     xvp partials, no reduce launch, and no third pass over the states.
// The V panel sits in LDS in natural [k][16] layout (the B read of MFMA j
// is the 64 consecutive floats at row 4j); the A read of the swizzled
// image, tile[fi*64 + ((j ^ fi) << 2) + g], touches 64 distinct banks (per
// 16-lane group 16 distinct slots, the groups 4 distinct dwords of a slot).
// xva[:, 0:16] is stored after the block's last K loop has read its xva
// rows; rows are block-private.
//
// LDS is the 2-deep ring (24 KB; images + V panel inside it, as in the
// per-panel kernel), registers are bounded for 4 blocks/CU: 2048 flagship
// row tiles on 256 CUs are then exactly two full waves of blocks.
// ---------------------------------------------------------------------------

struct EnvRowsArgs {
  FwdArgs g;       // X = xva, Wt = M, B = E, K, N = D, env_* (no rsum / xvp)
  float* xva;      // [E][K]: columns 0..15 receive next-state @ V
  int* t;          // [E] step counters (g.tcount aliases it)
  float* epr;      // [E]
  float* rewards;  // [E]
  float* dones;    // [E]
};

__launch_bounds__(FWD_WAVES * 64, 4)
__global__ void env_step_rows_kernel(EnvRowsArgs m) {
  constexpr int NT = GLDS_NT;
  constexpr int NW = GLDS_NW;
  constexpr int HR = ENV_HR;
  constexpr int RING = 2;
  static_assert(RING * GLDS_SLOT >= FWD_WAVES * HR * NW * 4 + NW * 16 * 4,
                "env epilogue image + V panel must fit the ring");
  __shared__ __attribute__((aligned(16))) char smem[RING * GLDS_SLOT];
  const FwdArgs& a = m.g;
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = tid / WAVE;

  const int64_t b0 = (int64_t)blockIdx.x * FWD_M;
  if (b0 >= a.B) return;

  float* tile = reinterpret_cast<float*>(smem) + wave * (HR * NW);
  float* vs = reinterpret_cast<float*>(smem) + FWD_WAVES * HR * NW;
  const unsigned seed = (unsigned)(*a.seed_dev);
  const float sigma = a.sigma;
  const int step = a.step;
  const int c4 = lane & 15;   // float4 slot inside the 64-col panel; also
                              // the A row / B column of the x@V fragments
  const int rsub = lane >> 4;
  const int64_t w0 = b0 + wave * M_WAVE;

  // done flag of this lane's 8 rows (pass h, row group j: row 16h+4j+rsub),
  // read once; the owning lane rewrites t after the last panel
  unsigned donebits = 0;
  #pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int64_t e = w0 + 4 * i + rsub;
    if (e < a.B && a.tcount[e] + 1 >= a.horizons[e]) donebits |= 1u << i;
  }

  // running pred^2 sum of row 4*c4 + rsub of the wave (lanes c4 < 8): after
  // the xor tree all 16 lanes of a row group hold the panel's sum, so lane
  // c4 keeps the one of the group's row pass c4/4, group c4%4 — one register
  // for the wave's 32 rows instead of eight
  float ssrow = 0.f;
  f32x4 xa[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};

  const int npanels = (a.N + NW - 1) / NW;
  for (int p = 0; p < npanels; ++p) {
    const int n0 = p * NW;
    f32x16 acc[NT];
    // opaque per panel: keeps the K loop's row pointers from being hoisted
    // and held (spilled) across the epilogue
    int64_t b0p = b0;
    asm volatile("" : "+s"(b0p));
    glds_fwd_mainloop<RING>(a, smem, b0p, n0, acc);

    // this panel's rows of V ([64][16]; rows >= D zero, never multiplied)
    // -> LDS, one float4 per thread
    {
      const int kl = tid >> 2;
      const int kr = n0 + kl;
      float4 vv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (kr < a.N)
        vv = *reinterpret_cast<const float4*>(
            &a.env_V[(int64_t)kr * 16 + 4 * (tid & 3)]);
      *reinterpret_cast<float4*>(&vs[kl * 16 + 4 * (tid & 3)]) = vv;
    }
    __syncthreads();

    const int d = n0 + 4 * c4;  // first of this lane's 4 dims
    const int c = d >> 2;       // env_finish_kernel's float4 chunk index
    const bool cok = d < a.N;   // N%4==0: a float4 is all in or all out
    float4 dv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cok) dv = *reinterpret_cast<const float4*>(&a.envd[d]);
    const int nj = min(16, (a.N - n0) >> 2);  // 4-column groups in the panel
    // opaque per panel: otherwise the 8 rows' addresses, bounds masks and
    // RNG hash prefixes are hoisted out of the panel loop and spill
    int rs = rsub;
    asm volatile("" : "+v"(rs));
    #pragma unroll
    for (int h = 0; h < 2; ++h) {
      env_tile_dump(tile, acc, h, lane);
      #pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int lr = 4 * j + rs;
        const int64_t e = w0 + HR * h + lr;
        float4* slot =
            reinterpret_cast<float4*>(&tile[lr * NW + ((c4 ^ lr) << 2)]);
        float4 v;
        float ss;
        env_tile_f4<true>(a, slot, e, d, c, e < a.B && cok, seed, sigma, step,
                          dv, (int)((donebits >> (4 * h + j)) & 1u), v, ss);
        if (c4 == 4 * h + j) ssrow += ss;
        // x@V operand: the state actually written (reset rows included),
        // zeros in pad rows
        *slot = v;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      #pragma unroll 4
      for (int j = 0; j < nj; ++j) {
        const float av = tile[c4 * NW + ((j ^ c4) << 2) + rsub];
        const float bv = vs[(4 * j + rsub) * 16 + c4];
        xa[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, xa[h], 0, 0, 0);
      }
    }
    // images and V panel are read; the next panel's K loop reuses the ring
    __syncthreads();
  }

  // per-env bookkeeping by the lane that owns the row's reward sum
  {
    const int64_t e = w0 + 4 * c4 + rsub;
    if (c4 < 8 && e < a.B) {
      int done;
      episode_step(ssrow, a.N, e, done, a.horizons, m.t, m.epr, m.rewards,
                   m.dones);
    }
  }
  // D reg r of pass h: row 16h + 4*(l/16) + r, col l%16; + 0.f is the
  // zero-bias add of the gemm_fwd call this replaces
  #pragma unroll
  for (int h = 0; h < 2; ++h) {
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t e = w0 + HR * h + 4 * rsub + r;
      if (e < a.B) m.xva[e * a.K + c4] = xa[h][r] + 0.f;
    }
  }
}

// ---------------------------------------------------------------------------
// Fused policy forward: L1 -> L2 -> heads (-> action sampling) for one
// 128-row tile, one launch.  L1 is gemm_fwd_glds_kernel<3>'s K loop
// (glds_fwd_mainloop); it ends with two accumulator tiles live and the
// 36 KB ring dead.  Each wave then keeps its own 32 rows in a private LDS
// image inside the ring and runs the two 64-deep products on it with the
// same MFMA and the same stage order as the split calls, so h1, h2, pdflat
// and v are bitwise what three gemm_fwd calls give — but the forward never
// reads h1 / h2 / pdflat back from HBM, and with SAMPLE the rollout's
// sample_kernel launch goes too.
//
// Image: [32 rows][IMG_LD = 65] floats per wave (4 x 8320 B = 33280 B).
// ds_write_b32 of an accumulator register: a 32-lane half writes 32
// consecutive columns of one row — 32 banks.  The A-fragment ds_read_b32:
// a half reads one column of 32 rows, stride 65 = 1 (mod 32) — 32 banks
// (an unpadded stride of 64 would put them all on one).  The two halves
// of either instruction never conflict.  A wave touches only its own
// image and its LDS operations complete in order, so nothing after the
// K loop needs a block barrier.
//
// B fragments of the two small products come straight from global: W2t
// and WhT are 16 KB each and L2-resident, 128 B per half-wave per load,
// and the four waves per SIMD cover the latency.
// ---------------------------------------------------------------------------

constexpr int IMG_LD = 65;

struct MlpFwdArgs {
  FwdArgs l1;          // X, Wt = W1t [D][64], bias = b1, C = h1, B, K = D
  const float* W2t;    // [64][64]
  const float* b2;     // [64]
  float* h2;           // [B][64]
  const float* WhT;    // [64][NH] padded transposed heads, NH = 2A + 2
  const float* bh;     // [NH]
  float* pdflat;       // [B][NH - 2]
  float* v;            // [B]
  int NH;
  // SAMPLE only (sample_kernel's arguments)
  float* actions;      // [B][A]
  float* xva;          // [B][xva_w]
  const long long* seed_dev;
  const float* eps_dev;
  int step, xva_w, va_off;
  float act_low, act_high;
};

// acc = image[32][64] @ W[64][N] in the split call's order: four 16-wide
// k-stages starting at stage `phase`, k ascending inside a stage.  Columns
// >= N read a clamped (valid) column and are discarded by the caller;
// tile 1 is skipped when N <= 32 (wave-uniform).
DEV_INLINE void img_gemm64(const float* img, const float* __restrict__ W,
                           int N, int phase, int lane,
                           f32x16 (&acc)[GLDS_NT]) {
  const int i_l = lane & 31;
  const int k_l = lane >> 5;
  #pragma unroll
  for (int t = 0; t < GLDS_NT; ++t)
    #pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  const int c0 = i_l < N ? i_l : N - 1;
  const int c1 = M_WAVE + i_l < N ? M_WAVE + i_l : N - 1;
  const bool two = N > M_WAVE;
  #pragma unroll 1
  for (int s = 0; s < 4; ++s) {
    const int kb = ((s + phase) & 3) * GLDS_BK;
    #pragma unroll
    for (int k2 = 0; k2 < GLDS_BK; k2 += 2) {
      const int k = kb + k2 + k_l;
      const float av = img[i_l * IMG_LD + k];
      const float b0v = W[k * N + c0];
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0v, acc[0], 0, 0, 0);
      if (two) {
        const float b1v = W[k * N + c1];
        acc[1] =
            __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1v, acc[1], 0, 0, 0);
      }
    }
  }
}

// hidden-layer epilogue (N = 64): act(acc + b) to global rows < B and to
// the wave's image
DEV_INLINE void hidden_epilogue(const f32x16 (&acc)[GLDS_NT],
                                const float* __restrict__ bias,
                                int activation, float* C, float* img,
                                int64_t row0, int64_t B, int lane) {
  #pragma unroll
  for (int t = 0; t < GLDS_NT; ++t) {
    const int col = t * M_WAVE + (lane & 31);
    const float bv = bias[col];
    #pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int lr = cd_row(r, lane);
      const float x = fwd_bias_act(acc[t][r], bv, activation);
      if (row0 + lr < B) C[(row0 + lr) * GLDS_NW + col] = x;
      img[lr * IMG_LD + col] = x;
    }
  }
}

template <bool SAMPLE>
__launch_bounds__(FWD_WAVES * 64, 4)
__global__ void mlp_fwd_fused_kernel(MlpFwdArgs m) {
  constexpr int RING = 3;
  static_assert(RING * GLDS_SLOT >= FWD_WAVES * M_WAVE * IMG_LD * 4,
                "per-wave images must fit the dead stage ring");
  __shared__ __attribute__((aligned(16))) char smem[RING * GLDS_SLOT];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = threadIdx.x / WAVE;
  const int64_t b0 = (int64_t)blockIdx.x * FWD_M;
  const int64_t B = m.l1.B;
  if (b0 >= B) return;

  f32x16 acc[GLDS_NT];
  glds_fwd_mainloop<RING>(m.l1, smem, b0, 0, acc);

  float* img = reinterpret_cast<float*>(smem) + wave * (M_WAVE * IMG_LD);
  const int64_t row0 = b0 + wave * M_WAVE;
  const int act = m.l1.activation;
  // the split L2 / heads calls rotate their four stages by the row block
  // (glds kernel); heads of N <= 32 take the unrotated pipe kernel there
  const int phase = (int)(blockIdx.x & 3u);
  const int hphase = m.NH > M_WAVE ? phase : 0;

  hidden_epilogue(acc, m.l1.bias, act, m.l1.C, img, row0, B, lane);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  img_gemm64(img, m.W2t, GLDS_NW, phase, lane, acc);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  hidden_epilogue(acc, m.b2, act, m.h2, img, row0, B, lane);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  img_gemm64(img, m.WhT, m.NH, hphase, lane, acc);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

  // heads epilogue (heads mode 2, no activation)
  const int NH = m.NH;
  #pragma unroll
  for (int t = 0; t < GLDS_NT; ++t) {
    const int col = t * M_WAVE + (lane & 31);
    if (col < NH) {
      const float bv = m.bh[col];
      #pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int lr = cd_row(r, lane);
        const float x = fwd_bias_act(acc[t][r], bv, 2);
        if (row0 + lr < B)
          fwd_store(m.pdflat, m.v, 2, NH, NH - 2, row0 + lr, col, x);
        if constexpr (SAMPLE) img[lr * IMG_LD + col] = x;
      }
    }
  }

  if constexpr (SAMPLE) {
    // sample_kernel's per-(env, j) work on the pd tile in the image
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const unsigned seed = (unsigned)*m.seed_dev;
    const float eps = *m.eps_dev;
    const int A = (NH - 2) >> 1;
    const int step = m.step;
    for (int idx = lane; idx < M_WAVE * A; idx += WAVE) {
      const int lr = idx / A;
      const int j = idx - lr * A;
      const int64_t e = row0 + lr;
      if (e < B) {
        const float mean = img[lr * IMG_LD + j];
        const float logstd = img[lr * IMG_LD + A + j];
        const float a_ = box_sample(mean, logstd, seed, e, step, j, eps,
                                    m.act_low, m.act_high);
        m.actions[e * A + j] = a_;
        m.xva[e * m.xva_w + m.va_off + j] = a_;
      }
    }
  }
}

// per-env finish after the fused env-step GEMM: reward from the pred^2
// partials, episode bookkeeping, and re-zero rsum for the next step
__global__ void env_finish2_kernel(const float* __restrict__ rsum,
                                   int* __restrict__ t,
                                   const int* __restrict__ horizons,
                                   float* __restrict__ epr,
                                   float* __restrict__ rewards,
                                   float* __restrict__ dones, int64_t E,
                                   int D, int npanels) {
  for (int64_t e = gidx(); e < E; e += gstride()) {
    float ss = 0.f;
    for (int p = 0; p < npanels; ++p) ss += rsum[(int64_t)p * E + e];
    int done;
    episode_step(ss, D, e, done, horizons, t, epr, rewards, dones);
  }
}

// x@V fold: sum the per-panel next-state @ V partials into the concat
// buffer's first 16 columns (the NEXT step's x@V; the G-GEMM that read
// xva for this step has finished in stream order).  Thread per
// (env, float4); fixed panel order, so deterministic.
__global__ void env_xv_reduce_kernel(const float* __restrict__ xvp,
                                     float* __restrict__ xva, int64_t E,
                                     int kw, int npanels) {
  for (int64_t i = gidx(); i < E * 4; i += gstride()) {
    const int64_t e = i >> 2;
    const int q = (int)(i & 3);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int p = 0; p < npanels; ++p) {
      const float4 v = *reinterpret_cast<const float4*>(
          &xvp[((int64_t)p * E + e) * 16 + 4 * q]);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    *reinterpret_cast<float4*>(&xva[e * kw + 4 * q]) = s;
  }
}

// ---------------------------------------------------------------------------
// dW accumulation: dW[out][in] += delta^T @ acts (+ db += sum delta)
// grid = (m_tiles, n_tiles, splits); one wave per block.
// ---------------------------------------------------------------------------

struct DwArgs {
  const float* delta;  // [B][out]
  const float* acts;   // [B][in]
  float* slab;         // [splits][out][in] per-split partials (plain stores
                       // — atomics measured 8.4M adds/launch and dominated)
  float* db_slab;      // [splits][out]
  int64_t B;
  int out_dim, in_dim;
  int nt;       // 32-col tiles per wave (<= MAX_NT)
  int splits;   // K splits
  int ablate;   // perf diagnosis only: 4 skip MFMA, 8 skip slab stores
};

template <int NT, int MT>  // MT row fragments of 32 (1 or 2)
// the hot <2,2> instantiation needs the allocator pressured to keep 3
// waves/SIMD with the two-pair pipeline (unforced: 200+ VGPR, 2 waves)
__launch_bounds__(64, (NT == 2 && MT == 2) ? 3 : 1)
__global__ void dw_mfma_kernel(DwArgs a) {
  const int lane = threadIdx.x;
  const int m0 = blockIdx.x * (M_WAVE * MT);
  const int n_base = blockIdx.y * a.nt * M_WAVE;
  const int split = blockIdx.z;

  const int64_t rows_per = (a.B + a.splits - 1) / a.splits;
  const int64_t k0 = split * rows_per;
  const int64_t k1 = min(a.B, k0 + rows_per);

  const int i_l = lane & 31;
  const int k_l = lane >> 5;
  int mcol[MT];
  bool m_ok[MT];
  #pragma unroll
  for (int m = 0; m < MT; ++m) {
    mcol[m] = m0 + m * M_WAVE + i_l;
    m_ok[m] = mcol[m] < a.out_dim;
  }

  f32x16 acc[MT][NT];
  #pragma unroll
  for (int m = 0; m < MT; ++m)
    #pragma unroll
    for (int t = 0; t < NT; ++t)
      #pragma unroll
      for (int r = 0; r < 16; ++r) acc[m][t][r] = 0.f;
  float dbacc[MT];
  #pragma unroll
  for (int m = 0; m < MT; ++m) dbacc[m] = 0.f;

  // column guards hoisted out of the K loop (tail tiles load col 0 and
  // discard at scatter time — a harmless re-read keeps the loop branchless)
  int bcol[NT];
  bool col_ok[NT];
  #pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int col = n_base + t * M_WAVE + i_l;
    col_ok[t] = col < a.in_dim;
    bcol[t] = col_ok[t] ? col : 0;
  }

  // two-pair ping-pong pipeline: TWO register sets alternate with no
  // copies, keeping two pairs of streamed loads in flight ahead of the
  // MFMAs (the one-pair version kept only ~16 B/wave outstanding and
  // measured load-phase-bound: 858 of 1079 us).  MFMA order stays k-
  // ascending -> results bitwise identical.
  const int64_t kend = k0 + ((k1 - k0) & ~1);
  int64_t k = k0;
  float av_A[MT], av_B[MT];
  float bv_A[NT], bv_B[NT];
  auto load_pair = [&](int64_t kk, float (&av)[MT], float (&bv)[NT]) {
    #pragma unroll
    for (int m = 0; m < MT; ++m)
      av[m] = m_ok[m] ? a.delta[(kk + k_l) * a.out_dim + mcol[m]] : 0.f;
    #pragma unroll
    for (int t = 0; t < NT; ++t)
      bv[t] = a.acts[(kk + k_l) * a.in_dim + bcol[t]];
  };
  auto fma_pair = [&](const float (&av)[MT], const float (&bv)[NT]) {
    if (!(a.ablate & 4)) {
      #pragma unroll
      for (int m = 0; m < MT; ++m) {
        dbacc[m] += av[m];
        #pragma unroll
        for (int t = 0; t < NT; ++t)
          acc[m][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m], bv[t],
                                                           acc[m][t], 0, 0, 0);
      }
    } else {
      #pragma unroll
      for (int m = 0; m < MT; ++m) dbacc[m] += av[m];
      #pragma unroll
      for (int t = 0; t < NT; ++t) dbacc[0] += bv[t] * 1e-38f;
    }
  };
  if (k < kend) load_pair(k, av_A, bv_A);
  if (k + 2 < kend) load_pair(k + 2, av_B, bv_B);
  #pragma unroll 1
  for (; k + 6 < kend; k += 4) {
    fma_pair(av_A, bv_A);
    load_pair(k + 4, av_A, bv_A);
    fma_pair(av_B, bv_B);
    load_pair(k + 6, av_B, bv_B);
  }
  if (k < kend) { fma_pair(av_A, bv_A); k += 2; }
  if (k < kend) { fma_pair(av_B, bv_B); k += 2; }
  #pragma unroll 1
  for (; k < kend; k += 2) {
    load_pair(k, av_A, bv_A);
    fma_pair(av_A, bv_A);
  }
  for (; k < k1; ++k) {
    #pragma unroll
    for (int m = 0; m < MT; ++m) {
      const float av =
          (m_ok[m] && k_l == 0) ? a.delta[k * a.out_dim + mcol[m]] : 0.f;
      if (k_l == 0) dbacc[m] += av;
      #pragma unroll
      for (int t = 0; t < NT; ++t) {
        const float bv = (k_l == 0) ? a.acts[k * a.in_dim + bcol[t]] : 0.f;
        acc[m][t] =
            __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[m][t], 0, 0, 0);
      }
    }
  }

  // ---- store accumulators to this split's slab (each (row,col) of a
  // split is owned by exactly one block: no atomics, no zero-init) ----
  float* slab = a.slab + (int64_t)split * a.out_dim * a.in_dim;
  if (a.ablate & 8) return;
  #pragma unroll
  for (int m = 0; m < MT; ++m) {
    #pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (col_ok[t]) {
        #pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int mrow = m0 + m * M_WAVE + cd_row(r, lane);
          if (mrow < a.out_dim)
            slab[(int64_t)mrow * a.in_dim + bcol[t]] = acc[m][t][r];
        }
      }
    }
  }
  if (blockIdx.y == 0) {
    #pragma unroll
    for (int m = 0; m < MT; ++m) {
      const float other = __shfl(dbacc[m], lane ^ 32, WAVE);
      if (lane < 32 && m_ok[m])
        a.db_slab[(int64_t)split * a.out_dim + mcol[m]] = dbacc[m] + other;
    }
  }
}

// ---------------------------------------------------------------------------
// dW glds kernel (round-2 lever #2): one 8-wave block owns the WHOLE
// [out<=64][in<=384] dW tile for one K split, with both operands staged
// row-major by global_load_lds into a 3-deep ring with counted vmcnt
// (same pipeline as gemm_fwd_glds_kernel).  Replaces the 1-wave
// dw_mfma_kernel's 4-B-per-lane streams for the big flagship dW calls:
// delta is read ONCE (the old n-tile grid re-read it 6x) and the block
// keeps two full stages in flight.
// Both MFMA operands are row-major-k, column-per-lane LDS reads
// (conflict-free); K-split tails zero the delta rows past the split so
// clamped/garbage rows contribute nothing.
// ---------------------------------------------------------------------------

constexpr int DWG_K = 16;        // k rows per stage

// Generic over the block geometry: MW m-wave-tiles x NWV n-wave-groups
// of NTW 32-col tiles (threads = MW*NWV*64).  <2,4,3> covers the wide
// dW1 tile [64][384]; <2,2,1> covers the narrow [64][64] shapes (dW2,
// padded heads dW) without idling 3/4 of the block.
template <int MW, int NWV, int NTW, int RING = 3>
__launch_bounds__(MW * NWV * 64, 2)
__global__ void dw_glds_kernel(DwArgs a) {
  constexpr int THREADS = MW * NWV * 64;
  constexpr int DWG_M = MW * 32;
  constexpr int DWG_N = NWV * NTW * 32;
  constexpr int DWG_DB = DWG_K * DWG_M * 4;
  constexpr int DWG_AB = DWG_K * DWG_N * 4;
  constexpr int DWG_SLOT = DWG_DB + DWG_AB;
  constexpr int DWG_PIECES = DWG_SLOT / 16;
  constexpr int DWG_PPT = (DWG_PIECES + THREADS - 1) / THREADS;
  // RING: the wide <2,4,3> tile is 28 KB/stage -> 1 block/CU at ANY ring
  // depth, so a 5-deep ring (4 stages = 112 KB in flight) is free and
  // covers loaded-chip HBM latency the 3-deep ring stalled on
  __shared__ __attribute__((aligned(16))) char smem[RING * DWG_SLOT + 4096];
  char* const pad = smem + RING * DWG_SLOT;  // dummy glds target (uniformity)
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = tid >> 6;
  const int i_l = lane & 31;
  const int k_l = lane >> 5;
  const int wm = wave / NWV;              // m-tile of 32
  const int wn = wave % NWV;              // n-group of NTW*32
  const int split = blockIdx.x;
  // n-panel (grid.y): narrow tiles with small per-stage LDS let 2 blocks
  // co-reside per CU so stage-barrier bubbles overlap across blocks; the
  // (small) delta stage is duplicated per panel
  const int nb0 = (int)blockIdx.y * DWG_N;

  const int64_t rows_per = (a.B + a.splits - 1) / a.splits;
  const int64_t k0 = (int64_t)split * rows_per;
  const int64_t k1 = min(a.B, k0 + rows_per);
  if (k0 >= a.B) return;
  const int S = (int)((k1 - k0 + DWG_K - 1) / DWG_K);

  // per-thread glds sources: piece q = tid + p*THREADS; rows past B
  // clamp to B-1 (garbage — the delta-row zeroing kills them)
  const float* base[DWG_PPT];
  int krow_p[DWG_PPT];
  int ld_p[DWG_PPT];
  unsigned dsto[DWG_PPT];
  #pragma unroll
  for (int p = 0; p < DWG_PPT; ++p) {
    const int q = tid + p * THREADS;
    if (q < DWG_DB / 16) {               // delta piece
      const int kq = q / (DWG_M / 4);
      int c4 = (q % (DWG_M / 4)) * 4;
      c4 = c4 + 3 < a.out_dim ? c4 : (a.out_dim > 4 ? a.out_dim - 4 : 0);
      base[p] = a.delta + c4;
      krow_p[p] = kq;
      ld_p[p] = a.out_dim;
      dsto[p] = q * 16;
    } else if (q < DWG_PIECES) {         // acts piece
      const int qq = q - DWG_DB / 16;
      const int kq = qq / (DWG_N / 4);
      int c4 = nb0 + (qq % (DWG_N / 4)) * 4;
      c4 = c4 + 3 < a.in_dim ? c4 : (a.in_dim > 4 ? a.in_dim - 4 : 0);
      base[p] = a.acts + c4;
      krow_p[p] = kq;
      ld_p[p] = a.in_dim;
      dsto[p] = q * 16;
    } else {                             // pad piece: dummy, uniform vmcnt
      base[p] = a.delta;
      krow_p[p] = 0;
      ld_p[p] = 0;
      dsto[p] = 0xFFFFFFFFu;
    }
  }

  auto issue = [&](int s) {
    char* slot = smem + (s % RING) * DWG_SLOT;
    #pragma unroll
    for (int p = 0; p < DWG_PPT; ++p) {
      int64_t row = k0 + (int64_t)s * DWG_K + krow_p[p];
      row = row < a.B ? row : a.B - 1;
      const float* g = base[p] + row * ld_p[p];
      char* dst = dsto[p] == 0xFFFFFFFFu ? pad + (tid & 255) * 16
                                         : slot + dsto[p];
      __builtin_amdgcn_global_load_lds(
          (const __attribute__((address_space(1))) unsigned*)g,
          (unsigned*)dst, 16, 0, 0);
    }
  };

  #pragma unroll
  for (int p = 0; p < RING - 1; ++p)
    if (p < S) issue(p);

  f32x16 acc[NTW];
  #pragma unroll
  for (int t = 0; t < NTW; ++t)
    #pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float dbacc = 0.f;
  const int mcol = wm * M_WAVE + i_l;

  for (int s = 0; s < S; ++s) {
    // stage s landed when only the rem in-flight later stages' loads
    // (DWG_PPT each) remain outstanding
    const int rem = min(S - 1 - s, RING - 2);
    if (RING >= 5 && rem >= 3)
      asm volatile("s_waitcnt vmcnt(%0)" :: "i"(3 * DWG_PPT) : "memory");
    else if (RING >= 4 && rem == 2)
      asm volatile("s_waitcnt vmcnt(%0)" :: "i"(2 * DWG_PPT) : "memory");
    else if (rem == 1)
      asm volatile("s_waitcnt vmcnt(%0)" :: "i"(DWG_PPT) : "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    char* slot = smem + (s % RING) * DWG_SLOT;
    float* ds = (float*)slot;                    // [16][DWG_M] delta
    float* as = (float*)(slot + DWG_DB);         // [16][DWG_N] acts
    const int64_t kb = k0 + (int64_t)s * DWG_K;
    const int kval = (int)((k1 - kb) < DWG_K ? (k1 - kb) : DWG_K);
    if (kval < DWG_K) {
      // zero the delta rows past the split (kills garbage contributions)
      for (int idx = tid; idx < (DWG_K - kval) * DWG_M; idx += THREADS)
        ds[kval * DWG_M + idx] = 0.f;
      __builtin_amdgcn_s_barrier();
    }
    // buf (s+RING-1)%RING == (s-1)%RING, freed by the barrier above
    if (s + RING - 1 < S) issue(s + RING - 1);
    #pragma unroll 4
    for (int k2 = 0; k2 < DWG_K; k2 += 2) {
      const float av = ds[(k2 + k_l) * DWG_M + mcol];
      dbacc += av;
      #pragma unroll
      for (int t = 0; t < NTW; ++t) {
        const float bv =
            as[(k2 + k_l) * DWG_N + wn * (NTW * M_WAVE) + t * M_WAVE + i_l];
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
      }
    }
  }

  // ---- store to this split's slab ----
  float* slab = a.slab + (int64_t)split * a.out_dim * a.in_dim;
  #pragma unroll
  for (int t = 0; t < NTW; ++t) {
    const int col = nb0 + wn * (NTW * M_WAVE) + t * M_WAVE + i_l;
    if (col < a.in_dim) {
      #pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int mrow = wm * M_WAVE + cd_row(r, lane);
        if (mrow < a.out_dim)
          slab[(int64_t)mrow * a.in_dim + col] = acc[t][r];
      }
    }
  }
  if (wn == 0 && blockIdx.y == 0) {
    const float other = __shfl(dbacc, lane ^ 32, WAVE);
    if (lane < 32 && mcol < a.out_dim)
      a.db_slab[(int64_t)split * a.out_dim + mcol] = dbacc + other;
  }
}

// Split-slab reduction into the flat grad, handling the optional
// combined-heads row split (rows < split_row -> dW/db, rest -> dW2/db2).
// Parallel over (element, split-chunk): a serial full-splits loop per
// element left the chip at <1 wave/SIMD and 480 us per call.
constexpr int DW_RED_CHUNK = 32;

__global__ void dw_reduce_kernel(const float* __restrict__ slab,
                                 const float* __restrict__ db_slab,
                                 float* __restrict__ dW, float* __restrict__ db,
                                 float* __restrict__ dW2,
                                 float* __restrict__ db2, int64_t out_dim,
                                 int64_t in_dim, int splits, int split_row) {
  const int64_t n = out_dim * in_dim;
  const int s0 = blockIdx.y * DW_RED_CHUNK;
  const int s1 = min(splits, s0 + DW_RED_CHUNK);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    float acc = 0.f;
    for (int s = s0; s < s1; ++s) acc += slab[(int64_t)s * n + i];
    const int64_t mrow = i / in_dim;
    float* dst = (split_row >= 0 && mrow >= split_row)
                     ? &dW2[(mrow - split_row) * in_dim + i % in_dim]
                     : &dW[i];
    atomicAdd(dst, acc);
  }
}

__global__ void db_reduce_kernel(const float* __restrict__ db_slab,
                                 float* __restrict__ db,
                                 float* __restrict__ db2, int64_t out_dim,
                                 int splits, int split_row) {
  // one wave per output column; lanes stride the splits axis
  const int m = blockIdx.x;
  if (m >= out_dim) return;
  const int lane = threadIdx.x;
  float acc = 0.f;
  for (int s = lane; s < splits; s += WAVE)
    acc += db_slab[(int64_t)s * out_dim + m];
  acc = wave_reduce_sum(acc);
  if (lane == 0) {
    if (split_row >= 0 && m >= split_row) db2[m - split_row] += acc;
    else if (db != nullptr) db[m] += acc;
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// Bindings
// ---------------------------------------------------------------------------

// Stage-ring depth of gemm_fwd_glds_kernel for a given K — the one place
// both gemm_fwd and gemm_env_step take it from.  Short-K GEMMs (few
// stages) run the 2-deep ring — 24 KB LDS lets 6 blocks/CU co-reside and
// prologue/drain is a large fraction of S (L2t K=64: 179 -> 157 us at
// B=1M); long-K streams keep the 3-deep ring (L1t K=376: wash; ring 4
// measured slower).  DPPO_FWD_RING=2/3/4 forces a depth.
static int fwd_ring_for(int K) {
  static const int ring_env = env_int("DPPO_FWD_RING", 0);  // 0 = by shape
  return ring_env ? ring_env : (K <= 128 ? 2 : 3);
}

// gemm_fwd_glds_kernel<ring, ENV> for a runtime ring depth (3 unless 2 or 4)
template <bool ENV>
static void launch_glds(int ring, dim3 grid, hipStream_t stream,
                        const FwdArgs& a) {
  const dim3 block(FWD_WAVES * 64);
  if (ring == 2)
    hipLaunchKernelGGL((gemm_fwd_glds_kernel<2, ENV>), grid, block, 0, stream,
                       a);
  else if (ring == 4)
    hipLaunchKernelGGL((gemm_fwd_glds_kernel<4, ENV>), grid, block, 0, stream,
                       a);
  else
    hipLaunchKernelGGL((gemm_fwd_glds_kernel<3, ENV>), grid, block, 0, stream,
                       a);
}

void gemm_fwd(torch::Tensor X, torch::Tensor Wt, torch::Tensor bias,
              int64_t activation, int64_t heads, torch::Tensor C,
              torch::Tensor v, torch::Tensor aux, int64_t wt_layout,
              int64_t ablate, int64_t ldc) {
  // C and (for heads) v are caller-allocated so activations can land
  // directly in the backward's blob layout.  ldc (0 = natural width) lets
  // C land in a column block of a wider row-major buffer; N > 128 runs as
  // column panels on the pipelined kernel (grid.y).
  const int64_t B = X.size(0);
  const int K = static_cast<int>(X.size(1));
  const int N = static_cast<int>(wt_layout ? Wt.size(0) : Wt.size(1));
  TORCH_CHECK(X.is_cuda() && X.is_contiguous() && Wt.is_contiguous());
  TORCH_CHECK(C.is_contiguous());
  TORCH_CHECK((wt_layout ? Wt.size(1) : Wt.size(0)) == K);
  TORCH_CHECK(activation >= 3 || bias.numel() == N);
  const int ncols = static_cast<int>(heads == 2 ? N - 2 : heads ? N - 1 : N);
  const int ldc_eff = static_cast<int>(ldc > 0 ? ldc : ncols);
  TORCH_CHECK(ldc_eff >= ncols);
  if (heads) {
    TORCH_CHECK(C.numel() >= (B - 1) * ldc_eff + ncols && v.numel() == B);
  } else {
    TORCH_CHECK(C.numel() >= (B - 1) * ldc_eff + ncols);
  }

  FwdArgs a{};
  a.X = X.data_ptr<float>();
  a.Wt = Wt.data_ptr<float>();
  a.bias = bias.data_ptr<float>();
  a.B = B;
  a.K = K;
  a.N = N;
  a.activation = static_cast<int>(activation);
  a.heads = static_cast<int>(heads);
  a.wt_layout = static_cast<int>(wt_layout);
  a.ablate = static_cast<int>(ablate);
  a.ldc = ldc_eff;
  a.C = C.data_ptr<float>();
  a.v = heads ? v.data_ptr<float>() : nullptr;
  if (activation >= 3) {
    TORCH_CHECK(aux.numel() == B * N, "dgrad mode needs aux = fwd activations");
    a.aux = aux.data_ptr<float>();
  }

  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  const int64_t tiles = (B + FWD_M - 1) / FWD_M;
  // plain kernel: capped grid + tile loop.  pipe kernel: one block per
  // tile — block scheduling hides the per-tile staging prologue.
  const int grid = static_cast<int>(std::min<int64_t>(tiles, 4096));
  const int grid_pipe = static_cast<int>(std::min<int64_t>(tiles, 1 << 22));
  const int NT = (N + M_WAVE - 1) / M_WAVE;
  // T14 register-pipelined variant (see gemm_fwd_pipe_kernel).  Its
  // branchless clamped loads need K>=4 (X / layout-1 W rows) and, for
  // layout 0, N>=4 (W rows); tiny shapes take the plain kernel.
  static const int pipe_env = env_int("DPPO_GEMM_PIPE", 1);
  static const int pbk_env = env_int("DPPO_GEMM_PBK", 0);  // 0 = by shape
  // K%4!=0 is allowed for the dgrad-from-gh call (activation>=3,
  // wt_layout 0): its X is the gh buffer, allocated with a float4 of
  // slack, and the overhang columns multiply zeroed W rows >= K.
  const bool pipe = pipe_env && !a.ablate && K >= 4 &&
                    (K % 4 == 0 || (wt_layout == 0 && activation >= 3)) &&
                    (wt_layout == 1 || (N >= 4 && N % 4 == 0));
  const int pbk = pbk_env ? pbk_env : 16;
  static const int glds_env = env_int("DPPO_GEMM_GLDS", 1);
  // glds 3-buffer streaming variant: NT==2 only (wave-uniform vmcnt),
  // layout-0 W, 16-B-aligned rows (K%4==0, N%4==0), no ablation hooks
  const bool glds_ok = glds_env && !a.ablate && wt_layout == 0 &&
                       K % 4 == 0 && K >= 4 && N % 4 == 0 && N >= 4 &&
                       a.activation != 9999;
  const int ring_sel = fwd_ring_for(a.K);
  #define DISPATCH_FWD(NTV, NPANEL)                                          \
    if (glds_ok && NTV == 2)                                                 \
      launch_glds<false>(ring_sel, dim3((unsigned)grid_pipe, NPANEL), stream, \
                         a);                                                 \
    else if (pipe && pbk == 32)                                              \
      hipLaunchKernelGGL((gemm_fwd_pipe_kernel<NTV, 32>),                    \
                         dim3(grid_pipe, NPANEL), dim3(FWD_WAVES * 64), 0,   \
                         stream, a);                                         \
    else if (pipe)                                                           \
      hipLaunchKernelGGL((gemm_fwd_pipe_kernel<NTV, 16>),                    \
                         dim3(grid_pipe, NPANEL), dim3(FWD_WAVES * 64), 0,   \
                         stream, a);                                         \
    else                                                                     \
      hipLaunchKernelGGL(gemm_fwd_kernel<NTV>, dim3(grid),                   \
                         dim3(FWD_WAVES * 64), 0, stream, a)
  if (N > MAX_NT * M_WAVE) {
    // wide N: NT=2 column panels (the NT=2 pipe schedule holds 4
    // waves/SIMD; NT=4 would drop to 2) — pipe-capable shapes only
    TORCH_CHECK(pipe, "N > 128 needs the pipelined path (K%4==0 etc.)");
    const int panels = (N + 2 * M_WAVE - 1) / (2 * M_WAVE);
    DISPATCH_FWD(2, panels);
  } else {
    switch (NT) {
      case 1: DISPATCH_FWD(1, 1); break;
      case 2: DISPATCH_FWD(2, 1); break;
      case 3: DISPATCH_FWD(3, 1); break;
      default: DISPATCH_FWD(4, 1); break;
    }
  }
  #undef DISPATCH_FWD
}

bool mlp_fwd_fused_supported(int64_t D, int64_t H1, int64_t H2, int64_t A) {
  const int64_t NH = 2 * A + 2;
  return D >= 4 && D % 4 == 0 && H1 == GLDS_NW && H2 == GLDS_NW && A >= 1 &&
         NH % 4 == 0 && NH <= GLDS_NW;
}

void mlp_fwd_fused(torch::Tensor X, torch::Tensor W1t, torch::Tensor b1,
                   torch::Tensor W2t, torch::Tensor b2, torch::Tensor WhT_pad,
                   torch::Tensor bh_pad, int64_t act_code, torch::Tensor h1,
                   torch::Tensor h2, torch::Tensor pdflat, torch::Tensor v,
                   torch::Tensor actions, torch::Tensor xva,
                   torch::Tensor seed_dev, torch::Tensor eps_dev, int64_t step,
                   int64_t va_off, double act_low, double act_high) {
  // actions non-empty: also sample (rollout); empty: forward only
  TORCH_CHECK(X.is_cuda() && X.dim() == 2 && X.scalar_type() == torch::kFloat);
  const int64_t B = X.size(0);
  const int64_t D = X.size(1);
  TORCH_CHECK(B >= 1 && WhT_pad.dim() == 2);
  const int64_t NH = WhT_pad.size(1);
  const int64_t A = (NH - 2) / 2;
  TORCH_CHECK(NH == 2 * A + 2 && mlp_fwd_fused_supported(D, W1t.size(1),
                                                          W2t.size(1), A),
              "mlp_fwd_fused: shape not eligible");
  TORCH_CHECK(act_code == 0 || act_code == 1, "mlp_fwd_fused: tanh or relu");
  for (const auto& t : {X, W1t, b1, W2t, b2, WhT_pad, bh_pad, h1, h2, pdflat, v})
    TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                t.scalar_type() == torch::kFloat);
  TORCH_CHECK(W1t.dim() == 2 && W1t.size(0) == D && W2t.dim() == 2 &&
              W2t.size(0) == GLDS_NW && WhT_pad.size(0) == GLDS_NW);
  TORCH_CHECK(b1.numel() == GLDS_NW && b2.numel() == GLDS_NW &&
              bh_pad.numel() == NH);
  TORCH_CHECK(h1.numel() == B * GLDS_NW && h2.numel() == B * GLDS_NW &&
              pdflat.numel() == B * (NH - 2) && v.numel() == B);

  MlpFwdArgs m{};
  m.l1.X = X.data_ptr<float>();
  m.l1.Wt = W1t.data_ptr<float>();
  m.l1.bias = b1.data_ptr<float>();
  m.l1.C = h1.data_ptr<float>();
  m.l1.B = B;
  m.l1.K = static_cast<int>(D);
  m.l1.N = GLDS_NW;
  m.l1.activation = static_cast<int>(act_code);
  m.l1.ldc = GLDS_NW;
  m.W2t = W2t.data_ptr<float>();
  m.b2 = b2.data_ptr<float>();
  m.h2 = h2.data_ptr<float>();
  m.WhT = WhT_pad.data_ptr<float>();
  m.bh = bh_pad.data_ptr<float>();
  m.pdflat = pdflat.data_ptr<float>();
  m.v = v.data_ptr<float>();
  m.NH = static_cast<int>(NH);
  const bool sample = actions.numel() > 0;
  if (sample) {
    TORCH_CHECK(actions.is_cuda() && actions.is_contiguous() &&
                actions.scalar_type() == torch::kFloat &&
                actions.numel() == B * A);
    TORCH_CHECK(xva.is_cuda() && xva.is_contiguous() && xva.dim() == 2 &&
                xva.scalar_type() == torch::kFloat && xva.size(0) == B &&
                va_off >= 0 && va_off + A <= xva.size(1));
    TORCH_CHECK(seed_dev.is_cuda() && seed_dev.scalar_type() == torch::kLong &&
                seed_dev.numel() == 1 && eps_dev.is_cuda() &&
                eps_dev.scalar_type() == torch::kFloat &&
                eps_dev.numel() == 1);
    m.actions = actions.data_ptr<float>();
    m.xva = xva.data_ptr<float>();
    m.seed_dev =
        reinterpret_cast<const long long*>(seed_dev.data_ptr<int64_t>());
    m.eps_dev = eps_dev.data_ptr<float>();
    m.step = static_cast<int>(step);
    m.xva_w = static_cast<int>(xva.size(1));
    m.va_off = static_cast<int>(va_off);
    m.act_low = static_cast<float>(act_low);
    m.act_high = static_cast<float>(act_high);
  }
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  const int64_t tiles = (B + FWD_M - 1) / FWD_M;
  TORCH_CHECK(tiles <= (1 << 22));
  if (sample)
    hipLaunchKernelGGL(mlp_fwd_fused_kernel<true>, dim3((unsigned)tiles),
                       dim3(FWD_WAVES * 64), 0, stream, m);
  else
    hipLaunchKernelGGL(mlp_fwd_fused_kernel<false>, dim3((unsigned)tiles),
                       dim3(FWD_WAVES * 64), 0, stream, m);
}

void gemm_env_step(torch::Tensor xva, torch::Tensor M, torch::Tensor xin,
                   torch::Tensor xout, torch::Tensor envd,
                   torch::Tensor horizons, torch::Tensor t,
                   torch::Tensor epr,
                   torch::Tensor rewards, torch::Tensor dones,
                   torch::Tensor rsum, torch::Tensor seed_dev, double sigma,
                   int64_t step, torch::Tensor V, torch::Tensor xvp) {
  // V / xvp non-empty: also fold the next step's x@V into the epilogue
  // (per-panel partials -> xvp, summed into xva[:, 0:16] afterwards)
  const int64_t E = xva.size(0);
  const int K = static_cast<int>(xva.size(1));
  const int D = static_cast<int>(M.size(1));
  TORCH_CHECK(xva.is_contiguous() && M.is_contiguous() &&
              xin.is_contiguous() && xout.is_contiguous());
  TORCH_CHECK(M.size(0) == K && xin.size(0) == E && xin.size(1) == D);
  TORCH_CHECK(xout.numel() == E * D);
  TORCH_CHECK(K % 4 == 0 && D % 4 == 0, "fused env step needs 16B rows");
  TORCH_CHECK(horizons.dtype() == torch::kInt32 && t.dtype() == torch::kInt32);
  const int panels_chk = (D + 63) / 64;
  TORCH_CHECK(rsum.numel() >= panels_chk * E);
  FwdArgs a{};
  a.X = xva.data_ptr<float>();
  a.Wt = M.data_ptr<float>();
  a.B = E;
  a.K = K;
  a.N = D;
  a.activation = 5;
  a.ldc = D;
  a.env_xin = xin.data_ptr<float>();
  a.env_x = xout.data_ptr<float>();
  a.envd = envd.data_ptr<float>();
  a.horizons = horizons.data_ptr<int>();
  a.tcount = t.data_ptr<int>();
  a.seed_dev = reinterpret_cast<const long long*>(seed_dev.data_ptr<int64_t>());
  a.env_rsum = rsum.data_ptr<float>();
  a.sigma = (float)sigma;
  a.step = (int)step;
  const int panels = (D + 63) / 64;
  const bool fold = xvp.numel() > 0;
  if (fold) {
    TORCH_CHECK(V.is_contiguous() && V.dim() == 2 && V.size(0) == D &&
                    V.size(1) == 16,
                "x@V fold needs V = [D][16]");
    TORCH_CHECK(K >= 16 && xvp.is_contiguous() &&
                xvp.numel() >= (int64_t)panels * E * 16);
    a.env_V = V.data_ptr<float>();
    a.env_xvp = xvp.data_ptr<float>();
  }
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  const int64_t tiles = (E + FWD_M - 1) / FWD_M;
  const dim3 grid((unsigned)tiles, (unsigned)panels);
  launch_glds<true>(fwd_ring_for(K), grid, stream, a);
  hipLaunchKernelGGL(env_finish2_kernel, dim3(elementwise_grid(E, 256)),
                     dim3(256), 0, stream, rsum.data_ptr<float>(),
                     t.data_ptr<int>(), horizons.data_ptr<int>(),
                     epr.data_ptr<float>(), rewards.data_ptr<float>(),
                     dones.data_ptr<float>(), E, D, panels);
  if (fold)
    hipLaunchKernelGGL(env_xv_reduce_kernel,
                       dim3(elementwise_grid(E * 4, 256)), dim3(256), 0,
                       stream, xvp.data_ptr<float>(), xva.data_ptr<float>(),
                       E, K, panels);
}

void env_step_rows(torch::Tensor xva, torch::Tensor M, torch::Tensor xin,
                   torch::Tensor xout, torch::Tensor envd,
                   torch::Tensor horizons, torch::Tensor t,
                   torch::Tensor epr, torch::Tensor rewards,
                   torch::Tensor dones, torch::Tensor seed_dev, double sigma,
                   int64_t step, torch::Tensor V) {
  // gemm_env_step + the next step's x@V gemm_fwd in one launch, bitwise
  // equal to that pair (env_step_rows_kernel)
  const int64_t E = xva.size(0);
  const int K = static_cast<int>(xva.size(1));
  const int D = static_cast<int>(M.size(1));
  for (const auto& x : {xva, M, xin, xout, envd, epr, rewards, dones, V})
    TORCH_CHECK(x.is_cuda() && x.is_contiguous() &&
                x.scalar_type() == torch::kFloat);
  TORCH_CHECK(E >= 1 && xva.dim() == 2 && M.dim() == 2 && xin.dim() == 2);
  TORCH_CHECK(M.size(0) == K && xin.size(0) == E && xin.size(1) == D);
  TORCH_CHECK(xout.numel() == E * D && envd.numel() == D);
  TORCH_CHECK(K % 4 == 0 && K >= 16 && D % 4 == 0 && D >= 4,
              "env_step_rows needs 16B rows and a 16-column x@V block");
  TORCH_CHECK(V.dim() == 2 && V.size(0) == D && V.size(1) == 16,
              "env_step_rows needs V = [D][16]");
  TORCH_CHECK(horizons.is_cuda() && t.is_cuda() && horizons.is_contiguous() &&
              t.is_contiguous() && horizons.dtype() == torch::kInt32 &&
              t.dtype() == torch::kInt32);
  TORCH_CHECK(horizons.numel() == E && t.numel() == E && epr.numel() == E &&
              rewards.numel() == E && dones.numel() == E);
  TORCH_CHECK(seed_dev.is_cuda() && seed_dev.scalar_type() == torch::kLong &&
              seed_dev.numel() == 1);
  // (int)e feeds the RNG hash, as in gemm_env_step
  EnvRowsArgs m{};
  FwdArgs& a = m.g;
  a.X = xva.data_ptr<float>();
  a.Wt = M.data_ptr<float>();
  a.B = E;
  a.K = K;
  a.N = D;
  a.activation = 5;
  a.ldc = D;
  a.env_xin = xin.data_ptr<float>();
  a.env_x = xout.data_ptr<float>();
  a.envd = envd.data_ptr<float>();
  a.horizons = horizons.data_ptr<int>();
  a.tcount = t.data_ptr<int>();
  a.seed_dev = reinterpret_cast<const long long*>(seed_dev.data_ptr<int64_t>());
  a.env_V = V.data_ptr<float>();
  a.sigma = (float)sigma;
  a.step = (int)step;
  m.xva = xva.data_ptr<float>();
  m.t = t.data_ptr<int>();
  m.epr = epr.data_ptr<float>();
  m.rewards = rewards.data_ptr<float>();
  m.dones = dones.data_ptr<float>();
  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  const int64_t tiles = (E + FWD_M - 1) / FWD_M;
  TORCH_CHECK(tiles <= (1 << 22));
  hipLaunchKernelGGL(env_step_rows_kernel, dim3((unsigned)tiles),
                     dim3(FWD_WAVES * 64), 0, stream, m);
}

// Grow-only scratch cache for the dW split slabs.  Allocating them per
// call fragmented the caching allocator against hipGraph private pools
// (tests with several captured engines measured SECONDS per eager dW
// call in hipMalloc/hipFree); a persistent buffer also gives captures a
// stable address.  Correctness: every (split, element) of the used
// region is overwritten each call (splits are clamped so k0 < B).
static torch::Tensor& dw_scratch(int idx, int64_t need,
                                 const torch::TensorOptions& opt) {
  static torch::Tensor cache[2];
  static std::vector<torch::Tensor> retired;  // graphs captured against an
                                              // old buffer must keep it
                                              // alive (grow-only, bounded
                                              // by the few distinct sizes)
  torch::Tensor& t = cache[idx];
  if (!t.defined() || t.numel() < need) {
    if (t.defined()) retired.push_back(t);
    t = torch::empty({need}, opt);
  }
  return t;
}

void dw_mfma(torch::Tensor delta, torch::Tensor acts, torch::Tensor grad_buf,
             int64_t w_off, int64_t b_off, int64_t split_row, int64_t w_off2,
             int64_t b_off2, int64_t ablate) {
  const int64_t B = delta.size(0);
  const int out_dim = static_cast<int>(delta.size(1));
  const int in_dim = static_cast<int>(acts.size(1));
  TORCH_CHECK(delta.is_contiguous() && acts.is_contiguous());

  DwArgs a{};
  a.delta = delta.data_ptr<float>();
  a.acts = acts.data_ptr<float>();
  a.B = B;
  a.out_dim = out_dim;
  a.in_dim = in_dim;
  a.ablate = static_cast<int>(ablate);
  // tile shape: maximize N per wave to avoid re-reading delta; wide
  // out_dim also takes 2 row fragments per wave (halves acts re-reads)
  // Wide out_dim: 2 row fragments with NT capped at 2 keeps the
  // accumulators at 64 AGPR (4 waves/SIMD) while halving the streamed
  // acts re-reads (MT=2 with NT=4 = 128 AGPR measured 17x stalls).
  const int mt = (out_dim >= 64) ? 2 : 1;
  a.nt = std::min(mt == 2 ? 2 : MAX_NT, (in_dim + M_WAVE - 1) / M_WAVE);
  const int m_tiles = (out_dim + M_WAVE * mt - 1) / (M_WAVE * mt);
  const int n_tiles = (in_dim + a.nt * M_WAVE - 1) / (a.nt * M_WAVE);

  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  static const int dwglds_env = env_int("DPPO_DW_GLDS", 1);
  // 8-wave LDS-staged variant: whole dW tile per block, delta read once
  // <2,4,3> covers wide-acts tiles (dW1: in=obs); <2,2,1> covers the
  // narrow [<=64][<=64] shapes (dW2, padded heads dW)
  const bool glds_wide = in_dim > 192 && in_dim <= 384;
  const bool glds_narrow = in_dim <= 64 && out_dim <= 64;
  const bool glds = dwglds_env && !a.ablate && out_dim <= 64 &&
                    (glds_wide || glds_narrow) && out_dim % 4 == 0 &&
                    in_dim % 4 == 0 && B >= 4096;
  if (glds) {
    // re-read per call: sweepable
    const int64_t split_cap = env_int("DPPO_DW_SPLITS", 1024);
    a.splits = static_cast<int>(
        std::min<int64_t>(split_cap, std::max<int64_t>(256, B / 4096)));
    a.splits = static_cast<int>(
        std::min<int64_t>(a.splits, std::max<int64_t>(1, B / DWG_K)));
    // no empty trailing split: dw_glds_kernel returns early on one and
    // leaves its slab rows unwritten for the reduce (B = 4099 with 256
    // splits of 17 rows left 14 of them stale)
    const int64_t rows_per = (B + a.splits - 1) / a.splits;
    a.splits = static_cast<int>((B + rows_per - 1) / rows_per);
  } else {
    // enough waves to hide the streamed-operand latency; slab stores make
    // extra splits nearly free (the reduce is split-chunk parallel)
    const int target_blocks = 4096;
    a.splits = std::max(1, target_blocks / std::max(1, m_tiles * n_tiles));
    a.splits = static_cast<int>(
        std::min<int64_t>(a.splits, std::max<int64_t>(1, B / 256)));
  }

  auto& slab = dw_scratch(0, (int64_t)a.splits * out_dim * in_dim,
                          delta.options());
  auto& db_slab = dw_scratch(1, (int64_t)a.splits * out_dim,
                             delta.options());
  // every used element is overwritten by the split grid, but a db tail
  // beyond this call's splits must not leak: zero the region
  db_slab.narrow(0, 0, (int64_t)a.splits * out_dim).zero_();
  a.slab = slab.data_ptr<float>();
  a.db_slab = db_slab.data_ptr<float>();

  if (glds && glds_wide) {
    // single 384-wide tile, 5-deep ring (measured: 2-panel <2,2,3,4>
    // grids with 2 blocks/CU ran 6% SLOWER — the duplicated delta
    // stage and shorter MFMA chains cost more than the cross-block
    // barrier overlap bought; both are ~60% of the f32-MFMA floor)
    hipLaunchKernelGGL((dw_glds_kernel<2, 4, 3, 5>),
                       dim3((unsigned)a.splits, 1), dim3(512), 0, stream, a);
  } else if (glds) {
    hipLaunchKernelGGL((dw_glds_kernel<2, 2, 1>), dim3((unsigned)a.splits),
                       dim3(256), 0, stream, a);
  } else {
    const dim3 grid(m_tiles, n_tiles, a.splits);
    const int key = a.nt * 10 + mt;
    switch (key) {
      case 11: hipLaunchKernelGGL((dw_mfma_kernel<1, 1>), grid, dim3(WAVE), 0, stream, a); break;
      case 21: hipLaunchKernelGGL((dw_mfma_kernel<2, 1>), grid, dim3(WAVE), 0, stream, a); break;
      case 31: hipLaunchKernelGGL((dw_mfma_kernel<3, 1>), grid, dim3(WAVE), 0, stream, a); break;
      case 41: hipLaunchKernelGGL((dw_mfma_kernel<4, 1>), grid, dim3(WAVE), 0, stream, a); break;
      case 12: hipLaunchKernelGGL((dw_mfma_kernel<1, 2>), grid, dim3(WAVE), 0, stream, a); break;
      case 22: hipLaunchKernelGGL((dw_mfma_kernel<2, 2>), grid, dim3(WAVE), 0, stream, a); break;
      case 32: hipLaunchKernelGGL((dw_mfma_kernel<3, 2>), grid, dim3(WAVE), 0, stream, a); break;
      default: hipLaunchKernelGGL((dw_mfma_kernel<4, 2>), grid, dim3(WAVE), 0, stream, a); break;
    }
  }

  float* dW = grad_buf.data_ptr<float>() + w_off;
  float* db = (b_off >= 0) ? grad_buf.data_ptr<float>() + b_off : nullptr;
  float* dW2 = (split_row >= 0) ? grad_buf.data_ptr<float>() + w_off2 : nullptr;
  float* db2 = (split_row >= 0 && b_off2 >= 0)
                   ? grad_buf.data_ptr<float>() + b_off2
                   : nullptr;
  const int n_chunks = (a.splits + DW_RED_CHUNK - 1) / DW_RED_CHUNK;
  const dim3 rgrid(elementwise_grid((int64_t)out_dim * in_dim, 256), n_chunks);
  hipLaunchKernelGGL(dw_reduce_kernel, rgrid, dim3(256), 0, stream, a.slab,
                     a.db_slab, dW, db, dW2, db2, out_dim, in_dim, a.splits,
                     static_cast<int>(split_row));
  hipLaunchKernelGGL(db_reduce_kernel, dim3(out_dim), dim3(WAVE), 0, stream,
                     a.db_slab, db, db2, out_dim, a.splits,
                     static_cast<int>(split_row));
}
