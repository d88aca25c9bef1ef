// Fused middle of the MLP update step (gfx950): from the layer-1
// activations to dz1 without the per-row intermediates ever leaving the
// CU.
//
// One update step of the two-hidden-layer Box policy used to run, between
// the L1 forward and dW1:  ppo_gh_tile_kernel -> dgrad heads -> dgrad L2 ->
// dW2 (+reduce) -> heads dW (+reduce), with gh [B][36] and dz2 [B][64]
// each written to HBM once and read back twice.  The PPO gradient of a row
// depends on that row alone, so here a wave takes 32 rows from
// (h1, h2, pdflat, v, loss inputs) to dz1 on-chip:
//
//   gh   = d loss / d [pd | v]            (ppo_math.h, serial j order)
//   dWh += gh^T . h2        dbh += sum gh
//   dz2  = act'(h2) * (gh . Wh)
//   dW2 += dz2^T . h1       db2 += sum dz2
//   dz1  = act'(h1) * (dz2 . W2)          -> HBM, for dW1
//
// All four products are v_mfma_f32_32x32x2_f32 (fragment layout:
// mfma_frag.h).  What makes it cheap is that the MFMA C layout (lane =
// column, the 16 registers = rows) is also the A/B layout of a product
// that sums over ROWS: h1 and h2 are loaded from HBM straight into that
// layout (coalesced 128-B row segments, no LDS) and serve as the B operand
// of the two dW products and as the act' factor of the two dgrad
// epilogues; the dz2 accumulators are the A operand of dW2 as they stand.
// Only the two row-parallel products need a lane = row operand: gh is
// built that way in LDS (one lane per row), and dz2 takes one trip through
// a per-wave [32][H2+1] LDS image.  Every LDS image is private to its wave,
// so the row loop has no block barrier.
//
// Grid is persistent: each wave walks row tiles with a grid stride and
// keeps its dW2/dWh/db partials in registers; at the end it writes one
// slab with plain stores and mid_reduce_kernel folds the slabs into the
// flat grad (rows < P of the heads slab -> Wp/bp, row P -> Wv/bv; pad rows
// and columns are never stored).  No float atomics in the mid kernel.
//
// The slab is per WAVE, not per block (1024 slabs, ~26 MB written and read
// back per step on the flagship shape, against the GBs of gh/dz2 traffic
// removed): each wave holds the full dW2/dWh accumulators for its own 32
// rows, so a per-block slab would need a cross-wave reduction through LDS
// at the end for no measurable saving.  The other arrangement the design
// allowed -- waves splitting the dW tiles and contracting over all 128
// rows, 16-32 accumulator registers and one block barrier per tile -- was
// not built, so there is no measurement against it; it is the route to two
// waves per SIMD if this kernel is taken further.
//
// h2, pdflat and v are read from memory (the LOAD operand mode).  A
// RECOMPUTE mode that rebuilt them on-chip from the h1 tile (two more MFMA
// products and two more trips through the per-wave LDS image, no L2 /
// heads forward in the update) was built, passed the same tests and was
// measured: 11.97 ms against 7.79 + 4.49 ms for this kernel plus the
// forward it drops, and a slower bench.py round in every alternated run.
// It was removed again; figures in profiles/r05_update_mid_fused.txt.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <c10/hip/HIPStream.h>

#include "common.h"
#include "mfma_frag.h"
#include "ppo_math.h"

namespace {

constexpr int MID_WAVES = 4;
constexpr int MID_ROWS = 32;                     // rows per wave tile
constexpr int MID_TILE = MID_WAVES * MID_ROWS;   // rows per block tile
constexpr int MID_GRID = N_CU;                   // one block per CU (below)
constexpr int MID_SPLITS = MID_GRID * MID_WAVES; // one slab per wave
constexpr int MID_RED_CHUNK = 32;

struct MidArgs {
  const float* h1;       // [B][H1]
  const float* h2;       // [B][H2]
  const float* pd;       // [B][P]
  const float* v;        // [B]
  const float* oldflat;  // [B][P]
  const float* oldv;     // [B]
  const float* act;      // [B][A]
  const float* adv;      // [B]
  const float* etr;      // [B]
  const float* W2;       // [H2][H1] torch layout
  const float* Wp;       // [P][H2]
  const float* Wv;       // [1][H2]
  const float* clip_dev; // nullptr -> `clip`
  float* dz1;            // [B][H1]
  float* slab_w2;        // [MID_SPLITS][H2][H1]
  float* slab_b2;        // [MID_SPLITS][H2]
  float* slab_wh;        // [MID_SPLITS][P+1][H2]
  float* slab_bh;        // [MID_SPLITS][P+1]
  int64_t B;
  int64_t n_tiles;
  int A;
  int act_code;          // 0 relu, 1 tanh
  int vec_ok;            // pd/oldflat/act base pointers are 16-B aligned
  float clip, entcoeff, vcoeff;
};

// wave-local LDS hand-over: DS ops of one wave execute in order, so all
// that is needed is that the compiler keeps them in program order
DEV_INLINE void wave_lds_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// rows*w contiguous floats -> LDS rows of stride `ld` (this wave's lanes)
DEV_INLINE void stage_rows(const float* __restrict__ src, float* dst, int w,
                           int ld, int n, float inv_w, int lane) {
  for (int e = lane; e < n; e += WAVE) {
    const int r = __float2int_rz((e + 0.5f) * inv_w);
    dst[r * ld + (e - r * w)] = src[e];
  }
}

// 16-B loads of n4 float4 (this wave's contiguous rows) into registers ...
template <int MAXV>
DEV_INLINE void stage_load4(const float* __restrict__ src, int n4, int lane,
                            float4 (&t)[MAXV]) {
  const float4* s4 = reinterpret_cast<const float4*>(src);
  #pragma unroll
  for (int u = 0; u < MAXV; ++u) {
    const int i = lane + u * WAVE;
    if (i < n4) t[u] = s4[i];
  }
}

// ... and from there into LDS rows of w floats at stride ld
template <int MAXV>
DEV_INLINE void stage_write4(const float4 (&t)[MAXV], float* dst, int w,
                             int ld, int n4, float inv_w, int lane) {
  #pragma unroll
  for (int u = 0; u < MAXV; ++u) {
    const int i = lane + u * WAVE;
    if (i < n4) {
      const int e = 4 * i;
      int r = __float2int_rz((e + 0.5f) * inv_w);
      int cc = e - r * w;
      const float vv[4] = {t[u].x, t[u].y, t[u].z, t[u].w};
      #pragma unroll
      for (int k = 0; k < 4; ++k) {
        dst[r * ld + cc] = vv[k];
        if (++cc == w) { cc = 0; ++r; }
      }
    }
  }
}

// One wave per SIMD: the <2,2,2> instantiation holds 128 accumulator
// registers plus the h1/h2/dz2 tiles (256 VGPR + 189 AGPR of the 512, no
// scratch); with __launch_bounds__(256, 2) an earlier build of it spilled
// 632 B/lane.  The LDS (78 KB on the flagship shape) would admit two
// blocks per CU, the registers do not.  Resource lines per instantiation:
// profiles/r05_update_mid_fused.txt.
template <int NT1, int NT2, int NPT>
__launch_bounds__(MID_WAVES * WAVE, 1)
__global__ void mlp_mid_kernel(MidArgs a) {
  constexpr int H1 = NT1 * 32, H2 = NT2 * 32;
  constexpr int LD1 = H1 + 1, LD2 = H2 + 1;
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  const int lane0 = tid & (WAVE - 1);
  const int wave = tid / WAVE;
  const int A = a.A, P = 2 * A, NH = P + 1;
  const int KP = P + 2;   // heads contraction length, padded to even
  const int sg = P + 3;   // gh row stride (odd); columns NH.. are zero
  const int sp = P + 1;   // pdflat row stride (odd)
  const int sa = A | 1;   // action row stride (odd)
  // mirrored on the host (lds_bytes)
  const int un_floats = max(MID_ROWS * LD2, MID_ROWS * (sp + sa + 4));

  float* w2s = lds;                 // [H2][LD1]
  float* whs = w2s + H2 * LD1;      // [KP][LD2], rows >= NH zero
  float* wv_base = whs + KP * LD2;
  float* og = wv_base + wave * (MID_ROWS * sg + un_floats);  // [32][sg]
  float* un = og + MID_ROWS * sg;   // staging, later the dz2 image
  float* l_pd = un;                 // [32][sp]
  float* l_ac = l_pd + MID_ROWS * sp;   // [32][sa]
  float* l_sc = l_ac + MID_ROWS * sa;   // [4][32]: v | oldv | adv | etr

  float clip = a.clip;
  if (a.clip_dev != nullptr) clip = a.clip_dev[0];

  for (int i = tid; i < H2 * H1; i += MID_WAVES * WAVE)
    w2s[(i / H1) * LD1 + (i % H1)] = a.W2[i];
  for (int i = tid; i < KP * H2; i += MID_WAVES * WAVE) {
    const int p = i / H2, n = i % H2;
    whs[p * LD2 + n] =
        p < P ? a.Wp[i] : (p == P ? a.Wv[n] : 0.f);
  }
  __syncthreads();

  f32x16 dW2[NT2][NT1], dWh[NPT][NT2];
  float db2[NT2], dbh[NPT];
  #pragma unroll
  for (int m = 0; m < NT2; ++m) {
    db2[m] = 0.f;
    #pragma unroll
    for (int n = 0; n < NT1; ++n)
      #pragma unroll
      for (int r = 0; r < 16; ++r) dW2[m][n][r] = 0.f;
  }
  #pragma unroll
  for (int m = 0; m < NPT; ++m) {
    dbh[m] = 0.f;
    #pragma unroll
    for (int n = 0; n < NT2; ++n)
      #pragma unroll
      for (int r = 0; r < 16; ++r) dWh[m][n][r] = 0.f;
  }

  const float inv_p = 1.f / (float)P, inv_a = 1.f / (float)A;

  for (int64_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
    const int64_t rb = tile * MID_TILE + (int64_t)wave * MID_ROWS;
    const int nrows = (int)max((int64_t)0, min((int64_t)MID_ROWS, a.B - rb));

    // ---- loss inputs of this wave's rows -> registers -> LDS rows.
    // Every one of these loads is issued before the first LDS write waits
    // on one, so the memory latency is paid once per tile and not once per
    // load: with a load->ds_write loop the kernel took 13.3 ms at B = 16.8M
    // (about 62k cycles per tile, against 14.6k of MFMA issue), with the
    // batched loads 7.8 ms (profiles/r05_update_mid_fused.txt).
    const bool vec = a.vec_ok && nrows == MID_ROWS;
    // every LDS and row address below depends on the lane alone; left
    // visible, the compiler hoists some hundred of them out of the tile
    // loop and keeps them in registers next to the accumulators (spills).
    // Launder the lane id so they are recomputed per tile.
    int lane = lane0;
    asm volatile("" : "+v"(lane));
    const int c = lane & 31, half = lane >> 5;
    float4 pd4[8], og4[8], ac4[4];
    float sc2[2];
    if (vec) {
      stage_load4(a.pd + rb * P, 8 * P, lane, pd4);
      stage_load4(a.oldflat + rb * P, 8 * P, lane, og4);
      stage_load4(a.act + rb * A, 8 * A, lane, ac4);
    }
    #pragma unroll
    for (int u = 0; u < 2; ++u) {
      const float* src = u == 0 ? (half ? a.oldv : a.v)
                                : (half ? a.etr : a.adv);
      sc2[u] = c < nrows ? src[rb + c] : 0.f;
    }

    if (vec) {
      stage_write4(pd4, l_pd, P, sp, 8 * P, inv_p, lane);
      stage_write4(og4, og, P, sg, 8 * P, inv_p, lane);
      stage_write4(ac4, l_ac, A, sa, 8 * A, inv_a, lane);
    } else {  // row tail / unaligned views: element-wise
      stage_rows(a.pd + rb * P, l_pd, P, sp, nrows * P, inv_p, lane);
      stage_rows(a.oldflat + rb * P, og, P, sg, nrows * P, inv_p, lane);
      stage_rows(a.act + rb * A, l_ac, A, sa, nrows * A, inv_a, lane);
    }
    l_sc[lane] = sc2[0];        // [v | oldv]
    l_sc[WAVE + lane] = sc2[1]; // [adv | etr]
    wave_lds_sync();

    // ---- h1 / h2 straight into the C layout ----
    // Issued only now, so that the staging registers above are dead (all
    // of them live at once spilled); the gh pass below covers the latency.
    float h1r[NT1][16], h2r[NT2][16];
    #pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = cd_row(r, lane);
      const bool ok = row < nrows;
      const int64_t g = ok ? rb + row : 0;
      #pragma unroll
      for (int t = 0; t < NT2; ++t) {
        const float x = a.h2[g * H2 + 32 * t + c];
        h2r[t][r] = ok ? x : 0.f;
      }
      #pragma unroll
      for (int t = 0; t < NT1; ++t) {
        const float x = a.h1[g * H1 + 32 * t + c];
        h1r[t][r] = ok ? x : 0.f;
      }
    }


    // ---- gh rows (ppo_gh_tile_kernel's math, same serial j order).
    // Lanes c and c+32 share row c: the lower half sums the pi terms, the
    // upper half the old-policy terms, then each writes every other j.
    {
      const float* pdr = l_pd + c * sp;
      const float* ac = l_ac + c * sa;
      float* ghr = og + c * sg;
      const float* pr = half ? ghr : pdr;
      float s1 = 0.f, s2 = 0.f;
      // rows >= nrows read unwritten LDS here; their results are discarded
      // (the c < nrows branch below writes zeros for them)
      #pragma unroll 4
      for (int j = 0; j < A; ++j) {
        const float ls = pr[A + j];
        const float z = (ac[j] - pr[j]) * __expf(-ls);
        s1 += -0.5f * z * z - ls;
        s2 += ls;
      }
      const float cc = 0.5f * PPO_LOG_2PI * A;
      GaussRow row;
      row.logp_pi = __shfl(s1, c, WAVE) - cc;
      row.logp_old = __shfl(s1, c + 32, WAVE) - cc;
      row.ent = __shfl(s2, c, WAVE) + 0.5f * (PPO_LOG_2PI + 1.f) * A;
      const PPORowGrads g = ppo_row_grads(
          row, l_sc[c], l_sc[MID_ROWS + c], l_sc[WAVE + c],
          l_sc[WAVE + MID_ROWS + c], a.B, clip, a.entcoeff, a.vcoeff, 1.f);
      wave_lds_sync();  // the old-policy row is read; gh may overwrite it
      if (c < nrows) {
        #pragma unroll 4
        for (int j = half; j < A; j += 2) {
          const float lsp = pdr[A + j];
          const float inv_s = __expf(-lsp);
          const float z = (ac[j] - pdr[j]) * inv_s;
          ghr[j] = g.g_logp * z * inv_s;
          ghr[A + j] = g.g_logp * (z * z - 1.f) + g.g_ent;
        }
        if (half == 0) ghr[P] = g.g_v;
        else { ghr[P + 1] = 0.f; ghr[P + 2] = 0.f; }
      } else {
        for (int j = half; j < sg; j += 2) ghr[j] = 0.f;  // pad rows: nothing
      }
    }
    wave_lds_sync();

    // ---- dWh += gh^T . h2, dbh += sum gh (sum over rows: C layouts) ----
    #pragma unroll
    for (int m = 0; m < NPT; ++m) {
      const int col = min(32 * m + c, NH);  // column NH is zero
      float ghc[16];
      #pragma unroll
      for (int r = 0; r < 16; ++r) ghc[r] = og[cd_row(r, lane) * sg + col];
      float s = 0.f;
      #pragma unroll
      for (int r = 0; r < 16; ++r) s += ghc[r];
      dbh[m] += s;
      #pragma unroll
      for (int r = 0; r < 16; ++r)
        #pragma unroll
        for (int n = 0; n < NT2; ++n)
          dWh[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(
              ghc[r], h2r[n][r], dWh[m][n], 0, 0, 0);
    }

    // ---- dz2 = act'(h2) * (gh . Wh) ----
    f32x16 dz2[NT2];
    #pragma unroll
    for (int t = 0; t < NT2; ++t)
      #pragma unroll
      for (int r = 0; r < 16; ++r) dz2[t][r] = 0.f;
    #pragma unroll 6
    for (int k = half; k < KP; k += 2) {
      const float av = og[c * sg + k];
      #pragma unroll
      for (int t = 0; t < NT2; ++t)
        dz2[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(
            av, whs[k * LD2 + 32 * t + c], dz2[t], 0, 0, 0);
    }
    #pragma unroll
    for (int t = 0; t < NT2; ++t) {
      float s = 0.f;
      #pragma unroll
      for (int r = 0; r < 16; ++r) {
        dz2[t][r] *= act_grad(h2r[t][r], a.act_code == 1);
        s += dz2[t][r];
      }
      db2[t] += s;
    }

    // ---- dW2 += dz2^T . h1 ----
    #pragma unroll
    for (int r = 0; r < 16; ++r)
      #pragma unroll
      for (int m = 0; m < NT2; ++m)
        #pragma unroll
        for (int n = 0; n < NT1; ++n)
          dW2[m][n] = __builtin_amdgcn_mfma_f32_32x32x2f32(
              dz2[m][r], h1r[n][r], dW2[m][n], 0, 0, 0);

    // ---- dz2 -> lane = row image (the staging area is dead by now) ----
    #pragma unroll
    for (int t = 0; t < NT2; ++t)
      #pragma unroll
      for (int r = 0; r < 16; ++r)
        un[cd_row(r, lane) * LD2 + 32 * t + c] = dz2[t][r];
    wave_lds_sync();

    // ---- dz1 = act'(h1) * (dz2 . W2) ----
    f32x16 dz1[NT1];
    #pragma unroll
    for (int t = 0; t < NT1; ++t)
      #pragma unroll
      for (int r = 0; r < 16; ++r) dz1[t][r] = 0.f;
    #pragma unroll 8
    for (int k = half; k < H2; k += 2) {
      const float av = un[c * LD2 + k];
      #pragma unroll
      for (int t = 0; t < NT1; ++t)
        dz1[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(
            av, w2s[k * LD1 + 32 * t + c], dz1[t], 0, 0, 0);
    }
    #pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = cd_row(r, lane);
      if (row < nrows) {
        #pragma unroll
        for (int t = 0; t < NT1; ++t)
          a.dz1[(rb + row) * H1 + 32 * t + c] =
              dz1[t][r] * act_grad(h1r[t][r], a.act_code == 1);
      }
    }
    wave_lds_sync();  // next tile's staging overwrites og / un
  }

  // ---- one slab per wave, plain stores ----
  const int lane = lane0, c = lane & 31, half = lane >> 5;
  const int64_t sidx = (int64_t)blockIdx.x * MID_WAVES + wave;
  float* sw2 = a.slab_w2 + sidx * (H2 * H1);
  #pragma unroll
  for (int m = 0; m < NT2; ++m)
    #pragma unroll
    for (int n = 0; n < NT1; ++n)
      #pragma unroll
      for (int r = 0; r < 16; ++r)
        sw2[(32 * m + cd_row(r, lane)) * H1 + 32 * n + c] = dW2[m][n][r];
  float* swh = a.slab_wh + sidx * ((int64_t)NH * H2);
  #pragma unroll
  for (int m = 0; m < NPT; ++m)
    #pragma unroll
    for (int n = 0; n < NT2; ++n)
      #pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = 32 * m + cd_row(r, lane);
        if (row < NH) swh[row * H2 + 32 * n + c] = dWh[m][n][r];
      }
  #pragma unroll
  for (int t = 0; t < NT2; ++t) {
    const float s = db2[t] + __shfl_xor(db2[t], 32, WAVE);
    if (half == 0) a.slab_b2[sidx * H2 + 32 * t + c] = s;
  }
  #pragma unroll
  for (int m = 0; m < NPT; ++m) {
    const float s = dbh[m] + __shfl_xor(dbh[m], 32, WAVE);
    if (half == 0 && 32 * m + c < NH) a.slab_bh[sidx * NH + 32 * m + c] = s;
  }
}

// Slab reduction into the flat grad, parallel over (element, split
// chunk) like dw_reduce_kernel.  blockIdx.z picks the segment: 0 W2,
// 1 b2, 2 heads W (rows < P -> Wp, row P -> Wv), 3 heads b.
struct MidRedArgs {
  const float* slab[4];
  float* dst[4];    // W2, b2, Wp, bp
  float* dst2[2];   // Wv, bv
  int n[4];
  int split_at[2];  // element index where the heads slab turns to Wv / bv
  int splits;
};

__global__ void mid_reduce_kernel(MidRedArgs a) {
  const int z = blockIdx.z;
  const int n = a.n[z];
  const float* slab = a.slab[z];
  const int s0 = blockIdx.y * MID_RED_CHUNK;
  const int s1 = min(a.splits, s0 + MID_RED_CHUNK);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += gridDim.x * blockDim.x) {
    float acc = 0.f;
    for (int s = s0; s < s1; ++s) acc += slab[(int64_t)s * n + i];
    float* dst = a.dst[z] + i;
    if (z >= 2 && i >= a.split_at[z - 2])
      dst = a.dst2[z - 2] + (i - a.split_at[z - 2]);
    atomicAdd(dst, acc);
  }
}

// Persistent slab scratch: stable address for captured graphs, no
// allocator traffic per step (same reasoning as dw_scratch).
torch::Tensor& mid_scratch(int64_t need, const torch::TensorOptions& opt) {
  static torch::Tensor cache;
  static std::vector<torch::Tensor> retired;
  if (!cache.defined() || cache.numel() < need) {
    if (cache.defined()) retired.push_back(cache);
    cache = torch::empty({need}, opt);
  }
  return cache;
}

template <int NT1, int NT2, int NPT>
void launch_mid(const MidArgs& a, int lds_bytes, hipStream_t stream) {
  static bool attr_set = false;
  if (!attr_set) {
    C10_HIP_CHECK(hipFuncSetAttribute(
        reinterpret_cast<const void*>(&mlp_mid_kernel<NT1, NT2, NPT>),
        hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set = true;
  }
  hipLaunchKernelGGL((mlp_mid_kernel<NT1, NT2, NPT>), dim3(MID_GRID),
                     dim3(MID_WAVES * WAVE), lds_bytes, stream, a);
}

}  // namespace

bool mlp_mid_supported(int64_t H1, int64_t H2, int64_t A, int64_t n_hidden) {
  return n_hidden == 2 && (H1 == 32 || H1 == 64) && (H2 == 32 || H2 == 64) &&
         A >= 1 && 2 * A + 1 <= 63;
}

void mlp_mid_bwd(torch::Tensor params, std::vector<int64_t> offsets,
                 torch::Tensor h1, torch::Tensor h2, torch::Tensor pdflat,
                 torch::Tensor v, torch::Tensor oldflat, torch::Tensor oldv,
                 torch::Tensor act, torch::Tensor adv, torch::Tensor etr,
                 int64_t activation, torch::Tensor clip_dev, double clip,
                 double entcoeff, double vcoeff, torch::Tensor dz1,
                 torch::Tensor grad) {
  const int64_t B = h1.size(0);
  const int H1 = static_cast<int>(h1.size(1));
  const int H2 = static_cast<int>(h2.size(1));
  const int A = static_cast<int>(act.size(1));
  const int P = 2 * A, NH = P + 1;
  TORCH_CHECK(mlp_mid_supported(H1, H2, A, 2),
              "mlp_mid_bwd: unsupported shape H1=", H1, " H2=", H2, " A=", A);
  TORCH_CHECK(offsets.size() == 8, "mlp_mid_bwd: expects 8 param offsets");
  TORCH_CHECK(activation == 0 || activation == 1);
  TORCH_CHECK(params.scalar_type() == torch::kFloat32 &&
              h1.scalar_type() == torch::kFloat32);
  for (const auto& t : {h1, h2, pdflat, v, oldflat, oldv, act, adv, etr, dz1,
                        params, grad})
    TORCH_CHECK(t.is_contiguous() && t.is_cuda());
  TORCH_CHECK(h2.size(0) == B && pdflat.size(0) == B && pdflat.size(1) == P &&
              oldflat.size(0) == B && oldflat.size(1) == P &&
              v.numel() == B && oldv.numel() == B && act.size(0) == B &&
              adv.numel() == B && etr.numel() == B && dz1.size(0) == B &&
              dz1.size(1) == H1 && grad.numel() == params.numel());
  if (B == 0) return;

  const int64_t n_w2 = (int64_t)H2 * H1, n_wh = (int64_t)NH * H2;
  auto& slab = mid_scratch(MID_SPLITS * (n_w2 + H2 + n_wh + NH), h1.options());

  MidArgs a{};
  a.h1 = h1.data_ptr<float>();
  a.h2 = h2.data_ptr<float>();
  a.pd = pdflat.data_ptr<float>();
  a.v = v.data_ptr<float>();
  a.oldflat = oldflat.data_ptr<float>();
  a.oldv = oldv.data_ptr<float>();
  a.act = act.data_ptr<float>();
  a.adv = adv.data_ptr<float>();
  a.etr = etr.data_ptr<float>();
  const float* p = params.data_ptr<float>();
  // flat layout: W1 b1 W2 b2 Wv bv Wp bp
  a.W2 = p + offsets[2];
  a.Wv = p + offsets[4];
  a.Wp = p + offsets[6];
  a.clip_dev = clip_dev.numel() > 0 ? clip_dev.data_ptr<float>() : nullptr;
  a.dz1 = dz1.data_ptr<float>();
  a.slab_w2 = slab.data_ptr<float>();
  a.slab_b2 = a.slab_w2 + MID_SPLITS * n_w2;
  a.slab_wh = a.slab_b2 + MID_SPLITS * (int64_t)H2;
  a.slab_bh = a.slab_wh + MID_SPLITS * n_wh;
  a.B = B;
  a.n_tiles = (B + MID_TILE - 1) / MID_TILE;
  a.A = A;
  a.act_code = static_cast<int>(activation);
  a.vec_ok = ((reinterpret_cast<uintptr_t>(a.pd) |
               reinterpret_cast<uintptr_t>(a.oldflat) |
               reinterpret_cast<uintptr_t>(a.act)) & 15) == 0;
  a.clip = static_cast<float>(clip);
  a.entcoeff = static_cast<float>(entcoeff);
  a.vcoeff = static_cast<float>(vcoeff);

  const int sg = P + 3, sp = P + 1, sa = A | 1;
  const int un_floats =
      std::max(MID_ROWS * (H2 + 1), MID_ROWS * (sp + sa + 4));
  const int lds_bytes =
      (H2 * (H1 + 1) + (P + 2) * (H2 + 1) +
       MID_WAVES * (MID_ROWS * sg + un_floats)) * (int)sizeof(float);
  TORCH_CHECK(lds_bytes <= 160 * 1024);

  hipStream_t stream = c10::hip::getCurrentHIPStream().stream();
  const int npt = (NH + 31) / 32;
  const int key = (H1 / 32) * 100 + (H2 / 32) * 10 + npt;
  switch (key) {
    case 111: launch_mid<1, 1, 1>(a, lds_bytes, stream); break;
    case 112: launch_mid<1, 1, 2>(a, lds_bytes, stream); break;
    case 121: launch_mid<1, 2, 1>(a, lds_bytes, stream); break;
    case 122: launch_mid<1, 2, 2>(a, lds_bytes, stream); break;
    case 211: launch_mid<2, 1, 1>(a, lds_bytes, stream); break;
    case 212: launch_mid<2, 1, 2>(a, lds_bytes, stream); break;
    case 221: launch_mid<2, 2, 1>(a, lds_bytes, stream); break;
    default:  launch_mid<2, 2, 2>(a, lds_bytes, stream); break;
  }

  float* g = grad.data_ptr<float>();
  MidRedArgs r{};
  r.slab[0] = a.slab_w2; r.dst[0] = g + offsets[2]; r.n[0] = (int)n_w2;
  r.slab[1] = a.slab_b2; r.dst[1] = g + offsets[3]; r.n[1] = H2;
  r.slab[2] = a.slab_wh; r.dst[2] = g + offsets[6]; r.n[2] = (int)n_wh;
  r.slab[3] = a.slab_bh; r.dst[3] = g + offsets[7]; r.n[3] = NH;
  r.dst2[0] = g + offsets[4]; r.split_at[0] = P * H2;
  r.dst2[1] = g + offsets[5]; r.split_at[1] = P;
  r.splits = MID_SPLITS;
  const dim3 rgrid((unsigned)((n_w2 + 255) / 256),
                   (MID_SPLITS + MID_RED_CHUNK - 1) / MID_RED_CHUNK, 4);
  hipLaunchKernelGGL(mid_reduce_kernel, rgrid, dim3(256), 0, stream, r);
}
