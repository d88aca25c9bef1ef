// The output blob of every whole-rollout path, defined once.
//
// One float blob holds a rollout's results:
//   states[T][E][D] | pd params[T][E][P] | actions[T][E][actw] | values[T][E]
//   | rewards[T][E] | dones[T][E] | boot[E] | moments[5]
// The families with int64 actions (Categorical, MultiCategorical) have no
// float action region: their int64 [T][E][actw] region, 2*T*E*actw floats
// wide, leads the blob so it is 8-byte aligned.
//
// The launchers take their blob size and views from this struct; the engine's
// mirror is dppo_amd/ops/rollout_blob.py (tests/test_gpu_rollout_blob.py
// holds the two together).  rollout_kernel and classic_rollout_kernel still
// spell the same carve out themselves, because taking the offsets from the
// struct moved their generated code; the kernels write through their own
// carve and the tests read through these views, so the rollout tests'
// comparisons of every region (and test_gpu_rng_pin.py's pinned bits) fail if
// the two disagree.
#pragma once

#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include <cstdint>
#include <vector>

struct RolloutBlob {
  // float offsets into the blob
  int64_t actions, states, pd, values, rewards, dones, boot, moments, total;
  int64_t T, E, D, P, actw;
  bool int_actions;
};

__host__ __device__ inline RolloutBlob rollout_blob(int64_t T, int64_t E,
                                                    int64_t D, int64_t P,
                                                    int64_t actw,
                                                    bool int_actions) {
  RolloutBlob b;
  b.T = T; b.E = E; b.D = D; b.P = P; b.actw = actw;
  b.int_actions = int_actions;
  const int64_t TE = T * E;
  int64_t o = 0;
  if (int_actions) { b.actions = o; o += 2 * TE * actw; }
  b.states = o; o += TE * D;
  b.pd = o; o += TE * P;
  if (!int_actions) { b.actions = o; o += TE * actw; }
  b.values = o; o += TE;
  b.rewards = o; o += TE;
  b.dones = o; o += TE;
  b.boot = o;
  b.moments = b.boot + E;
  b.total = b.boot + E + 5;
  return b;
}

// ---- host helpers for the launchers ----------------------------------------

// The blob a launcher writes: out_buf when the caller sized it exactly (a
// persistent blob keeps the addresses stable for the hipGraph-captured
// update), else a fresh tensor like `like`.
inline torch::Tensor rollout_blob_tensor(const RolloutBlob& b,
                                         const torch::Tensor& out_buf,
                                         const torch::Tensor& like) {
  torch::Tensor out = (out_buf.numel() == b.total)
                          ? out_buf
                          : torch::empty({b.total}, like.options());
  TORCH_CHECK(out.is_cuda() && out.dtype() == torch::kFloat32 &&
                  out.is_contiguous(),
              "rollout output blob must be a contiguous f32 GPU tensor");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(out.data_ptr<float>()) % 8 == 0,
              "rollout output blob must be 8-byte aligned");
  return out;
}

// {states, pd, actions, values, rewards, dones, boot, moments}, the order
// every rollout binding returns.  scalar_actions: actions are [T][E], not
// [T][E][1] (Categorical).
inline std::vector<torch::Tensor> rollout_blob_views(const RolloutBlob& b,
                                                     const torch::Tensor& out,
                                                     bool scalar_actions) {
  auto view = [&](int64_t off, std::vector<int64_t> shape) {
    int64_t n = 1;
    for (int64_t d : shape) n *= d;
    return out.narrow(0, off, n).view(shape);
  };
  std::vector<int64_t> ashape{b.T, b.E, b.actw};
  if (scalar_actions) ashape.pop_back();
  torch::Tensor actions =
      b.int_actions ? out.narrow(0, b.actions, 2 * b.T * b.E * b.actw)
                          .view(torch::kInt64)
                          .view(ashape)
                    : view(b.actions, ashape);
  return {view(b.states, {b.T, b.E, b.D}), view(b.pd, {b.T, b.E, b.P}),
          actions, view(b.values, {b.T, b.E}), view(b.rewards, {b.T, b.E}),
          view(b.dones, {b.T, b.E}), view(b.boot, {b.E}),
          view(b.moments, {5})};
}
