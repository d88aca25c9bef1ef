"""The rollout's counter RNG (ops/hip/rollout_math.h) pinned from the host.

Every other RNG test compares one GPU path against another, so an edit to
the shared header would move all paths together and pass them all.  Here a
numpy replica of lowbias32 / rng_uniform gives the expected stream.

With eps = 1, low = 0 and high = 1 every Box action is exactly
rng_uniform(seed, env, step, 90010 + j): the decision draw (slot 90001) is
<= 1 and 0 + (1 - 0) * u is exact with or without contraction.  The hash is
uint32 arithmetic and the uniform is float32((h >> 8) + 1) * 2^-24 (the
kernel's `1.0f / 16777217.0f`: 2^24 + 1 is not a float32 and the literal
rounds to 2^24), both exact, so every comparison is torch.equal.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from dppo_amd import spaces
from dppo_amd.envs.synthetic import BatchedSyntheticEnv
from dppo_amd.models.mlp import PolicyValueMLP
from dppo_amd.ops import require_hip_ext
from test_gpu_fwd_fused import H, VA_OFF, out_buffers, run_fused, weights
from test_gpu_rollout_cat import weight_blob

SLOT_EPS_ACT = 90010
SEEDS = [0x5EED1234, (1 << 32) + 7]   # only the low 32 bits may matter


def lowbias32(x):
    x = x.astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x


def rng_uniform(seed, env, step, slot):
    """Broadcasts over env / step / slot; float32 in (0, 1]."""
    u32 = lambda v: np.asarray(v, dtype=np.int64).astype(np.uint32)
    h = lowbias32(np.uint32(seed & 0xFFFFFFFF)
                  ^ u32(env) * np.uint32(0x9E3779B9)
                  ^ u32(step) * np.uint32(0x85EBCA6B)
                  ^ u32(slot) * np.uint32(0xC2B2AE35))
    scale = np.float32(1.0) / np.float32(16777217.0)
    return ((h >> np.uint32(8)) + np.uint32(1)).astype(np.float32) * scale


def expected_box(seed, n_env, step, A):
    env = np.arange(n_env)[:, None]
    return torch.from_numpy(
        rng_uniform(seed, env, step, SLOT_EPS_ACT + np.arange(A)[None, :]))


def test_replica_is_exact_float32():
    u = rng_uniform(SEEDS[0], np.arange(4096), 0, SLOT_EPS_ACT)
    assert u.dtype == np.float32
    assert float(u.min()) > 0.0 and float(u.max()) <= 1.0
    assert np.array_equal(rng_uniform(SEEDS[1], np.arange(8), 3, 5),
                          rng_uniform(7, np.arange(8), 3, 5))


def _sample_inputs(B, A, seed):
    kw = ((VA_OFF + A + 3) // 4) * 4
    g = torch.Generator(device="cpu").manual_seed(B + A)
    return (torch.randn(B, kw, generator=g).cuda().contiguous(),
            torch.full((1,), seed, dtype=torch.int64, device="cuda"),
            torch.full((1,), 1.0, device="cuda"))


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("step", [0, 5])
def test_rollout_sample(step, seed):
    """B = 130 crosses a 128-row tile and leaves a tail."""
    B, A = 130, 3
    xva, seed_dev, eps_dev = _sample_inputs(B, A, seed)
    g = torch.Generator(device="cpu").manual_seed(step)
    pdflat = torch.randn(B, 2 * A, generator=g).cuda().contiguous()
    actions = torch.full((B, A), float("nan"), device="cuda")
    require_hip_ext().rollout_sample(pdflat, actions, xva, seed_dev, eps_dev,
                                     step, VA_OFF, 0.0, 1.0)
    want = expected_box(seed, B, step, A)
    assert torch.equal(actions.cpu(), want)
    assert torch.equal(xva[:, VA_OFF:VA_OFF + A].cpu(), want)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("step", [0, 5])
def test_mlp_fwd_fused_sampling(step, seed):
    """D = 8, A = 3: heads width 8, an eligible shape."""
    B, D, A = 130, 8, 3
    ext = require_hip_ext()
    assert ext.mlp_fwd_fused_supported(D, H, H, A)
    w = weights(D, A)
    g = torch.Generator(device="cpu").manual_seed(D + step)
    X = torch.randn(B, D, generator=g).cuda().contiguous()
    xva, seed_dev, eps_dev = _sample_inputs(B, A, seed)
    actions = torch.full((B, A), float("nan"), device="cuda")
    run_fused(ext, X, w, 1, out_buffers(B, A), sample=dict(
        actions=actions, xva=xva, seed=seed_dev, eps=eps_dev, step=step,
        va_off=VA_OFF, low=0.0, high=1.0))
    want = expected_box(seed, B, step, A)
    assert torch.equal(actions.cpu(), want)
    assert torch.equal(xva[:, VA_OFF:VA_OFF + A].cpu(), want)


def _whole_rollout_case(E, act_space):
    D = 6
    torch.manual_seed(11)
    pi = PolicyValueMLP(obs_dim=D, action_space=act_space, hidden_sizes=(16,),
                        activation="relu").cuda()
    env = BatchedSyntheticEnv(
        spaces.Box(low=-float("inf"), high=float("inf"), shape=(D,)),
        act_space, E, device="cuda", seed=3, horizon=16)
    env.reset()
    return pi, env, torch.zeros(E, device="cuda")


# E = 10 runs as five 2-env tiles, E = 11 as one 8-env tile plus a tail of 3
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("E", [10, 11])
def test_rollout_run_box(E, seed):
    T, A = 3, 3
    pi, env, epr = _whole_rollout_case(
        E, spaces.Box(low=0.0, high=1.0, shape=(A,)))
    blob, offsets, dims = weight_blob(pi)
    out = require_hip_ext().rollout_run(
        blob, offsets, dims, 0, env.blob, env.rank_eff, env.horizons_i32,
        0.05, 0.0, 1.0, 1.0, env.x, env.t, epr, T, A, seed,
        torch.empty(0, device="cuda"), 0)
    actions = out[2]
    assert actions.shape == (T, E, A)
    for t in range(T):
        assert torch.equal(actions[t].cpu(), expected_box(seed, E, t, A)), t


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("E", [10, 11])
def test_rollout_run_cat(E, seed):
    T, K = 3, 3
    pi, env, epr = _whole_rollout_case(E, spaces.Discrete(K))
    blob, offsets, dims = weight_blob(pi)
    out = require_hip_ext().rollout_run_cat(
        blob, offsets, dims, 0, env.blob, env.rank_eff, env.horizons_i32,
        0.05, 1.0, env.x, env.t, epr, T, K, seed,
        torch.empty(0, device="cuda"), 0)
    actions = out[2]
    assert actions.dtype == torch.long and actions.shape == (T, E)
    for t in range(T):
        u = rng_uniform(seed, np.arange(E), t, SLOT_EPS_ACT)
        want = np.minimum(K - 1, (u * np.float32(K)).astype(np.int64))
        assert torch.equal(actions[t].cpu(), torch.from_numpy(want)), t
