"""Fused Categorical rollout (rollout.hip, rollout_run_cat) vs eager
references.

The kernel's RNG is counter-based (not torch's), so — as in
test_gpu_rollout.py, whose tolerances these are — the checks are
RNG-independent invariants:
  - recorded logits/values/boot_v == eager pi(recorded states)
  - env transition x' = tanh(x*d + (x@V)@U + B[a]) holds at noise=0
  - reward definition, done schedule, episode moments, persisted epr/t
  - action counts follow softmax(recorded logits) within the binomial 5 sigma
  - degenerate heads and the epsilon overlay
Kernel tests build the policy and env directly so shapes are free of the
GAME preset table.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from dppo_amd import spaces
from dppo_amd.config import DPPOConfig
from dppo_amd.envs.synthetic import BatchedSyntheticEnv
from dppo_amd.models.mlp import PolicyValueMLP
from dppo_amd.ops import require_hip_ext
from dppo_amd.parallel.comm import Comm
from dppo_amd.trainer import DPPOEngine


def make_case(D, K, hidden, activation, E, spread=False, bias_class=None):
    """(pi, env, epr) on the GPU.  spread multiplies the policy head by 100:
    the 0.01 init makes every policy near-uniform and the checks vacuous.
    The trunk has the same 0.01 init and states are O(0.1), so the head
    scale alone still leaves logits ~1e-3 (measured: every p within 0.002
    of 1/K); spread therefore also scales the hidden layers by 100 and adds
    a +-1.5 logit ramp over the classes, which makes the policy both
    state-dependent and far from uniform."""
    torch.manual_seed(7)
    pi = PolicyValueMLP(obs_dim=D, action_space=spaces.Discrete(K),
                        hidden_sizes=hidden, activation=activation).cuda()
    with torch.no_grad():
        if spread:
            pi.pi.weight.mul_(100.0)
            for lay in pi.hidden:
                lay.weight.mul_(100.0)
            pi.pi.bias += torch.linspace(-1.5, 1.5, K, device="cuda")
        if bias_class is not None:
            pi.pi.bias[bias_class] += 40.0
    env = BatchedSyntheticEnv(
        spaces.Box(low=-float("inf"), high=float("inf"), shape=(D,)),
        spaces.Discrete(K), E, device="cuda", seed=3, horizon=16)
    env.reset()
    epr = torch.zeros(E, device="cuda")
    return pi, env, epr


def weight_blob(pi):
    """Wt[in][out] + b per hidden layer, Wv[H], bv, Wpt[H][K], bp."""
    parts = []
    for lay in pi.hidden:
        parts += [lay.weight.t().contiguous(), lay.bias]
    parts += [pi.vf.weight, pi.vf.bias, pi.pi.weight.t().contiguous(),
              pi.pi.bias]
    offsets, off = [], 0
    for p in parts:
        offsets.append(off)
        off += p.numel()
    with torch.no_grad():
        blob = torch.cat([p.reshape(-1) for p in parts])
    return blob, offsets, [pi.obs_dim, *pi.hidden_sizes]


def run_kernel(pi, env, epr, T, K, eps=0.0, noise=0.05, seed=1234):
    blob, offsets, dims = weight_blob(pi)
    out = require_hip_ext().rollout_run_cat(
        blob, offsets, dims, 1 if pi.activation == "tanh" else 0,
        env.blob, env.rank_eff, env.horizons_i32, float(noise), float(eps),
        env.x, env.t, epr, T, K, seed, torch.empty(0, device="cuda"), 0)
    states, logits, actions, values, rewards, dones, boot_v, mom = out
    E = env.num_envs
    assert actions.dtype == torch.long and actions.shape == (T, E)
    assert logits.shape == (T, E, K)
    assert int(actions.min()) >= 0 and int(actions.max()) < K
    return out


def check_policy_outputs(D, K, hidden, activation, E, T):
    pi, env, epr = make_case(D, K, hidden, activation, E, spread=True)
    states, logits, actions, values, rewards, dones, boot_v, mom = run_kernel(
        pi, env, epr, T, K)
    with torch.no_grad():
        v_ref, flat_ref = pi(states.reshape(T * E, D))
        vb, _ = pi(env.x)
    torch.testing.assert_close(logits.reshape(T * E, K), flat_ref,
                               atol=2e-4, rtol=2e-4)
    torch.testing.assert_close(values.reshape(T * E), v_ref,
                               atol=2e-4, rtol=2e-4)
    torch.testing.assert_close(boot_v, vb, atol=2e-4, rtol=2e-4)


# E=130: 2-env tiles; 131: 8-env tiles + 3-env tail; 2051: grid 257 > 256
# CUs -> 4-waves/SIMD instantiation, tail tile
@pytest.mark.parametrize("E", [130, 131, 2051])
def test_recorded_policy_outputs_match_eager_forward(E):
    check_policy_outputs(6, 3, (16,), "relu", E, 8)


# K+1 head columns wider than the trunk: the k-split partial rows must be
# sized for the heads, not for the widest hidden layer
@pytest.mark.parametrize("D,K,hidden,activation", [
    (5, 17, (8, 8), "tanh"),
    (5, 64, (16,), "tanh"),
    (4, 2, (16,), "relu"),   # CartPole's shape
])
def test_wide_head_over_narrow_trunk(D, K, hidden, activation):
    check_policy_outputs(D, K, hidden, activation, 131, 4)


def test_env_transition_exact_at_zero_noise():
    D, K, E, T = 6, 3, 128, 16
    pi, env, epr = make_case(D, K, (16,), "relu", E, spread=True)
    states, logits, actions, values, rewards, dones, *_ = run_kernel(
        pi, env, epr, T, K, noise=0.0)
    x = states
    for t in range(T - 1):
        pred = torch.tanh(x[t] * env.d + (x[t] @ env.V) @ env.U
                          + env.B[actions[t]])
        live = dones[t] == 0
        torch.testing.assert_close(x[t + 1][live], pred[live],
                                   atol=3e-5, rtol=3e-5)
        # reward is computed on the PRE-reset next state
        r_pred = 1.0 - pred.pow(2).mean(dim=-1)
        torch.testing.assert_close(rewards[t], r_pred, atol=3e-5, rtol=3e-5)


def test_done_schedule_and_episode_moments():
    D, K, E, T = 6, 3, 128, 48
    pi, env, epr_dev = make_case(D, K, (16,), "relu", E)
    epr0 = epr_dev.clone()
    *_, rewards, dones, boot_v, mom = run_kernel(pi, env, epr_dev, T, K)
    hor = env.horizons_i32.long().cpu()
    r, d = rewards.cpu(), dones.cpu()
    for e in range(8):
        h = int(hor[e])
        expect = torch.tensor(
            [1.0 if (t + 1) % h == 0 else 0.0 for t in range(T)])
        torch.testing.assert_close(d[:, e], expect)
    epr = epr0.cpu().clone()
    eps_list = []
    for t in range(T):
        epr += r[t]
        fin = d[t] > 0
        eps_list += epr[fin].tolist()
        epr[fin] = 0.0
    eps_t = torch.tensor(eps_list)
    assert int(mom[0]) == len(eps_list) > 0
    torch.testing.assert_close(float(mom[1]), float(eps_t.sum()),
                               atol=2e-2, rtol=1e-4)
    torch.testing.assert_close(float(mom[3]), float(eps_t.min()),
                               atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(float(mom[4]), float(eps_t.max()),
                               atol=1e-4, rtol=1e-4)
    # persisted per-env state
    torch.testing.assert_close(epr_dev.cpu(), epr, atol=1e-4, rtol=1e-4)
    assert torch.equal(env.t.long().cpu(), T % hor)


def assert_counts_follow(logits, actions, K):
    """|count_j - sum_n p_nj| <= 5 sqrt(sum_n p_nj (1 - p_nj)): the count of
    class j is a sum of independent Bernoulli(p_nj), so this is its 5 sigma
    bound (derived, not tuned)."""
    p = torch.softmax(logits.reshape(-1, K).double(), dim=-1)
    a = actions.reshape(-1)
    counts = torch.bincount(a, minlength=K).double()
    bound = 5.0 * (p * (1.0 - p)).sum(dim=0).sqrt()
    diff = (counts - p.sum(dim=0)).abs()
    assert bool((diff <= bound).all()), (counts.tolist(), p.sum(0).tolist(),
                                        bound.tolist())


def test_sampling_follows_recorded_logits():
    D, K = 6, 5
    pi, env, epr = make_case(D, K, (16,), "relu", 512, spread=True)
    states, logits, actions, *_ = run_kernel(pi, env, epr, 16, K, eps=0.0)
    # the policy is not near-uniform (else the check would be vacuous)
    assert float(torch.softmax(logits, -1).max(dim=-1).values.mean()) > 0.3
    assert_counts_follow(logits, actions, K)
    # step 0 alone, across envs: an RNG ignoring the env index fails here
    assert_counts_follow(logits[0], actions[0], K)
    # envs 0..7 across 256 steps: an RNG ignoring the step index fails here
    pi, env, epr = make_case(D, K, (16,), "relu", 64, spread=True)
    states, logits, actions, *_ = run_kernel(pi, env, epr, 256, K, eps=0.0)
    assert_counts_follow(logits[:, :8], actions[:, :8], K)


@pytest.mark.parametrize("K,j", [(5, 3), (64, 41), (2, 1)])
def test_degenerate_head_and_epsilon_overlay(K, j):
    D, E, T = 6, 512, 16
    N = E * T
    # +40 logit bias on class j, eps=0: the Gumbel noise spans < 20
    pi, env, epr = make_case(D, K, (16,), "relu", E, bias_class=j)
    _, _, actions, *_ = run_kernel(pi, env, epr, T, K, eps=0.0)
    assert bool((actions == j).all())
    # eps=1: uniform over the K classes
    pi, env, epr = make_case(D, K, (16,), "relu", E, bias_class=j)
    _, _, actions, *_ = run_kernel(pi, env, epr, T, K, eps=1.0)
    counts = torch.bincount(actions.reshape(-1), minlength=K).double()
    sigma = math.sqrt(N * (1.0 / K) * (1.0 - 1.0 / K))
    assert float((counts - N / K).abs().max()) <= 5.0 * sigma
    # eps=0.25 over the biased head: an explored action misses j w.p. (K-1)/K
    pi, env, epr = make_case(D, K, (16,), "relu", E, bias_class=j)
    _, _, actions, *_ = run_kernel(pi, env, epr, T, K, eps=0.25)
    q = 0.25 * (K - 1) / K
    share = float((actions != j).double().mean())
    assert abs(share - q) <= 5.0 * math.sqrt(q * (1.0 - q) / N)


# ---- engine level ----

def make_engine(**kw):
    base = dict(
        GAME="CartPole-v0", HIDDEN_SIZES=(16,), ACTIVATION="relu",
        NUM_ENVS=128, MAX_EPOCH_STEPS=32, EPOCH_MAX=1000, STOP_EPOCH=1000,
        NUM_WORKERS=1, LOG_FILE_PATH="/tmp/dppo_gpu_test_logs", DEVICE="cuda",
    )
    base.update(kw)
    return DPPOEngine(DPPOConfig(**base), comm=Comm(device="cuda:0"))


ENGINE_CASES = [
    dict(GAME="CartPole-v0", HIDDEN_SIZES=(16,), ACTIVATION="relu",
         NUM_ENVS=128),
    dict(GAME="LunarLander-v2", HIDDEN_SIZES=(64, 64), ACTIVATION="tanh",
         NUM_ENVS=256),
]


@pytest.mark.parametrize("kw", ENGINE_CASES, ids=["cartpole", "lunarlander"])
def test_engine_fused_cat_rollout(kw, monkeypatch):
    monkeypatch.setenv("DPPO_ROLLOUT_CAT", "0")
    ref = make_engine(**kw)
    assert ref._can_fuse_rollout_cat() and not ref._use_rollout_cat()
    calls = []
    eager = DPPOEngine._rollout_once_eager_loop
    monkeypatch.setattr(
        DPPOEngine, "_rollout_once_eager_loop",
        lambda self: (calls.append(1), eager(self))[1])
    b_ref, _ = ref.rollout_once()
    assert calls  # DPPO_ROLLOUT_CAT=0 takes the eager loop

    monkeypatch.setenv("DPPO_ROLLOUT_CAT", "1")

    def boom(self):
        raise AssertionError("eager loop entered with DPPO_ROLLOUT_CAT=1")

    monkeypatch.setattr(DPPOEngine, "_rollout_once_eager_loop", boom)
    eng = make_engine(**kw)
    assert eng._use_rollout_cat()
    batch, _ = eng.rollout_once()
    T, E, K = eng.cfg.MAX_EPOCH_STEPS, eng.cfg.NUM_ENVS, eng.act_space.n
    assert batch.actions.dtype == torch.long
    assert batch.oldflat.shape == (T * E, K)
    for f in ("states", "actions", "adv", "etr", "oldflat", "oldv",
              "ep_count", "ep_sum", "ep_sumsq", "ep_min", "ep_max"):
        got, want = getattr(batch, f), getattr(b_ref, f)
        assert got.dtype == want.dtype, f
        assert got.shape == want.shape, f
    assert isinstance(batch.valid, bool) and batch.valid
    p0 = eng.flat_pi.flat_param.detach().clone()
    for _ in range(3):
        stats, _ = eng.train_round()
    assert all(math.isfinite(v) for v in stats.values())
    assert not torch.equal(p0, eng.flat_pi.flat_param.detach())


def test_multidiscrete_is_never_eligible(monkeypatch):
    monkeypatch.setenv("DPPO_ROLLOUT_CAT", "1")
    eng = make_engine(GAME="MultiLever-v0")
    assert not eng._can_fuse_rollout_cat() and not eng._use_rollout_cat()
