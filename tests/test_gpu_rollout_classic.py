"""Lane-per-env physics rollout (classic_rollout.hip: classic_rollout_cat on
CartPole, classic_rollout_box on Pendulum) vs eager references.

The kernel's RNG is counter-based (not torch's), so, as in
test_gpu_rollout_cat.py, whose tolerances these are, the checks are
RNG-independent: recorded policy outputs == eager pi(recorded states) at
2e-4; every recorded transition replays through envs/classic.py's step
functions at 3e-5 with the dones exact; resets lie in their ranges; persisted
state and episode moments equal the replay; action statistics follow the
recorded distribution within 5 sigma; launches are deterministic per seed.
Kernel tests call the bindings directly.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from dppo_amd import spaces
from dppo_amd.config import DPPOConfig
from dppo_amd.envs.classic import (BatchedCartPole, BatchedPendulum,
                                   cartpole_step, pendulum_obs, pendulum_step)
from dppo_amd.models.mlp import PolicyValueMLP
from dppo_amd.ops import require_hip_ext
from dppo_amd.parallel.comm import Comm
from dppo_amd.trainer import DPPOEngine

STEP_TOL = dict(atol=3e-5, rtol=3e-5)
PI_TOL = dict(atol=2e-4, rtol=2e-4)
NAMES = ("states", "pdflats", "actions", "values", "rewards", "dones",
         "boot_v", "moments")


def make_case(game, hidden, activation, E, spread=False, bias_class=None,
              time_limit=200, stagger=False):
    """(pi, env, epr) on the GPU, after test_gpu_rollout_cat.py::make_case:
    spread scales the 0.01-init trunk and head by 100 and adds a +-1.5 ramp
    over the head columns, so the heads are state-dependent and far from
    uniform.  stagger starts env e at step counter e % time_limit."""
    torch.manual_seed(7)
    if game == "cartpole":
        env = BatchedCartPole(E, device="cuda", seed=3, time_limit=time_limit)
    else:
        env = BatchedPendulum(E, device="cuda", seed=3, time_limit=time_limit)
    D = env.obs_dim
    pi = PolicyValueMLP(obs_dim=D, action_space=env.action_space,
                        hidden_sizes=hidden, activation=activation).cuda()
    with torch.no_grad():
        if spread:
            pi.pi.weight.mul_(100.0)
            pi.vf.weight.mul_(100.0)
            for lay in pi.hidden:
                lay.weight.mul_(100.0)
            pi.pi.bias += torch.linspace(-1.5, 1.5, 2, device="cuda")
            pi.vf.bias += 0.5
        if bias_class is not None:
            pi.pi.bias[bias_class] += 40.0
    env.reset()
    if stagger:
        env.t = (torch.arange(E, device="cuda") % time_limit).to(torch.int32)
    epr = torch.zeros(E, device="cuda")
    return pi, env, epr


def weight_blob(pi):
    """Wt[in][out] + b per hidden layer, Wv[H], bv, Wpt[H][2], bp."""
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


def run_kernel(pi, env, epr, T, eps=0.0, seed=1234):
    blob, offsets, dims = weight_blob(pi)
    ext = require_hip_ext()
    act = 1 if pi.activation == "tanh" else 0
    E = env.num_envs
    empty = torch.empty(0, device="cuda")
    if isinstance(env, BatchedCartPole):
        out = ext.classic_rollout_cat(
            blob, offsets, dims, act, env.ENV_ID, env.s, env.time_limit,
            float(eps), env.x, env.t, epr, T, 2, seed, empty)
        assert out[2].dtype == torch.long and out[2].shape == (T, E)
        assert int(out[2].min()) >= 0 and int(out[2].max()) < 2
    else:
        out = ext.classic_rollout_box(
            blob, offsets, dims, act, env.ENV_ID, env.s, env.time_limit,
            -1.0, 1.0, float(eps), env.x, env.t, epr, T, 1, seed, empty)
        assert out[2].dtype == torch.float32 and out[2].shape == (T, E, 1)
    assert out[0].shape == (T, E, env.obs_dim)
    assert out[1].shape == (T, E, 2)
    return dict(zip(NAMES, out))


# ---- policy outputs ----------------------------------------------------------

# E: a lone lane, an exact wave, a wave plus a 1-lane tail, several blocks
# with a tail.  (64, 64) is the widest trunk the kernel takes and the only
# shape here that goes through the [unit][lane] image of layer 1.
@pytest.mark.parametrize("E", [1, 64, 65, 200])
@pytest.mark.parametrize("game,hidden,activation", [
    ("cartpole", (16,), "relu"),
    ("cartpole", (32,), "tanh"),
    ("cartpole", (64, 64), "tanh"),
    ("pendulum", (16,), "relu"),
    ("pendulum", (64, 64), "tanh"),
])
def test_recorded_policy_outputs_match_eager_forward(game, hidden, activation,
                                                     E):
    T = 8
    pi, env, epr = make_case(game, hidden, activation, E, spread=True)
    o = run_kernel(pi, env, epr, T)
    D = env.obs_dim
    with torch.no_grad():
        v_ref, flat_ref = pi(o["states"].reshape(T * E, D))
        vb, _ = pi(env.x)
    # not a degenerate policy: the heads vary over the batch
    if E > 1:
        assert float(flat_ref.std(dim=0).max()) > 1e-2
    torch.testing.assert_close(o["pdflats"].reshape(T * E, 2), flat_ref,
                               **PI_TOL)
    torch.testing.assert_close(o["values"].reshape(T * E), v_ref, **PI_TOL)
    torch.testing.assert_close(o["boot_v"], vb, **PI_TOL)


# widths that are no multiple of the kernel's 4-unit tile: the padded units
# must contribute nothing
@pytest.mark.parametrize("game,hidden", [("cartpole", (13,)),
                                         ("pendulum", (7, 30))])
def test_widths_off_the_unit_tile(game, hidden):
    T, E = 4, 65
    pi, env, epr = make_case(game, hidden, "tanh", E, spread=True)
    o = run_kernel(pi, env, epr, T)
    with torch.no_grad():
        v_ref, flat_ref = pi(o["states"].reshape(T * E, env.obs_dim))
    torch.testing.assert_close(o["pdflats"].reshape(T * E, 2), flat_ref,
                               **PI_TOL)
    torch.testing.assert_close(o["values"].reshape(T * E), v_ref, **PI_TOL)


# ---- transition replay, resets, persistence, moments ------------------------

def recover_state(env, obs):
    """Internal state of an observation: CartPole's is the observation;
    Pendulum's theta comes back through atan2."""
    if isinstance(env, BatchedCartPole):
        return obs
    return torch.stack([torch.atan2(obs[..., 1], obs[..., 0]), obs[..., 2]],
                       dim=-1)


def oracle_step(env, s, a):
    """(next observation, reward, terminated) of one classic.py step."""
    if isinstance(env, BatchedCartPole):
        return cartpole_step(s, a)
    s2, r, term = pendulum_step(s, a)
    return pendulum_obs(s2), r, term


def assert_reset_rows(env, rows):
    """Observation rows of freshly reset envs lie in the reset ranges."""
    if isinstance(env, BatchedCartPole):
        assert bool((rows.abs() <= 0.05).all())
    else:
        assert bool((rows[:, 2].abs() <= 1.0).all())
        torch.testing.assert_close(rows[:, 0] ** 2 + rows[:, 1] ** 2,
                                   torch.ones_like(rows[:, 0]),
                                   atol=1e-5, rtol=0)


def replay(env, o, t0, epr0, T):
    """Replays the recorded run through the oracle step, asserting every
    transition; returns (step counters, running returns, finished-episode
    returns, terminations, truncations) at the end of the run."""
    states, actions = o["states"], o["actions"]
    rewards, dones = o["rewards"], o["dones"]
    E = env.num_envs
    tc = t0.clone().long()
    epr = epr0.clone()
    finished, n_term, n_trunc = [], 0, 0
    reset_rows = []
    for t in range(T):
        nxt, r, term = oracle_step(env, recover_state(env, states[t]),
                                   actions[t])
        tc += 1
        trunc = tc >= env.time_limit
        done = term | trunc
        assert torch.equal(dones[t] > 0, done), t
        assert bool(((dones[t] == 0) | (dones[t] == 1)).all())
        torch.testing.assert_close(rewards[t], r, **STEP_TOL)
        following = states[t + 1] if t + 1 < T else env.x
        torch.testing.assert_close(following[~done], nxt[~done], **STEP_TOL)
        assert_reset_rows(env, following[done])
        reset_rows.append(following[done])
        n_term += int(term.sum())
        n_trunc += int((trunc & ~term).sum())
        epr += rewards[t]
        finished += epr[done].tolist()
        epr[done] = 0.0
        tc[done] = 0
    reset_rows = torch.cat(reset_rows)
    assert E == 1 or reset_rows.shape[0] >= 2
    # different envs / steps draw different fresh states
    assert int(torch.unique(reset_rows, dim=0).shape[0]) == reset_rows.shape[0]
    return tc, epr, finished, n_term, n_trunc


def check_replay(game, hidden, activation, **case_kw):
    E, T = 130, 48
    pi, env, epr_dev = make_case(game, hidden, activation, E, time_limit=11,
                                 stagger=True, **case_kw)
    t0, epr0 = env.t.clone(), epr_dev.clone()
    x0 = env.x.clone()
    o = run_kernel(pi, env, epr_dev, T)
    assert torch.equal(o["states"][0], x0)
    tc, epr, finished, n_term, n_trunc = replay(env, o, t0, epr0, T)
    # persisted per-env state (env.x was checked against the replay above)
    assert torch.equal(env.t.long(), tc)
    torch.testing.assert_close(epr_dev, epr, atol=1e-4, rtol=1e-4)
    if isinstance(env, BatchedCartPole):
        assert torch.equal(env.s, env.x)
    else:
        torch.testing.assert_close(pendulum_obs(env.s), env.x, atol=1e-6,
                                   rtol=0)
        assert bool((env.s[:, 0].abs() <= math.pi + 1e-6).all())
    # episode moments == the episode list rebuilt from rewards / dones
    mom = o["moments"]
    ep = torch.tensor(finished, dtype=torch.float64)
    assert int(mom[0]) == len(finished) > 0
    torch.testing.assert_close(float(mom[1]), float(ep.sum()),
                               atol=2e-2, rtol=1e-4)
    torch.testing.assert_close(float(mom[2]), float((ep * ep).sum()),
                               atol=2e-2, rtol=1e-4)
    torch.testing.assert_close(float(mom[3]), float(ep.min()),
                               atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(float(mom[4]), float(ep.max()),
                               atol=1e-4, rtol=1e-4)
    # a second launch continues where the first stopped
    x1 = env.x.clone()
    o2 = run_kernel(pi, env, epr_dev, 2, seed=99)
    assert torch.equal(o2["states"][0], x1)
    return n_term, n_trunc


def test_cartpole_replay_spread_policy():
    check_replay("cartpole", (16,), "relu", spread=True)


def test_cartpole_replay_with_terminations():
    # a constant push to the right ends an episode in 8..11 steps, the
    # staggered counters make the first episodes hit the 11-step limit
    n_term, n_trunc = check_replay("cartpole", (64, 64), "tanh", bias_class=1)
    assert n_term >= 10 and n_trunc >= 10, (n_term, n_trunc)


def test_pendulum_replay():
    n_term, n_trunc = check_replay("pendulum", (16,), "relu", spread=True)
    assert n_term == 0 and n_trunc >= 10


# ---- sampling ------------------------------------------------------------------

def assert_counts_follow(logits, actions, K):
    """|count_j - sum_n p_nj| <= 5 sqrt(sum_n p_nj (1 - p_nj)): the count of
    class j is a sum of independent Bernoulli(p_nj), so this is its 5 sigma
    bound (derived, not tuned)."""
    p = torch.softmax(logits.reshape(-1, K).double(), dim=-1)
    counts = torch.bincount(actions.reshape(-1), minlength=K).double()
    bound = 5.0 * (p * (1.0 - p)).sum(dim=0).sqrt()
    diff = (counts - p.sum(dim=0)).abs()
    assert bool((diff <= bound).all()), (counts.tolist(), p.sum(0).tolist(),
                                        bound.tolist())


def test_cartpole_sampling_follows_recorded_logits():
    pi, env, epr = make_case("cartpole", (16,), "relu", 512, spread=True)
    o = run_kernel(pi, env, epr, 16)
    logits, actions = o["pdflats"], o["actions"]
    p_max = torch.softmax(logits, -1).max(dim=-1).values
    assert 0.6 < float(p_max.mean()) < 0.999   # neither uniform nor one-hot
    assert_counts_follow(logits, actions, 2)
    # step 0 alone, across envs: an RNG ignoring the env index fails here
    assert_counts_follow(logits[0], actions[0], 2)
    # envs 0..7 across 256 steps: an RNG ignoring the step index fails here
    pi, env, epr = make_case("cartpole", (16,), "relu", 64, spread=True)
    o = run_kernel(pi, env, epr, 256)
    assert_counts_follow(o["pdflats"][:, :8], o["actions"][:, :8], 2)


def test_cartpole_full_exploration_is_uniform():
    E, T = 512, 16
    pi, env, epr = make_case("cartpole", (16,), "relu", E, bias_class=1)
    actions = run_kernel(pi, env, epr, T, eps=1.0)["actions"]
    counts = torch.bincount(actions.reshape(-1), minlength=2).double()
    N = E * T
    assert float((counts - N / 2).abs().max()) <= 5.0 * math.sqrt(N * 0.25)
    # and without exploration the +40 logit always wins
    pi, env, epr = make_case("cartpole", (16,), "relu", E, bias_class=1)
    assert bool((run_kernel(pi, env, epr, T)["actions"] == 1).all())


def test_pendulum_exploration_and_degenerate_std():
    E, T = 512, 16
    N = E * T
    pi, env, epr = make_case("pendulum", (16,), "relu", E, spread=True)
    a = run_kernel(pi, env, epr, T, eps=1.0)["actions"]
    assert float(a.min()) >= -1.0 and float(a.max()) <= 1.0
    # uniform on [-1, 1]: variance 1/3
    assert abs(float(a.double().mean())) <= 5.0 * math.sqrt(1.0 / (3.0 * N))
    assert float(a.std()) > 0.5
    # logstd = -20, eps = 0: the action is the mean
    pi, env, epr = make_case("pendulum", (16,), "relu", E, spread=True)
    with torch.no_grad():
        pi.pi.weight[1].zero_()
        pi.pi.bias[1] = -20.0
    o = run_kernel(pi, env, epr, T)
    assert float(o["pdflats"][..., 0].std()) > 1e-2
    torch.testing.assert_close(o["actions"][..., 0], o["pdflats"][..., 0],
                               atol=1e-6, rtol=0)


# ---- determinism --------------------------------------------------------------

@pytest.mark.parametrize("game", ["cartpole", "pendulum"])
def test_same_seed_is_bitwise_and_other_seed_differs(game):
    def run(seed):
        pi, env, epr = make_case(game, (32,), "tanh", 130, spread=True,
                                 time_limit=11)
        o = run_kernel(pi, env, epr, 24, eps=0.2, seed=seed)
        return o, (env.s, env.x, env.t, epr)

    a, pa = run(5)
    b, pb = run(5)
    for k in NAMES:
        assert torch.equal(a[k], b[k]), k
    for u, w in zip(pa, pb):
        assert torch.equal(u, w)
    c, _ = run(6)
    assert not torch.equal(a["actions"], c["actions"])


# ---- engine level ---------------------------------------------------------------

def make_engine(**kw):
    base = dict(
        GAME="CartPole-v0", ENV_DYNAMICS="physics", HIDDEN_SIZES=(16,),
        ACTIVATION="relu", NUM_ENVS=128, MAX_EPOCH_STEPS=32, EPOCH_MAX=1000,
        STOP_EPOCH=1000, NUM_WORKERS=1,
        LOG_FILE_PATH="/tmp/dppo_gpu_test_logs", DEVICE="cuda",
    )
    base.update(kw)
    return DPPOEngine(DPPOConfig(**base), comm=Comm(device="cuda:0"))


ENGINE_CASES = [
    dict(GAME="CartPole-v0", HIDDEN_SIZES=(16,), ACTIVATION="relu"),
    dict(GAME="Pendulum-v1", HIDDEN_SIZES=(64, 64), ACTIVATION="tanh"),
]


@pytest.mark.parametrize("kw", ENGINE_CASES, ids=["cartpole", "pendulum"])
def test_engine_takes_the_classic_rollout(kw, monkeypatch):
    monkeypatch.delenv("DPPO_ROLLOUT_CLASSIC", raising=False)

    def boom(self):
        raise AssertionError("eager loop entered on an eligible physics env")

    with monkeypatch.context() as m:
        m.setattr(DPPOEngine, "_rollout_once_eager_loop", boom)
        eng = make_engine(**kw)
        assert eng._can_rollout_classic() and eng._use_rollout_classic()
        assert not eng._can_fuse_rollout() and not eng._can_rollout_v3()
        assert not eng._can_fuse_rollout_cat()
        assert not eng._can_fuse_rollout_multi()
        p0 = eng.flat_pi.flat_param.detach().clone()
        for _ in range(2):
            stats, _ = eng.train_round()
            assert all(math.isfinite(v) for v in stats.values())
        assert eng.classic_rollout_launches >= 2
        assert not torch.equal(p0, eng.flat_pi.flat_param.detach())

    monkeypatch.setenv("DPPO_ROLLOUT_CLASSIC", "0")
    ref = make_engine(**kw)
    assert ref._can_rollout_classic() and not ref._use_rollout_classic()
    stats, _ = ref.train_round()
    assert all(math.isfinite(v) for v in stats.values())
    assert ref.classic_rollout_launches == 0


def test_wide_trunk_is_not_eligible():
    eng = make_engine(HIDDEN_SIZES=(128,))
    assert not eng._can_rollout_classic()
    assert not make_engine(HIDDEN_SIZES=(16, 16, 16))._can_rollout_classic()
    assert not make_engine(ENV_DYNAMICS="synthetic")._can_rollout_classic()


def test_ppo_learns_cartpole_through_the_kernel(monkeypatch):
    """The CPU learning test's config on the GPU: rollout kernel, GAE, the
    fused Discrete update and Adam together learn the real task."""
    monkeypatch.delenv("DPPO_ROLLOUT_CLASSIC", raising=False)
    eng = make_engine(
        NUM_ENVS=64, MAX_EPOCH_STEPS=100, HIDDEN_SIZES=(32,),
        ACTIVATION="tanh", LEARNING_RATE=1e-2, EPOCH_MAX=60, STOP_EPOCH=500,
        SEED=0)
    assert eng._use_rollout_classic()
    curve = [eng.train_round()[0]["epr_mean"] for _ in range(50)]
    print("epr_mean by round:", [round(v, 1) for v in curve])
    assert eng.classic_rollout_launches >= 50
    assert curve[0] < 30.0
    assert max(curve[45:50]) >= 100.0
