"""Lane-per-env MountainCar-v0 (classic_rollout_cat, env_id 3, three logits)
and MountainCarContinuous-v0 (classic_rollout_box, env_id 4) rollouts vs eager
references, after test_gpu_rollout_acrobot.py.

The checks do not depend on the kernel's counter RNG: recorded policy outputs
== eager pi(recorded states) at 2e-4; every recorded transition replays
through envs/classic.py's mountaincar_step / mountaincar_cont_step at 2e-6
(atol, rtol 0: kernel and torch are each within about five half-ulp roundings
of values <= 1.2, 3e-7, of the exact step; the project's 3e-5 env tolerance is
the ceiling); dones and the left wall's velocity zeroing are exact outside the
bands |z - goal| < 1e-6, |z + 1.2| < 1e-6 (z the unclamped new position) and
|v'| < 1e-7 next to the goal, where the replay follows the kernel's flag (at
most 1 % of the rows); resets lie in (-0.6, -0.4] x {0}; persisted state and
episode moments equal the replay; a hand-set energy-pumping policy climbs the
hill inside the kernel; action statistics follow the recorded distribution
within 5 sigma; launches are deterministic per seed.  Kernel tests call the
bindings directly.

Replay seeding (seed 5): the same states stepped by the torch env on the CPU
under a torch-sampled spread policy gave 34 / 34 terminations, 25 / 24 wall
hits and 556 / 556 truncations ((16,) relu / (64, 64) tanh) on MountainCar-v0
and 38 / 38, 25 / 25 and 552 / 552 on MountainCarContinuous-v0 (seeds 6 and 7
gave 39-42, 22-28 and 549-551): at least twice the floors of 10 the test
asserts.  The kernel's own runs gave 34 / 38 terminations, 24 / 25 wall hits
and 556 / 552 truncations, no row inside a band, and a worst live-row
difference of 0.0 (MountainCar-v0) and 6.0e-8 (MountainCarContinuous-v0).
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from dppo_amd.config import DPPOConfig
from dppo_amd.envs.classic import (CLASSIC_ENVS, BatchedMountainCar,
                                   BatchedMountainCarContinuous,
                                   mountaincar_cont_step, mountaincar_step)
from dppo_amd.models.mlp import PolicyValueMLP
from dppo_amd.ops import require_hip_ext
from dppo_amd.parallel.comm import Comm
from dppo_amd.trainer import DPPOEngine

STEP_TOL = dict(atol=2e-6, rtol=0.0)
# three float32 roundings of max(100, 0.1 a^2): one ulp at 100 is 7.6e-6
REWARD_TOL = dict(atol=2e-5, rtol=1e-6)
PI_TOL = dict(atol=2e-4, rtol=2e-4)
POS_BAND = 1e-6
VEL_BAND = 1e-7
NAMES = ("states", "pdflats", "actions", "values", "rewards", "dones",
         "boot_v", "moments")
CAT, BOX = "MountainCar-v0", "MountainCarContinuous-v0"
GAMES = [CAT, BOX]
ENV = {CAT: BatchedMountainCar, BOX: BatchedMountainCarContinuous}
STEP = {CAT: mountaincar_step, BOX: mountaincar_cont_step}
GOAL = {CAT: 0.5, BOX: 0.45}
MIN_POS = -1.2


def replay_states(E, seed):
    """A quarter of the envs next to the goal (p in [0.40, 0.6), v in [0,
    0.07]), a quarter next to the left wall (p in [-1.2, -1.1], v in [-0.07,
    0]), the rest over the whole range."""
    gen = torch.Generator().manual_seed(seed)
    u = torch.rand(E, 2, generator=gen)
    q = E // 4
    lo = torch.tensor([[-1.2, -0.07]]).repeat(E, 1)
    hi = torch.tensor([[0.6, 0.07]]).repeat(E, 1)
    lo[:q], hi[:q] = torch.tensor([0.40, 0.0]), torch.tensor([0.6, 0.07])
    lo[q:2 * q] = torch.tensor([-1.2, -0.07])
    hi[q:2 * q] = torch.tensor([-1.1, 0.0])
    s = (lo + (hi - lo) * u).float()
    s[:, 0] = s[:, 0].clamp(-1.2, 0.6 - 1e-6)
    s[:, 1] = s[:, 1].clamp(-0.07, 0.07)
    return s


def make_case(game, hidden, activation, E, spread=False, bias_class=None,
              time_limit=None, stagger=False, state_seed=None,
              device="cuda"):
    """(pi, env, epr).  spread scales the 0.01-init trunk and heads by 100
    and offsets the head columns (a -1.5 / 0 / +1.5 ramp over the logits;
    mean + 0.3 and logstd - 0.5, so the sampled forces fall on both sides of
    the clip), so every column is state-dependent.  stagger starts env e at
    step counter e % time_limit.  state_seed overwrites the reset states with
    replay_states."""
    torch.manual_seed(7)
    kw = {} if time_limit is None else dict(time_limit=time_limit)
    env = ENV[game](E, device=device, seed=3, **kw)
    pi = PolicyValueMLP(obs_dim=env.obs_dim, action_space=env.action_space,
                        hidden_sizes=hidden, activation=activation).to(device)
    with torch.no_grad():
        if spread:
            pi.pi.weight.mul_(100.0)
            pi.vf.weight.mul_(100.0)
            for lay in pi.hidden:
                lay.weight.mul_(100.0)
            if game == CAT:
                pi.pi.bias += torch.linspace(-1.5, 1.5, 3, device=device)
            else:
                pi.pi.bias += torch.tensor([0.3, -0.5], device=device)
            pi.vf.bias += 0.5
        if bias_class is not None:
            pi.pi.bias[bias_class] += 40.0
    env.reset()
    if state_seed is not None:
        env.s = replay_states(E, state_seed).to(device)
        env.x = env.s.clone()
    if stagger:
        env.t = (torch.arange(E, device=device)
                 % env.time_limit).to(torch.int32)
    epr = torch.zeros(E, device=device)
    return pi, env, epr


def weight_blob(pi):
    """Wt[in][out] + b per hidden layer, Wv[H], bv, Wpt[H][P], bp."""
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
    if isinstance(env, BatchedMountainCar):
        out = ext.classic_rollout_cat(
            blob, offsets, dims, act, env.ENV_ID, env.s, env.time_limit,
            float(eps), env.x, env.t, epr, T, 3, seed, empty)
        assert out[2].dtype == torch.long and out[2].shape == (T, E)
        assert int(out[2].min()) >= 0 and int(out[2].max()) < 3
        assert out[1].shape == (T, E, 3)
    else:
        out = ext.classic_rollout_box(
            blob, offsets, dims, act, env.ENV_ID, env.s, env.time_limit,
            -1.0, 1.0, float(eps), env.x, env.t, epr, T, 1, seed, empty)
        assert out[2].dtype == torch.float32 and out[2].shape == (T, E, 1)
        assert out[1].shape == (T, E, 2)
    assert out[0].shape == (T, E, 2)
    return dict(zip(NAMES, out))


# ---- policy outputs ----------------------------------------------------------

def assert_policy_outputs(pi, env, o, T, E):
    Pn = o["pdflats"].shape[-1]
    with torch.no_grad():
        v_ref, flat_ref = pi(o["states"].reshape(T * E, 2))
        vb, _ = pi(env.x)
    if E > 1:   # every head column varies over the batch
        assert float(flat_ref.std(dim=0).min()) > 1e-2
    torch.testing.assert_close(o["pdflats"].reshape(T * E, Pn), flat_ref,
                               **PI_TOL)
    torch.testing.assert_close(o["values"].reshape(T * E), v_ref, **PI_TOL)
    torch.testing.assert_close(o["boot_v"], vb, **PI_TOL)


# E: a lone lane, an exact wave, a wave plus a 1-lane tail, several blocks
# with a tail.  (64, 64) is the widest trunk the kernel takes and goes through
# the [unit][lane] image of layer 1.
@pytest.mark.parametrize("E", [1, 64, 65, 200])
@pytest.mark.parametrize("hidden,activation", [((16,), "relu"),
                                               ((64, 64), "tanh")])
@pytest.mark.parametrize("game", GAMES)
def test_recorded_policy_outputs_match_eager_forward(game, hidden, activation,
                                                     E):
    T = 8
    pi, env, epr = make_case(game, hidden, activation, E, spread=True,
                             state_seed=21)
    o = run_kernel(pi, env, epr, T)
    assert_policy_outputs(pi, env, o, T, E)


# widths that are no multiple of the kernel's 4-unit tile: the padded units
# must contribute nothing to any head column
@pytest.mark.parametrize("hidden", [(13,), (7, 30)])
@pytest.mark.parametrize("game", GAMES)
def test_widths_off_the_unit_tile(game, hidden):
    T, E = 4, 65
    pi, env, epr = make_case(game, hidden, "tanh", E, spread=True,
                             state_seed=22)
    o = run_kernel(pi, env, epr, T)
    assert_policy_outputs(pi, env, o, T, E)


# ---- transition replay, resets, persistence, moments ------------------------

def unclamped(game, s, a):
    """float64 (z, v2): the new position before its clamp and the new,
    clamped velocity, for the bands."""
    p, v = s.double().unbind(-1)
    a = a.reshape(-1).double()
    if game == CAT:
        v2 = v + (a - 1.0) * 0.001 - 0.0025 * torch.cos(3.0 * p)
    else:
        v2 = v + a.clamp(-1.0, 1.0) * 0.0015 - 0.0025 * torch.cos(3.0 * p)
    v2 = v2.clamp(-0.07, 0.07)
    return p + v2, v2


def is_wall(s2):
    f32_min = torch.tensor(MIN_POS, dtype=torch.float32, device=s2.device)
    return (s2[:, 0] == f32_min) & (s2[:, 1] == 0.0)


def replay(game, env, o, t0, epr0, T):
    """Replays the recorded run through envs/classic.py's step, asserting
    every transition; returns (step counters, running returns, finished-
    episode returns, terminations, wall hits, truncations, band rows)."""
    states, actions = o["states"], o["actions"]
    rewards, dones = o["rewards"], o["dones"]
    goal = GOAL[game]
    tc = t0.clone().long()
    epr = epr0.clone()
    finished, n_term, n_wall, n_trunc, n_band = [], 0, 0, 0, 0
    reset_rows, worst = [], 0.0
    for t in range(T):
        s2, r, term = STEP[game](states[t], actions[t])
        z, v2 = unclamped(game, states[t], actions[t])
        v3 = torch.where(z <= MIN_POS, torch.zeros_like(v2), v2)
        band = ((z - goal).abs() < POS_BAND) \
            | ((z - MIN_POS).abs() < POS_BAND) \
            | ((v3.abs() < VEL_BAND) & (z >= goal - POS_BAND))
        n_band += int(band.sum())
        tc += 1
        trunc = tc >= env.time_limit
        kdone = dones[t] > 0
        assert bool(((dones[t] == 0) | (dones[t] == 1)).all())
        # outside the bands the flag is exact; inside them the replay follows
        # the kernel's flag, which a truncated row shows only in the
        # continuous env's reward
        term = torch.where(band & ~trunc, kdone, term)
        if game == BOX:
            term = torch.where(band & trunc, rewards[t] > 50.0, term)
        done = term | trunc
        assert torch.equal(kdone, done), t
        if game == CAT:
            assert bool((rewards[t] == -1.0).all()), t
        else:
            af = actions[t].reshape(-1)
            want = torch.where(term, 100.0, 0.0) - 0.1 * af * af
            torch.testing.assert_close(rewards[t], want, **REWARD_TOL)
        following = states[t + 1] if t + 1 < T else env.x
        live = ~done & ~band
        if bool(live.any()):
            worst = max(worst, float((following[live] - s2[live]).abs().max()))
        torch.testing.assert_close(following[live], s2[live], **STEP_TOL)
        # the wall rule, bit for bit: position float32(-1.2), velocity 0
        wall = is_wall(s2)
        assert torch.equal(is_wall(following)[live], wall[live]), t
        fresh = following[done]
        assert bool(((fresh[:, 0] > -0.6) & (fresh[:, 0] <= -0.4)).all())
        assert bool((fresh[:, 1] == 0.0).all())
        reset_rows.append(fresh)
        n_term += int(term.sum())
        n_wall += int((wall & ~band).sum())
        n_trunc += int((trunc & ~term).sum())
        epr += rewards[t]
        finished += epr[done].tolist()
        epr[done] = 0.0
        tc[done] = 0
    print(game, "replay: max |kernel - torch step| over live rows =", worst,
          "band rows:", n_band, "terminations:", n_term, "wall hits:", n_wall,
          "truncations:", n_trunc)
    reset_rows = torch.cat(reset_rows)
    assert reset_rows.shape[0] >= 2
    # different envs / steps draw different fresh states
    assert int(torch.unique(reset_rows, dim=0).shape[0]) == reset_rows.shape[0]
    return tc, epr, finished, n_term, n_wall, n_trunc, n_band


@pytest.mark.parametrize("hidden,activation", [((16,), "relu"),
                                               ((64, 64), "tanh")])
@pytest.mark.parametrize("game", GAMES)
def test_replay_of_every_transition(game, hidden, activation):
    E, T = 130, 48
    pi, env, epr_dev = make_case(game, hidden, activation, E, spread=True,
                                 time_limit=11, stagger=True, state_seed=5)
    t0, epr0 = env.t.clone(), epr_dev.clone()
    x0 = env.x.clone()
    o = run_kernel(pi, env, epr_dev, T)
    assert torch.equal(o["states"][0], x0)
    tc, epr, finished, n_term, n_wall, n_trunc, n_band = replay(
        game, env, o, t0, epr0, T)
    assert n_band <= 0.01 * T * E
    assert n_term >= 10 and n_wall >= 10 and n_trunc >= 10, (
        n_term, n_wall, n_trunc)
    if game == CAT:
        assert set(o["actions"].unique().tolist()) == {0, 1, 2}
    else:   # forces on both sides of the clip
        a = o["actions"]
        assert int((a.abs() > 1.0).sum()) >= 100
        assert int((a.abs() < 1.0).sum()) >= 100
    # persisted per-env state (env.x was checked against the replay above)
    assert torch.equal(env.t.long(), tc)
    torch.testing.assert_close(epr_dev, epr, atol=1e-4, rtol=1e-4)
    assert torch.equal(env.s, env.x)
    assert bool((env.s[:, 0] >= MIN_POS - 1e-6).all())
    assert bool((env.s[:, 0] <= 0.6 + 1e-6).all())
    assert bool((env.s[:, 1].abs() <= 0.07 + 1e-6).all())
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


# ---- the dynamics' signs, inside the kernel -----------------------------------

def pumping_policy(game, device="cuda"):
    """(16,) tanh trunk set by hand: unit 0 = tanh(1000 v), every other unit
    0; logits (-20 h, 0, 20 h), or mean = h with logstd = -5: push along the
    velocity."""
    space = ENV[game](1).action_space
    pi = PolicyValueMLP(obs_dim=2, action_space=space, hidden_sizes=(16,),
                        activation="tanh").to(device)
    with torch.no_grad():
        for m in [*pi.hidden, pi.vf, pi.pi]:
            m.weight.zero_()
            m.bias.zero_()
        pi.hidden[0].weight[0, 1] = 1000.0
        if game == CAT:
            pi.pi.weight[0, 0] = -20.0
            pi.pi.weight[2, 0] = 20.0
        else:
            pi.pi.weight[0, 0] = 1.0
            pi.pi.bias[1] = -5.0
    return pi


@pytest.mark.parametrize("game", GAMES)
def test_pumping_policy_climbs_the_hill_in_the_kernel(game):
    """With the torch reference under the same policy, three seeds:
    MountainCar-v0 finishes 420-430 episodes, all by the goal, mean return
    -116.8..-118.1; MountainCarContinuous-v0 568-578 episodes, returns
    89.2..92.65.  The bounds leave room for the kernel's own RNG; a sign
    error in gravity or force finishes no episode by the goal."""
    E, T = 256, 256
    env = ENV[game](E, device="cuda", seed=3)
    env.reset()
    epr = torch.zeros(E, device="cuda")
    o = run_kernel(pumping_policy(game), env, epr, T)
    count, total, _, lo, hi = (float(v) for v in o["moments"])
    print(game, "episodes:", count, "mean return:", total / max(count, 1.0),
          "min:", lo, "max:", hi)
    if game == CAT:
        assert count >= 256
        assert -135.0 <= total / count <= -100.0
    else:
        assert count >= 384
        assert lo >= 85.0 and hi <= 95.0


# ---- sampling ------------------------------------------------------------------

def assert_counts_follow(logits, actions):
    """|count_j - sum_n p_nj| <= 5 sqrt(sum_n p_nj (1 - p_nj)): the count of
    class j is a sum of independent Bernoulli(p_nj), so this is its 5 sigma
    bound (derived, not tuned)."""
    p = torch.softmax(logits.reshape(-1, 3).double(), dim=-1)
    counts = torch.bincount(actions.reshape(-1), minlength=3).double()
    bound = 5.0 * (p * (1.0 - p)).sum(dim=0).sqrt()
    diff = (counts - p.sum(dim=0)).abs()
    assert bool((diff <= bound).all()), (counts.tolist(), p.sum(0).tolist(),
                                        bound.tolist())


def test_discrete_sampling_follows_recorded_logits():
    pi, env, epr = make_case(CAT, (16,), "relu", 512, spread=True,
                             state_seed=31)
    o = run_kernel(pi, env, epr, 16)
    logits, actions = o["pdflats"], o["actions"]
    p = torch.softmax(logits, -1)
    # neither uniform nor one-hot, and every class is drawn
    assert 0.4 < float(p.max(dim=-1).values.mean()) < 0.999
    assert float(p.reshape(-1, 3).mean(dim=0).min()) > 0.02
    assert_counts_follow(logits, actions)
    # step 0 alone, across envs: an RNG ignoring the env index fails here
    assert_counts_follow(logits[0], actions[0])
    # envs 0..7 across 256 steps: an RNG ignoring the step index fails here
    pi, env, epr = make_case(CAT, (16,), "relu", 64, spread=True,
                             state_seed=32)
    o = run_kernel(pi, env, epr, 256)
    assert_counts_follow(o["pdflats"][:, :8], o["actions"][:, :8])


def test_discrete_full_exploration_is_uniform_over_three_classes():
    E, T = 512, 16
    N = E * T
    # eps = 1: the overlay redraws every action uniformly over K = 3, against
    # a policy that would always choose class 2
    pi, env, epr = make_case(CAT, (16,), "relu", E, bias_class=2)
    actions = run_kernel(pi, env, epr, T, eps=1.0)["actions"]
    counts = torch.bincount(actions.reshape(-1), minlength=3).double()
    sigma = math.sqrt(N * (1.0 / 3.0) * (2.0 / 3.0))
    assert float((counts - N / 3.0).abs().max()) <= 5.0 * sigma, counts
    # eps = 0: the +40 logit of the third column always wins
    pi, env, epr = make_case(CAT, (16,), "relu", E, bias_class=2)
    assert bool((run_kernel(pi, env, epr, T)["actions"] == 2).all())


def test_continuous_sampling_is_standard_normal_about_the_mean():
    E, T = 512, 16
    N = E * T
    pi, env, epr = make_case(BOX, (16,), "relu", E, spread=True,
                             state_seed=33)
    o = run_kernel(pi, env, epr, T)
    mean, logstd = o["pdflats"].double().unbind(-1)
    assert float(mean.std()) > 1e-2 and float(logstd.std()) > 1e-2
    z = ((o["actions"][..., 0].double() - mean) / logstd.exp()).reshape(-1)
    # the mean of N standard normals has sigma 1 / sqrt(N); their mean
    # square has sigma sqrt(2 / N)
    assert abs(float(z.mean())) <= 5.0 / math.sqrt(N)
    assert abs(float(z.var()) - 1.0) <= 5.0 * math.sqrt(2.0 / N)


def test_continuous_full_exploration_is_uniform():
    E, T = 512, 16
    N = E * T
    pi, env, epr = make_case(BOX, (16,), "relu", E, spread=True)
    a = run_kernel(pi, env, epr, T, eps=1.0)["actions"].double().reshape(-1)
    assert float(a.min()) >= -1.0 and float(a.max()) <= 1.0
    # uniform on [-1, 1]: mean 0 with variance 1/3; a^2 has mean 1/3 and
    # variance 1/5 - 1/9 = 4/45
    assert abs(float(a.mean())) <= 5.0 * math.sqrt(1.0 / (3.0 * N))
    assert abs(float((a * a).mean()) - 1.0 / 3.0) <= 5.0 * math.sqrt(
        4.0 / (45.0 * N))


# ---- determinism --------------------------------------------------------------

@pytest.mark.parametrize("game", GAMES)
def test_same_seed_is_bitwise_and_other_seed_differs(game):
    def run(seed):
        pi, env, epr = make_case(game, (32,), "tanh", 130, spread=True,
                                 time_limit=11, state_seed=41)
        o = run_kernel(pi, env, epr, 24, eps=0.2, seed=seed)
        return o, (env.s, env.x, env.t, epr)

    a, pa = run(5)
    b, pb = run(5)
    for k in NAMES:
        assert torch.equal(a[k], b[k]), k
    for u, w in zip(pa, pb):
        assert torch.equal(u, w)
    # the continuous env's returns are sums of non-trivial floats
    assert float(a["moments"][0]) > 0
    c, _ = run(6)
    assert not torch.equal(a["actions"], c["actions"])


# ---- binding checks -------------------------------------------------------------

@pytest.mark.parametrize("env_id,n_actions", [(3, 2), (4, 3)])
def test_cat_rejects_unsupported_pairs(env_id, n_actions):
    """Host-side checks: nothing is launched, the env tensors are untouched."""
    pi, env, epr = make_case(CAT, (16,), "relu", 4)
    blob, offsets, dims = weight_blob(pi)
    s0, x0, t0 = env.s.clone(), env.x.clone(), env.t.clone()
    with pytest.raises(RuntimeError, match=r"\(0, 2\).*\(2, 3\).*\(3, 3\)"):
        require_hip_ext().classic_rollout_cat(
            blob, offsets, dims, 0, env_id, env.s, env.time_limit, 0.0,
            env.x, env.t, epr, 4, n_actions, 1, torch.empty(0, device="cuda"))
    assert torch.equal(env.s, s0) and torch.equal(env.x, x0)
    assert torch.equal(env.t, t0)


@pytest.mark.parametrize("env_id", [0, 3])
def test_box_rejects_other_envs(env_id):
    pi, env, epr = make_case(BOX, (16,), "relu", 4)
    blob, offsets, dims = weight_blob(pi)
    s0, x0, t0 = env.s.clone(), env.x.clone(), env.t.clone()
    with pytest.raises(RuntimeError, match=r"env_id 1 .* 4 "):
        require_hip_ext().classic_rollout_box(
            blob, offsets, dims, 0, env_id, env.s, env.time_limit, -1.0, 1.0,
            0.0, env.x, env.t, epr, 4, 1, 1, torch.empty(0, device="cuda"))
    assert torch.equal(env.s, s0) and torch.equal(env.x, x0)
    assert torch.equal(env.t, t0)


# ---- engine level ---------------------------------------------------------------

def make_engine(game, **kw):
    base = dict(
        GAME=game, ENV_DYNAMICS="physics", HIDDEN_SIZES=(16,),
        ACTIVATION="relu", NUM_ENVS=128, MAX_EPOCH_STEPS=32, EPOCH_MAX=1000,
        STOP_EPOCH=1000, NUM_WORKERS=1,
        LOG_FILE_PATH="/tmp/dppo_gpu_test_logs", DEVICE="cuda",
    )
    base.update(kw)
    eng = DPPOEngine(DPPOConfig(**base), comm=Comm(device="cuda:0"))
    assert type(eng.env) is CLASSIC_ENVS[game]
    near_the_limit(eng)
    return eng


def near_the_limit(eng):
    """No MountainCar episode of an untrained policy ends inside a 32-step
    rollout of fresh envs, and the continuous env's 999 steps outlast a
    round's 16 retries as well: move every counter to 20 steps before the
    limit, so that the next rollout finishes episodes."""
    eng.env.t.clamp_(min=eng.env.time_limit - 20)


ENGINE_CASES = [
    dict(HIDDEN_SIZES=(16,), ACTIVATION="relu"),
    dict(HIDDEN_SIZES=(64, 64), ACTIVATION="tanh"),
]


@pytest.mark.parametrize("kw", ENGINE_CASES, ids=["h16", "h64x64"])
@pytest.mark.parametrize("game", [CAT, BOX, "CartPole-v1"])
def test_engine_takes_the_classic_rollout(game, kw, monkeypatch):
    monkeypatch.delenv("DPPO_ROLLOUT_CLASSIC", raising=False)

    def boom(self):
        raise AssertionError("eager loop entered on an eligible physics env")

    with monkeypatch.context() as m:
        m.setattr(DPPOEngine, "_rollout_once_eager_loop", boom)
        eng = make_engine(game, **kw)
        assert eng._can_rollout_classic() and eng._use_rollout_classic()
        assert not eng._can_fuse_rollout() and not eng._can_rollout_v3()
        assert not eng._can_fuse_rollout_cat()
        assert not eng._can_fuse_rollout_multi()
        # the fused update, graphed: its batch is the kernel's blob
        assert eng._can_fuse_update() and eng._batch_is_persistent()
        p0 = eng.flat_pi.flat_param.detach().clone()
        for _ in range(2):
            near_the_limit(eng)
            stats, _ = eng.train_round()
            assert all(math.isfinite(v) for v in stats.values())
        assert eng.classic_rollout_launches >= 2
        assert not torch.equal(p0, eng.flat_pi.flat_param.detach())
        if game != BOX:     # the fused Discrete update was captured
            assert eng._upd_graph is not None and not eng._graph_failed

    monkeypatch.setenv("DPPO_ROLLOUT_CLASSIC", "0")
    ref = make_engine(game, **kw)
    assert ref._can_rollout_classic() and not ref._use_rollout_classic()
    stats, _ = ref.train_round()
    assert all(math.isfinite(v) for v in stats.values())
    assert ref.classic_rollout_launches == 0
