"""Real MountainCar-v0 and MountainCarContinuous-v0 dynamics, and the
CartPole-v1 registration (envs/classic.py: mountaincar_step,
mountaincar_cont_step, BatchedMountainCar, BatchedMountainCarContinuous,
BatchedCartPoleV1), on the CPU: config wiring, one step against an independent
float64 transcription of gym's equations, the termination and left-wall rules,
time limits and the off-centre reset, and the hill climbed by a known
energy-pumping policy.

State tolerance 1e-6 (atol, rtol 0): a step is at most about five float32
roundings of values <= 1.2, each half an ulp (6e-8), so 3e-7 bounds it.
Continuous reward tolerance 2e-5: one ulp at 100 is 7.6e-6.  Termination, the
wall rule and the clamps are exact outside three bands in which float32 and
float64 may fall on different sides: |z - goal| < 1e-6, |z + 1.2| < 1e-6 (z
the unclamped new position) and |v'| < 1e-7 next to the goal; at most 1 % of
the grid may lie inside them.
"""

import math

import pytest
import torch

from dppo_amd import spaces
from dppo_amd.config import GAME_SHAPES, PHYSICS_GAMES, DPPOConfig
from dppo_amd.envs import (BatchedAcrobot, BatchedCartPole, BatchedCartPoleV1,
                           BatchedMountainCar, BatchedMountainCarContinuous,
                           BatchedPendulum, make_env)
from dppo_amd.envs.classic import (CLASSIC_ENVS, MOUNTAINCAR,
                                   MOUNTAINCAR_CONT, mountaincar_cont_step,
                                   mountaincar_step)
from dppo_amd.parallel.comm import Comm
from dppo_amd.trainer import DPPOEngine

STATE_TOL = dict(atol=1e-6, rtol=0.0)
REWARD_TOL = dict(atol=2e-5, rtol=0.0)
POS_BAND = 1e-6
VEL_BAND = 1e-7
N_GRID = 6000
F32_MIN_POS = torch.tensor(-1.2, dtype=torch.float32)
F32_MAX_POS = torch.tensor(0.6, dtype=torch.float32)

DISCRETE, CONTINUOUS = "MountainCar-v0", "MountainCarContinuous-v0"
STEP = {DISCRETE: mountaincar_step, CONTINUOUS: mountaincar_cont_step}
ENV = {DISCRETE: BatchedMountainCar, CONTINUOUS: BatchedMountainCarContinuous}


# ---- float64 oracle: gym's formulation, symbolic constants -------------------

def mountaincar_oracle(game, s, a):
    """s [N, 2], a [N] -> dict of float64 results after gym's step(): the
    unclamped new position z, the new state, reward, termination flag."""
    min_position, max_position, max_speed = -1.2, 0.6, 0.07
    goal_velocity = 0.0
    position, velocity = s.double().unbind(-1)
    a = a.double()
    if game == DISCRETE:
        force, gravity, goal_position = 0.001, 0.0025, 0.5
        velocity = (velocity + (a - 1.0) * force
                    + torch.cos(3.0 * position) * (-gravity))
    else:
        power, goal_position = 0.0015, 0.45
        min_action, max_action = -1.0, 1.0
        force = torch.minimum(torch.maximum(a, torch.tensor(min_action).double()),
                              torch.tensor(max_action).double())
        velocity = (velocity + force * power
                    - 0.0025 * torch.cos(3.0 * position))
    velocity = torch.where(velocity > max_speed, max_speed, velocity)
    velocity = torch.where(velocity < -max_speed, -max_speed, velocity)
    z = position + velocity
    position = torch.where(z > max_position, max_position, z)
    position = torch.where(position < min_position, min_position, position)
    wall = (position == min_position) & (velocity < 0)
    velocity = torch.where(wall, 0.0, velocity)
    term = (position >= goal_position) & (velocity >= goal_velocity)
    if game == DISCRETE:
        reward = torch.full_like(z, -1.0)
    else:
        reward = torch.where(term, 100.0, 0.0) - a ** 2 * 0.1
    band = ((z - goal_position).abs() < POS_BAND) \
        | ((z - min_position).abs() < POS_BAND) \
        | ((velocity.abs() < VEL_BAND)
           & (position >= goal_position - POS_BAND))
    return dict(z=z, s2=torch.stack([position, velocity], dim=-1),
                reward=reward, term=term, wall=wall, band=band,
                right=z > max_position)


def grid_for(game, seed):
    gen = torch.Generator().manual_seed(seed)
    u = torch.rand(N_GRID, 3, generator=gen)
    s = torch.stack([-1.2 + 1.8 * u[:, 0], -0.07 + 0.14 * u[:, 1]],
                    dim=-1).float()
    s[:, 0] = s[:, 0].clamp(-1.2, 0.6)
    s[:, 1] = s[:, 1].clamp(-0.07, 0.07)
    if game == DISCRETE:
        a = torch.randint(3, (N_GRID,), generator=gen)
        a[:3] = torch.arange(3)
    else:
        a = (-1.5 + 3.0 * u[:, 2]).float()      # raw, beyond the clip
    return s, a


@pytest.fixture(scope="module", params=[DISCRETE, CONTINUOUS])
def grid(request):
    """6000 rows with their oracle and float32 results."""
    game = request.param
    s, a = grid_for(game, seed=11)
    return game, s, a, mountaincar_oracle(game, s, a), STEP[game](s, a)


# ---- config wiring -----------------------------------------------------------

WIRING = [
    (DISCRETE, BatchedMountainCar, 3, 2, 2, "discrete", 3, 200),
    (CONTINUOUS, BatchedMountainCarContinuous, 4, 2, 2, "box", 1, 999),
    ("CartPole-v1", BatchedCartPoleV1, 0, 4, 4, "discrete", 2, 500),
]


@pytest.mark.parametrize("game,cls,env_id,obs_dim,S,kind,n,limit", WIRING,
                         ids=[w[0] for w in WIRING])
def test_physics_config_and_env_wiring(game, cls, env_id, obs_dim, S, kind, n,
                                       limit):
    # raises without the feature: the game has no shape and no physics
    cfg = DPPOConfig(GAME=game, ENV_DYNAMICS="physics", NUM_ENVS=5)
    assert game in PHYSICS_GAMES and GAME_SHAPES[game] == (obs_dim, kind, n)
    env = make_env(cfg, "cpu", 0)
    assert type(env) is cls and env.num_envs == 5
    assert CLASSIC_ENVS[game] is cls
    assert env.ENV_ID == env_id
    assert env.obs_dim == obs_dim
    if kind == "discrete":
        assert isinstance(env.action_space, spaces.Discrete)
        assert env.action_space.n == n
    else:
        assert isinstance(env.action_space, spaces.Box)
        assert env.action_space.shape == (n,)
    assert env.time_limit == limit
    assert bool((env.horizons_i32 == limit).all())
    assert env.reset().shape == (5, obs_dim) and env.s.shape == (5, S)
    assert cls(2, time_limit=9).time_limit == 9
    assert cls(2).time_limit == limit


def test_env_ids_and_the_registrations_that_stay():
    assert (MOUNTAINCAR, MOUNTAINCAR_CONT) == (3, 4)
    assert issubclass(BatchedCartPoleV1, BatchedCartPole)
    assert BatchedCartPoleV1.GAME == "CartPole-v1"
    assert BatchedCartPole(2).time_limit == 200
    assert BatchedCartPole.GAME == "CartPole-v0"
    assert CLASSIC_ENVS["CartPole-v0"] is BatchedCartPole
    assert len(CLASSIC_ENVS) == 6
    # synthetic presets of the new names exist as well
    for game in (DISCRETE, CONTINUOUS, "CartPole-v1"):
        DPPOConfig(GAME=game)


# ---- one step against the float64 oracle ------------------------------------

def test_one_step_matches_float64(grid):
    game, s, a, want, (s2, reward, term) = grid
    clear = ~want["band"]
    print(game, "rows inside a band:", int(want["band"].sum()))
    assert int(want["band"].sum()) <= 0.01 * N_GRID
    err = (s2.double() - want["s2"])[clear].abs().max()
    print("max |state - oracle| =", float(err))
    torch.testing.assert_close(s2.double()[clear], want["s2"][clear],
                               **STATE_TOL)
    if game == DISCRETE:
        assert set(a.tolist()) == {0, 1, 2}
        assert torch.equal(reward, torch.full((N_GRID,), -1.0))
    else:
        # the clip and the unclipped penalty both show
        assert int((a.abs() > 1.0).sum()) >= 100
        assert int((a.abs() < 1.0).sum()) >= 100
        rerr = (reward.double() - want["reward"])[clear].abs().max()
        print("max |reward - oracle| =", float(rerr))
        torch.testing.assert_close(reward.double()[clear],
                                   want["reward"][clear], **REWARD_TOL)
        # a raw action of 1.5 costs 0.225, not the 0.1 of the clipped force
        big = (a.abs() > 1.4) & ~want["term"] & clear
        assert int(big.sum()) >= 20
        assert bool((reward[big] < -0.19).all())


def test_termination_wall_and_clamps_are_exact_outside_the_bands(grid):
    game, s, a, want, (s2, reward, term) = grid
    clear = ~want["band"]
    assert torch.equal(term[clear], want["term"][clear])
    n_term = int((want["term"] & clear).sum())
    wall = want["wall"] & clear
    right = want["right"] & (want["z"] > 0.6 + POS_BAND)
    print(game, "terminating:", n_term, "wall:", int(wall.sum()),
          "right clamp:", int(right.sum()))
    assert n_term >= 20 and int(wall.sum()) >= 20 and int(right.sum()) >= 20
    # on the wall: position exactly float32(-1.2), velocity exactly 0
    assert bool((s2[wall, 0] == F32_MIN_POS).all())
    assert bool((s2[wall, 1] == 0.0).all())
    # nowhere else is a moving car stopped
    moving = clear & ~want["wall"] & (want["s2"][:, 1].abs() > 1e-6)
    assert bool((s2[moving, 1] != 0.0).all())
    assert bool((s2[right, 0] == F32_MAX_POS).all())
    assert bool((s2[:, 0] >= F32_MIN_POS).all())
    assert bool((s2[:, 0] <= F32_MAX_POS).all())
    assert bool((s2[:, 1].abs() <= torch.tensor(0.07).float()).all())
    # a car past the goal but rolling back has not arrived
    goal = 0.5 if game == DISCRETE else 0.45
    back = clear & (want["s2"][:, 0] >= goal) & (want["s2"][:, 1] < -VEL_BAND)
    assert int(back.sum()) >= 5 and not bool(term[back].any())


# ---- bookkeeping ---------------------------------------------------------------

def in_reset_range(s):
    return bool(((s[:, 0] > -0.6) & (s[:, 0] <= -0.4)).all()
                and (s[:, 1] == 0.0).all())


@pytest.mark.parametrize("game", [DISCRETE, CONTINUOUS])
@pytest.mark.parametrize("limit", [None, 7])
def test_time_limit_truncates_and_resets(game, limit):
    E = 16
    cls = ENV[game]
    env = cls(E, seed=5) if limit is None else cls(E, seed=5, time_limit=limit)
    L = cls.TIME_LIMIT if limit is None else limit
    assert env.time_limit == L
    env.reset()
    assert in_reset_range(env.s)
    assert int(torch.unique(env.s[:, 0]).numel()) == E
    # no push from rest in the valley: the car never gets out
    a = (torch.ones(E, dtype=torch.long) if game == DISCRETE
         else torch.zeros(E, 1))
    steps = L + 3 if limit is None else 3 * L
    for step in range(steps):
        s_before = env.s.clone()
        x, r, done, _ = env.step(a)
        assert bool(done.all()) == bool(done.any()) == (step % L == L - 1)
        assert bool((r == (-1.0 if game == DISCRETE else 0.0)).all())
        assert bool((env.t == (step + 1) % L).all())
        assert x is env.x and torch.equal(x, env.s)
        if step % L == L - 1:
            # the observation on a done step is the fresh one
            assert in_reset_range(x)
            assert not torch.equal(env.s, s_before)
            assert int(torch.unique(env.s[:, 0]).numel()) == E


def test_terminating_step_resets_and_pays(grid):
    game, s, a, want, (s2, reward, term) = grid
    n = 2048
    env = ENV[game](n, seed=1)
    env.reset()
    env.s = s[:n].clone()
    x, r, done, _ = env.step(a[:n])
    assert torch.equal(done, term[:n]) and int(done.sum()) >= 20
    assert torch.equal(r, reward[:n])
    if game == DISCRETE:
        assert bool((r == -1.0).all())
    else:
        af = a[:n]
        torch.testing.assert_close(r[done], 100.0 - 0.1 * af[done] ** 2,
                                   **REWARD_TOL)
        torch.testing.assert_close(r[~done], -0.1 * af[~done] ** 2,
                                   **REWARD_TOL)
    assert torch.equal(x[~done], s2[:n][~done])
    assert in_reset_range(x[done])
    assert bool((env.t[done] == 0).all()) and bool((env.t[~done] == 1).all())


@pytest.mark.parametrize("cls", [BatchedCartPole, BatchedPendulum,
                                 BatchedAcrobot])
def test_symmetric_resets_keep_their_bits(cls):
    """seed_state of the three symmetric envs == (2u - 1) * half, recomputed
    from the same generator, bit for bit (-0.0 and 0.0 told apart)."""
    E = 257
    env = cls(E, seed=13)
    gen = torch.Generator().manual_seed(13)
    half = torch.tensor(cls.RESET_HALF)
    for _ in range(3):
        u = 1.0 - torch.rand(E, cls.S, generator=gen)
        want = (2.0 * u - 1.0) * half
        got = env.seed_state()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ---- dynamics sanity -----------------------------------------------------------

def first_arrivals(env, policy, steps):
    """Step of each env's first done (0: none) and the return it ended on."""
    E = env.num_envs
    env.reset()
    first = torch.zeros(E, dtype=torch.long)
    ret = torch.zeros(E)
    epr = torch.zeros(E)
    for step in range(steps):
        live = first == 0
        _, r, done, _ = env.step(policy(env.s))
        epr = epr + r
        hit = live & done
        first = torch.where(hit, torch.tensor(step + 1), first)
        ret = torch.where(hit, epr, ret)
    return first, ret


def test_energy_pumping_policy_reaches_the_goal():
    """Pushing along the velocity (right from rest) pumps energy into the
    swing.  On 1024 envs every MountainCar-v0 episode reached the goal in
    113..125 steps (median 121), every continuous one in 105..111 (mean
    return 89.3); no uniform-random MountainCar-v0 episode reached it inside
    the 200-step limit.  A sign error in gravity or force fails one of the
    assertions."""
    E = 1024
    first, _ = first_arrivals(
        BatchedMountainCar(E, seed=4),
        lambda s: torch.where(s[:, 1] >= 0, 2, 0), 200)
    hit = first[(first > 0) & (first < 200)]    # step 200 is the truncation
    print("MountainCar-v0 reached:", hit.numel() / E, "steps:",
          int(hit.min()), "..", int(hit.max()), "median", float(hit.median()))
    assert hit.numel() >= 0.95 * E and int(hit.min()) >= 80

    first, ret = first_arrivals(
        BatchedMountainCarContinuous(E, seed=4),
        lambda s: torch.where(s[:, 1] >= 0, 1.0, -1.0), 200)
    ok = first > 0                              # the limit is 999: no truncation
    hit = first[ok]
    print("MountainCarContinuous-v0 reached:", hit.numel() / E, "steps:",
          int(hit.min()), "..", int(hit.max()), "mean return",
          float(ret[ok].mean()))
    assert hit.numel() >= 0.95 * E and int(hit.min()) >= 80
    # full force costs 0.1 per step and the goal pays 100
    torch.testing.assert_close(ret[ok], 100.0 - 0.1 * hit.float(),
                               atol=1e-3, rtol=0.0)

    gen = torch.Generator().manual_seed(9)
    first, _ = first_arrivals(
        BatchedMountainCar(E, seed=4),
        lambda s: torch.randint(3, (E,), generator=gen), 200)
    reached = int(((first > 0) & (first < 200)).sum())
    print("random policy reached:", reached / E)
    assert reached < 0.05 * E


# ---- engine --------------------------------------------------------------------

@pytest.mark.parametrize("game", [DISCRETE, CONTINUOUS, "CartPole-v1"])
def test_cpu_round_is_finite_and_never_takes_the_kernel(game, monkeypatch):
    monkeypatch.setenv("DPPO_ROLLOUT_CLASSIC", "1")
    cfg = DPPOConfig(
        GAME=game, ENV_DYNAMICS="physics", NUM_ENVS=8,
        MAX_EPOCH_STEPS=16, HIDDEN_SIZES=(16,), ACTIVATION="tanh",
        EPOCH_MAX=60, NUM_WORKERS=1, SEED=0,
        LOG_FILE_PATH="/tmp/dppo_test_logs", DEVICE="cpu")
    eng = DPPOEngine(cfg, comm=Comm(device="cpu"))
    assert type(eng.env) is CLASSIC_ENVS[game]
    assert not eng._can_rollout_classic() and not eng._use_rollout_classic()
    # no episode of an untrained policy ends inside a 16-step rollout of
    # fresh envs, so start the counters near the limit
    eng.env.t += eng.env.time_limit - 10
    stats, stop = eng.train_round()
    assert not stop
    assert all(math.isfinite(v) for v in stats.values())
    assert eng.classic_rollout_launches == 0
    # the greedy eval loop's step: one env of the game's class, act() on a row
    env = CLASSIC_ENVS[game](1, device="cpu", seed=1)
    x = env.reset()
    for _ in range(3):
        x, r, done, _ = env.step(eng.act(x[0]).unsqueeze(0))
        assert x.shape == (1, env.obs_dim) and math.isfinite(float(r[0]))
