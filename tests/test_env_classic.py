"""Real CartPole / Pendulum dynamics (envs/classic.py) on the CPU: config
wiring, one-step physics against an independent float64 transcription of the
equations, time limits, terminations, resets, and PPO learning CartPole.

Tolerance 3e-5 (atol = rtol) is the project's env-transition tolerance.
"""

import math

import pytest
import torch

from dppo_amd.config import DPPOConfig
from dppo_amd.envs import BatchedSyntheticEnv, make_env
from dppo_amd.envs.classic import (BatchedCartPole, BatchedPendulum,
                                   cartpole_step, pendulum_obs, pendulum_step)
from dppo_amd.parallel.comm import Comm
from dppo_amd.trainer import DPPOEngine

TOL = dict(atol=3e-5, rtol=3e-5)


# ---- float64 oracles, transcribed from the issue's equations ----------------

def cartpole_oracle(s, a):
    """s [N, 4] float64, a [N] -> (s' float64, terminated bool)."""
    x, xd, th, thd = s.double().unbind(-1)
    F = torch.where(a == 1, 10.0, -10.0).double()
    sin, cos = torch.sin(th), torch.cos(th)
    temp = (F + 0.05 * thd ** 2 * sin) / 1.1
    thacc = (9.8 * sin - cos * temp) / (0.5 * (4.0 / 3.0 - 0.1 * cos ** 2 / 1.1))
    xacc = temp - 0.05 * thacc * cos / 1.1
    s2 = torch.stack([x + 0.02 * xd, xd + 0.02 * xacc, th + 0.02 * thd,
                      thd + 0.02 * thacc], dim=-1)
    term = (s2[:, 0].abs() > 2.4) | (s2[:, 2].abs() > 0.20943951)
    return s2, term


def pendulum_oracle(s, a):
    """s [N, 2] float64, a [N] -> (s', reward, pre-wrap angle z)."""
    th, thd = s.double().unbind(-1)
    u = 2.0 * a.double().clamp(-1.0, 1.0)
    r = -(th ** 2 + 0.1 * thd ** 2 + 0.001 * u ** 2)
    thd2 = (thd + (15.0 * torch.sin(th) + 3.0 * u) * 0.05).clamp(-8.0, 8.0)
    z = th + 0.05 * thd2
    th2 = z - 2.0 * math.pi * torch.floor((z + math.pi) / (2.0 * math.pi))
    return torch.stack([th2, thd2], dim=-1), r, z


def cartpole_grid():
    """64 states: a 4 x 2 x 4 x 2 grid whose last 8 rows are replaced by
    states whose next x / theta lands 1e-3 inside and 1e-3 outside each of
    the four termination bounds."""
    g = torch.cartesian_prod(
        torch.tensor([-2.0, -0.7, 0.7, 2.0]), torch.tensor([-1.5, 1.5]),
        torch.tensor([-0.15, -0.05, 0.05, 0.15]), torch.tensor([-2.0, 2.0]))
    edge = []
    for sign in (1.0, -1.0):
        for off in (-1e-3, 1e-3):   # inside, outside
            # x' = x + 0.02 * xd with xd = 1.5 * sign
            edge.append([sign * (2.4 - 0.03 + off), sign * 1.5, 0.01, 0.0])
            # theta' = theta + 0.02 * thd with thd = 1.0 * sign
            edge.append([0.1, 0.0, sign * (0.20943951 - 0.02 + off),
                         sign * 1.0])
    g[-8:] = torch.tensor(edge)
    return g.float()


# ---- config wiring -----------------------------------------------------------

def test_physics_config_constructs():
    cfg = DPPOConfig(ENV_DYNAMICS="physics")
    assert cfg.ENV_DYNAMICS == "physics" and cfg.GAME == "CartPole-v0"
    assert DPPOConfig().ENV_DYNAMICS == "synthetic"
    assert DPPOConfig.from_dict(
        {"GAME": "Pendulum-v1", "ENV_DYNAMICS": "physics"}
    ).ENV_DYNAMICS == "physics"


def test_bad_dynamics_value_raises():
    with pytest.raises(ValueError):
        DPPOConfig(ENV_DYNAMICS="mujoco")


def test_physics_without_a_model_raises():
    with pytest.raises(ValueError, match="CartPole-v0.*Pendulum-v1"):
        DPPOConfig(GAME="Humanoid-v4", ENV_DYNAMICS="physics")


def test_default_env_is_still_synthetic():
    assert isinstance(make_env(DPPOConfig(), "cpu", 0), BatchedSyntheticEnv)
    env = make_env(DPPOConfig(ENV_DYNAMICS="physics", NUM_ENVS=5), "cpu", 0)
    assert isinstance(env, BatchedCartPole) and env.num_envs == 5
    assert env.time_limit == 200
    assert bool((env.horizons_i32 == 200).all())
    env = make_env(DPPOConfig(GAME="Pendulum-v1", ENV_DYNAMICS="physics"),
                   "cpu", 0)
    assert isinstance(env, BatchedPendulum)
    assert env.reset().shape == (64, 3) and env.s.shape == (64, 2)
    assert env.t.dtype == torch.int32


# ---- one-step physics ---------------------------------------------------------

@pytest.mark.parametrize("action", [0, 1])
def test_cartpole_one_step_matches_float64(action):
    s = cartpole_grid()
    a = torch.full((64,), action, dtype=torch.long)
    want, term = cartpole_oracle(s, a)
    got, reward, got_term = cartpole_step(s, a)
    torch.testing.assert_close(got.double(), want, **TOL)
    assert bool((reward == 1.0).all())
    assert torch.equal(got_term, term)
    # the 8 edge rows: inside / outside alternate per bound
    assert term[-8:].tolist() == [False, False, True, True] * 2
    # the same through the env object (live rows keep s', done rows reset)
    env = BatchedCartPole(64, time_limit=200)
    env.reset()
    env.s = s.clone()
    x, r, done, _ = env.step(a)
    assert torch.equal(done, term)
    torch.testing.assert_close(x[~done].double(), want[~done], **TOL)
    assert bool((x[done].abs() <= 0.05).all())


def pendulum_states():
    """64 states: |theta| near pi (the wrap) x |theta_dot| near 8 (the
    clip), plus interior values."""
    th = torch.tensor([-(math.pi - 0.01), -(math.pi - 0.15), -3.0, -1.0,
                       1.0, 3.0, math.pi - 0.15, math.pi - 0.01])
    thd = torch.tensor([-7.95, -7.0, -3.0, -0.5, 0.5, 3.0, 7.0, 7.95])
    return torch.cartesian_prod(th, thd).float()


@pytest.mark.parametrize("action", [-3.0, -1.0, 0.0, 0.5, 3.0])
def test_pendulum_one_step_matches_float64(action):
    s = pendulum_states()
    a = torch.full((64, 1), action)
    want, r_want, z = pendulum_oracle(s, a.reshape(-1))
    # the inputs exercise the wrap and the clip, and no pre-wrap angle sits
    # on the wrap boundary, where float32 (error ~1e-6 at this magnitude)
    # and float64 could floor differently
    assert bool((z.abs() > math.pi).any())
    assert bool((want[:, 1].abs() == 8.0).any())
    assert float(((z.abs() - math.pi).abs()).min()) > 1e-4
    got, r, term = pendulum_step(s, a)
    torch.testing.assert_close(got.double(), want, **TOL)
    torch.testing.assert_close(r.double(), r_want, **TOL)
    assert not bool(term.any())
    assert bool((got[:, 0] >= -math.pi).all() and (got[:, 0] < math.pi).all())
    obs = pendulum_obs(got)
    torch.testing.assert_close(
        obs.double(),
        torch.stack([want[:, 0].cos(), want[:, 0].sin(), want[:, 1]], -1),
        **TOL)


# ---- time limit, termination, resets ----------------------------------------

def test_pendulum_time_limit_and_resets():
    E = 16
    env = BatchedPendulum(E, seed=5, time_limit=7)
    env.reset()
    gen = torch.Generator().manual_seed(0)
    for step in range(21):
        a = 4.0 * torch.rand(E, 1, generator=gen) - 2.0
        x, r, done, _ = env.step(a)
        assert bool(done.all()) == (step % 7 == 6)
        assert bool(done.any()) == (step % 7 == 6)
        assert bool((env.t == (step + 1) % 7).all())
        assert float((x[:, 0] ** 2 + x[:, 1] ** 2 - 1.0).abs().max()) <= 1e-5
        assert x is env.x and r.shape == (E,)
        if step % 7 == 6:   # the fresh observation / state
            assert bool((env.s[:, 0].abs() <= math.pi + 1e-6).all())
            assert bool((env.s[:, 1].abs() <= 1.0).all())
            assert bool((x[:, 2].abs() <= 1.0).all())
            assert float(env.s[:, 0].std()) > 0.5   # not all alike


def test_cartpole_constant_push_terminates():
    E = 32
    env = BatchedCartPole(E, seed=2, time_limit=200)
    env.reset()
    assert bool((env.s.abs() <= 0.05).all())
    a = torch.ones(E, dtype=torch.long)
    first_done = torch.full((E,), -1)
    for step in range(20):
        _, term = cartpole_oracle(env.s, a)
        x, r, done, _ = env.step(a)
        assert torch.equal(done, term)
        assert bool((r == 1.0).all())
        assert bool((x[done].abs() <= 0.05).all())
        assert bool((env.t[done] == 0).all())
        first_done = torch.where((first_done < 0) & done,
                                 torch.tensor(step), first_done)
    assert bool((first_done >= 0).all()), first_done.tolist()


# ---- engine -------------------------------------------------------------------

def physics_engine(**kw):
    base = dict(
        GAME="CartPole-v0", ENV_DYNAMICS="physics", NUM_ENVS=64,
        MAX_EPOCH_STEPS=100, HIDDEN_SIZES=(32,), ACTIVATION="tanh",
        LEARNING_RATE=1e-2, EPOCH_MAX=60, NUM_WORKERS=1, SEED=0,
        LOG_FILE_PATH="/tmp/dppo_test_logs", DEVICE="cpu",
    )
    base.update(kw)
    cfg = DPPOConfig(**base)
    return DPPOEngine(cfg, comm=Comm(device=cfg.DEVICE))


def test_ppo_learns_cartpole_on_cpu():
    """A random policy scores about 21 per episode; the prototype reached
    148-175 by round 49 on five seeds, 100 leaves room for another reset
    RNG."""
    eng = physics_engine()
    curve = [eng.train_round()[0]["epr_mean"] for _ in range(50)]
    print("epr_mean by round:", [round(v, 1) for v in curve])
    assert curve[0] < 30.0
    assert max(curve[45:50]) >= 100.0


@pytest.mark.parametrize("game", ["CartPole-v0", "Pendulum-v1"])
def test_cpu_round_is_finite_and_never_takes_the_kernel(game, monkeypatch):
    monkeypatch.setenv("DPPO_ROLLOUT_CLASSIC", "1")
    eng = physics_engine(GAME=game, NUM_ENVS=8, MAX_EPOCH_STEPS=16,
                         HIDDEN_SIZES=(16,))
    assert not eng._can_rollout_classic() and not eng._use_rollout_classic()
    assert not eng._can_fuse_rollout() and not eng._can_fuse_rollout_cat()
    assert not eng._can_fuse_rollout_multi() and not eng._can_rollout_v3()
    stats, stop = eng.train_round()
    assert not stop
    assert all(math.isfinite(v) for v in stats.values())
    assert eng.classic_rollout_launches == 0
