"""Real Acrobot-v1 dynamics (envs/classic.py: acrobot_step, acrobot_obs,
BatchedAcrobot) on the CPU: config wiring, one RK4 step against an independent
float64 transcription of gym's unfolded "book" equations, the velocity clamps,
the angle wrap, time limits and resets, and a swing-up sanity check under a
known energy-pumping policy.

Tolerance 3e-5 (atol = rtol) is the project's env-transition tolerance.  The
comparison grid is bounded (|omega1| <= 4, |omega2| <= 6): on the full
velocity range a float32 RK4 step does not track float64 to 3e-5, so the full
range is used only for the clamps, where the result is an exact bound.
"""

import math

import pytest
import torch

from dppo_amd import spaces
from dppo_amd.config import DPPOConfig
from dppo_amd.envs import BatchedAcrobot, make_env
from dppo_amd.envs.classic import (ACROBOT, CLASSIC_ENVS, BatchedCartPole,
                                   BatchedPendulum, acrobot_obs, acrobot_step)
from dppo_amd.parallel.comm import Comm
from dppo_amd.trainer import DPPOEngine

TOL = dict(atol=3e-5, rtol=3e-5)
PI = math.pi
MAX_VEL_1, MAX_VEL_2 = 4.0 * PI, 9.0 * PI
#: |-cos th1' - cos(th1' + th2') - 1| below this in the oracle: float32 and
#: float64 may fall on different sides of the bar
TERM_BAND = 1e-4


# ---- float64 oracle: gym's unfolded form, symbolic constants ----------------

def _dsdt(y, tau):
    m1 = m2 = l1 = 1.0
    lc1 = lc2 = 0.5
    I1 = I2 = 1.0
    g = 9.8
    th1, th2, w1, w2 = y
    d1 = (m1 * lc1 ** 2
          + m2 * (l1 ** 2 + lc2 ** 2 + 2 * l1 * lc2 * torch.cos(th2))
          + I1 + I2)
    d2 = m2 * (lc2 ** 2 + l1 * lc2 * torch.cos(th2)) + I2
    phi2 = m2 * lc2 * g * torch.cos(th1 + th2 - PI / 2.0)
    phi1 = (-m2 * l1 * lc2 * w2 ** 2 * torch.sin(th2)
            - 2 * m2 * l1 * lc2 * w2 * w1 * torch.sin(th2)
            + (m1 * lc1 + m2 * l1) * g * torch.cos(th1 - PI / 2.0) + phi2)
    a2 = ((tau + d2 / d1 * phi1 - m2 * l1 * lc2 * w1 ** 2 * torch.sin(th2)
           - phi2) / (m2 * lc2 ** 2 + I2 - d2 ** 2 / d1))
    a1 = -(d2 * a2 + phi1) / d1
    return torch.stack([w1, w2, a1, a2])


def acrobot_oracle(s, a):
    """s [N, 4], a [N] -> dict of float64 results: the pre-wrap / pre-clamp
    RK4 result `raw` [N, 4], the new state `s2`, its observation, the bar
    margin -cos th1' - cos(th1' + th2') - 1 and the termination flag."""
    y = s.double().t()
    tau = a.double() - 1.0
    dt = 0.2
    k1 = _dsdt(y, tau)
    k2 = _dsdt(y + dt / 2.0 * k1, tau)
    k3 = _dsdt(y + dt / 2.0 * k2, tau)
    k4 = _dsdt(y + dt * k3, tau)
    raw = y + dt / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    th = raw[:2] - 2.0 * PI * torch.floor((raw[:2] + PI) / (2.0 * PI))
    w1 = raw[2].clamp(-MAX_VEL_1, MAX_VEL_1)
    w2 = raw[3].clamp(-MAX_VEL_2, MAX_VEL_2)
    s2 = torch.stack([th[0], th[1], w1, w2], dim=-1)
    obs = torch.stack([th[0].cos(), th[0].sin(), th[1].cos(), th[1].sin(),
                       w1, w2], dim=-1)
    margin = -th[0].cos() - (th[0] + th[1]).cos() - 1.0
    return dict(raw=raw.t(), s2=s2, obs=obs, margin=margin, term=margin > 0)


def random_states(n, w1_max, w2_max, seed):
    gen = torch.Generator().manual_seed(seed)
    u = torch.rand(n, 4, generator=gen)
    lo = torch.tensor([-PI, -PI, -w1_max, -w2_max])
    hi = torch.tensor([PI, PI, w1_max, w2_max])
    s = (lo + (hi - lo) * u).float()
    s[:, :2] = s[:, :2].clamp(-PI, PI - 1e-6)
    a = torch.randint(3, (n,), generator=gen)
    a[:3] = torch.arange(3)
    return s, a


@pytest.fixture(scope="module")
def moderate():
    """6000 rows of the moderate grid with their oracle and float32 results."""
    s, a = random_states(6000, 4.0, 6.0, seed=11)
    return s, a, acrobot_oracle(s, a), acrobot_step(s, a)


@pytest.fixture(scope="module")
def full_range():
    s, a = random_states(6000, MAX_VEL_1, MAX_VEL_2, seed=12)
    return s, a, acrobot_oracle(s, a), acrobot_step(s, a)


# ---- config wiring -----------------------------------------------------------

def test_acrobot_physics_config_and_env_wiring():
    cfg = DPPOConfig(GAME="Acrobot-v1", ENV_DYNAMICS="physics", NUM_ENVS=5)
    env = make_env(cfg, "cpu", 0)
    assert isinstance(env, BatchedAcrobot) and env.num_envs == 5
    assert env.ENV_ID == ACROBOT == 2
    assert CLASSIC_ENVS["Acrobot-v1"] is BatchedAcrobot
    assert env.obs_dim == 6
    assert isinstance(env.action_space, spaces.Discrete)
    assert env.action_space.n == 3
    assert env.time_limit == 500
    assert bool((env.horizons_i32 == 500).all())
    assert env.reset().shape == (5, 6) and env.s.shape == (5, 4)
    assert BatchedAcrobot(2, time_limit=9).time_limit == 9
    # the other two keep the 200 of their gym registrations
    assert BatchedCartPole(2).time_limit == 200
    assert BatchedPendulum(2).time_limit == 200
    for game in ("CartPole-v0", "Pendulum-v1"):
        e = make_env(DPPOConfig(GAME=game, ENV_DYNAMICS="physics"), "cpu", 0)
        assert e.time_limit == 200


# ---- one step against the float64 oracle ------------------------------------

def test_one_step_matches_float64_on_the_moderate_grid(moderate):
    s, a, want, (s2, reward, term) = moderate
    assert set(a.tolist()) == {0, 1, 2}
    obs = acrobot_obs(s2)
    err = (obs.double() - want["obs"]).abs().max()
    print("max |obs - oracle| =", float(err))
    torch.testing.assert_close(obs.double(), want["obs"], **TOL)
    # rewards are exactly -1, or 0 on a terminating step
    assert torch.equal(reward, torch.where(term, 0.0, -1.0))
    # termination is exact outside the band around the bar
    clear = want["margin"].abs() >= TERM_BAND
    print("rows inside the termination band:", int((~clear).sum()),
          "terminated:", int(want["term"].sum()))
    assert int((~clear).sum()) <= 0.01 * s.shape[0]
    assert torch.equal(term[clear], want["term"][clear])
    assert bool(term.any()) and bool((~term).any())


def test_velocity_clamps_are_exact(full_range):
    s, a, want, (s2, _, _) = full_range
    raw = want["raw"]
    cases = [(2, MAX_VEL_1, 1.0), (2, MAX_VEL_1, -1.0),
             (3, MAX_VEL_2, 1.0), (3, MAX_VEL_2, -1.0)]
    for col, bound, sign in cases:
        rows = sign * raw[:, col] >= bound + 1e-2
        assert int(rows.sum()) >= 5, (col, sign, int(rows.sum()))
        got = s2[rows, col]
        assert bool((got == torch.tensor(sign * bound).float()).all())
    assert bool((s2[:, 2].abs() <= torch.tensor(MAX_VEL_1).float()).all())
    assert bool((s2[:, 3].abs() <= torch.tensor(MAX_VEL_2).float()).all())


def test_wrapped_angles_stay_in_range_and_match(moderate):
    s, a, want, (s2, _, _) = moderate
    raw = want["raw"]
    for col in (0, 1):
        rows = (raw[:, col] < -PI) | (raw[:, col] >= PI)
        # the observation is continuous across the seam, so the comparison
        # below holds even where the two precisions floor differently
        assert int(rows.sum()) >= 5, (col, int(rows.sum()))
        assert bool((s2[rows, col] >= -PI).all())
        assert bool((s2[rows, col] < PI).all())
        torch.testing.assert_close(acrobot_obs(s2)[rows].double(),
                                   want["obs"][rows], **TOL)
    assert bool((s2[:, :2] >= -PI).all() and (s2[:, :2] < PI).all())


# ---- bookkeeping ---------------------------------------------------------------

@pytest.mark.parametrize("limit", [None, 7])
def test_time_limit_truncates_and_resets(limit):
    E = 16
    env = (BatchedAcrobot(E, seed=5) if limit is None
           else BatchedAcrobot(E, seed=5, time_limit=limit))
    L = 500 if limit is None else limit
    assert env.time_limit == L
    env.reset()
    assert bool((env.s.abs() <= 0.1).all())
    assert float(env.s.std()) > 0.01
    # no torque from a near-rest start: nothing reaches the bar
    a = torch.ones(E, dtype=torch.long)
    steps = L + 3 if limit is None else 3 * L
    for step in range(steps):
        s_before = env.s.clone()
        x, r, done, _ = env.step(a)
        assert bool(done.all()) == bool(done.any()) == (step % L == L - 1)
        assert bool((r == -1.0).all())
        assert bool((env.t == (step + 1) % L).all())
        assert x is env.x
        assert torch.equal(x, acrobot_obs(env.s))
        if step % L == L - 1:
            # the observation on a done step is the fresh one
            assert bool((env.s.abs() <= 0.1).all())
            assert not torch.equal(env.s, s_before)
            assert int(torch.unique(env.s, dim=0).shape[0]) == E


def test_terminating_step_resets_and_pays_zero(moderate):
    s, a, want, (s2, reward, term) = moderate
    n = 512
    env = BatchedAcrobot(n, seed=1)
    env.reset()
    env.s = s[:n].clone()
    x, r, done, _ = env.step(a[:n])
    assert torch.equal(done, term[:n]) and bool(done.any())
    assert torch.equal(r, reward[:n])
    assert bool((r[done] == 0.0).all()) and bool((r[~done] == -1.0).all())
    assert torch.equal(x[~done], acrobot_obs(s2[:n])[~done])
    assert bool((env.s[done].abs() <= 0.1).all())
    assert bool((env.t[done] == 0).all()) and bool((env.t[~done] == 1).all())


# ---- dynamics sanity -----------------------------------------------------------

def test_energy_pumping_policy_swings_up():
    """Torque sign(omega2) from reset pumps energy into the second link.  On
    4096 envs 99.8 % terminated within 500 steps, the median at step 75 and
    none before step 65; a uniform-random policy terminated 1.2 %.  A sign
    error in the equations fails one of the two assertions."""
    E = 1024
    env = BatchedAcrobot(E, seed=4)
    env.reset()
    first = torch.full((E,), -1)
    for step in range(500):
        a = torch.where(env.s[:, 3] > 0, 2, 0)
        live = first < 0
        _, _, done, _ = env.step(a)
        first = torch.where(live & done, torch.tensor(step + 1), first)
    hit = first[first > 0]
    print("terminated:", hit.numel() / E, "median:", float(hit.median()),
          "earliest:", int(hit.min()))
    # step 500 is the truncation, not the bar
    assert int((hit < 500).sum()) >= 0.95 * E
    assert int(hit.min()) >= 50


# ---- engine --------------------------------------------------------------------

def test_cpu_round_is_finite_and_never_takes_the_kernel(monkeypatch):
    monkeypatch.setenv("DPPO_ROLLOUT_CLASSIC", "1")
    cfg = DPPOConfig(
        GAME="Acrobot-v1", ENV_DYNAMICS="physics", NUM_ENVS=8,
        MAX_EPOCH_STEPS=16, HIDDEN_SIZES=(16,), ACTIVATION="tanh",
        EPOCH_MAX=60, NUM_WORKERS=1, SEED=0,
        LOG_FILE_PATH="/tmp/dppo_test_logs", DEVICE="cpu")
    eng = DPPOEngine(cfg, comm=Comm(device="cpu"))
    assert isinstance(eng.env, BatchedAcrobot)
    assert not eng._can_rollout_classic() and not eng._use_rollout_classic()
    # a 500-step episode cannot end inside a 16-step rollout of fresh envs,
    # so start the counters near the limit
    eng.env.t += 490
    stats, stop = eng.train_round()
    assert not stop
    assert all(math.isfinite(v) for v in stats.values())
    assert eng.classic_rollout_launches == 0
