"""Batched classic-control environments with real dynamics, resident on the
training device.

The reference steps gym's CartPole-v0 (reference main.py:13, Worker.py:10).
CartPole, Pendulum, Acrobot and the two MountainCars are a dozen closed-form
lines each, so they need no simulator: E envs per rank live as device tensors and step with batched torch
ops (capture-safe, no host sync; this is also the CPU path) or inside the
lane-per-env HIP rollout (ops/hip/classic_rollout.hip), whose device math in
ops/hip/classic_env.h reproduces the float32 expressions below.

CartPole-v0: state = observation = (x, x_dot, theta, theta_dot), Discrete(2),
reward 1 per step, terminates when |x| > 2.4 or |theta| > 12 degrees.
Pendulum-v1: state (theta, theta_dot), observation (cos, sin, theta_dot),
Box(-1, 1, (1,)) scaled to a torque in [-2, 2], never terminates.
Acrobot-v1: state (theta1, theta2, omega1, omega2), observation (cos theta1,
sin theta1, cos theta2, sin theta2, omega1, omega2), Discrete(3) giving a
torque of -1 / 0 / +1 on the second joint, one RK4 step of gym's "book"
dynamics per env step, reward -1 per step until the tip clears the bar
(-cos theta1 - cos(theta1 + theta2) > 1), which terminates with reward 0.
MountainCar-v0: state = observation = (position, velocity), Discrete(3)
pushing left / not at all / right, reward -1 per step, terminates at
position >= 0.5.  MountainCarContinuous-v0: the same hill under a
Box(-1, 1, (1,)) force, terminates at position >= 0.45 with reward 100, and
every step costs 0.1 a^2 of the raw action.  Both start at rest with the
position uniform in (-0.6, -0.4].  CartPole-v1 is CartPole-v0 with a time
limit of 500.
All truncate at `time_limit` steps (200, 200, 500, 200 and 999 by default).  As everywhere in this project the
observation returned on a done step is the fresh one and the reward belongs
to the pre-reset transition.
"""

from __future__ import annotations

import math

import torch

from .. import spaces
from ..config import DPPOConfig, game_spaces

CARTPOLE, PENDULUM = 0, 1       # env ids of the HIP rollout bindings
ACROBOT = 2
MOUNTAINCAR, MOUNTAINCAR_CONT = 3, 4

X_LIMIT = 2.4
THETA_LIMIT = 0.20943951        # 12 degrees
TWO_PI = 2.0 * math.pi


def cartpole_step(s: torch.Tensor, a: torch.Tensor):
    """One Euler step of CartPole from states s [N, 4] under actions a [N]
    (1 pushes right, anything else left): (s' [N, 4], reward [N],
    terminated [N] bool)."""
    x, xd, th, thd = s.unbind(-1)
    force = torch.where(a.reshape(-1) == 1, 10.0, -10.0).to(s.dtype)
    sin, cos = torch.sin(th), torch.cos(th)
    temp = (force + 0.05 * thd * thd * sin) / 1.1
    thacc = (9.8 * sin - cos * temp) / (
        0.5 * (4.0 / 3.0 - 0.1 * cos * cos / 1.1))
    xacc = temp - 0.05 * thacc * cos / 1.1
    tau = 0.02
    s2 = torch.stack(
        [x + tau * xd, xd + tau * xacc, th + tau * thd, thd + tau * thacc],
        dim=-1)
    term = (s2[..., 0].abs() > X_LIMIT) | (s2[..., 2].abs() > THETA_LIMIT)
    return s2, torch.ones_like(x), term


def pendulum_step(s: torch.Tensor, a: torch.Tensor):
    """One step of Pendulum from states s [N, 2] = (theta, theta_dot) under
    actions a [N] or [N, 1]: (s' [N, 2], reward [N], terminated [N] bool,
    never set).  The action is clipped to [-1, 1] here, inside the physics,
    and theta' is wrapped into [-pi, pi)."""
    th, thd = s.unbind(-1)
    u = 2.0 * a.reshape(-1).to(s.dtype).clamp(-1.0, 1.0)
    reward = -(th * th + 0.1 * thd * thd + 0.001 * u * u)
    thd2 = (thd + (15.0 * torch.sin(th) + 3.0 * u) * 0.05).clamp(-8.0, 8.0)
    z = th + 0.05 * thd2
    th2 = z - TWO_PI * torch.floor((z + math.pi) / TWO_PI)
    return (torch.stack([th2, thd2], dim=-1), reward,
            torch.zeros_like(th, dtype=torch.bool))


def pendulum_obs(s: torch.Tensor) -> torch.Tensor:
    th, thd = s.unbind(-1)
    return torch.stack([torch.cos(th), torch.sin(th), thd], dim=-1)


ACROBOT_DT = 0.2
ACROBOT_MAX_VEL_1 = 4.0 * math.pi
ACROBOT_MAX_VEL_2 = 9.0 * math.pi


def _acrobot_deriv(th1, th2, w1, w2, tau):
    """(alpha1, alpha2) of gym's "book" Acrobot with every link constant 1,
    lc = 0.5, I = 1, g = 9.8, the constants folded and cos(x - pi/2) written
    as sin x."""
    s1, s2, c2 = torch.sin(th1), torch.sin(th2), torch.cos(th2)
    d1 = 3.5 + c2
    d2 = 1.25 + 0.5 * c2
    phi2 = 4.9 * torch.sin(th1 + th2)
    phi1 = -0.5 * w2 * w2 * s2 - w2 * w1 * s2 + 14.7 * s1 + phi2
    a2 = (tau + d2 / d1 * phi1 - 0.5 * w1 * w1 * s2 - phi2) / (
        1.25 - d2 * d2 / d1)
    a1 = -(d2 * a2 + phi1) / d1
    return a1, a2


def acrobot_step(s: torch.Tensor, a: torch.Tensor):
    """One classical RK4 step (dt = 0.2, torque a - 1 held constant) of
    Acrobot from states s [N, 4] = (theta1, theta2, omega1, omega2) under
    actions a [N] in {0, 1, 2}: (s' [N, 4], reward [N], terminated [N] bool).
    The angles of s' are wrapped into [-pi, pi), omega1' is clamped to
    +-4 pi and omega2' to +-9 pi; the reward is -1, or 0 on a terminating
    step.  The weighted sum k1 + 2 k2 + 2 k3 + k4 is accumulated stage by
    stage, in this order, as the kernel does."""
    y = s.unbind(-1)
    tau = a.reshape(-1).to(s.dtype) - 1.0
    h = ACROBOT_DT

    def f(th1, th2, w1, w2):
        a1, a2 = _acrobot_deriv(th1, th2, w1, w2, tau)
        return (w1, w2, a1, a2)

    k = f(*y)                                               # k1
    acc = k
    k = f(*(yi + (0.5 * h) * ki for yi, ki in zip(y, k)))   # k2
    acc = tuple(ai + 2.0 * ki for ai, ki in zip(acc, k))
    k = f(*(yi + (0.5 * h) * ki for yi, ki in zip(y, k)))   # k3
    acc = tuple(ai + 2.0 * ki for ai, ki in zip(acc, k))
    k = f(*(yi + h * ki for yi, ki in zip(y, k)))           # k4
    acc = tuple(ai + ki for ai, ki in zip(acc, k))
    z1, z2, w1, w2 = (yi + (h / 6.0) * ai for yi, ai in zip(y, acc))
    th1 = z1 - TWO_PI * torch.floor((z1 + math.pi) / TWO_PI)
    th2 = z2 - TWO_PI * torch.floor((z2 + math.pi) / TWO_PI)
    w1 = w1.clamp(-ACROBOT_MAX_VEL_1, ACROBOT_MAX_VEL_1)
    w2 = w2.clamp(-ACROBOT_MAX_VEL_2, ACROBOT_MAX_VEL_2)
    term = -torch.cos(th1) - torch.cos(th1 + th2) > 1.0
    reward = torch.where(term, 0.0, -1.0).to(s.dtype)
    return torch.stack([th1, th2, w1, w2], dim=-1), reward, term


def acrobot_obs(s: torch.Tensor) -> torch.Tensor:
    th1, th2, w1, w2 = s.unbind(-1)
    return torch.stack([torch.cos(th1), torch.sin(th1), torch.cos(th2),
                        torch.sin(th2), w1, w2], dim=-1)


MC_MIN_POS, MC_MAX_POS = -1.2, 0.6
MC_MAX_SPEED = 0.07


def _shared_tail(p, v2, goal):
    """The end of both MountainCar steps from the old position p and the new,
    clamped velocity v2: the position is clamped to [-1.2, 0.6], the velocity
    is zeroed where the car sits on the left wall still moving left, and the
    episode terminates at position >= goal with a velocity >= 0:
    (s' [N, 2], terminated [N] bool)."""
    p2 = (p + v2).clamp(MC_MIN_POS, MC_MAX_POS)
    v3 = torch.where((p2 == MC_MIN_POS) & (v2 < 0.0), torch.zeros_like(v2),
                     v2)
    term = (p2 >= goal) & (v3 >= 0.0)
    return torch.stack([p2, v3], dim=-1), term


def mountaincar_step(s: torch.Tensor, a: torch.Tensor):
    """One step of MountainCar-v0 from states s [N, 2] = (position, velocity)
    under actions a [N] in {0, 1, 2} (push left, none, right): (s' [N, 2],
    reward [N], terminated [N] bool).  The reward is -1 on every step, the
    terminating one included."""
    p, v = s.unbind(-1)
    push = a.reshape(-1).to(s.dtype) - 1.0
    v2 = (v + push * 0.001 + torch.cos(3.0 * p) * (-0.0025)).clamp(
        -MC_MAX_SPEED, MC_MAX_SPEED)
    s2, term = _shared_tail(p, v2, 0.5)
    return s2, -torch.ones_like(p), term


def mountaincar_cont_step(s: torch.Tensor, a: torch.Tensor):
    """One step of MountainCarContinuous-v0 from states s [N, 2] = (position,
    velocity) under actions a [N] or [N, 1]: (s' [N, 2], reward [N],
    terminated [N] bool).  The force is the action clipped to [-1, 1] here,
    inside the physics, as in pendulum_step.  The reward is 100 on the
    terminating step and 0 elsewhere, less 0.1 a^2 of the RAW, unclipped
    action, as gym has it: the policy's sampler does not clip, so an action
    outside [-1, 1] pushes no harder but costs more."""
    p, v = s.unbind(-1)
    a = a.reshape(-1).to(s.dtype)
    f = a.clamp(-1.0, 1.0)
    v2 = (v + f * 0.0015 - 0.0025 * torch.cos(3.0 * p)).clamp(
        -MC_MAX_SPEED, MC_MAX_SPEED)
    s2, term = _shared_tail(p, v2, 0.45)
    reward = torch.where(term, 100.0, 0.0).to(s.dtype) - 0.1 * a * a
    return s2, reward, term


class BatchedClassicEnv:
    """E parallel physics envs on one device, with BatchedSyntheticEnv's
    vectorised API: reset() -> obs [E, obs_dim]; step(actions) -> (obs,
    reward [E], done [E], info) with auto-reset.  `s` [E, S] is the internal
    state, `x` the current observation, `t` the per-env step counter."""

    ENV_ID: int
    GAME: str
    S: int                      # state width
    #: reset range per state dim: s_d uniform in (RESET_CENTER[d] -
    #: RESET_HALF[d], RESET_CENTER[d] + RESET_HALF[d]]; no RESET_CENTER means
    #: all zero
    RESET_HALF: tuple
    RESET_CENTER = None
    #: the game's registered episode length, the default `time_limit`
    TIME_LIMIT = 200

    def __init__(self, num_envs: int, device: str = "cpu", seed: int = 0,
                 time_limit: int = TIME_LIMIT):
        self.observation_space, self.action_space = game_spaces(self.GAME)
        self.num_envs = num_envs
        self.device = torch.device(device)
        self.time_limit = int(time_limit)
        self.dtype = torch.float32
        self.obs_dim = self.observation_space.shape[0]
        self._gen = torch.Generator(device=self.device.type).manual_seed(seed)
        self._half = torch.tensor(self.RESET_HALF, device=self.device)
        center = self.RESET_CENTER
        self._center = (
            torch.tensor(center, device=self.device)
            if center is not None and any(c != 0.0 for c in center) else None)
        self.horizons_i32 = torch.full(
            (num_envs,), self.time_limit, device=self.device,
            dtype=torch.int32)
        self.s = torch.zeros(num_envs, self.S, device=self.device)
        self.x = self._obs(self.s)
        self.t = torch.zeros(num_envs, device=self.device, dtype=torch.int32)

    # -- per-game pieces -------------------------------------------------
    def _physics(self, s, a):
        raise NotImplementedError

    def _obs(self, s: torch.Tensor) -> torch.Tensor:
        return s.clone()

    # --------------------------------------------------------------------
    def seed_state(self) -> torch.Tensor:
        # u in (0, 1], as the HIP rollout's rng_uniform
        u = 1.0 - torch.rand(self.num_envs, self.S, generator=self._gen,
                             device=self.device)
        s = (2.0 * u - 1.0) * self._half
        # an all-zero centre is not added: the symmetric envs keep their bits
        return s if self._center is None else self._center + s

    def reset(self) -> torch.Tensor:
        self.s = self.seed_state()
        self.x = self._obs(self.s)
        self.t.zero_()
        return self.x

    def step(self, actions: torch.Tensor):
        s2, reward, term = self._physics(self.s, actions)
        t2 = self.t + 1
        done = term | (t2 >= self.time_limit)
        # auto-reset (capture-safe): done envs restart from a fresh state
        self.s = torch.where(done.unsqueeze(-1), self.seed_state(), s2)
        self.x = self._obs(self.s)
        self.t = torch.where(done, torch.zeros_like(t2), t2)
        return self.x, reward, done, {}


class BatchedCartPole(BatchedClassicEnv):
    ENV_ID, GAME, S = CARTPOLE, "CartPole-v0", 4
    RESET_HALF = (0.05, 0.05, 0.05, 0.05)

    def _physics(self, s, a):
        return cartpole_step(s, a)


class BatchedPendulum(BatchedClassicEnv):
    ENV_ID, GAME, S = PENDULUM, "Pendulum-v1", 2
    RESET_HALF = (math.pi, 1.0)

    def _physics(self, s, a):
        return pendulum_step(s, a)

    def _obs(self, s):
        return pendulum_obs(s)


class BatchedAcrobot(BatchedClassicEnv):
    ENV_ID, GAME, S = ACROBOT, "Acrobot-v1", 4
    RESET_HALF = (0.1, 0.1, 0.1, 0.1)
    TIME_LIMIT = 500

    def __init__(self, num_envs: int, device: str = "cpu", seed: int = 0,
                 time_limit: int = TIME_LIMIT):
        super().__init__(num_envs, device=device, seed=seed,
                         time_limit=time_limit)

    def _physics(self, s, a):
        return acrobot_step(s, a)

    def _obs(self, s):
        return acrobot_obs(s)


class BatchedCartPoleV1(BatchedCartPole):
    """CartPole-v0's physics under CartPole-v1's time limit."""
    GAME = "CartPole-v1"
    TIME_LIMIT = 500

    def __init__(self, num_envs: int, device: str = "cpu", seed: int = 0,
                 time_limit: int = TIME_LIMIT):
        super().__init__(num_envs, device=device, seed=seed,
                         time_limit=time_limit)


class BatchedMountainCar(BatchedClassicEnv):
    ENV_ID, GAME, S = MOUNTAINCAR, "MountainCar-v0", 2
    RESET_HALF = (0.1, 0.0)     # at rest
    RESET_CENTER = (-0.5, 0.0)

    def _physics(self, s, a):
        return mountaincar_step(s, a)


class BatchedMountainCarContinuous(BatchedClassicEnv):
    ENV_ID, GAME, S = MOUNTAINCAR_CONT, "MountainCarContinuous-v0", 2
    RESET_HALF = (0.1, 0.0)
    RESET_CENTER = (-0.5, 0.0)
    TIME_LIMIT = 999

    def __init__(self, num_envs: int, device: str = "cpu", seed: int = 0,
                 time_limit: int = TIME_LIMIT):
        super().__init__(num_envs, device=device, seed=seed,
                         time_limit=time_limit)

    def _physics(self, s, a):
        return mountaincar_cont_step(s, a)


CLASSIC_ENVS = {cls.GAME: cls for cls in (
    BatchedCartPole, BatchedPendulum, BatchedAcrobot, BatchedMountainCar,
    BatchedMountainCarContinuous, BatchedCartPoleV1)}


def make_classic_env(cfg: DPPOConfig, device: str,
                     seed: int) -> BatchedClassicEnv:
    return CLASSIC_ENVS[cfg.GAME](cfg.NUM_ENVS, device=device, seed=seed)
