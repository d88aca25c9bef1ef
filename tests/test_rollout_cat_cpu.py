"""Discrete presets and fused-Categorical-rollout eligibility (no GPU)."""

import math

from dppo_amd import spaces
from dppo_amd.config import DPPOConfig, game_spaces
from dppo_amd.parallel.comm import Comm
from dppo_amd.trainer import DPPOEngine


def cpu_engine(**kw):
    base = dict(
        GAME="Acrobot-v1", NUM_ENVS=8, MAX_EPOCH_STEPS=16, EPOCH_MAX=10,
        STOP_EPOCH=10, HIDDEN_SIZES=(16,), LEARNING_RATE=1e-3, NUM_WORKERS=1,
        LOG_FILE_PATH="/tmp/dppo_test_logs", DEVICE="cpu",
    )
    base.update(kw)
    return DPPOEngine(DPPOConfig(**base), comm=Comm(device="cpu"))


def test_new_discrete_presets_resolve():
    for game, obs_dim, n in [("Acrobot-v1", 6, 3), ("LunarLander-v2", 8, 4)]:
        obs, act = game_spaces(game)
        assert obs.shape == (obs_dim,)
        assert isinstance(act, spaces.Discrete) and act.n == n


def test_acrobot_cpu_round_is_finite():
    eng = cpu_engine()
    stats, stop = eng.train_round()
    assert not stop
    assert all(math.isfinite(v) for v in stats.values())


def test_cat_rollout_not_eligible_on_cpu_or_box(monkeypatch):
    monkeypatch.setenv("DPPO_ROLLOUT_CAT", "1")
    assert not cpu_engine()._can_fuse_rollout_cat()
    assert not cpu_engine(GAME="Pendulum-v1")._can_fuse_rollout_cat()
