"""MultiDiscrete / MultiBinary fused-rollout eligibility and loss dispatch
(no GPU)."""

import math

import pytest
import torch

from dppo_amd.distributions import BernoulliPdType, MultiCategoricalPdType
from dppo_amd.config import DPPOConfig
from dppo_amd.ops.ppo_loss import PPOLossCoeffs, ppo_losses, ppo_losses_ref
from dppo_amd.parallel.comm import Comm
from dppo_amd.trainer import DPPOEngine


def cpu_engine(**kw):
    base = dict(
        GAME="MultiLever-v0", NUM_ENVS=8, MAX_EPOCH_STEPS=16, EPOCH_MAX=10,
        STOP_EPOCH=10, HIDDEN_SIZES=(16,), LEARNING_RATE=1e-3, NUM_WORKERS=1,
        LOG_FILE_PATH="/tmp/dppo_test_logs", DEVICE="cpu",
    )
    base.update(kw)
    return DPPOEngine(DPPOConfig(**base), comm=Comm(device="cpu"))


@pytest.mark.parametrize("game", ["MultiLever-v0", "BitFlipper-v0",
                                  "Pendulum-v1", "CartPole-v0"])
def test_multi_rollout_not_eligible_on_cpu(game, monkeypatch):
    monkeypatch.setenv("DPPO_ROLLOUT_MULTI", "1")
    eng = cpu_engine(GAME=game)
    assert not eng._can_fuse_rollout_multi()
    assert not eng._use_rollout_multi()


@pytest.mark.parametrize("game", ["Pendulum-v1", "CartPole-v0"])
def test_multi_rollout_not_eligible_for_box_and_discrete(game, monkeypatch):
    """With the device and kernel gate forced open, the family still says no."""
    monkeypatch.setenv("DPPO_ROLLOUT_MULTI", "1")
    eng = cpu_engine(GAME=game)
    monkeypatch.setattr(
        DPPOEngine, "_hip_path",
        lambda self, act_kind, dtype="float32": self._act_kind == act_kind)
    assert not eng._can_fuse_rollout_multi()
    assert not eng._use_rollout_multi()


@pytest.mark.parametrize("game", ["MultiLever-v0", "BitFlipper-v0"])
def test_family_limits_and_knob(game, monkeypatch):
    """The presets are inside the kernel limits; the knob's 0 wins."""
    eng = cpu_engine(GAME=game)
    monkeypatch.setattr(
        DPPOEngine, "_hip_path",
        lambda self, act_kind, dtype="float32": self._act_kind == act_kind)
    assert eng._can_fuse_rollout_multi()
    assert not eng._can_fuse_rollout_cat() and not eng._can_fuse_rollout()
    monkeypatch.setenv("DPPO_ROLLOUT_MULTI", "0")
    assert not eng._use_rollout_multi()
    monkeypatch.setenv("DPPO_ROLLOUT_MULTI", "1")
    assert eng._use_rollout_multi()
    eng.cfg.HIDDEN_SIZES = (256,)  # wider than the kernel's trunk limit
    assert not eng._can_fuse_rollout_multi()


@pytest.mark.parametrize("game", ["MultiLever-v0", "BitFlipper-v0"])
def test_cpu_round_is_finite_with_knob_on(game, monkeypatch):
    monkeypatch.setenv("DPPO_ROLLOUT_MULTI", "1")
    stats, stop = cpu_engine(GAME=game).train_round()
    assert not stop
    assert all(math.isfinite(v) for v in stats.values())


@pytest.mark.parametrize("pdt", [MultiCategoricalPdType((3, 3, 4)),
                                 BernoulliPdType(8)],
                         ids=["mcat", "bern"])
def test_cpu_losses_are_the_reference(pdt):
    """No accidental dispatch: CPU tensors take ppo_losses_ref."""
    g = torch.Generator().manual_seed(0)
    B, P = 64, pdt.param_shape()[0]
    lpi = torch.randn(B, P, generator=g)
    lold = lpi + 0.1 * torch.randn(B, P, generator=g)
    v, oldv, adv, etr = (torch.randn(B, generator=g) for _ in range(4))
    a = pdt.pdfromflat(lold).sample()
    coeffs = PPOLossCoeffs(0.2, 0.01, 0.5)
    args = (pdt.pdfromflat(lpi), pdt.pdfromflat(lold), v, oldv, a, adv, etr,
            coeffs)
    out, ref = ppo_losses(*args), ppo_losses_ref(*args)
    assert out.keys() == ref.keys()
    for k in ref:
        assert torch.equal(out[k], ref[k]), k


def test_multicategorical_pd_exposes_nvec():
    pd = MultiCategoricalPdType([3, 3, 4]).pdfromflat(torch.zeros(2, 10))
    assert pd.nvec == (3, 3, 4)
    assert [p.logits.shape[-1] for p in pd.categoricals] == [3, 3, 4]
