"""The fused MFMA update (and its hipGraph-captured form) for Discrete,
MultiDiscrete and MultiBinary policies against the autograd update loop that
DPPO_UPDATE_DISC=0 keeps.  Tolerances are those of the Box tests in
tests/test_gpu_mlp.py for the same GEMM chain."""

import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from dppo_amd.config import GAME_SHAPES, DPPOConfig
from dppo_amd.ops.ppo_loss import PPOLossCoeffs, ppo_losses_ref
from dppo_amd.parallel.comm import Comm
from dppo_amd.trainer import DPPOEngine

PRESETS = {
    "cartpole": dict(GAME="CartPole-v0", HIDDEN_SIZES=(16,), ACTIVATION="relu"),
    "acrobot": dict(GAME="Acrobot-v1", HIDDEN_SIZES=(32, 32),
                    ACTIVATION="tanh"),
    "multilever": dict(GAME="MultiLever-v0", HIDDEN_SIZES=(32,),
                       ACTIVATION="tanh"),
    "bitflipper": dict(GAME="BitFlipper-v0", HIDDEN_SIZES=(64, 64),
                       ACTIVATION="tanh"),
}
presets = pytest.mark.parametrize("preset", sorted(PRESETS))

# head widths at the gh kernels' limits: name -> GAME_SHAPES entry
EDGE_GAMES = {
    "Discrete63-v0": (8, "discrete", 63),      # ldgh 64: exact-fit row
    "Discrete64-v0": (8, "discrete", 64),      # ldgh 68: the widest row
    "MultiBinary32-v0": (16, "multibinary", 32),
}


def make_engine(preset=None, **kw):
    base = dict(
        NUM_ENVS=128, MAX_EPOCH_STEPS=16, EPOCH_MAX=1000, STOP_EPOCH=1000,
        NUM_WORKERS=1, LOG_FILE_PATH="/tmp/dppo_gpu_test_logs", DEVICE="cuda",
    )
    if preset is not None:
        base.update(PRESETS[preset])
    base.update(kw)
    return DPPOEngine(DPPOConfig(**base), comm=Comm(device="cuda:0"))


def engine_pair(preset, **kw):
    eng1, eng2 = make_engine(preset, **kw), make_engine(preset, **kw)
    torch.testing.assert_close(eng1.flat_pi.flat_param, eng2.flat_pi.flat_param)
    eng1.sync_oldpi()
    eng2.sync_oldpi()
    return eng1, eng2


def clone_batch(batch):
    out = copy.copy(batch)
    for f in ("states", "actions", "adv", "etr", "oldflat", "oldv"):
        setattr(out, f, getattr(batch, f).clone())
    return out


@presets
@pytest.mark.parametrize("knob", [None, "1"], ids=["unset", "on"])
def test_fused_update_is_taken(preset, knob, monkeypatch):
    if knob is None:
        monkeypatch.delenv("DPPO_UPDATE_DISC", raising=False)
    else:
        monkeypatch.setenv("DPPO_UPDATE_DISC", knob)
    eng = make_engine(preset)
    assert eng._can_fuse_update()
    eng.sync_oldpi()
    batch = eng.collect()

    def boom(*a, **k):
        raise AssertionError("autograd loss entered on the fused update")

    monkeypatch.setattr(eng, "_losses", boom)
    p0 = eng.flat_pi.flat_param.detach().clone()
    eng.update(batch, 0.9)
    torch.cuda.synchronize()
    assert not torch.equal(p0, eng.flat_pi.flat_param.detach())
    assert bool(torch.isfinite(eng.flat_pi.flat_param).all())


@presets
def test_knob_zero_keeps_the_autograd_loop(preset, monkeypatch):
    monkeypatch.setenv("DPPO_UPDATE_DISC", "0")
    eng = make_engine(preset)
    assert not eng._can_fuse_update()
    eng.sync_oldpi()
    batch = eng.collect()
    real, calls = eng._losses, []
    monkeypatch.setattr(
        eng, "_losses", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    eng.update(batch, 0.9)
    assert len(calls) == eng.cfg.UPDATE_STEPS


@presets
def test_fused_forward_matches_eager(preset):
    eng = make_engine(preset)
    B = 4099  # no multiple of the 128-row tile: exercises tail masking
    states = torch.randn(B, eng.obs_space.shape[0], device="cuda") * 0.5
    acts, a_views, v, pdflat = eng._fused_forward(states)
    # both heads routes are covered: glds (padded) for CartPole and
    # MultiLever, whose P + 2 is a multiple of 4, pipe for the other two
    P = eng.pi.pdtype.param_shape()[0]
    assert eng._mw["heads_pad"] == ((P + 2) % 4 == 0)
    with torch.no_grad():
        v_ref, flat_ref = eng.pi(states)
    assert pdflat.shape == flat_ref.shape
    torch.testing.assert_close(v, v_ref, atol=3e-5, rtol=3e-5)
    torch.testing.assert_close(pdflat, flat_ref, atol=3e-5, rtol=3e-5)


def check_backward(eng, B):
    states = torch.randn(B, eng.obs_space.shape[0], device="cuda") * 0.5
    acts, a_views, v, pdflat = eng._fused_forward(states)
    pdt = eng.pi.pdtype
    with torch.no_grad():
        oldflat = pdflat + 0.05 * torch.randn_like(pdflat)
        oldv = v + 0.1 * torch.randn_like(v)
        actions = pdt.pdfromflat(oldflat).sample()
        adv = torch.randn(B, device="cuda")
        etr = torch.randn(B, device="cuda")
    clip, entc, vc = 0.2, eng.cfg.ENTCOEFF, eng.cfg.VCOEFF

    eng.flat_pi.zero_grad()
    v2, flat2 = eng.pi(states)
    out = ppo_losses_ref(pdt.pdfromflat(flat2), pdt.pdfromflat(oldflat),
                         v2, oldv, actions, adv, etr,
                         PPOLossCoeffs(clip, entc, vc))
    out["total_loss"].backward()
    ref_grad = eng.flat_pi.flat_grad.clone()

    eng.flat_pi.zero_grad()
    eng._fused_backward(states, acts, a_views, v, pdflat, oldflat, oldv,
                        actions, adv, etr, clip)
    grad = eng.flat_pi.flat_grad
    scale = float(ref_grad.abs().max())
    torch.testing.assert_close(grad, ref_grad, atol=scale * 2e-4 + 1e-8,
                               rtol=2e-3)


@presets
@pytest.mark.parametrize("B", [4096, 4099])  # 4099: a tail for the glds dW
def test_fused_backward_matches_autograd(preset, B):
    eng = make_engine(preset)
    assert eng._can_fuse_update()
    check_backward(eng, B)


@pytest.mark.parametrize("game", sorted(EDGE_GAMES))
def test_fused_backward_edge_head_widths(game, monkeypatch):
    monkeypatch.setitem(GAME_SHAPES, game, EDGE_GAMES[game])
    eng = make_engine(GAME=game, HIDDEN_SIZES=(32,), ACTIVATION="tanh")
    assert eng._can_fuse_update()
    check_backward(eng, 4096)


@presets
def test_fused_update_matches_autograd_update(preset, monkeypatch):
    """One full update (4 steps), fused vs DPPO_UPDATE_DISC=0, from identical
    params on the SAME batch ends at nearly identical parameters."""
    monkeypatch.delenv("DPPO_UPDATE_DISC", raising=False)
    eng1, eng2 = engine_pair(preset, SEED=11)
    batch = eng1.collect()
    assert eng1._can_fuse_update()
    eng1.update(batch, 0.9)
    monkeypatch.setenv("DPPO_UPDATE_DISC", "0")
    assert not eng2._can_fuse_update()
    eng2.update(batch, 0.9)
    torch.testing.assert_close(
        eng1.flat_pi.flat_param, eng2.flat_pi.flat_param, atol=2e-5, rtol=1e-3)


@presets
def test_graphed_update_matches_ungraphed(preset, monkeypatch):
    """The hipGraph-captured update replays to (nearly) the same parameters
    as the uncaptured fused path across rounds with varying l_mul."""
    monkeypatch.delenv("DPPO_UPDATE_DISC", raising=False)
    eng1, eng2 = engine_pair(preset, SEED=21, MAX_EPOCH_STEPS=32)
    # update() routes these families to the captured update
    assert eng1._can_fuse_update() and eng1._batch_is_persistent()
    for l_mul in (0.9, 0.7):
        batch = eng1.collect()
        # the capture requires batch views over eng1's persistent buffers;
        # the plain path gets the same data in tensors of its own
        batch2 = clone_batch(batch)
        eng1.update(batch, l_mul)
        eng2._update_fused(batch2, l_mul)
    assert eng1._upd_graph is not None or eng1._graph_failed
    # Tolerance: Adam's early-step normalizer acts like sign(g), so the fp
    # nondeterminism of the dW reduce (atomic chunk ordering, on BOTH paths)
    # amplifies to ~+-lr per element per step; the bound is steps x lr
    bound = 8 * eng1.cfg.LEARNING_RATE
    torch.testing.assert_close(
        eng1.flat_pi.flat_param, eng2.flat_pi.flat_param, atol=bound, rtol=0.0)


@presets
def test_minibatched_update_matches_autograd(preset, monkeypatch):
    """MINIBATCH_SIZE 600 over B = 2048: three full chunks and a 248-row
    tail, fused chunk steps vs the autograd minibatch loop."""
    monkeypatch.delenv("DPPO_UPDATE_DISC", raising=False)
    eng1, eng2 = engine_pair(preset, SEED=31, MINIBATCH_SIZE=600)
    batch = eng1.collect()
    assert batch.states.shape[0] % 600 != 0
    assert eng1._can_fuse_update()
    eng1.update(batch, 0.9)
    monkeypatch.setenv("DPPO_UPDATE_DISC", "0")
    eng2.update(batch, 0.9)
    torch.testing.assert_close(
        eng1.flat_pi.flat_param, eng2.flat_pi.flat_param, atol=2e-5, rtol=1e-3)


@presets
def test_training_rounds(preset, monkeypatch):
    monkeypatch.delenv("DPPO_UPDATE_DISC", raising=False)
    eng = make_engine(preset, MAX_EPOCH_STEPS=32)
    p0 = eng.flat_pi.flat_param.detach().clone()
    for _ in range(3):
        stats, _ = eng.train_round()
        assert all(math.isfinite(x) for x in stats.values())
    assert not torch.equal(p0, eng.flat_pi.flat_param.detach())
    assert bool(torch.isfinite(eng.flat_pi.flat_param).all())
