"""Fused update-middle kernel (mlp_mid.hip) vs autograd and vs the
per-layer backward chain it replaces.

Shapes are the smallest at which the kernel can still go wrong: a row tail
(4099 = 32 tiles of 128 + 3), fewer tiles than persistent blocks (200 rows:
all but two blocks write an all-zero slab), heads widths whose 2A+1 pads
differently (35 -> two 32-column MFMA tiles, 13 -> one), the narrower
hidden width and relu.  Bounds are the project's existing ones for the
fused backward (test_gpu_mlp.test_fused_backward_matches_autograd)."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from dppo_amd.config import DPPOConfig
from dppo_amd.distributions import DiagGaussianPdType
from dppo_amd.ops import hip_ext
from dppo_amd.ops.ppo_loss import PPOLossCoeffs, ppo_losses_ref
from dppo_amd.parallel.comm import Comm
from dppo_amd.trainer import DPPOEngine

# the modes the kernel has; a RECOMPUTE mode ran this same matrix and was
# removed on its measurements (profiles/r05_update_mid_fused.txt)
MODES = ("load",)

SHAPES = {
    "humanoid_tail": dict(B=4099, kw={}),
    "humanoid_few_tiles": dict(B=200, kw={}),
    "halfcheetah": dict(B=4099, kw=dict(GAME="HalfCheetah-v4")),
    "h32": dict(B=4099, kw=dict(HIDDEN_SIZES=(32, 32))),
    "relu": dict(B=4099, kw=dict(ACTIVATION="relu")),
}


def make_engine(**kw):
    base = dict(
        GAME="Humanoid-v4", HIDDEN_SIZES=(64, 64), ACTIVATION="tanh",
        NUM_ENVS=128, MAX_EPOCH_STEPS=16, EPOCH_MAX=1000, STOP_EPOCH=1000,
        NUM_WORKERS=1, LOG_FILE_PATH="/tmp/dppo_gpu_test_logs", DEVICE="cuda",
    )
    base.update(kw)
    return DPPOEngine(DPPOConfig(**base), comm=Comm(device="cuda:0"))


def chain_dz1(eng, a_views, v, pdflat, oldflat, oldv, actions, adv, etr,
              clip):
    """dz1 of the per-layer chain: gh kernel + the two dgrad GEMMs."""
    ext = hip_ext()
    c = eng.cfg
    code = 3 if c.ACTIVATION == "tanh" else 4
    gh = ext.ppo_loss_gauss_gh(pdflat, oldflat, v, oldv, actions, adv, etr,
                               clip, c.ENTCOEFF, c.VCOEFF,
                               torch.empty(0, device="cuda"))
    Wh = torch.zeros(gh.shape[1], a_views[1].shape[1], device="cuda")
    Wh_cat = torch.cat([eng.pi.pi.weight, eng.pi.vf.weight], 0).detach()
    Wh[:Wh_cat.shape[0]] = Wh_cat
    dummy = torch.zeros(1, device="cuda")
    dz2 = torch.empty_like(a_views[1])
    ext.gemm_fwd(gh, Wh, dummy, code, 0, dz2, dz2, a_views[1], 0, 0, 0)
    dz1 = torch.empty_like(a_views[0])
    ext.gemm_fwd(dz2, eng.pi.hidden[1].weight.detach(), dummy, code, 0,
                 dz1, dz1, a_views[0], 0, 0, 0)
    return dz1


@pytest.fixture(scope="module")
def cases():
    """Per shape: engine, inputs, and the autograd / chain references,
    computed once and left unchanged."""
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        spec = SHAPES[name]
        torch.manual_seed(1234)
        eng = make_engine(**spec["kw"])
        B = spec["B"]
        A = eng.act_space.shape[0]
        states = torch.randn(B, eng.obs_space.shape[0], device="cuda") * 0.5
        acts, a_views, v, pdflat = eng._fused_forward(states)
        pdt = DiagGaussianPdType(A)
        with torch.no_grad():
            oldflat = pdflat + 0.05 * torch.randn_like(pdflat)
            oldv = v + 0.1 * torch.randn_like(v)
            actions = pdt.pdfromflat(oldflat).sample().contiguous()
            adv = torch.randn(B, device="cuda")
            etr = torch.randn(B, device="cuda")
        clip = 0.2
        eng.flat_pi.zero_grad()
        v2, flat2 = eng.pi(states)
        out = ppo_losses_ref(
            pdt.pdfromflat(flat2), pdt.pdfromflat(oldflat), v2, oldv,
            actions, adv, etr,
            PPOLossCoeffs(clip, eng.cfg.ENTCOEFF, eng.cfg.VCOEFF))
        out["total_loss"].backward()
        ref_grad = eng.flat_pi.flat_grad.clone()

        args = (a_views, v, pdflat, oldflat, oldv, actions, adv, etr)
        eng.flat_pi.zero_grad()
        eng._mid_fused_mode = lambda: ""
        eng._fused_backward(states, acts, *args, clip)
        del eng._mid_fused_mode
        chain_grad = eng.flat_pi.flat_grad.clone()
        dz1_ref = chain_dz1(eng, *args, clip)
        cache[name] = dict(eng=eng, states=states, acts=acts, args=args,
                           clip=clip, ref_grad=ref_grad,
                           chain_grad=chain_grad, dz1_ref=dz1_ref)
        return cache[name]

    return get


def run_mid(case, monkeypatch, mode, clip_dev=False):
    eng = case["eng"]
    monkeypatch.setenv("DPPO_MID_FUSED", mode)
    assert eng._mid_fused_mode() == mode
    eng.flat_pi.zero_grad()
    if clip_dev:
        eng._clip_dev = torch.tensor([case["clip"]], device="cuda")
        clip_arg = 0.0  # must be ignored
    else:
        eng._clip_dev = None
        clip_arg = case["clip"]
    try:
        dz1 = eng._mid_backward(case["states"], *case["args"], clip_arg)
    finally:
        eng._clip_dev = None
    return eng.flat_pi.flat_grad.clone(), dz1


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_mid_grad_matches_autograd_and_chain(cases, monkeypatch, name, mode):
    case = cases(name)
    grad, dz1 = run_mid(case, monkeypatch, mode)
    sl = case["eng"].flat_pi.slices
    for tag, ref in (("autograd", case["ref_grad"]),
                     ("chain", case["chain_grad"])):
        scale = float(ref.abs().max())
        for seg, what in ((slice(sl[2].start, ref.numel()), "mid segments"),
                          (slice(0, sl[2].start), "L1 via dw_mfma(dz1)")):
            err = float((grad[seg] - ref[seg]).abs().max())
            print(f"{name}/{mode} vs {tag}, {what}: max err {err:.3e} "
                  f"(scale {scale:.3e})")
            torch.testing.assert_close(grad[seg], ref[seg],
                                       atol=scale * 2e-4 + 1e-8, rtol=2e-3)
    dscale = float(case["dz1_ref"].abs().max())
    derr = float((dz1 - case["dz1_ref"]).abs().max())
    print(f"{name}/{mode} dz1: max err {derr:.3e} (scale {dscale:.3e})")
    torch.testing.assert_close(dz1, case["dz1_ref"], atol=dscale * 2e-4,
                               rtol=0.0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_mid_clip_device_scalar_matches_host_arg(cases, monkeypatch, name,
                                                 mode):
    case = cases(name)
    g_host, dz_host = run_mid(case, monkeypatch, mode, clip_dev=False)
    g_dev, dz_dev = run_mid(case, monkeypatch, mode, clip_dev=True)
    # same clip value either way: dz1 is bitwise the same; the grad differs
    # only by the slab reduce's atomic chunk order
    assert torch.equal(dz_host, dz_dev)
    # fp32 atomics in a different order over <= 32 chunk partials: a few
    # ulp of the largest element
    scale = float(case["ref_grad"].abs().max())
    torch.testing.assert_close(g_dev, g_host, atol=scale * 1e-5, rtol=0.0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(SHAPES))
def test_mid_accumulates_and_pads_route_nowhere(cases, monkeypatch, name,
                                                mode):
    """The kernel adds into the flat grad.  With every element pre-filled
    with a sentinel, each one must come out as sentinel + gradient: a pad
    row or pad column of the heads tile that landed anywhere would show
    as an element off by more than the bound."""
    case = cases(name)
    eng = case["eng"]
    monkeypatch.setenv("DPPO_MID_FUSED", mode)
    scale = float(case["ref_grad"].abs().max())
    sentinel = 4.0 * scale
    eng.flat_pi.zero_grad()
    eng.flat_pi.flat_grad.fill_(sentinel)
    eng._mid_backward(case["states"], *case["args"], case["clip"])
    got = eng.flat_pi.flat_grad.clone() - sentinel
    eng.flat_pi.zero_grad()
    # the sentinel costs ulp(5*scale)/2 of rounding per accumulation
    torch.testing.assert_close(got, case["chain_grad"],
                               atol=scale * 2e-4 + 1e-8, rtol=2e-3)


def test_mid_ineligible_shapes_keep_the_chain(monkeypatch):
    monkeypatch.setenv("DPPO_MID_FUSED", "load")
    assert make_engine(HIDDEN_SIZES=(64,))._mid_fused_mode() == ""
    assert make_engine(HIDDEN_SIZES=(128, 128))._mid_fused_mode() == ""
    monkeypatch.setenv("DPPO_MID_FUSED", "bogus")
    with pytest.raises(ValueError):
        make_engine()._mid_fused_mode()


def test_mid_train_rounds_match_chain(monkeypatch):
    """Two rounds end to end, chain vs the default mode, same seed.  Bound:
    steps x lr (test_gpu_mlp.test_graphed_update_matches_ungraphed: Adam's
    early-step normaliser turns reduce-order noise into ~lr per step)."""
    finals = []
    for mode in ("0", None):
        if mode is None:
            monkeypatch.delenv("DPPO_MID_FUSED", raising=False)
        else:
            monkeypatch.setenv("DPPO_MID_FUSED", mode)
        eng = make_engine(SEED=31)
        # batches this small go to the single-kernel chunk step; switch it
        # off so the GEMM-shaped update (and with it the mid kernel) runs
        eng.CHUNK_KERNEL_MAX_B = 0
        B = eng.cfg.NUM_ENVS * eng.cfg.MAX_EPOCH_STEPS
        assert not eng._can_chunk_kernel(B) and eng._can_fuse_update()
        want = {"0": "", None: DPPOEngine.MID_FUSED_DEFAULT}.get(mode, mode)
        assert eng._mid_fused_mode() == want
        for _ in range(2):
            stats, _ = eng.train_round()
        assert all(math.isfinite(x) for x in stats.values())
        finals.append(eng.flat_pi.flat_param.detach().clone())
        lr = eng.cfg.LEARNING_RATE
    for other in finals[1:]:
        err = float((finals[0] - other).abs().max())
        print(f"end-to-end max param diff {err:.3e} (bound {8 * lr:.3e})")
        torch.testing.assert_close(finals[0], other, atol=8 * lr, rtol=0.0)
