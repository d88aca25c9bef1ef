"""Fused MultiCategorical / Bernoulli PPO loss and samplers
(ops/hip/multi_loss.hip) vs the eager reference (ppo_losses_ref + autograd).

Tolerances are those of the Categorical tests in test_gpu_kernels.py: losses
atol 1e-5 / rtol 1e-4, total atol 2e-5, grads atol 1e-6 / rtol 1e-4.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from dppo_amd.distributions import BernoulliPdType, MultiCategoricalPdType
from dppo_amd.ops import ppo_loss as ppo_loss_mod
from dppo_amd.ops import require_hip_ext
from dppo_amd.ops.ppo_loss import PPOLossCoeffs, ppo_losses, ppo_losses_ref

CLIP, ENTC, VC = 0.2, 0.01, 0.5
COEFFS = PPOLossCoeffs(CLIP, ENTC, VC)
LOSS_KEYS = ("policyLoss", "entropyLoss", "valueLoss", "total_loss")
LOSS_ATOL = (1e-5, 1e-5, 1e-5, 2e-5)
GRAD_ATOL = 1e-6

# the preset; P = 64 / C = 32, the widest; one component (== Categorical);
# a component straddling lane 32; unaligned segments
NVECS = [(3, 3, 4), (2,) * 32, (64,), (5, 59), (2, 7, 3)]
BERN_NS = [1, 8, 32, 64]
# fewer rows than waves of the grid (8192); several rows per wave + ragged tail
BS = [1000, 20011]


@pytest.fixture(scope="module")
def ext():
    return require_hip_ext()


def make_case(pdt, P, B, seed=0, scale=1.0, pin=None):
    """Logits randn * scale (two of them set to +-pin), oldpi a 0.1
    perturbation, actions from oldpi."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    lpi = torch.randn(B, P, device="cuda", generator=g) * scale
    if pin is not None:
        lpi[0, 0], lpi[1, P - 1] = pin, -pin
    lold = lpi + 0.1 * torch.randn(B, P, device="cuda", generator=g)
    v = torch.randn(B, device="cuda", generator=g)
    oldv = v + 0.3 * torch.randn(B, device="cuda", generator=g)
    with torch.no_grad():
        actions = pdt.pdfromflat(lold).sample()
    adv = torch.randn(B, device="cuda", generator=g)
    etr = torch.randn(B, device="cuda", generator=g)
    return lpi, lold, v, oldv, actions, adv, etr


def ref_losses_and_grads(pdt, case, dtype=torch.float32):
    lpi, lold, v, oldv, a, adv, etr = case
    c = lambda t: t.to(dtype)
    p = c(lpi).clone().requires_grad_(True)
    vr = c(v).clone().requires_grad_(True)
    ref = ppo_losses_ref(pdt.pdfromflat(p), pdt.pdfromflat(c(lold)), vr,
                         c(oldv), a, c(adv), c(etr), COEFFS)
    ref["total_loss"].backward()
    return torch.stack([ref[k].detach() for k in LOSS_KEYS]), p.grad, vr.grad


def fused_raw(ext, pdt, case):
    """(losses[4], g_logits, g_v) straight from the fwd / bwd bindings."""
    gt = torch.ones((), device="cuda")
    if isinstance(pdt, MultiCategoricalPdType):
        nv = list(pdt.nvec)
        losses = ext.ppo_loss_mcat_fwd(*case, nv, CLIP, ENTC, VC)
        g_l, g_v = ext.ppo_loss_mcat_bwd(*case, nv, CLIP, ENTC, VC, gt)
    else:
        losses = ext.ppo_loss_bern_fwd(*case, CLIP, ENTC, VC)
        g_l, g_v = ext.ppo_loss_bern_bwd(*case, CLIP, ENTC, VC, gt)
    return losses, g_l, g_v


def check_family(ext, pdt, P, B):
    case = make_case(pdt, P, B, seed=B % 97)
    ref_l, ref_gl, ref_gv = ref_losses_and_grads(pdt, case)
    losses, g_l, g_v = fused_raw(ext, pdt, case)
    for i, atol in enumerate(LOSS_ATOL):
        torch.testing.assert_close(losses[i], ref_l[i], atol=atol, rtol=1e-4)
    torch.testing.assert_close(g_l, ref_gl, atol=GRAD_ATOL, rtol=1e-4)
    torch.testing.assert_close(g_v, ref_gv, atol=GRAD_ATOL, rtol=1e-4)
    # end to end through the autograd Function (ppo_losses dispatch)
    lpi, lold, v, oldv, a, adv, etr = case
    p1 = lpi.clone().requires_grad_(True)
    v1 = v.clone().requires_grad_(True)
    out = ppo_losses(pdt.pdfromflat(p1), pdt.pdfromflat(lold), v1, oldv, a,
                     adv, etr, COEFFS, policy="always")
    out["total_loss"].backward()
    torch.testing.assert_close(out["total_loss"], ref_l[3], atol=2e-5,
                               rtol=1e-4)
    torch.testing.assert_close(p1.grad, ref_gl, atol=GRAD_ATOL, rtol=1e-4)
    torch.testing.assert_close(v1.grad, ref_gv, atol=GRAD_ATOL, rtol=1e-4)
    return case, losses, g_l, g_v


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("nvec", NVECS, ids=lambda nv: "x".join(map(str, nv))
                         if len(nv) < 5 else f"{nv[0]}^{len(nv)}")
def test_mcat_loss_matches_ref(ext, nvec, B):
    pdt = MultiCategoricalPdType(nvec)
    case, losses, g_l, g_v = check_family(ext, pdt, sum(nvec), B)
    if len(nvec) == 1:
        # one component IS a Categorical: the two kernels agree too
        lpi, lold, v, oldv, a, adv, etr = case
        a1 = a.reshape(-1).contiguous()
        gt = torch.ones((), device="cuda")
        cat_l = ext.ppo_loss_cat_fwd(lpi, lold, v, oldv, a1, adv, etr, CLIP,
                                     ENTC, VC)
        cat_gl, cat_gv = ext.ppo_loss_cat_bwd(lpi, lold, v, oldv, a1, adv, etr,
                                              CLIP, ENTC, VC, gt)
        for i, atol in enumerate(LOSS_ATOL):
            torch.testing.assert_close(losses[i], cat_l[i], atol=atol,
                                       rtol=1e-4)
        torch.testing.assert_close(g_l, cat_gl, atol=GRAD_ATOL, rtol=1e-4)
        torch.testing.assert_close(g_v, cat_gv, atol=GRAD_ATOL, rtol=1e-4)


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("n", BERN_NS)
def test_bern_loss_matches_ref(ext, n, B):
    pdt = BernoulliPdType(n)
    case = check_family(ext, pdt, n, B)[0]
    assert set(case[4].unique().tolist()) <= {0.0, 1.0}


def saturation_errors(ext, pdt, P):
    """Max abs errors [policy, entropy, value, total, g_logits, g_v] against
    the float64 eager evaluation, for the fused kernels and for the float32
    eager path."""
    case = make_case(pdt, P, 4096, seed=11, scale=10.0, pin=40.0)
    assert float(case[0].max()) >= 40.0 and float(case[0].min()) <= -40.0
    r64 = ref_losses_and_grads(pdt, case, torch.float64)
    r32 = ref_losses_and_grads(pdt, case, torch.float32)
    fused = fused_raw(ext, pdt, case)
    for t in fused:
        assert bool(torch.isfinite(t).all())

    def err(got):
        dl = (got[0].double() - r64[0]).abs().tolist()
        return dl + [float((g.double() - w).abs().max())
                     for g, w in zip(got[1:], r64[1:])]

    return err(fused), err(r32)


def check_saturation(ext, pdt, P):
    e_fused, e_eager = saturation_errors(ext, pdt, P)
    fmt = lambda es: " ".join(f"{e:.1e}" for e in es)
    print(f"saturation {type(pdt).__name__} P={P}: fused {fmt(e_fused)} | "
          f"eager32 {fmt(e_eager)}")
    floors = LOSS_ATOL + (GRAD_ATOL, GRAD_ATOL)
    for ef, ee, floor in zip(e_fused, e_eager, floors):
        # the kernels use __expf/__logf: 4x the float32 eager error
        assert ef <= max(4.0 * ee, floor), (e_fused, e_eager)


@pytest.mark.parametrize("nvec", [(3, 3, 4), (5, 59)], ids=["3x3x4", "5x59"])
def test_mcat_saturated_logits(ext, nvec):
    """Logits randn * 10 reaching +-40, B = 4096: outputs finite, and the
    error against float64 eager within 4x the float32 eager path's (floor:
    the atols above).  Measured max abs errors, [policy, entropy, value,
    total, g_logits, g_v]:
      (3,3,4) fused   2.9e-09 1.4e-10 7.5e-09 5.0e-08 4.4e-10 5.8e-11
              eager32 5.9e-09 1.4e-10 7.5e-09 5.0e-08 1.0e-09 5.8e-11
      (5,59)  fused   3.0e-09 4.7e-11 7.5e-09 1.5e-08 2.9e-10 5.8e-11
              eager32 2.0e-08 4.7e-11 7.5e-09 1.5e-08 1.3e-09 5.8e-11
    i.e. every error is far below its atol floor (1e-5 / 2e-5 / 1e-6)."""
    check_saturation(ext, MultiCategoricalPdType(nvec), sum(nvec))


@pytest.mark.parametrize("n", [8, 64])
def test_bern_saturated_logits(ext, n):
    """As test_mcat_saturated_logits.  Measured:
      n=8   fused   1.7e-09 3.8e-10 7.5e-09 1.3e-08 4.4e-10 5.8e-11
            eager32 2.7e-10 1.3e-09 7.5e-09 1.3e-08 9.8e-10 5.8e-11
      n=64  fused   8.8e-09 3.3e-09 7.5e-09 2.2e-08 1.3e-09 5.8e-11
            eager32 2.1e-08 3.3e-09 7.5e-09 2.2e-08 2.6e-09 5.8e-11"""
    check_saturation(ext, BernoulliPdType(n), n)


def test_dispatch_takes_fused_kernels(ext, monkeypatch):
    def stub(*a, **k):
        raise RuntimeError("eager reference entered")

    monkeypatch.setattr(ppo_loss_mod, "ppo_losses_ref", stub)
    for pdt, P in ((MultiCategoricalPdType((3, 3, 4)), 10),
                   (BernoulliPdType(8), 8)):
        lpi, lold, v, oldv, a, adv, etr = make_case(pdt, P, 256)
        out = ppo_losses(pdt.pdfromflat(lpi), pdt.pdfromflat(lold), v, oldv, a,
                         adv, etr, COEFFS)
        assert bool(torch.isfinite(out["total_loss"]))
    # sum(nvec) = 65: wider than a wave -> the eager reference
    pdt = MultiCategoricalPdType((32, 33))
    lpi, lold, v, oldv, a, adv, etr = make_case(pdt, 65, 256)
    with pytest.raises(RuntimeError, match="eager reference entered"):
        ppo_losses(pdt.pdfromflat(lpi), pdt.pdfromflat(lold), v, oldv, a, adv,
                   etr, COEFFS)


def assert_counts_follow(p, hits):
    """|count - sum_n p_n| <= 5 sqrt(sum_n p_n (1 - p_n)) per column: the
    count is a sum of independent Bernoulli(p_n), so this is its 5 sigma
    bound (derived, not tuned; test_gpu_rollout_cat.assert_counts_follow).
    p, hits: [N, cols], probability and 0/1 outcome of each column."""
    p = p.double()
    counts = hits.double().sum(dim=0)
    bound = 5.0 * (p * (1.0 - p)).sum(dim=0).sqrt()
    diff = (counts - p.sum(dim=0)).abs()
    assert bool((diff <= bound).all()), (counts.tolist(), p.sum(0).tolist(),
                                        bound.tolist())


@pytest.mark.parametrize("nvec", [(3, 3, 4), (5, 59), (2,) * 32],
                         ids=["3x3x4", "5x59", "2^32"])
def test_mcat_sample_distribution(ext, nvec):
    N, P, C = 20000, sum(nvec), len(nvec)
    g = torch.Generator(device="cuda").manual_seed(5)
    logits = torch.randn(N, P, device="cuda", generator=g) * 1.5
    a = ext.mcat_sample(logits, list(nvec), 1234, 1)
    assert a.dtype == torch.int64 and a.shape == (N, C)
    off = 0
    for c, n in enumerate(nvec):
        assert int(a[:, c].min()) >= 0 and int(a[:, c].max()) < n
        p = torch.softmax(logits[:, off:off + n].double(), dim=-1)
        hits = torch.nn.functional.one_hot(a[:, c], n)
        assert_counts_follow(p, hits)
        off += n
    a2 = ext.mcat_sample(logits, list(nvec), 1234, 2)
    assert not torch.equal(a, a2)  # another counter, other draws


@pytest.mark.parametrize("n", [1, 8, 33])
def test_bern_sample_distribution(ext, n):
    N = 20000
    g = torch.Generator(device="cuda").manual_seed(6)
    logits = torch.randn(N, n, device="cuda", generator=g) * 1.5
    a = ext.bern_sample(logits, 1234, 1)
    assert a.dtype == torch.float32 and a.shape == (N, n)
    assert bool(((a == 0) | (a == 1)).all())
    assert_counts_follow(torch.sigmoid(logits.double()), a)
    a2 = ext.bern_sample(logits, 1234, 2)
    assert not torch.equal(a, a2)
