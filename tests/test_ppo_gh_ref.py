"""ppo_gh_ref — the eager definition of the update's loss-gradient operand
gh = [d total_loss/d logits | d total_loss/d vpred | 0-pad] — for the three
discrete policy families, in float64 on the CPU."""

import pytest
import torch

from dppo_amd.distributions import (
    BernoulliPd, CategoricalPd, MultiCategoricalPd)
from dppo_amd.ops.ppo_loss import PPOLossCoeffs, ppo_gh_ref, ppo_losses_ref

B = 5
COEFFS = PPOLossCoeffs(clip_param=0.2, entcoeff=0.01, vcoeff=0.5)
NVEC = (3, 3, 4)


def make_pd(fam, flat):
    if fam == "cat":
        return CategoricalPd(flat)
    if fam == "mcat":
        return MultiCategoricalPd(NVEC, flat)
    return BernoulliPd(flat)


def make_case(fam, step_one=False):
    g = torch.Generator().manual_seed({"cat": 1, "mcat": 2, "bern": 3}[fam])

    def rnd(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)

    if fam == "cat":
        P = 4
        actions = torch.randint(0, P, (B,), generator=g)
    elif fam == "mcat":
        P = sum(NVEC)
        actions = torch.stack(
            [torch.randint(0, n, (B,), generator=g) for n in NVEC], dim=1)
    else:
        P = 6
        actions = torch.randint(0, 2, (B, P), generator=g).double()
    lpi, v = rnd(B, P), rnd(B)
    if step_one:
        lold, oldv = lpi.clone(), v.clone()
    else:
        lold, oldv = lpi + 0.3 * rnd(B, P), v + 0.3 * rnd(B)
    return dict(fam=fam, P=P, lpi=lpi, lold=lold, v=v, oldv=oldv,
                actions=actions, adv=rnd(B), etr=rnd(B))


def gh_of(c):
    return ppo_gh_ref(make_pd(c["fam"], c["lpi"]), make_pd(c["fam"], c["lold"]),
                      c["v"], c["oldv"], c["actions"], c["adv"], c["etr"],
                      COEFFS)


def total_loss(c, lpi, v):
    return ppo_losses_ref(make_pd(c["fam"], lpi), make_pd(c["fam"], c["lold"]),
                          v, c["oldv"], c["actions"], c["adv"], c["etr"],
                          COEFFS)["total_loss"]


@pytest.mark.parametrize("fam", ["cat", "mcat", "bern"])
def test_layout_and_finite_difference(fam):
    c = make_case(fam)
    P = c["P"]
    gh = gh_of(c)
    ldgh = (P + 1 + 3) & ~3
    assert gh.shape == (B, ldgh) and gh.dtype == torch.float64
    assert bool((gh[:, P + 1:] == 0).all())

    g = torch.Generator().manual_seed(7)
    dl = torch.randn(B, P, generator=g, dtype=torch.float64)
    dv = torch.randn(B, generator=g, dtype=torch.float64)
    h = 1e-5
    fd = (total_loss(c, c["lpi"] + h * dl, c["v"] + h * dv)
          - total_loss(c, c["lpi"] - h * dl, c["v"] - h * dv)) / (2 * h)
    got = (gh[:, :P] * dl).sum() + (gh[:, P] * dv).sum()
    assert abs(float(got - fd)) <= 1e-6 * abs(float(fd)), (float(got), float(fd))


@pytest.mark.parametrize("fam", ["cat", "mcat", "bern"])
def test_step_one_is_the_limit_of_the_generic_case(fam):
    """lold == lpi and oldv == v — every round's first update step: the ratio
    is exactly 1 and the value difference exactly 0, both on the ties of
    min / clamp / max.  The gradient is the limit from inside the clip window:
    flow = 1 (d policy/d logp = -adv/B) and gv = 2 (v - etr)."""
    c = make_case(fam, step_one=True)
    P = c["P"]
    gh = gh_of(c)

    lpi = c["lpi"].clone().requires_grad_(True)
    pd = make_pd(fam, lpi)
    surrogate = (-(c["adv"] * pd.logp(c["actions"])).sum()
                 - COEFFS.entcoeff * pd.entropy().sum()) / B
    (want_l,) = torch.autograd.grad(surrogate, lpi)
    want_v = COEFFS.vcoeff * 2.0 * (c["v"] - c["etr"]) / B
    torch.testing.assert_close(gh[:, :P], want_l, atol=1e-14, rtol=1e-12)
    torch.testing.assert_close(gh[:, P], want_v, atol=1e-14, rtol=1e-12)
    assert bool((gh[:, P + 1:] == 0).all())
