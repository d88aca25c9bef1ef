"""The row-per-lane loss-gradient kernels of the discrete policy families
(ops/hip/disc_gh.hip: ppo_loss_cat_gh / ppo_loss_mcat_gh / ppo_loss_bern_gh)
against the eager definition of their output, ops.ppo_loss.ppo_gh_ref, and
against the wave-per-row backward kernels they share their formulas with.

Tolerances are tests/test_gpu_multi_loss.py's gradient tolerances for the
same math: atol 1e-6, rtol 1e-4."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from dppo_amd.distributions import (
    BernoulliPd, CategoricalPd, MultiCategoricalPd)
from dppo_amd.ops import require_hip_ext
from dppo_amd.ops.ppo_loss import PPOLossCoeffs, ppo_gh_ref

CLIP, ENTC, VC = 0.2, 0.01, 0.5
TOL = dict(atol=1e-6, rtol=1e-4)

# family, head: Categorical K | MultiCategorical nvec | Bernoulli n
HEADS = ([("cat", K) for K in (2, 3, 4, 63, 64)]
         + [("mcat", nv) for nv in ((2, 2), (3, 3, 4), (5, 2, 6), (2,) * 32)]
         + [("bern", n) for n in (1, 8, 33, 64)])


def head_id(h):
    fam, head = h
    if fam == "mcat":
        head = "x".join(map(str, head)) if len(head) < 8 else f"2x{len(head)}"
    return f"{fam}{head}"


def dims(fam, head):
    """(P logit columns, W action columns) of a head."""
    if fam == "cat":
        return head, 1
    if fam == "mcat":
        return sum(head), len(head)
    return head, head


def make_pd(fam, head, flat):
    if fam == "cat":
        return CategoricalPd(flat)
    if fam == "mcat":
        return MultiCategoricalPd(head, flat)
    return BernoulliPd(flat)


def make_inputs(fam, head, B, step_one=False):
    """CPU fp32 operands: logits on a +-1.5 ramp with a x3 spread, oldpi
    logits perturbed so the ratio straddles both clip edges (the per-dim
    perturbation shrinks with the action width: the log-ratio sums over it),
    oldv perturbed across the value clip."""
    P, W = dims(fam, head)
    g = torch.Generator().manual_seed(1000 * P + W)
    ramp = torch.linspace(-1.5, 1.5, P) if P > 1 else torch.zeros(1)
    lpi = ramp + 3.0 * torch.rand(B, P, generator=g) - 1.5
    v = torch.randn(B, generator=g)
    if step_one:
        lold, oldv = lpi.clone(), v.clone()
    else:
        lold = lpi + (0.6 / math.sqrt(W)) * torch.randn(B, P, generator=g)
        oldv = v + 0.3 * torch.randn(B, generator=g)
    if fam == "cat":
        act = torch.randint(0, P, (B,), generator=g)
    elif fam == "mcat":
        act = torch.stack(
            [torch.randint(0, n, (B,), generator=g) for n in head], dim=1)
    else:
        act = torch.randint(0, 2, (B, P), generator=g).float()
    adv = torch.randn(B, generator=g)
    etr = v + torch.randn(B, generator=g)
    return dict(lpi=lpi, lold=lold, v=v, oldv=oldv, act=act, adv=adv, etr=etr)


def assert_every_branch_occurs(fam, head, x, clip=CLIP):
    """All three `flow` regimes and all value branches are in the inputs, and
    no row sits on a branch boundary (where fp32 and the reference may
    legitimately pick different sides).  Evaluated in float64."""
    d = {k: (t.double() if t.is_floating_point() else t) for k, t in x.items()}
    pd, old = make_pd(fam, head, d["lpi"]), make_pd(fam, head, d["lold"])
    ratio = torch.exp(pd.logp(d["act"]) - old.logp(d["act"]))
    lo, hi = 1.0 - clip, 1.0 + clip
    adv = d["adv"]
    assert bool(((ratio > lo) & (ratio < hi)).any()), "no unclipped row"
    assert bool(((ratio < lo) & (adv < 0)).any()), "no clipped-low row"
    assert bool(((ratio > hi) & (adv > 0)).any()), "no clipped-high row"
    assert float(torch.minimum((ratio - lo).abs(), (ratio - hi).abs()).min()) \
        > 1e-4
    diff = d["v"] - d["oldv"]
    vf1 = (d["v"] - d["etr"]) ** 2
    vf2 = (d["oldv"] + diff.clamp(-clip, clip) - d["etr"]) ** 2
    outside = diff.abs() > clip
    assert bool((~outside).any()), "no row inside the value clip"
    assert bool((outside & (vf1 > vf2)).any()), "no unclipped-value row"
    assert bool((outside & (vf1 < vf2)).any()), "no clipped-value row"
    assert float((diff.abs() - clip).abs().min()) > 1e-5
    assert float((vf1 - vf2)[outside].abs().min()) > 1e-5


def on_gpu(x, B):
    return {k: t[:B].cuda().contiguous() for k, t in x.items()}


def run_gh(fam, head, x, clip=CLIP, clip_dev=None):
    ext = require_hip_ext()
    cd = torch.empty(0, device="cuda") if clip_dev is None else clip_dev
    args = (x["lpi"], x["lold"], x["v"], x["oldv"], x["act"], x["adv"],
            x["etr"])
    if fam == "cat":
        return ext.ppo_loss_cat_gh(*args, clip, ENTC, VC, cd)
    if fam == "mcat":
        return ext.ppo_loss_mcat_gh(*args, list(head), clip, ENTC, VC, cd)
    return ext.ppo_loss_bern_gh(*args, clip, ENTC, VC, cd)


def run_bwd(fam, head, x, clip=CLIP):
    ext = require_hip_ext()
    one = torch.ones((), device="cuda")
    args = (x["lpi"], x["lold"], x["v"], x["oldv"], x["act"], x["adv"],
            x["etr"])
    if fam == "cat":
        return ext.ppo_loss_cat_bwd(*args, clip, ENTC, VC, one)
    if fam == "mcat":
        return ext.ppo_loss_mcat_bwd(*args, list(head), clip, ENTC, VC, one)
    return ext.ppo_loss_bern_bwd(*args, clip, ENTC, VC, one)


def ref_gh(fam, head, x, clip=CLIP):
    return ppo_gh_ref(make_pd(fam, head, x["lpi"]),
                      make_pd(fam, head, x["lold"]), x["v"], x["oldv"],
                      x["act"], x["adv"], x["etr"],
                      PPOLossCoeffs(clip, ENTC, VC))


def nan_poison(B, ldgh):
    """Leave a NaN-filled block of the output's size in the caching
    allocator, which the binding's torch::empty is then likely to get."""
    t = torch.full((B, ldgh), float("nan"), device="cuda")
    del t


@pytest.mark.parametrize("fam,head", HEADS, ids=map(head_id, HEADS))
def test_gh_matches_reference_and_backward_kernels(fam, head):
    P, W = dims(fam, head)
    ldgh = (P + 1 + 3) & ~3
    tile = require_hip_ext().ppo_gh_disc_tile(P, W)
    assert tile in (64, 128)
    sizes = (1, tile - 1, tile, tile + 1, 2 * tile + 3)
    full = make_inputs(fam, head, sizes[-1])
    assert_every_branch_occurs(fam, head, full)
    for B in sizes:
        x = on_gpu(full, B)
        nan_poison(B, ldgh)
        gh = run_gh(fam, head, x)
        assert gh.shape == (B, ldgh) and gh.dtype == torch.float32
        # pad columns: bitwise zero
        assert bool((gh[:, P + 1:].contiguous().view(torch.int32) == 0).all()), B
        torch.testing.assert_close(gh, ref_gh(fam, head, x), **TOL,
                                   msg=lambda m: f"B={B} vs ppo_gh_ref: {m}")
        g_logits, g_v = run_bwd(fam, head, x)
        torch.testing.assert_close(gh[:, :P], g_logits, **TOL,
                                   msg=lambda m: f"B={B} vs bwd kernel: {m}")
        torch.testing.assert_close(gh[:, P], g_v, **TOL,
                                   msg=lambda m: f"B={B} vs bwd kernel: {m}")


@pytest.mark.parametrize("fam,head", [("cat", 3), ("mcat", (3, 3, 4)),
                                      ("bern", 8)], ids=["cat", "mcat", "bern"])
def test_clip_dev_overrides_clip(fam, head):
    x_cpu = make_inputs(fam, head, 259)
    assert_every_branch_occurs(fam, head, x_cpu, clip=0.15)
    x = on_gpu(x_cpu, 259)
    gh = run_gh(fam, head, x, clip=0.35,
                clip_dev=torch.tensor([0.15], device="cuda"))
    torch.testing.assert_close(gh, ref_gh(fam, head, x, clip=0.15), **TOL)
    assert not torch.allclose(gh, ref_gh(fam, head, x, clip=0.35), **TOL)


@pytest.mark.parametrize("fam,head", [("cat", 2), ("cat", 64),
                                      ("mcat", (3, 3, 4)), ("bern", 8)],
                         ids=["cat2", "cat64", "mcat", "bern"])
def test_step_one_ratio_exactly_one(fam, head):
    """lold == lpi, oldv == v: every round's first update step."""
    P, _ = dims(fam, head)
    x = on_gpu(make_inputs(fam, head, 131, step_one=True), 131)
    gh = run_gh(fam, head, x)
    torch.testing.assert_close(gh, ref_gh(fam, head, x), **TOL)
    # flow = 1 and gv = 2 (v - etr): nothing is clipped away
    want_v = VC * 2.0 * (x["v"] - x["etr"]) / 131
    torch.testing.assert_close(gh[:, P], want_v, **TOL)
    assert bool((gh[:, :P].abs().sum(dim=1) > 0).all())


def _bad_cases():
    def cat(K=3, B=4, **over):
        x = on_gpu(make_inputs("cat", K, B), B)
        x.update({k: f(x) for k, f in over.items()})
        return "cat", K, x

    def mcat(nvec, P=None, B=4):
        P = sum(nvec) if P is None else P
        x = dict(lpi=torch.zeros(B, P), lold=torch.zeros(B, P),
                 v=torch.zeros(B), oldv=torch.zeros(B),
                 act=torch.zeros(B, len(nvec), dtype=torch.int64),
                 adv=torch.zeros(B), etr=torch.zeros(B))
        return "mcat", nvec, on_gpu(x, B)

    def bern(n, B=4):
        x = dict(lpi=torch.zeros(B, n), lold=torch.zeros(B, n),
                 v=torch.zeros(B), oldv=torch.zeros(B), act=torch.zeros(B, n),
                 adv=torch.zeros(B), etr=torch.zeros(B))
        return "bern", n, on_gpu(x, B)

    def wide_cat(K):
        x = dict(lpi=torch.zeros(4, K), lold=torch.zeros(4, K),
                 v=torch.zeros(4), oldv=torch.zeros(4),
                 act=torch.zeros(4, dtype=torch.int64), adv=torch.zeros(4),
                 etr=torch.zeros(4))
        return "cat", K, on_gpu(x, 4)

    return {
        "cat_K1": lambda: wide_cat(1),
        "cat_K65": lambda: wide_cat(65),
        "cat_act_int32": lambda: cat(act=lambda x: x["act"].int()),
        "cat_adv_rows": lambda: cat(adv=lambda x: torch.zeros(5, device="cuda")),
        "cat_lold_shape": lambda: cat(
            lold=lambda x: torch.zeros(4, 4, device="cuda")),
        "cat_fp64": lambda: cat(lpi=lambda x: x["lpi"].double()),
        "cat_strided": lambda: cat(
            lpi=lambda x: torch.zeros(3, 4, device="cuda").t()),
        "mcat_sum65": lambda: mcat((32, 33)),
        "mcat_size1": lambda: mcat((3, 1, 4)),
        "mcat_33comps": lambda: mcat((2,) * 33, P=64),
        "mcat_width": lambda: mcat((3, 3, 4), P=11),
        "bern_n65": lambda: bern(65),
        "bern_n0": lambda: bern(0),
    }


@pytest.mark.parametrize("case", sorted(_bad_cases()))
def test_binding_limits_raise_before_launch(case):
    fam, head, x = _bad_cases()[case]()
    with pytest.raises(RuntimeError, match="supports|needs"):
        run_gh(fam, head, x)
    torch.cuda.synchronize()
