"""Fused MultiCategorical / Bernoulli rollouts (rollout.hip, rollout_run_mcat
and rollout_run_bern) vs eager references.

As in test_gpu_rollout_cat.py, whose tolerances these are (2e-4 policy
outputs, 3e-5 transition and reward): the kernel's RNG is counter-based (not
torch's), so the checks are RNG-independent invariants or derived 5-sigma
binomial bounds, never trajectory equality with the eager loop.  Kernel tests
build the policy and env directly so shapes are free of the GAME preset table.
A family is an nvec tuple (MultiDiscrete) or an int n (MultiBinary).
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from dppo_amd import spaces
from dppo_amd.config import DPPOConfig
from dppo_amd.envs.synthetic import BatchedSyntheticEnv
from dppo_amd.models.mlp import PolicyValueMLP
from dppo_amd.ops import require_hip_ext
from dppo_amd.parallel.comm import Comm
from dppo_amd.trainer import DPPOEngine


def is_mcat(fam):
    return isinstance(fam, tuple)


def act_space(fam):
    return spaces.MultiDiscrete(list(fam)) if is_mcat(fam) \
        else spaces.MultiBinary(fam)


def width(fam):
    return sum(fam) if is_mcat(fam) else fam


def make_case(D, fam, hidden, activation, E, spread=False, head_bias=None):
    """(pi, env, epr) on the GPU.  spread: test_gpu_rollout_cat.make_case's
    recipe (head and hidden weights x100 and a +-1.5 logit ramp), which makes
    the policy state-dependent and far from uniform.  head_bias [P]: zero the
    head weights and set the bias, so every row has exactly these logits."""
    torch.manual_seed(7)
    P = width(fam)
    pi = PolicyValueMLP(obs_dim=D, action_space=act_space(fam),
                        hidden_sizes=hidden, activation=activation).cuda()
    with torch.no_grad():
        if spread:
            pi.pi.weight.mul_(100.0)
            for lay in pi.hidden:
                lay.weight.mul_(100.0)
            pi.pi.bias += torch.linspace(-1.5, 1.5, P, device="cuda")
        if head_bias is not None:
            pi.pi.weight.zero_()
            pi.pi.bias.copy_(torch.as_tensor(head_bias, dtype=torch.float32))
    env = BatchedSyntheticEnv(
        spaces.Box(low=-float("inf"), high=float("inf"), shape=(D,)),
        act_space(fam), E, device="cuda", seed=3, horizon=16)
    env.reset()
    epr = torch.zeros(E, device="cuda")
    return pi, env, epr


def weight_blob(pi):
    """Wt[in][out] + b per hidden layer, Wv[H], bv, Wpt[H][P], bp."""
    parts = []
    for lay in pi.hidden:
        parts += [lay.weight.t().contiguous(), lay.bias]
    parts += [pi.vf.weight, pi.vf.bias, pi.pi.weight.t().contiguous(),
              pi.pi.bias]
    offsets, off = [], 0
    for p in parts:
        offsets.append(off)
        off += p.numel()
    with torch.no_grad():
        blob = torch.cat([p.reshape(-1) for p in parts])
    return blob, offsets, [pi.obs_dim, *pi.hidden_sizes]


def run_kernel(pi, env, epr, T, fam, eps=0.0, noise=0.05, seed=1234):
    blob, offsets, dims = weight_blob(pi)
    ext = require_hip_ext()
    run = ext.rollout_run_mcat if is_mcat(fam) else ext.rollout_run_bern
    out = run(
        blob, offsets, dims, 1 if pi.activation == "tanh" else 0,
        env.blob, env.rank_eff, env.horizons_i32, float(noise), float(eps),
        env.x, env.t, epr, T, list(fam) if is_mcat(fam) else fam, seed,
        torch.empty(0, device="cuda"), 0)
    states, logits, actions, values, rewards, dones, boot_v, mom = out
    E = env.num_envs
    assert logits.shape == (T, E, width(fam))
    if is_mcat(fam):
        assert actions.dtype == torch.long
        assert actions.shape == (T, E, len(fam))
        assert int(actions.min()) >= 0
        assert bool((actions < torch.tensor(fam, device="cuda")).all())
    else:
        assert actions.dtype == torch.float32 and actions.shape == (T, E, fam)
        assert bool(((actions == 0) | (actions == 1)).all())
    return out


def check_policy_outputs(D, fam, hidden, activation, E, T):
    pi, env, epr = make_case(D, fam, hidden, activation, E, spread=True)
    states, logits, actions, values, rewards, dones, boot_v, mom = run_kernel(
        pi, env, epr, T, fam)
    P = width(fam)
    with torch.no_grad():
        v_ref, flat_ref = pi(states.reshape(T * E, D))
        vb, _ = pi(env.x)
    torch.testing.assert_close(logits.reshape(T * E, P), flat_ref,
                               atol=2e-4, rtol=2e-4)
    torch.testing.assert_close(values.reshape(T * E), v_ref,
                               atol=2e-4, rtol=2e-4)
    torch.testing.assert_close(boot_v, vb, atol=2e-4, rtol=2e-4)


FAMS = [(3, 3, 4), 8]
FAM_IDS = ["mcat", "bern"]


# E=130: 2-env tiles; 131: 8-env tiles + 3-env tail; 2051: grid 257 > 256
# CUs -> 4-waves/SIMD instantiation, tail tile
@pytest.mark.parametrize("E", [130, 131, 2051])
@pytest.mark.parametrize("fam", FAMS, ids=FAM_IDS)
def test_recorded_policy_outputs_match_eager_forward(fam, E):
    check_policy_outputs(6, fam, (16,), "relu", E, 8)


# P+1 head columns wider than the trunk: the k-split partial rows must be
# sized for the heads, not for the widest hidden layer
@pytest.mark.parametrize("fam,hidden", [((2,) * 32, (16,)), (32, (8, 8))],
                         ids=["mcat-2^32", "bern-32"])
def test_wide_head_over_narrow_trunk(fam, hidden):
    check_policy_outputs(5, fam, hidden, "tanh", 131, 4)


def action_input(env, fam, a):
    """a_in of recorded actions a [E, C] / [E, n], the eager env.step's."""
    if is_mcat(fam):
        off = torch.tensor([0] + list(fam[:-1]), device="cuda").cumsum(0)
        return env.B[a + off].sum(dim=1)
    return a @ env.B


@pytest.mark.parametrize("fam", FAMS, ids=FAM_IDS)
def test_env_transition_exact_at_zero_noise(fam):
    # horizon=16: horizons are 8..23, so no env finishes before step index 7
    # and no row of steps 0..6 is excluded
    D, E, T = 6, 128, 8
    pi, env, epr = make_case(D, fam, (16,), "relu", E, spread=True)
    states, logits, actions, values, rewards, dones, *_ = run_kernel(
        pi, env, epr, T, fam, noise=0.0)
    assert float(dones[:T - 1].sum()) == 0
    x = states
    for t in range(T - 1):
        pred = torch.tanh(x[t] * env.d + (x[t] @ env.V) @ env.U
                          + action_input(env, fam, actions[t]))
        torch.testing.assert_close(x[t + 1], pred, atol=3e-5, rtol=3e-5)
        r_pred = 1.0 - pred.pow(2).mean(dim=-1)
        torch.testing.assert_close(rewards[t], r_pred, atol=3e-5, rtol=3e-5)


@pytest.mark.parametrize("fam", FAMS, ids=FAM_IDS)
def test_done_schedule_and_episode_moments(fam):
    D, E, T = 6, 128, 48
    pi, env, epr_dev = make_case(D, fam, (16,), "relu", E)
    epr0 = epr_dev.clone()
    *_, rewards, dones, boot_v, mom = run_kernel(pi, env, epr_dev, T, fam)
    hor = env.horizons_i32.long().cpu()
    r, d = rewards.cpu(), dones.cpu()
    for e in range(8):
        h = int(hor[e])
        expect = torch.tensor(
            [1.0 if (t + 1) % h == 0 else 0.0 for t in range(T)])
        torch.testing.assert_close(d[:, e], expect)
    epr = epr0.cpu().clone()
    eps_list = []
    for t in range(T):
        epr += r[t]
        fin = d[t] > 0
        eps_list += epr[fin].tolist()
        epr[fin] = 0.0
    eps_t = torch.tensor(eps_list)
    assert int(mom[0]) == len(eps_list) > 0
    torch.testing.assert_close(float(mom[1]), float(eps_t.sum()),
                               atol=2e-2, rtol=1e-4)
    torch.testing.assert_close(float(mom[3]), float(eps_t.min()),
                               atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(float(mom[4]), float(eps_t.max()),
                               atol=1e-4, rtol=1e-4)
    # persisted per-env state
    torch.testing.assert_close(epr_dev.cpu(), epr, atol=1e-4, rtol=1e-4)
    assert torch.equal(env.t.long().cpu(), T % hor)


def assert_within_5_sigma(count, p_sum, var_sum):
    """|count - sum_n p_n| <= 5 sqrt(sum_n p_n (1 - p_n)), elementwise: each
    count is a sum of independent Bernoulli(p_n) (derived, not tuned)."""
    bound = 5.0 * var_sum.sqrt()
    diff = (count - p_sum).abs()
    assert bool((diff <= bound).all()), (count.tolist(), p_sum.tolist(),
                                        bound.tolist())


def assert_counts_follow(logits, actions, fam):
    """test_gpu_rollout_cat.assert_counts_follow per (component, class) of a
    MultiCategorical, per dim of a Bernoulli."""
    lg = logits.reshape(-1, width(fam)).double()
    a = actions.reshape(-1, actions.shape[-1])
    if is_mcat(fam):
        off = 0
        for c, n in enumerate(fam):
            p = torch.softmax(lg[:, off:off + n], dim=-1)
            counts = torch.bincount(a[:, c], minlength=n).double()
            assert_within_5_sigma(counts, p.sum(0), (p * (1 - p)).sum(0))
            off += n
    else:
        p = torch.sigmoid(lg)
        assert_within_5_sigma(a.double().sum(0), p.sum(0),
                              (p * (1 - p)).sum(0))


def assert_not_near_uniform(actions, fam):
    """Else the sampling check would be vacuous: in every component (in some
    dim) the draws must FAIL the same 5-sigma check against the uniform
    policy, so following the recorded logits is distinguishable from it."""
    a = actions.reshape(-1, actions.shape[-1])
    N = a.shape[0]
    if is_mcat(fam):
        for c, n in enumerate(fam):
            counts = torch.bincount(a[:, c], minlength=n).double()
            sigma = math.sqrt(N * (1.0 / n) * (1.0 - 1.0 / n))
            assert float((counts - N / n).abs().max()) > 5.0 * sigma
    else:
        ones = a.double().sum(0)
        assert float((ones - N / 2).abs().max()) > 5.0 * math.sqrt(N / 4)


@pytest.mark.parametrize("fam", [(3, 3, 4), (5, 2, 6), 8],
                         ids=["mcat", "mcat-5x2x6", "bern"])
def test_sampling_follows_recorded_logits(fam):
    D = 6
    pi, env, epr = make_case(D, fam, (16,), "relu", 512, spread=True)
    states, logits, actions, *_ = run_kernel(pi, env, epr, 16, fam, eps=0.0)
    assert_not_near_uniform(actions, fam)
    assert_counts_follow(logits, actions, fam)
    # step 0 alone, across envs: an RNG ignoring the env index fails here
    assert_counts_follow(logits[0], actions[0], fam)
    # envs 0..7 across 256 steps: an RNG ignoring the step index fails here
    pi, env, epr = make_case(D, fam, (16,), "relu", 64, spread=True)
    states, logits, actions, *_ = run_kernel(pi, env, epr, 256, fam, eps=0.0)
    assert_counts_follow(logits[:, :8], actions[:, :8], fam)


def test_components_draw_independently():
    """Marginals cannot see shared draws.  Two components (dims) with EQUAL
    logits: with shared uniforms a_0 == a_1 always; independent draws agree
    with probability sum_j p_j^2 (Bernoulli: p^2 + (1-p)^2)."""
    D, E, T = 6, 512, 16
    N = E * T
    bias = torch.tensor([0.0, 1.0, -0.5, 0.3])
    fam = (4, 4)
    pi, env, epr = make_case(D, fam, (16,), "relu", E,
                             head_bias=torch.cat([bias, bias]))
    _, _, actions, *_ = run_kernel(pi, env, epr, T, fam)
    q = float(torch.softmax(bias.double(), 0).pow(2).sum())
    share = float((actions[..., 0] == actions[..., 1]).double().mean())
    assert abs(share - q) <= 5.0 * math.sqrt(q * (1.0 - q) / N)

    pi, env, epr = make_case(D, 2, (16,), "relu", E, head_bias=[0.8, 0.8])
    _, _, actions, *_ = run_kernel(pi, env, epr, T, 2)
    p = 1.0 / (1.0 + math.exp(-0.8))
    q = p * p + (1.0 - p) * (1.0 - p)
    share = float((actions[..., 0] == actions[..., 1]).double().mean())
    assert abs(share - q) <= 5.0 * math.sqrt(q * (1.0 - q) / N)


@pytest.mark.parametrize("nvec,picks", [((3, 3, 4), (1, 0, 3)),
                                        ((5, 59), (4, 40)),
                                        ((2,) * 32, (1, 0) * 16)],
                         ids=["3x3x4", "5x59", "2^32"])
def test_mcat_degenerate_head_and_epsilon_overlay(nvec, picks):
    D, E, T = 6, 512, 16
    N = E * T
    bias = torch.zeros(sum(nvec))
    off = 0
    for n, j in zip(nvec, picks):
        bias[off + j] = 40.0
        off += n
    want = torch.tensor(picks, device="cuda")
    nv = torch.tensor(nvec, dtype=torch.float64)

    def actions_at(eps):
        pi, env, epr = make_case(D, nvec, (16,), "relu", E, head_bias=bias)
        return run_kernel(pi, env, epr, T, nvec, eps=eps)[2].reshape(N, -1)

    # +40 logit on one class per component, eps=0: the Gumbel noise spans < 20
    assert bool((actions_at(0.0) == want).all())
    # eps=1: every component uniform over its classes
    a = actions_at(1.0)
    for c, n in enumerate(nvec):
        counts = torch.bincount(a[:, c], minlength=n).double()
        sigma = math.sqrt(N * (1.0 / n) * (1.0 - 1.0 / n))
        assert float((counts - N / n).abs().max()) <= 5.0 * sigma
    # eps=0.25: ONE decision per (env, step), and an explored row redraws all
    # components independently, so
    #   P(component c deviates) = eps (n_c - 1) / n_c
    #   P(row deviates anywhere) = eps (1 - prod_c 1 / n_c)
    #   P(c and c' both deviate) = eps (n_c - 1)/n_c (n_c' - 1)/n_c'
    # (per-component decisions would give eps^2 in the last one)
    dev = actions_at(0.25) != want

    def check_share(share, q):
        assert abs(share - q) <= 5.0 * math.sqrt(q * (1.0 - q) / N), (share, q)

    for c, n in enumerate(nvec):
        check_share(float(dev[:, c].double().mean()), 0.25 * (n - 1) / n)
    check_share(float(dev.any(dim=1).double().mean()),
                0.25 * (1.0 - float((1.0 / nv).prod())))
    if len(nvec) > 1:
        check_share(float((dev[:, 0] & dev[:, 1]).double().mean()),
                    0.25 * (nvec[0] - 1) / nvec[0] * (nvec[1] - 1) / nvec[1])


@pytest.mark.parametrize("n", [1, 8, 32])
def test_bern_degenerate_head_and_epsilon_overlay(n):
    D, E, T = 6, 512, 16
    N = E * T
    want = (torch.arange(n) % 2 == 0).float()  # dims 0, 2, ... on
    bias = 80.0 * want - 40.0
    want = want.cuda()

    def actions_at(eps):
        pi, env, epr = make_case(D, n, (16,), "relu", E, head_bias=bias)
        return run_kernel(pi, env, epr, T, n, eps=eps)[2].reshape(N, n)

    # +-40 logits, eps=0: sigmoid saturates, always 1 / always 0
    assert bool((actions_at(0.0) == want).all())
    # eps=1: Bernoulli(0.5) per dim
    ones = actions_at(1.0).double().sum(0)
    assert float((ones - N / 2).abs().max()) <= 5.0 * math.sqrt(N / 4)
    # eps=0.25: one decision per (env, step); an explored row redraws every
    # dim as Bernoulli(0.5) independently, so
    #   P(dim j deviates) = eps / 2
    #   P(row deviates anywhere) = eps (1 - 2^-n)
    #   P(dims 0 and 1 both deviate) = eps / 4
    dev = actions_at(0.25) != want

    def check_share(share, q):
        assert abs(share - q) <= 5.0 * math.sqrt(q * (1.0 - q) / N), (share, q)

    for j in range(n):
        check_share(float(dev[:, j].double().mean()), 0.125)
    check_share(float(dev.any(dim=1).double().mean()),
                0.25 * (1.0 - 0.5 ** n))
    if n > 1:
        check_share(float((dev[:, 0] & dev[:, 1]).double().mean()), 0.0625)


@pytest.mark.parametrize("fam", [(32, 33), (3, 1, 4), 33],
                         ids=["sum65", "size1", "bern33"])
def test_binding_limits_raise_before_launch(fam):
    # a valid policy / env of another shape: the limit check comes first
    pi, env, epr = make_case(6, 8, (16,), "relu", 16)
    with pytest.raises(RuntimeError, match="supports|needs"):
        run_kernel(pi, env, epr, 4, fam)
    torch.cuda.synchronize()


# ---- engine level ----

def make_engine(**kw):
    base = dict(
        GAME="MultiLever-v0", HIDDEN_SIZES=(32,), ACTIVATION="tanh",
        NUM_ENVS=128, MAX_EPOCH_STEPS=32, EPOCH_MAX=1000, STOP_EPOCH=1000,
        NUM_WORKERS=1, LOG_FILE_PATH="/tmp/dppo_gpu_test_logs", DEVICE="cuda",
    )
    base.update(kw)
    return DPPOEngine(DPPOConfig(**base), comm=Comm(device="cuda:0"))


ENGINE_CASES = [
    dict(GAME="MultiLever-v0", HIDDEN_SIZES=(32,), NUM_ENVS=128),
    dict(GAME="BitFlipper-v0", HIDDEN_SIZES=(64, 64), NUM_ENVS=256),
]


@pytest.mark.parametrize("kw", ENGINE_CASES, ids=["multilever", "bitflipper"])
def test_engine_fused_multi_rollout(kw, monkeypatch):
    monkeypatch.setenv("DPPO_ROLLOUT_MULTI", "0")
    ref = make_engine(**kw)
    assert ref._can_fuse_rollout_multi() and not ref._use_rollout_multi()
    assert not ref._can_fuse_rollout_cat() and not ref._can_fuse_rollout()
    calls = []
    eager = DPPOEngine._rollout_once_eager_loop
    monkeypatch.setattr(
        DPPOEngine, "_rollout_once_eager_loop",
        lambda self: (calls.append(1), eager(self))[1])
    b_ref, _ = ref.rollout_once()
    assert calls  # DPPO_ROLLOUT_MULTI=0 takes the eager loop

    monkeypatch.setenv("DPPO_ROLLOUT_MULTI", "1")

    def boom(self):
        raise AssertionError("eager loop entered with DPPO_ROLLOUT_MULTI=1")

    monkeypatch.setattr(DPPOEngine, "_rollout_once_eager_loop", boom)
    eng = make_engine(**kw)
    assert eng._use_rollout_multi() and not eng._can_fuse_rollout_cat()
    batch, _ = eng.rollout_once()
    T, E = eng.cfg.MAX_EPOCH_STEPS, eng.cfg.NUM_ENVS
    P = eng.pi.pdtype.param_shape()[0]
    assert batch.oldflat.shape == (T * E, P)
    for f in ("states", "actions", "adv", "etr", "oldflat", "oldv",
              "ep_count", "ep_sum", "ep_sumsq", "ep_min", "ep_max"):
        got, want = getattr(batch, f), getattr(b_ref, f)
        assert got.dtype == want.dtype, f
        assert got.shape == want.shape, f
    assert isinstance(batch.valid, bool) and batch.valid
    p0 = eng.flat_pi.flat_param.detach().clone()
    for _ in range(3):
        stats, _ = eng.train_round()
    assert all(math.isfinite(v) for v in stats.values())
    assert not torch.equal(p0, eng.flat_pi.flat_param.detach())
