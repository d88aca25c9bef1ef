"""Lane-per-env Acrobot rollout (classic_rollout.hip: classic_rollout_cat with
env_id 2, three logits, one RK4 step per env step) vs eager references.

As in test_gpu_rollout_classic.py, whose tolerances these are, the checks do
not depend on the kernel's counter RNG: recorded policy outputs == eager
pi(recorded states) at 2e-4; every recorded transition replays through
envs/classic.py's acrobot_step / acrobot_obs at 3e-5; dones are exact except
where the replay's own bar margin |-cos th1' - cos(th1' + th2') - 1| is below
1e-4 (at most 1 % of the rows; there the replay follows the kernel's flag);
resets lie in range; persisted state and episode moments equal the replay;
action statistics follow the recorded distribution within 5 sigma; launches
are deterministic per seed.  Kernel tests call the binding directly.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from dppo_amd.config import DPPOConfig
from dppo_amd.envs.classic import BatchedAcrobot, acrobot_obs, acrobot_step
from dppo_amd.models.mlp import PolicyValueMLP
from dppo_amd.ops import require_hip_ext
from dppo_amd.parallel.comm import Comm
from dppo_amd.trainer import DPPOEngine

STEP_TOL = dict(atol=3e-5, rtol=3e-5)
PI_TOL = dict(atol=2e-4, rtol=2e-4)
TERM_BAND = 1e-4
NAMES = ("states", "pdflats", "actions", "values", "rewards", "dones",
         "boot_v", "moments")
K = 3


def make_case(hidden, activation, E, spread=False, bias_class=None,
              time_limit=500, stagger=False, moderate_seed=None):
    """(pi, env, epr) on the GPU.  spread scales the 0.01-init trunk and heads
    by 100 and adds a three-point -1.5 / 0 / +1.5 ramp over the logit columns,
    so all three columns are state-dependent and far from uniform.  stagger
    starts env e at step counter e % time_limit.  moderate_seed overwrites the
    reset states with seeded states of the moderate grid (angles over
    [-pi, pi), |omega1| <= 4, |omega2| <= 6), many of which are at or near the
    bar."""
    torch.manual_seed(7)
    env = BatchedAcrobot(E, device="cuda", seed=3, time_limit=time_limit)
    pi = PolicyValueMLP(obs_dim=env.obs_dim, action_space=env.action_space,
                        hidden_sizes=hidden, activation=activation).cuda()
    with torch.no_grad():
        if spread:
            pi.pi.weight.mul_(100.0)
            pi.vf.weight.mul_(100.0)
            for lay in pi.hidden:
                lay.weight.mul_(100.0)
            pi.pi.bias += torch.linspace(-1.5, 1.5, K, device="cuda")
            pi.vf.bias += 0.5
        if bias_class is not None:
            pi.pi.bias[bias_class] += 40.0
    env.reset()
    if moderate_seed is not None:
        gen = torch.Generator().manual_seed(moderate_seed)
        u = 2.0 * torch.rand(E, 4, generator=gen) - 1.0
        s = u * torch.tensor([math.pi, math.pi, 4.0, 6.0])
        s[:, :2] = s[:, :2].clamp(-math.pi, math.pi - 1e-6)
        env.s = s.float().cuda()
        env.x = acrobot_obs(env.s)
    if stagger:
        env.t = (torch.arange(E, device="cuda") % time_limit).to(torch.int32)
    epr = torch.zeros(E, device="cuda")
    return pi, env, epr


def weight_blob(pi):
    """Wt[in][out] + b per hidden layer, Wv[H], bv, Wpt[H][3], bp."""
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


def run_kernel(pi, env, epr, T, eps=0.0, seed=1234):
    blob, offsets, dims = weight_blob(pi)
    ext = require_hip_ext()
    act = 1 if pi.activation == "tanh" else 0
    E = env.num_envs
    out = ext.classic_rollout_cat(
        blob, offsets, dims, act, env.ENV_ID, env.s, env.time_limit,
        float(eps), env.x, env.t, epr, T, K, seed,
        torch.empty(0, device="cuda"))
    assert out[2].dtype == torch.long and out[2].shape == (T, E)
    assert int(out[2].min()) >= 0 and int(out[2].max()) < K
    assert out[0].shape == (T, E, 6)
    assert out[1].shape == (T, E, K)
    return dict(zip(NAMES, out))


# ---- policy outputs ----------------------------------------------------------

def assert_policy_outputs(pi, env, o, T, E):
    with torch.no_grad():
        v_ref, flat_ref = pi(o["states"].reshape(T * E, 6))
        vb, _ = pi(env.x)
    if E > 1:   # all three columns vary over the batch
        assert float(flat_ref.std(dim=0).min()) > 1e-2
    assert o["pdflats"].shape == (T, E, K)
    torch.testing.assert_close(o["pdflats"].reshape(T * E, K), flat_ref,
                               **PI_TOL)
    torch.testing.assert_close(o["values"].reshape(T * E), v_ref, **PI_TOL)
    torch.testing.assert_close(o["boot_v"], vb, **PI_TOL)


# E: a lone lane, an exact wave, a wave plus a 1-lane tail, several blocks
# with a tail.  (64, 64) is the widest trunk the kernel takes and goes through
# the [unit][lane] image of layer 1.
@pytest.mark.parametrize("E", [1, 64, 65, 200])
@pytest.mark.parametrize("hidden,activation", [((16,), "relu"),
                                               ((64, 64), "tanh")])
def test_recorded_policy_outputs_match_eager_forward(hidden, activation, E):
    T = 8
    pi, env, epr = make_case(hidden, activation, E, spread=True,
                             moderate_seed=21)
    o = run_kernel(pi, env, epr, T)
    assert_policy_outputs(pi, env, o, T, E)


# widths that are no multiple of the kernel's 4-unit tile: the padded units
# must contribute nothing to any of the three logits
@pytest.mark.parametrize("hidden", [(13,), (7, 30)])
def test_widths_off_the_unit_tile(hidden):
    T, E = 4, 65
    pi, env, epr = make_case(hidden, "tanh", E, spread=True, moderate_seed=22)
    o = run_kernel(pi, env, epr, T)
    assert_policy_outputs(pi, env, o, T, E)


# ---- transition replay, resets, persistence, moments ------------------------

def recover_state(obs):
    return torch.stack([torch.atan2(obs[..., 1], obs[..., 0]),
                        torch.atan2(obs[..., 3], obs[..., 2]),
                        obs[..., 4], obs[..., 5]], dim=-1)


def replay(env, o, t0, epr0, T):
    """Replays the recorded run through acrobot_step, asserting every
    transition; returns (step counters, running returns, finished-episode
    returns, terminations, truncations, rows inside the bar band)."""
    states, actions = o["states"], o["actions"]
    rewards, dones = o["rewards"], o["dones"]
    tc = t0.clone().long()
    epr = epr0.clone()
    finished, n_term, n_trunc, n_band = [], 0, 0, 0
    reset_rows, worst = [], 0.0
    for t in range(T):
        s2, _, term = acrobot_step(recover_state(states[t]), actions[t])
        nxt = acrobot_obs(s2)
        th1, th2 = s2[:, 0].double(), s2[:, 1].double()
        margin = -torch.cos(th1) - torch.cos(th1 + th2) - 1.0
        band = margin.abs() < TERM_BAND
        n_band += int(band.sum())
        tc += 1
        trunc = tc >= env.time_limit
        kdone = dones[t] > 0
        assert bool(((dones[t] == 0) | (dones[t] == 1)).all())
        # outside the band the flag is exact; inside it the replay follows
        # the kernel's flag, which a truncated row shows only in its reward
        term = torch.where(band & ~trunc, kdone, term)
        term = torch.where(band & trunc, rewards[t] == 0.0, term)
        done = term | trunc
        assert torch.equal(kdone, done), t
        # reward: 0 exactly on a terminating step, -1 elsewhere
        assert torch.equal(rewards[t], torch.where(term, 0.0, -1.0)), t
        following = states[t + 1] if t + 1 < T else env.x
        live = ~done
        if bool(live.any()):
            worst = max(worst, float((following[live] - nxt[live]).abs().max()))
        torch.testing.assert_close(following[live], nxt[live], **STEP_TOL)
        fresh = recover_state(following[done])
        assert bool((fresh.abs() <= 0.1 + 1e-6).all())
        reset_rows.append(following[done])
        n_term += int(term.sum())
        n_trunc += int((trunc & ~term).sum())
        epr += rewards[t]
        finished += epr[done].tolist()
        epr[done] = 0.0
        tc[done] = 0
    print("replay: max |kernel - acrobot_step| over live rows =", worst,
          "band rows:", n_band)
    reset_rows = torch.cat(reset_rows)
    assert reset_rows.shape[0] >= 2
    # different envs / steps draw different fresh states
    assert int(torch.unique(reset_rows, dim=0).shape[0]) == reset_rows.shape[0]
    return tc, epr, finished, n_term, n_trunc, n_band


@pytest.mark.parametrize("hidden,activation", [((16,), "relu"),
                                               ((64, 64), "tanh")])
def test_replay_of_every_transition(hidden, activation):
    E, T = 130, 48
    pi, env, epr_dev = make_case(hidden, activation, E, spread=True,
                                 time_limit=11, stagger=True, moderate_seed=5)
    t0, epr0 = env.t.clone(), epr_dev.clone()
    x0 = env.x.clone()
    o = run_kernel(pi, env, epr_dev, T)
    assert torch.equal(o["states"][0], x0)
    tc, epr, finished, n_term, n_trunc, n_band = replay(env, o, t0, epr0, T)
    assert n_band <= 0.01 * T * E
    assert n_term >= 10 and n_trunc >= 10, (n_term, n_trunc)
    assert set(o["actions"].unique().tolist()) == {0, 1, 2}
    # persisted per-env state (env.x was checked against the replay above)
    assert torch.equal(env.t.long(), tc)
    torch.testing.assert_close(epr_dev, epr, atol=1e-4, rtol=1e-4)
    assert bool((env.s[:, :2] >= -math.pi).all())
    assert bool((env.s[:, :2] < math.pi).all())
    torch.testing.assert_close(acrobot_obs(env.s), env.x, atol=1e-6, rtol=0)
    # episode moments == the episode list rebuilt from rewards / dones
    mom = o["moments"]
    ep = torch.tensor(finished, dtype=torch.float64)
    assert int(mom[0]) == len(finished) > 0
    torch.testing.assert_close(float(mom[1]), float(ep.sum()),
                               atol=2e-2, rtol=1e-4)
    torch.testing.assert_close(float(mom[2]), float((ep * ep).sum()),
                               atol=2e-2, rtol=1e-4)
    torch.testing.assert_close(float(mom[3]), float(ep.min()),
                               atol=1e-4, rtol=1e-4)
    torch.testing.assert_close(float(mom[4]), float(ep.max()),
                               atol=1e-4, rtol=1e-4)
    # a second launch continues where the first stopped
    x1 = env.x.clone()
    o2 = run_kernel(pi, env, epr_dev, 2, seed=99)
    assert torch.equal(o2["states"][0], x1)


# ---- sampling ------------------------------------------------------------------

def assert_counts_follow(logits, actions):
    """|count_j - sum_n p_nj| <= 5 sqrt(sum_n p_nj (1 - p_nj)): the count of
    class j is a sum of independent Bernoulli(p_nj), so this is its 5 sigma
    bound (derived, not tuned)."""
    p = torch.softmax(logits.reshape(-1, K).double(), dim=-1)
    counts = torch.bincount(actions.reshape(-1), minlength=K).double()
    bound = 5.0 * (p * (1.0 - p)).sum(dim=0).sqrt()
    diff = (counts - p.sum(dim=0)).abs()
    assert bool((diff <= bound).all()), (counts.tolist(), p.sum(0).tolist(),
                                        bound.tolist())


def test_sampling_follows_recorded_logits():
    pi, env, epr = make_case((16,), "relu", 512, spread=True, moderate_seed=31)
    o = run_kernel(pi, env, epr, 16)
    logits, actions = o["pdflats"], o["actions"]
    p = torch.softmax(logits, -1)
    # neither uniform nor one-hot, and every class is drawn
    assert 0.4 < float(p.max(dim=-1).values.mean()) < 0.999
    assert float(p.reshape(-1, K).mean(dim=0).min()) > 0.02
    assert_counts_follow(logits, actions)
    # step 0 alone, across envs: an RNG ignoring the env index fails here
    assert_counts_follow(logits[0], actions[0])
    # envs 0..7 across 256 steps: an RNG ignoring the step index fails here
    pi, env, epr = make_case((16,), "relu", 64, spread=True, moderate_seed=32)
    o = run_kernel(pi, env, epr, 256)
    assert_counts_follow(o["pdflats"][:, :8], o["actions"][:, :8])


def test_full_exploration_is_uniform_over_three_classes():
    E, T = 512, 16
    N = E * T
    # eps = 1: the overlay redraws every action uniformly over K = 3, against
    # a policy that would always choose class 2 (an n = 2 left in the overlay
    # never draws class 2)
    pi, env, epr = make_case((16,), "relu", E, bias_class=2)
    actions = run_kernel(pi, env, epr, T, eps=1.0)["actions"]
    counts = torch.bincount(actions.reshape(-1), minlength=K).double()
    sigma = math.sqrt(N * (1.0 / 3.0) * (2.0 / 3.0))
    assert float((counts - N / 3.0).abs().max()) <= 5.0 * sigma, counts
    # eps = 0: the +40 logit of the third column always wins
    pi, env, epr = make_case((16,), "relu", E, bias_class=2)
    assert bool((run_kernel(pi, env, epr, T)["actions"] == 2).all())


# ---- determinism --------------------------------------------------------------

def test_same_seed_is_bitwise_and_other_seed_differs():
    def run(seed):
        pi, env, epr = make_case((32,), "tanh", 130, spread=True,
                                 time_limit=11, moderate_seed=41)
        o = run_kernel(pi, env, epr, 24, eps=0.2, seed=seed)
        return o, (env.s, env.x, env.t, epr)

    a, pa = run(5)
    b, pb = run(5)
    for k in NAMES:
        assert torch.equal(a[k], b[k]), k
    for u, w in zip(pa, pb):
        assert torch.equal(u, w)
    c, _ = run(6)
    assert not torch.equal(a["actions"], c["actions"])


# ---- binding checks -------------------------------------------------------------

@pytest.mark.parametrize("env_id,n_actions", [(2, 2), (0, 3)])
def test_unsupported_env_and_action_pairs_raise(env_id, n_actions):
    """Host-side checks: nothing is launched, the env tensors are untouched."""
    pi, env, epr = make_case((16,), "relu", 4)
    blob, offsets, dims = weight_blob(pi)
    s0, x0, t0 = env.s.clone(), env.x.clone(), env.t.clone()
    with pytest.raises(RuntimeError, match=r"\(0, 2\).*\(2, 3\)"):
        require_hip_ext().classic_rollout_cat(
            blob, offsets, dims, 0, env_id, env.s, env.time_limit, 0.0,
            env.x, env.t, epr, 4, n_actions, 1, torch.empty(0, device="cuda"))
    assert torch.equal(env.s, s0) and torch.equal(env.x, x0)
    assert torch.equal(env.t, t0)


# ---- engine level ---------------------------------------------------------------

def make_engine(**kw):
    base = dict(
        GAME="Acrobot-v1", ENV_DYNAMICS="physics", HIDDEN_SIZES=(16,),
        ACTIVATION="relu", NUM_ENVS=128, MAX_EPOCH_STEPS=32, EPOCH_MAX=1000,
        STOP_EPOCH=1000, NUM_WORKERS=1,
        LOG_FILE_PATH="/tmp/dppo_gpu_test_logs", DEVICE="cuda",
    )
    base.update(kw)
    eng = DPPOEngine(DPPOConfig(**base), comm=Comm(device="cuda:0"))
    # episodes last up to 500 steps and a rollout 32: start the counters
    # near the limit so that the first rollout already finishes episodes
    if isinstance(eng.env, BatchedAcrobot):
        eng.env.t += 480
    return eng


ENGINE_CASES = [
    dict(HIDDEN_SIZES=(16,), ACTIVATION="relu"),
    dict(HIDDEN_SIZES=(64, 64), ACTIVATION="tanh"),
]


@pytest.mark.parametrize("kw", ENGINE_CASES, ids=["h16", "h64x64"])
def test_engine_takes_the_classic_rollout(kw, monkeypatch):
    monkeypatch.delenv("DPPO_ROLLOUT_CLASSIC", raising=False)

    def boom(self):
        raise AssertionError("eager loop entered on an eligible physics env")

    with monkeypatch.context() as m:
        m.setattr(DPPOEngine, "_rollout_once_eager_loop", boom)
        eng = make_engine(**kw)
        assert isinstance(eng.env, BatchedAcrobot)
        assert eng._can_rollout_classic() and eng._use_rollout_classic()
        assert not eng._can_fuse_rollout() and not eng._can_rollout_v3()
        assert not eng._can_fuse_rollout_cat()
        assert not eng._can_fuse_rollout_multi()
        # the fused Discrete update, graphed: its batch is the kernel's blob
        assert eng._can_fuse_update() and eng._batch_is_persistent()
        p0 = eng.flat_pi.flat_param.detach().clone()
        for _ in range(2):
            stats, _ = eng.train_round()
            assert all(math.isfinite(v) for v in stats.values())
        assert eng.classic_rollout_launches >= 2
        assert not torch.equal(p0, eng.flat_pi.flat_param.detach())

    monkeypatch.setenv("DPPO_ROLLOUT_CLASSIC", "0")
    ref = make_engine(**kw)
    assert ref._can_rollout_classic() and not ref._use_rollout_classic()
    stats, _ = ref.train_round()
    assert all(math.isfinite(v) for v in stats.values())
    assert ref.classic_rollout_launches == 0


def test_wide_trunk_is_not_eligible():
    assert not make_engine(HIDDEN_SIZES=(128,))._can_rollout_classic()
    assert not make_engine(HIDDEN_SIZES=(16, 16, 16))._can_rollout_classic()
    assert not make_engine(ENV_DYNAMICS="synthetic")._can_rollout_classic()


def test_ppo_learns_acrobot_through_the_kernel(monkeypatch):
    """Rollout kernel, GAE, the fused Discrete update and Adam together learn
    the swing-up.  E = 256, T = 512, (32,) tanh, lr 1e-2, 400 rounds (about
    2 s): epr_mean starts at -500 (no env reaches the bar inside the time
    limit) and at round 390 measured -102.5 / -152.2 / -126.0 on seeds
    0 / 1 / 2, and -121.5 on a second run of seed 0 (a training run is not
    bitwise repeatable); -250 leaves room for that and for another reset
    RNG.  The energy-pumping policy of test_env_acrobot.py
    scores about -75."""
    monkeypatch.delenv("DPPO_ROLLOUT_CLASSIC", raising=False)
    cfg = DPPOConfig(
        GAME="Acrobot-v1", ENV_DYNAMICS="physics", NUM_ENVS=256,
        MAX_EPOCH_STEPS=512, HIDDEN_SIZES=(32,), ACTIVATION="tanh",
        LEARNING_RATE=1e-2, EPOCH_MAX=410, STOP_EPOCH=10**6, NUM_WORKERS=1,
        SEED=0, LOG_FILE_PATH="/tmp/dppo_gpu_test_logs", DEVICE="cuda")
    eng = DPPOEngine(cfg, comm=Comm(device="cuda:0"))
    assert eng._use_rollout_classic()
    curve = [eng.train_round()[0]["epr_mean"] for _ in range(400)]
    print("epr_mean every 10th round:", [round(v, 1) for v in curve[::10]])
    assert eng.classic_rollout_launches >= 400
    assert curve[0] < -450.0
    assert max(curve[390:400]) >= -250.0
