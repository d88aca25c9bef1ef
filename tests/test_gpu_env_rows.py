"""Row-owning env step (env_step_rows, DPPO_ENV_ROWS=1) against the path it
replaces: gemm_env_step with the fold off, followed by the x@V gemm_fwd of
the states just written.

One block owns every column panel of its rows, so the reward partials are
summed in env_finish2_kernel's order and the next step's x@V is one
ascending-k MFMA chain, as in gemm_fwd: everything is compared with
torch.equal, op level and engine level.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from dppo_amd.config import DPPOConfig
from dppo_amd.ops import require_hip_ext
from dppo_amd.parallel.comm import Comm
from dppo_amd.trainer import DPPOEngine

R = 16   # env rank = width of the x@V block of the concat buffer
SEED = 0x5EED1234
OUT_KEYS = ("xout", "dones", "t", "epr", "rewards", "xva")


def make_engine(**kw):
    base = dict(
        GAME="Humanoid-v4", HIDDEN_SIZES=(64, 64), ACTIVATION="tanh",
        NUM_ENVS=64, MAX_EPOCH_STEPS=12, EPOCH_MAX=1000, STOP_EPOCH=1000,
        NUM_WORKERS=1, LOG_FILE_PATH="/tmp/dppo_gpu_test_logs", DEVICE="cuda",
        USE_GRAPHS=False,
    )
    base.update(kw)
    return DPPOEngine(DPPOConfig(**base), comm=Comm(device="cuda:0"))


def v3_views(eng):
    """states, pdflats, actions, values, rewards, dones, boot_v"""
    c = eng.cfg
    T, E = c.MAX_EPOCH_STEPS, c.NUM_ENVS
    D = eng.obs_space.shape[0]
    A = eng.act_space.shape[0]
    out, o, res = eng._rollout_out, 0, []
    for shape in [(T, E, D), (T, E, 2 * A), (T, E, A), (T, E), (T, E),
                  (T, E), (E,)]:
        n = 1
        for sd in shape:
            n *= sd
        res.append(out.narrow(0, o, n).view(shape))
        o += n
    return res


def op_inputs(E, D, K):
    """As test_gpu_env_fused.op_inputs, with the concat width K a parameter:
    every third env sits on its last step, so reset rows feed the chain."""
    g = torch.Generator(device="cpu").manual_seed(1000 * E + D + 7 * K)

    def rnd(*shape):
        return torch.randn(*shape, generator=g)

    horizons = torch.randint(3, 9, (E,), generator=g, dtype=torch.int32)
    t = (torch.randint(0, 1 << 20, (E,), generator=g, dtype=torch.int32)
         % (horizons - 1))
    t[::3] = horizons[::3] - 1
    cpu = dict(
        xva=rnd(E, K), M=0.2 * rnd(K, D), xin=torch.tanh(rnd(E, D)),
        envd=0.5 * rnd(D), horizons=horizons, t=t, epr=rnd(E),
        V=0.1 * rnd(D, R),
    )
    return {k: v.cuda().contiguous() for k, v in cpu.items()}


def step_ref(inp, xva, xin, t, epr, sigma, step):
    """Today's default: gemm_env_step (fold off) + x@V gemm_fwd into xva.
    xva, t and epr are updated in place."""
    ext = require_hip_ext()
    E, D = xin.shape
    kw = xva.shape[1]
    dev = "cuda"
    xout = torch.full((E, D), float("nan"), device=dev)
    rewards = torch.empty(E, device=dev)
    dones = torch.empty(E, device=dev)
    seed = torch.full((1,), SEED, dtype=torch.int64, device=dev)
    empty = torch.empty(0, device=dev)
    rsum = torch.zeros(((D + 63) // 64) * E, device=dev)
    ext.gemm_env_step(xva, inp["M"], xin, xout, inp["envd"], inp["horizons"],
                      t, epr, rewards, dones, rsum, seed, sigma, step, empty,
                      empty)
    ext.gemm_fwd(xout, inp["V"], torch.zeros(R, device=dev), 2, 0, xva, xva,
                 xva, 0, 0, kw)
    torch.cuda.synchronize()
    return dict(xout=xout, dones=dones, t=t, epr=epr, rewards=rewards,
                xva=xva)


def step_rows(inp, xva, xin, t, epr, sigma, step):
    ext = require_hip_ext()
    E, D = xin.shape
    dev = "cuda"
    xout = torch.full((E, D), float("nan"), device=dev)
    rewards = torch.empty(E, device=dev)
    dones = torch.empty(E, device=dev)
    seed = torch.full((1,), SEED, dtype=torch.int64, device=dev)
    ext.env_step_rows(xva, inp["M"], xin, xout, inp["envd"], inp["horizons"],
                      t, epr, rewards, dones, seed, sigma, step, inp["V"])
    torch.cuda.synchronize()
    return dict(xout=xout, dones=dones, t=t, epr=epr, rewards=rewards,
                xva=xva)


def assert_same(ref, got, where=""):
    for k in OUT_KEYS:
        assert torch.equal(ref[k], got[k]), (k, where)


# (1, 376); (130, 376): partial row tile + last panel of 56 columns;
# (257, 64): exactly one panel; (128, 8): one panel narrower than one MFMA
# group of 16 columns; (129, 132): three panels, the last 4 columns wide
OP_SHAPES = [(1, 376), (130, 376), (257, 64), (128, 8), (129, 132)]


@pytest.mark.parametrize("K", [36, 20])   # 20: A = 1
@pytest.mark.parametrize("sigma", [0.05, 0.0])
@pytest.mark.parametrize("E,D", OP_SHAPES)
def test_op_bitwise_matches_env_step_plus_xv(E, D, sigma, K):
    inp = op_inputs(E, D, K)
    ref = step_ref(inp, inp["xva"].clone(), inp["xin"], inp["t"].clone(),
                   inp["epr"].clone(), sigma, 3)
    got = step_rows(inp, inp["xva"].clone(), inp["xin"], inp["t"].clone(),
                    inp["epr"].clone(), sigma, 3)
    if E > 1:
        assert ref["dones"].sum() > 0
    assert not torch.isnan(got["xout"]).any()
    assert_same(ref, got)
    # the action / pad columns of the concat buffer are not this op's
    assert torch.equal(got["xva"][:, R:], inp["xva"][:, R:])
    # and the x@V block is that of the written states
    want = got["xout"].double() @ inp["V"].double()
    torch.testing.assert_close(got["xva"][:, :R].double(), want, atol=3e-5,
                               rtol=3e-5)


@pytest.mark.parametrize("sigma", [0.05, 0.0])
def test_three_chained_calls(sigma):
    """Step s's xva (its x@V block) feeds step s+1; new action columns are
    written between the calls, as the policy forward does."""
    E, D, K = 130, 376, 36
    inp = op_inputs(E, D, K)
    g = torch.Generator(device="cpu").manual_seed(5)
    ra = dict(xva=inp["xva"].clone(), xin=inp["xin"], t=inp["t"].clone(),
              epr=inp["epr"].clone())
    rb = dict(xva=inp["xva"].clone(), xin=inp["xin"], t=inp["t"].clone(),
              epr=inp["epr"].clone())
    n_done = 0
    for s in range(3):
        act = torch.randn(E, K - R, generator=g).cuda()
        ra["xva"][:, R:] = act
        rb["xva"][:, R:] = act
        ref = step_ref(inp, ra["xva"], ra["xin"], ra["t"], ra["epr"], sigma,
                       s)
        got = step_rows(inp, rb["xva"], rb["xin"], rb["t"], rb["epr"], sigma,
                        s)
        assert_same(ref, got, where=f"call {s}")
        n_done += int(ref["dones"].sum())
        ra["xin"], rb["xin"] = ref["xout"], got["xout"]
    assert n_done > 0


def rollout_and_train(monkeypatch, rows, **kw):
    monkeypatch.setenv("DPPO_ENV_ROWS", rows)
    torch.manual_seed(0)
    eng = make_engine(**kw)
    batch, _ = eng.rollout_once()
    views = v3_views(eng)
    snap = dict(states=batch.states.clone(), actions=batch.actions.clone(),
                oldflat=batch.oldflat.clone(), values=views[3].clone(),
                rewards=views[4].clone(), dones=views[5].clone(),
                env_x=eng.env.x.clone())
    launches = eng.env_rows_launches
    eng.train_round()
    eng.train_round()
    snap["flat_param"] = eng.flat_pi.flat_param.detach().clone()
    return snap, launches, eng


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("num_envs", [64, 130])
def test_engine_rows_bitwise_matches_default_path(monkeypatch, num_envs,
                                                  graphs):
    monkeypatch.setenv("DPPO_ROLLOUT_V3", "1")
    monkeypatch.delenv("DPPO_ENV_FUSED", raising=False)
    monkeypatch.delenv("DPPO_XV_FOLD", raising=False)
    kw = dict(NUM_ENVS=num_envs, MAX_EPOCH_STEPS=12, SEED=41,
              USE_GRAPHS=graphs)
    on, n_on, eng_on = rollout_and_train(monkeypatch, "1", **kw)
    off, n_off, eng_off = rollout_and_train(monkeypatch, "0", **kw)
    T = kw["MAX_EPOCH_STEPS"]
    assert n_on >= T and n_on % T == 0
    assert n_off == 0 and eng_off.env_rows_launches == 0
    if graphs:
        assert eng_on._v3_graph is not None
        assert eng_off._v3_graph is not None
    assert off["dones"].sum() > 0
    for k in ("states", "actions", "oldflat", "values", "rewards", "dones",
              "env_x", "flat_param"):
        assert torch.equal(on[k], off[k]), k


def test_knob_validation(monkeypatch):
    monkeypatch.setenv("DPPO_ROLLOUT_V3", "1")
    monkeypatch.delenv("DPPO_ENV_FUSED", raising=False)
    monkeypatch.delenv("DPPO_XV_FOLD", raising=False)
    monkeypatch.setenv("DPPO_ENV_ROWS", "2")
    eng = make_engine()
    with pytest.raises(ValueError, match="DPPO_ENV_ROWS"):
        eng.rollout_once()


def test_fold_keeps_its_own_path(monkeypatch):
    monkeypatch.setenv("DPPO_ROLLOUT_V3", "1")
    monkeypatch.delenv("DPPO_ENV_FUSED", raising=False)
    monkeypatch.setenv("DPPO_XV_FOLD", "1")
    monkeypatch.setenv("DPPO_ENV_ROWS", "1")
    eng = make_engine()
    v3 = eng._v3_buffers()
    v3["xvp"].fill_(float("nan"))
    eng.rollout_once()
    assert eng.env_rows_launches == 0
    assert not torch.isnan(v3["xvp"]).any()   # the fold wrote its partials
