"""Fused env-step epilogue of the rollout's G-GEMM (gemm_env_step) and the
x@V fold, against the split path (G-GEMM + rollout_env_step) and eager.

The split path is the reference: the fused epilogue repacks the GEMM
accumulators into env_finish_kernel's lane layout and runs the same
expression with the same RNG slots, so states are bitwise equal; only the
reward sum (per-panel partials) and, with the fold, x@V (per-panel
partials) are reassociated.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from dppo_amd.config import DPPOConfig
from dppo_amd.ops import require_hip_ext
from dppo_amd.parallel.comm import Comm
from dppo_amd.trainer import DPPOEngine

K = 36   # [x@V (16) | action (17) | pad (3)] — the flagship concat width
R = 16   # env rank


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


def op_inputs(E, D):
    g = torch.Generator(device="cpu").manual_seed(1000 * E + D)

    def rnd(*shape):
        return torch.randn(*shape, generator=g)

    horizons = torch.randint(3, 9, (E,), generator=g, dtype=torch.int32)
    # every third env sits on its last step -> done + reset this call
    t = (torch.randint(0, 1 << 20, (E,), generator=g, dtype=torch.int32)
         % (horizons - 1))
    t[::3] = horizons[::3] - 1
    cpu = dict(
        xva=rnd(E, K), M=0.2 * rnd(K, D), xin=torch.tanh(rnd(E, D)),
        envd=0.5 * rnd(D), horizons=horizons, t=t, epr=rnd(E),
        V=0.1 * rnd(D, R),
    )
    return {k: v.cuda().contiguous() for k, v in cpu.items()}


def run_op(inp, fused, sigma, fold=False, step=3):
    ext = require_hip_ext()
    E, D = inp["xin"].shape
    dev = "cuda"
    xva = inp["xva"].clone()
    t, epr = inp["t"].clone(), inp["epr"].clone()
    xout = torch.full((E, D), float("nan"), device=dev)
    rewards = torch.empty(E, device=dev)
    dones = torch.empty(E, device=dev)
    seed = torch.full((1,), 0x5EED1234, dtype=torch.int64, device=dev)
    empty = torch.empty(0, device=dev)
    if fused:
        npan = (D + 63) // 64
        rsum = torch.zeros(npan * E, device=dev)
        xvp = (torch.full((npan * E * R,), float("nan"), device=dev)
               if fold else empty)
        ext.gemm_env_step(xva, inp["M"], inp["xin"], xout, inp["envd"],
                          inp["horizons"], t, epr, rewards, dones, rsum,
                          seed, sigma, step, inp["V"] if fold else empty, xvp)
    else:
        G = torch.empty(E, D, device=dev)
        ext.gemm_fwd(xva, inp["M"], torch.zeros(D, device=dev), 2, 0, G, G,
                     G, 0, 0, 0)
        ext.rollout_env_step(inp["xin"], xout, G, inp["envd"],
                             inp["horizons"], t, epr, rewards, dones, seed,
                             sigma, step)
    torch.cuda.synchronize()
    return dict(xout=xout, dones=dones, t=t, epr=epr, rewards=rewards,
                xva=xva)


# (1, 376); (130, 376): partial row tile + last panel 56 of 64 columns;
# (128, 8): one panel narrower than a 32-column tile; (257, 64): exactly
# one full panel
OP_SHAPES = [(1, 376), (130, 376), (128, 8), (257, 64)]


@pytest.mark.parametrize("sigma", [0.05, 0.0])
@pytest.mark.parametrize("E,D", OP_SHAPES)
def test_op_fused_bitwise_matches_split(E, D, sigma):
    inp = op_inputs(E, D)
    ref = run_op(inp, fused=False, sigma=sigma)
    got = run_op(inp, fused=True, sigma=sigma)
    assert ref["dones"].sum() > 0 or E == 1
    assert not torch.isnan(got["xout"]).any()
    print("max |d reward| =",
          float((got["rewards"] - ref["rewards"]).abs().max()),
          " max |d epr| =", float((got["epr"] - ref["epr"]).abs().max()))
    for k in ("xout", "dones", "t", "epr"):
        assert torch.equal(ref[k], got[k]), k
    torch.testing.assert_close(got["rewards"], ref["rewards"], rtol=1e-6,
                               atol=1e-6)


@pytest.mark.parametrize("E,D", OP_SHAPES)
def test_op_fold_matches_eager_xv(E, D):
    """The folded x@V of the state actually written (reset rows included);
    pad columns of a partial last panel and pad rows must add nothing."""
    inp = op_inputs(E, D)
    off = run_op(inp, fused=True, sigma=0.05)
    on = run_op(inp, fused=True, sigma=0.05, fold=True)
    assert torch.equal(off["xout"], on["xout"])
    assert torch.equal(off["rewards"], on["rewards"])
    want = on["xout"].double() @ inp["V"].double()
    torch.testing.assert_close(on["xva"][:, :R].double(), want, atol=3e-5,
                               rtol=3e-5)
    # action / pad columns of the concat buffer are not the fold's
    assert torch.equal(on["xva"][:, R:], inp["xva"][:, R:])
    assert torch.equal(off["xva"], inp["xva"])


def test_engine_fused_matches_split_fold_off(monkeypatch):
    monkeypatch.setenv("DPPO_ROLLOUT_V3", "1")
    monkeypatch.setenv("DPPO_XV_FOLD", "0")
    kw = dict(NUM_ENVS=200, MAX_EPOCH_STEPS=12, SEED=41)
    torch.manual_seed(0)
    a = make_engine(**kw)
    torch.manual_seed(0)
    b = make_engine(**kw)
    assert a._env_fused()
    ba, _ = a.rollout_once()           # fused default
    monkeypatch.setenv("DPPO_ENV_FUSED", "0")
    assert not b._env_fused()
    bb, _ = b.rollout_once()           # split reference
    sa, sb = v3_views(a), v3_views(b)
    assert sb[5].sum() > 0
    assert torch.equal(ba.states, bb.states)
    assert torch.equal(ba.actions, bb.actions)
    assert torch.equal(sa[5], sb[5])  # dones
    assert torch.equal(a.env.x, b.env.x)
    torch.testing.assert_close(sa[4], sb[4], rtol=1e-6, atol=1e-6)


def test_engine_fold_xv_matches_eager(monkeypatch):
    """After a rollout the concat buffer holds the fold's x@V of the final
    state (some rows reset on the last step: horizons 3..8 divide T=12).
    E=130: partial last row tile; D=376: partial last panel."""
    monkeypatch.setenv("DPPO_ROLLOUT_V3", "1")
    monkeypatch.setenv("DPPO_XV_FOLD", "1")
    eng = make_engine(NUM_ENVS=130, MAX_EPOCH_STEPS=12)
    assert eng.obs_space.shape[0] % 64 != 0
    v3 = eng._v3_buffers()
    r = eng.env.rank_eff
    assert v3["xvp"] is not None and r == R
    v3["xvp"].fill_(float("nan"))   # every partial must be written
    eng.rollout_once()
    states, _, _, _, _, dones, _ = v3_views(eng)
    assert 0 < dones[-1].sum() < dones[-1].numel()
    want = eng.env.x.double() @ eng.env.V.double()
    torch.testing.assert_close(v3["xva"][:, :r].double(), want, atol=3e-5,
                               rtol=3e-5)


def test_engine_fold_on_matches_fold_off(monkeypatch):
    monkeypatch.setenv("DPPO_ROLLOUT_V3", "1")
    kw = dict(NUM_ENVS=64, MAX_EPOCH_STEPS=8, SEED=21)
    monkeypatch.setenv("DPPO_XV_FOLD", "0")
    torch.manual_seed(0)
    a = make_engine(**kw)
    ba, _ = a.rollout_once()
    monkeypatch.setenv("DPPO_XV_FOLD", "1")
    torch.manual_seed(0)
    b = make_engine(**kw)
    bb, _ = b.rollout_once()
    sa, sb = v3_views(a), v3_views(b)
    torch.testing.assert_close(ba.states, bb.states, atol=2e-3, rtol=2e-3)
    torch.testing.assert_close(ba.actions, bb.actions, atol=2e-3, rtol=2e-3)
    torch.testing.assert_close(sa[4], sb[4], atol=2e-3, rtol=2e-3)
    assert torch.equal(sa[5], sb[5])  # dones


@pytest.mark.parametrize("fold", [None, "1"])
def test_default_graphed_bitwise_matches_ungraphed(monkeypatch, fold):
    """Graph capture/replay of the default configuration (and of the
    opt-in fold) against eager per-step launches."""
    monkeypatch.setenv("DPPO_ROLLOUT_V3", "1")
    monkeypatch.delenv("DPPO_ENV_FUSED", raising=False)
    monkeypatch.delenv("DPPO_XV_FOLD", raising=False)
    if fold is not None:
        monkeypatch.setenv("DPPO_XV_FOLD", fold)
    a = make_engine(NUM_ENVS=64, MAX_EPOCH_STEPS=12, USE_GRAPHS=False)
    b = make_engine(NUM_ENVS=64, MAX_EPOCH_STEPS=12, USE_GRAPHS=True)
    ba, _ = a.rollout_once()
    bb, _ = b.rollout_once()
    assert b._v3_graph is not None
    assert torch.equal(ba.states, bb.states)
    assert torch.equal(ba.actions, bb.actions)
    assert torch.equal(ba.oldflat, bb.oldflat)
    a.train_round()
    b.train_round()
    assert torch.equal(a.flat_pi.flat_param, b.flat_pi.flat_param)
