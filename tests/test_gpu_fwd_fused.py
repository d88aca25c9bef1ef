"""Fused policy forward (mlp_fwd_fused: L1 + L2 + heads, optionally action
sampling, in one launch) against the split chain it replaces: three
gemm_fwd calls plus rollout_sample.

The f32 MFMA is a k-ordered fma chain and the fused kernel shares the L1
loop and the epilogue code with gemm_fwd and keeps each layer's stage
order, so every output is bitwise equal: torch.equal, no tolerance.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from dppo_amd.ops import require_hip_ext
from test_gpu_env_fused import make_engine, v3_views

H = 64
GUARD = 96          # floats after every output buffer that must stay put
SENTINEL = -12345.5
VA_OFF = 16


def weights(D, A, seed=0):
    g = torch.Generator(device="cpu").manual_seed(977 * D + A + seed)

    def rnd(*shape, scale=1.0):
        return (torch.randn(*shape, generator=g) * scale).cuda().contiguous()

    P = 2 * A
    WhT = torch.zeros(H, P + 2)
    WhT[:, :P + 1] = torch.randn(H, P + 1, generator=g) * 0.2
    bh = torch.zeros(P + 2)
    bh[:P + 1] = torch.randn(P + 1, generator=g) * 0.1
    return dict(W1t=rnd(D, H, scale=D ** -0.5), b1=rnd(H, scale=0.1),
                W2t=rnd(H, H, scale=0.2), b2=rnd(H, scale=0.1),
                WhT=WhT.cuda().contiguous(), bh=bh.cuda().contiguous())


def guarded(rows, cols):
    """[rows][cols] view filled with NaN, followed by a sentinel guard."""
    n = rows * cols
    buf = torch.full((n + GUARD,), SENTINEL, device="cuda")
    buf[:n] = float("nan")
    view = buf.narrow(0, 0, n)
    return buf, (view.view(rows, cols) if cols > 1 else view)


def out_buffers(B, A):
    return {k: guarded(B, c) for k, c in
            (("h1", H), ("h2", H), ("pdflat", 2 * A), ("v", 1))}


def run_split(ext, X, w, act_code, out):
    h1, h2, pd, v = (out[k][1] for k in ("h1", "h2", "pdflat", "v"))
    ext.gemm_fwd(X, w["W1t"], w["b1"], act_code, 0, h1, h1, h1, 0, 0, 0)
    ext.gemm_fwd(h1, w["W2t"], w["b2"], act_code, 0, h2, h2, h2, 0, 0, 0)
    ext.gemm_fwd(h2, w["WhT"], w["bh"], 2, 2, pd, v, pd, 0, 0, 0)


def run_fused(ext, X, w, act_code, out, sample=None):
    h1, h2, pd, v = (out[k][1] for k in ("h1", "h2", "pdflat", "v"))
    e = torch.empty(0, device="cuda")
    s = sample or dict(actions=e, xva=e, seed=e, eps=e, step=0, va_off=0,
                       low=0.0, high=0.0)
    ext.mlp_fwd_fused(X, w["W1t"], w["b1"], w["W2t"], w["b2"], w["WhT"],
                      w["bh"], act_code, h1, h2, pd, v, s["actions"],
                      s["xva"], s["seed"], s["eps"], s["step"], s["va_off"],
                      s["low"], s["high"])


def check_outputs(ref, got):
    for k in ("h1", "h2", "pdflat", "v"):
        (rbuf, rview), (gbuf, gview) = ref[k], got[k]
        assert not torch.isnan(gview).any(), f"{k}: element not written"
        assert torch.equal(rview, gview), k
        assert bool((gbuf[-GUARD:] == SENTINEL).all()), f"{k}: guard touched"


@pytest.mark.parametrize("act_code", [1, 0], ids=["tanh", "relu"])
@pytest.mark.parametrize("A", [1, 17, 31])
@pytest.mark.parametrize("D", [376, 64, 20])
@pytest.mark.parametrize("B", [1, 127, 129, 3077])
def test_op_fused_bitwise_matches_three_gemm_fwd(B, D, A, act_code):
    """B = 3077 is 25 row blocks: every L1 phase of K = 376 (24 stages)
    and every L2 / heads phase occurs.  D = 20 exercises the K tail;
    A = 1 / 17 / 31 give heads widths 4 / 36 / 64."""
    ext = require_hip_ext()
    assert ext.mlp_fwd_fused_supported(D, H, H, A)
    w = weights(D, A)
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + D)
    X = torch.randn(B, D, generator=g).cuda().contiguous()
    ref, got = out_buffers(B, A), out_buffers(B, A)
    run_split(ext, X, w, act_code, ref)
    run_fused(ext, X, w, act_code, got)
    torch.cuda.synchronize()
    check_outputs(ref, got)


@pytest.mark.parametrize("eps", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("B,D,A", [(129, 376, 17), (3077, 64, 31),
                                   (127, 20, 1)])
def test_op_sampling_bitwise_matches_rollout_sample(B, D, A, eps):
    ext = require_hip_ext()
    w = weights(D, A, seed=1)
    g = torch.Generator(device="cpu").manual_seed(B + D + A)
    X = torch.randn(B, D, generator=g).cuda().contiguous()
    kw = ((VA_OFF + A + 3) // 4) * 4
    xva0 = torch.randn(B, kw, generator=g).cuda().contiguous()
    seed = torch.full((1,), 0x5EED1234, dtype=torch.int64, device="cuda")
    eps_dev = torch.full((1,), eps, device="cuda")
    step, low, high = 5, -0.4, 0.4

    ref = out_buffers(B, A)
    run_split(ext, X, w, 1, ref)
    ref_act_buf, ref_act = guarded(B, A)
    ref_xva = xva0.clone()
    ext.rollout_sample(ref["pdflat"][1], ref_act.view(B, A), ref_xva, seed,
                       eps_dev, step, VA_OFF, low, high)

    got = out_buffers(B, A)
    got_act_buf, got_act = guarded(B, A)
    got_xva = xva0.clone()
    run_fused(ext, X, w, 1, got, sample=dict(
        actions=got_act.view(B, A), xva=got_xva, seed=seed, eps=eps_dev,
        step=step, va_off=VA_OFF, low=low, high=high))
    torch.cuda.synchronize()

    check_outputs(ref, got)
    assert not torch.isnan(got_act).any()
    assert torch.equal(ref_act, got_act)
    assert bool((got_act_buf[-GUARD:] == SENTINEL).all())
    assert torch.equal(ref_xva[:, VA_OFF:VA_OFF + A],
                       got_xva[:, VA_OFF:VA_OFF + A])
    assert torch.equal(got_xva[:, VA_OFF:VA_OFF + A], got_act.view(B, A))
    assert torch.equal(got_xva[:, :VA_OFF], xva0[:, :VA_OFF])
    assert torch.equal(got_xva[:, VA_OFF + A:], xva0[:, VA_OFF + A:])
    if eps == 1.0:   # every action is the uniform draw
        assert bool(((got_act >= low) & (got_act <= high)).all())


def test_supported_shapes():
    ext = require_hip_ext()
    assert ext.mlp_fwd_fused_supported(376, 64, 64, 17)
    assert not ext.mlp_fwd_fused_supported(376, 32, 32, 17)   # hidden width
    assert not ext.mlp_fwd_fused_supported(376, 64, 64, 16)   # (2A+2) % 4
    assert not ext.mlp_fwd_fused_supported(378, 64, 64, 17)   # D % 4
    assert not ext.mlp_fwd_fused_supported(376, 64, 64, 33)   # 2A+2 > 64


def _engine_pair(monkeypatch, **kw):
    monkeypatch.setenv("DPPO_ROLLOUT_V3", "1")
    monkeypatch.setenv("DPPO_FWD_FUSED", "1")
    torch.manual_seed(0)
    on = make_engine(**kw)
    torch.manual_seed(0)
    off = make_engine(**kw)
    # batches this small take the single-kernel chunk step by default;
    # route the update through the per-layer GEMM path, as at scale, so
    # that _fused_forward (update steps 2..) is part of the comparison
    on.CHUNK_KERNEL_MAX_B = off.CHUNK_KERNEL_MAX_B = 0
    return on, off


def _compare_engines(monkeypatch, on, off):
    """Rollout, then two training rounds, knob 1 against knob 0."""
    monkeypatch.setenv("DPPO_FWD_FUSED", "1")
    b_on, _ = on.rollout_once()
    monkeypatch.setenv("DPPO_FWD_FUSED", "0")
    b_off, _ = off.rollout_once()
    s_on, s_off = v3_views(on), v3_views(off)
    assert torch.equal(b_on.states, b_off.states)
    assert torch.equal(b_on.actions, b_off.actions)
    assert torch.equal(b_on.oldflat, b_off.oldflat)
    assert torch.equal(s_on[3], s_off[3])     # values
    assert torch.equal(s_on[6], s_off[6])     # bootstrap value
    for _ in range(2):
        monkeypatch.setenv("DPPO_FWD_FUSED", "1")
        on.train_round()
        monkeypatch.setenv("DPPO_FWD_FUSED", "0")
        off.train_round()
    assert torch.equal(on.flat_pi.flat_param, off.flat_pi.flat_param)


@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
def test_engine_knob_on_bitwise_matches_knob_off(monkeypatch, graphs):
    """NUM_ENVS = 192 is not a multiple of the 128-row tile."""
    on, off = _engine_pair(monkeypatch, NUM_ENVS=192, MAX_EPOCH_STEPS=6,
                           SEED=17, USE_GRAPHS=graphs)
    _compare_engines(monkeypatch, on, off)
    if graphs:
        assert on._v3_graph is not None and off._v3_graph is not None
    used = getattr(on, "fwd_fused_launches", {})
    assert used.get("rollout", 0) >= 6 and used.get("boot", 0) >= 1
    assert used.get("update", 0) >= 1
    assert not getattr(off, "fwd_fused_launches", {})


def test_engine_ineligible_shape_falls_back(monkeypatch):
    """Hidden width 32 is not the fused kernel's: knob 1 stays on the
    split chain and matches knob 0."""
    on, off = _engine_pair(monkeypatch, NUM_ENVS=192, MAX_EPOCH_STEPS=6,
                           SEED=17, HIDDEN_SIZES=(32, 32))
    assert not on._fwd_fused()
    _compare_engines(monkeypatch, on, off)
    assert not getattr(on, "fwd_fused_launches", {})


def test_knob_rejects_unknown_value(monkeypatch):
    monkeypatch.setenv("DPPO_FWD_FUSED", "yes")
    eng = make_engine()
    with pytest.raises(ValueError, match="DPPO_FWD_FUSED"):
        eng._fwd_fused()
