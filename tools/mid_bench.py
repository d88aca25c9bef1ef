"""Update-middle micro-bench: the per-layer backward chain (gh kernel, two
dgrad GEMMs, dW2 and heads dW with their reduces) against the fused
mlp_mid_bwd kernel, on the flagship layer shapes.

Both arms are warmed, then alternated in one process and timed with hip
events; the figure is the median over --iters alternations.
    python tools/mid_bench.py                  # B = 1M and 16.8M
    python tools/mid_bench.py --B 4194304
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
import torch


def bench_one(ext, B, H1, H2, A, iters, act_code):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    P = 2 * A

    def rn(*s, scale=1.0):
        return torch.randn(*s, device=dev, generator=g) * scale

    # flat params: W1 b1 W2 b2 Wv bv Wp bp (W1/b1 unused by either arm)
    sizes = [0, 0, H2 * H1, H2, H2, 1, P * H2, P]
    offsets, o = [], 0
    for s in sizes:
        offsets.append(o)
        o += s
    params = rn(o, scale=0.1)
    grad = torch.zeros(o, device=dev)
    W2 = params[offsets[2]:offsets[3]].view(H2, H1)
    Wv = params[offsets[4]:offsets[5]].view(1, H2)
    Wp = params[offsets[6]:offsets[7]].view(P, H2)
    h1 = torch.tanh(rn(B, H1))
    h2 = torch.tanh(rn(B, H2))
    pdflat = rn(B, P, scale=0.3)
    oldflat = pdflat + 0.05 * rn(B, P)
    v = rn(B)
    oldv = v + 0.1 * rn(B)
    act = rn(B, A)
    adv, etr = rn(B), rn(B)
    clip_dev = torch.empty(0, device=dev)
    ldp = (P + 1 + 3) & ~3
    Wh_pad = torch.zeros(ldp, H2, device=dev)
    Wh_pad[:P] = Wp
    Wh_pad[P] = Wv[0]
    dummy = torch.zeros(1, device=dev)
    dz2 = torch.empty_like(h2)
    dz1 = torch.empty_like(h1)
    dcode = 3 if act_code == 1 else 4

    def chain():
        gh = ext.ppo_loss_gauss_gh(pdflat, oldflat, v, oldv, act, adv, etr,
                                   0.2, 0.01, 0.5, clip_dev)
        ext.gemm_fwd(gh, Wh_pad, dummy, dcode, 0, dz2, dz2, h2, 0, 0, 0)
        ext.gemm_fwd(dz2, W2, dummy, dcode, 0, dz1, dz1, h1, 0, 0, 0)
        ext.dw_mfma(dz2, h1, grad, offsets[2], offsets[3], -1, -1, -1, 0)
        ext.dw_mfma(gh, h2, grad, offsets[6], offsets[7], P, offsets[4],
                    offsets[5], 0)

    def mid():
        ext.mlp_mid_bwd(params, offsets, h1, h2, pdflat, v, oldflat, oldv,
                        act, adv, etr, act_code, clip_dev, 0.2, 0.01, 0.5,
                        dz1, grad)

    arms = {"chain": chain, "mid_load": mid}
    check = {}
    for name, fn in arms.items():
        for _ in range(3):
            grad.zero_()
            fn()
        check[name] = (grad.clone(), dz1.clone())
    torch.cuda.synchronize()
    gs = float(check["chain"][0].abs().max())
    ds = float(check["chain"][1].abs().max())
    print(f"  agreement: grad max|diff|/max|ref| "
          f"{float((check['chain'][0] - check['mid_load'][0]).abs().max()) / gs:.2e}"
          f", dz1 {float((check['chain'][1] - check['mid_load'][1]).abs().max()) / ds:.2e}")

    times = {k: [] for k in arms}
    for _ in range(iters):
        for name, fn in arms.items():
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    # bytes the middle truly needs (LOAD mode also reads h2, pdflat, v)
    need = B * 4 * (H1 + H2 + 2 * P + A + 5 + H1)
    for name in arms:
        med = statistics.median(times[name])
        print(f"  {name:9s} B={B}: median {med:.3f} ms  "
              f"min {min(times[name]):.3f}  max {max(times[name]):.3f}"
              + (f"  ({need / med / 1e9:.2f} TB/s of LOAD-mode bytes)"
                 if name != "chain" else ""))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="*",
                    default=[1 << 20, 16 * 1024 * 1024])
    ap.add_argument("--H1", type=int, default=64)
    ap.add_argument("--H2", type=int, default=64)
    ap.add_argument("--A", type=int, default=17)
    ap.add_argument("--relu", action="store_true")
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    from dppo_amd.ops import hip_ext

    ext = hip_ext()
    for B in args.B:
        print(f"B={B} H1={args.H1} H2={args.H2} A={args.A}")
        bench_one(ext, B, args.H1, args.H2, args.A, args.iters,
                  0 if args.relu else 1)


if __name__ == "__main__":
    main()
