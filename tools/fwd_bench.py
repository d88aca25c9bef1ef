"""Policy-forward micro-bench: the split chain (three gemm_fwd calls, plus
rollout_sample in the sampling arm) against the fused mlp_fwd_fused kernel,
on the flagship layer shapes.

Per B both uses are timed: forward only (update forward, bootstrap value)
and forward + action sampling (a rollout step).  Arms are warmed, then
alternated in one process and timed with hip events; the figure is the
median over --iters alternations.
    python tools/fwd_bench.py                  # B = 262144, 1M and 16.8M
    python tools/fwd_bench.py --B 4194304
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
import torch

H = 64
VA_OFF = 16


def bench_one(ext, B, D, A, iters, act_code):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    P = 2 * A

    def rn(*s, scale=1.0):
        return torch.randn(*s, device=dev, generator=g) * scale

    X = rn(B, D)
    W1t, b1 = rn(D, H, scale=D ** -0.5), rn(H, scale=0.1)
    W2t, b2 = rn(H, H, scale=0.2), rn(H, scale=0.1)
    WhT = torch.zeros(H, P + 2, device=dev)
    WhT[:, :P + 1] = rn(H, P + 1, scale=0.2)
    bh = torch.zeros(P + 2, device=dev)
    bh[:P + 1] = rn(P + 1, scale=0.1)
    kw = ((VA_OFF + A + 3) // 4) * 4
    seed = torch.full((1,), 0x5EED1234, dtype=torch.int64, device=dev)
    eps = torch.full((1,), 0.1, device=dev)
    empty = torch.empty(0, device=dev)

    def outs():
        return dict(h1=torch.empty(B, H, device=dev),
                    h2=torch.empty(B, H, device=dev),
                    pd=torch.empty(B, P, device=dev),
                    v=torch.empty(B, device=dev),
                    act=torch.empty(B, A, device=dev),
                    xva=torch.zeros(B, kw, device=dev))

    oc, of = outs(), outs()

    def chain(sample):
        o = oc
        ext.gemm_fwd(X, W1t, b1, act_code, 0, o["h1"], o["h1"], o["h1"],
                     0, 0, 0)
        ext.gemm_fwd(o["h1"], W2t, b2, act_code, 0, o["h2"], o["h2"],
                     o["h2"], 0, 0, 0)
        ext.gemm_fwd(o["h2"], WhT, bh, 2, 2, o["pd"], o["v"], o["pd"],
                     0, 0, 0)
        if sample:
            ext.rollout_sample(o["pd"], o["act"], o["xva"], seed, eps, 3,
                               VA_OFF, -0.4, 0.4)

    def fused(sample):
        o = of
        ext.mlp_fwd_fused(X, W1t, b1, W2t, b2, WhT, bh, act_code, o["h1"],
                          o["h2"], o["pd"], o["v"],
                          o["act"] if sample else empty,
                          o["xva"] if sample else empty, seed, eps, 3,
                          VA_OFF, -0.4, 0.4)

    # bytes the forward truly needs: read X, write h1, h2, pdflat, v
    need = B * 4 * (D + 2 * H + P + 1)
    for sample in (False, True):
        arms = {"chain": chain, "fused": fused}
        for fn in arms.values():
            for _ in range(3):
                fn(sample)
        torch.cuda.synchronize()
        same = all(torch.equal(oc[k], of[k]) for k in
                   (("h1", "h2", "pd", "v") + (("act", "xva") if sample
                                               else ())))
        times = {k: [] for k in arms}
        for _ in range(iters):
            for name, fn in arms.items():
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(sample)
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
        use = "fwd+sample" if sample else "fwd only  "
        for name in arms:
            med = statistics.median(times[name])
            print(f"  {use} {name:5s} B={B}: median {med:.3f} ms  "
                  f"min {min(times[name]):.3f}  max {max(times[name]):.3f}"
                  f"  ({need / med / 1e9:.2f} TB/s of needed bytes)"
                  f"  bitwise_equal={same}")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="*",
                    default=[262144, 1 << 20, 16 * 1024 * 1024])
    ap.add_argument("--D", type=int, default=376)
    ap.add_argument("--A", type=int, default=17)
    ap.add_argument("--relu", action="store_true")
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    from dppo_amd.ops import require_hip_ext

    ext = require_hip_ext()
    for B in args.B:
        print(f"B={B} D={args.D} H={H} A={args.A}")
        bench_one(ext, B, args.D, args.A, args.iters, 0 if args.relu else 1)


if __name__ == "__main__":
    main()
