"""Env-step micro-bench: gemm_env_step + the x@V gemm_fwd of the states it
wrote (arm A, three launches) against env_step_rows (arm B, one launch), on
the flagship rollout shape.

Both arms are warmed, then alternated in one process and timed with hip
events; the figure is the median over --iters alternations, with min and
max.  Bitwise equality of every output is re-checked at the benchmarked
size.  sigma = 0.05 and 0 are both timed, so the Box-Muller share of the
epilogue stays visible.
    python tools/env_step_bench.py               # E = 262144
    python tools/env_step_bench.py --E 1048576
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
import torch

R = 16  # env rank


def bench_one(ext, E, D, A, iters, sigma):
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)

    def rn(*s, scale=1.0):
        return torch.randn(*s, device=dev, generator=g) * scale

    kw = ((R + A + 3) // 4) * 4
    xva0 = rn(E, kw)
    M = rn(kw, D, scale=0.2)
    xin = torch.tanh(rn(E, D))
    envd = rn(D, scale=0.5)
    V = rn(D, R, scale=0.1)
    horizons = torch.randint(3, 9, (E,), device=dev, generator=g,
                             dtype=torch.int32)
    t0 = (torch.randint(0, 1 << 20, (E,), device=dev, generator=g,
                        dtype=torch.int32) % (horizons - 1))
    t0[::3] = horizons[::3] - 1
    epr0 = rn(E)
    seed = torch.full((1,), 0x5EED1234, dtype=torch.int64, device=dev)
    empty = torch.empty(0, device=dev)
    bz = torch.zeros(R, device=dev)
    npan = (D + 63) // 64

    def state():
        return dict(xva=xva0.clone(), t=t0.clone(), epr=epr0.clone(),
                    xout=torch.empty(E, D, device=dev),
                    rewards=torch.empty(E, device=dev),
                    dones=torch.empty(E, device=dev))

    sa, sb = state(), state()
    rsum = torch.zeros(npan * E, device=dev)

    def reset(s):
        s["xva"].copy_(xva0)
        s["t"].copy_(t0)
        s["epr"].copy_(epr0)

    def arm_a():
        s = sa
        ext.gemm_env_step(s["xva"], M, xin, s["xout"], envd, horizons,
                          s["t"], s["epr"], s["rewards"], s["dones"], rsum,
                          seed, sigma, 3, empty, empty)
        ext.gemm_fwd(s["xout"], V, bz, 2, 0, s["xva"], s["xva"], s["xva"],
                     0, 0, kw)

    def arm_b():
        s = sb
        ext.env_step_rows(s["xva"], M, xin, s["xout"], envd, horizons,
                          s["t"], s["epr"], s["rewards"], s["dones"], seed,
                          sigma, 3, V)

    arms = {"env_step+xv": (arm_a, sa), "env_step_rows": (arm_b, sb)}
    for fn, _ in arms.values():
        for _ in range(3):
            fn()
    # equality from identical inputs (the timed calls below keep stepping
    # t / epr / xva, which is what a rollout does)
    for fn, s in arms.values():
        reset(s)
        fn()
    torch.cuda.synchronize()
    same = all(torch.equal(sa[k], sb[k]) for k in sa)
    times = {k: [] for k in arms}
    for _ in range(iters):
        for name, (fn, s) in arms.items():
            reset(s)
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    # bytes the step truly needs: read x, write x' (the concat buffer and
    # the per-env vectors are 3 % of that)
    need = 2 * E * D * 4
    for name in arms:
        med = statistics.median(times[name])
        print(f"  sigma={sigma:<4} {name:13s} E={E}: median {med:.3f} ms  "
              f"min {min(times[name]):.3f}  max {max(times[name]):.3f}"
              f"  ({need / med / 1e9:.2f} TB/s of needed bytes)"
              f"  bitwise_equal={same}")
    return same


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--E", type=int, nargs="*", default=[262144])
    ap.add_argument("--D", type=int, default=376)
    ap.add_argument("--A", type=int, default=17)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    from dppo_amd.ops import require_hip_ext

    ext = require_hip_ext()
    ok = True
    for E in args.E:
        print(f"E={E} D={args.D} A={args.A}")
        for sigma in (0.05, 0.0):
            ok &= bench_one(ext, E, args.D, args.A, args.iters, sigma)
    if not ok:
        raise SystemExit("env_step_rows is not bitwise equal to "
                         "gemm_env_step + gemm_fwd")


if __name__ == "__main__":
    main()
