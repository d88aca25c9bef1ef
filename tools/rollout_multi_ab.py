"""A/B: eager MultiDiscrete / MultiBinary rollout loop (DPPO_ROLLOUT_MULTI=0)
vs the fused MultiCategorical / Bernoulli whole-rollout kernels
(DPPO_ROLLOUT_MULTI=1), and the fused PPO loss of both families
(ops/hip/multi_loss.hip) vs the eager reference, forward + backward.

Both arms are warmed up, then alternated in one process (REPEATS timed
windows each, a device synchronise before every clock read); the tables
report each arm's median window and its min..max spread.

Usage: python tools/rollout_multi_ab.py [E ...]   (default 128 4096 65536)
       python tools/rollout_multi_ab.py --loss [B ...]  (default 65536 1048576)
"""
import os, statistics, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
from dppo_amd.config import DPPOConfig
from dppo_amd.distributions import BernoulliPdType, MultiCategoricalPdType
from dppo_amd.ops.ppo_loss import PPOLossCoeffs, ppo_losses, ppo_losses_ref
from dppo_amd.parallel.comm import Comm
from dppo_amd.trainer import DPPOEngine

T = 64
REPEATS = 3
SHAPES = [("MultiLever-v0", (32,), "tanh"), ("BitFlipper-v0", (64, 64), "tanh")]
ARMS = [("eager", "0"), ("fused", "1")]
LOSS_FAMILIES = [("MultiCategorical (3,3,4)", MultiCategoricalPdType((3, 3, 4))),
                 ("MultiCategorical (2,)*32", MultiCategoricalPdType((2,) * 32)),
                 ("Bernoulli n=8", BernoulliPdType(8)),
                 ("Bernoulli n=64", BernoulliPdType(64))]


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def alternate(fns):
    """{arm: per-call seconds of each of REPEATS alternated windows}, n."""
    n = {}
    for name, fn in fns.items():  # warm-up, then size the timed window
        timed(fn, 3)
        n[name] = max(3, min(200, int(0.25 / timed(fn, 2)) + 1))
    times = {name: [] for name in fns}
    for _ in range(REPEATS):
        for name, fn in fns.items():
            times[name].append(timed(fn, n[name]))
    return times, n


def row(times, n):
    return "  ".join(
        f"{k} {statistics.median(v)*1e3:8.3f} [{min(v)*1e3:8.3f}.."
        f"{max(v)*1e3:8.3f}] (n={n[k]})" for k, v in times.items())


def rollout_once(eng, knob):
    os.environ["DPPO_ROLLOUT_MULTI"] = knob
    eng.rollout_once()


def rollouts(sizes):
    print(f"# {torch.cuda.get_device_name(0)}; T={T}, {REPEATS} alternated "
          "windows per arm; ms per rollout_once(): median [min..max]")
    for game, hidden, act in SHAPES:
        for E in sizes:
            cfg = DPPOConfig(GAME=game, HIDDEN_SIZES=hidden, ACTIVATION=act,
                             NUM_ENVS=E, MAX_EPOCH_STEPS=T, EPOCH_MAX=10**6,
                             STOP_EPOCH=10**6, NUM_WORKERS=1,
                             LOG_FILE_PATH="/tmp/l", DEVICE="cuda")
            engs = {name: DPPOEngine(cfg, comm=Comm(device="cuda:0"))
                    for name, _ in ARMS}
            assert engs["fused"]._can_fuse_rollout_multi()
            times, n = alternate({
                name: (lambda e=engs[name], k=knob: rollout_once(e, k))
                for name, knob in ARMS})
            med = {k: statistics.median(v) for k, v in times.items()}
            print(f"{game:15s} {str(hidden):9s} {act:4s} E={E:6d}  "
                  f"{row(times, n)}  "
                  f"eager/fused {med['eager']/med['fused']:6.2f}x  "
                  f"fused {E*T/med['fused']/1e6:8.1f}M env-steps/s",
                  flush=True)
            del engs
            torch.cuda.empty_cache()


def losses(sizes):
    print(f"# {torch.cuda.get_device_name(0)}; PPO loss forward + backward, "
          f"{REPEATS} alternated windows per arm; ms: median [min..max]")
    coeffs = PPOLossCoeffs(0.2, 0.01, 0.5)
    for label, pdt in LOSS_FAMILIES:
        P = pdt.param_shape()[0]
        for B in sizes:
            lpi = torch.randn(B, P, device="cuda", requires_grad=True)
            lold = (lpi + 0.1 * torch.randn(B, P, device="cuda")).detach()
            v = torch.randn(B, device="cuda", requires_grad=True)
            oldv, adv, etr = (torch.randn(B, device="cuda") for _ in range(3))
            a = pdt.pdfromflat(lold).sample()

            def step(fn):
                lpi.grad = v.grad = None
                out = fn(pdt.pdfromflat(lpi), pdt.pdfromflat(lold), v, oldv,
                         a, adv, etr, coeffs)
                out["total_loss"].backward()

            times, n = alternate({
                "eager": lambda: step(ppo_losses_ref),
                "fused": lambda: step(
                    lambda *args: ppo_losses(*args, policy="always"))})
            med = {k: statistics.median(t) for k, t in times.items()}
            print(f"{label:25s} B={B:8d}  {row(times, n)}  "
                  f"eager/fused {med['eager']/med['fused']:6.2f}x", flush=True)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--loss"]:
        losses([int(a) for a in sys.argv[2:]] or [65536, 1048576])
    else:
        rollouts([int(a) for a in sys.argv[1:]] or [128, 4096, 65536])
