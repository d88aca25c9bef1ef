"""A/B: the autograd update loop of Discrete / MultiDiscrete / MultiBinary
policies (DPPO_UPDATE_DISC=0, the path before the fused update existed) vs
the fused MFMA update (DPPO_UPDATE_DISC=1: gemm_fwd chain, disc_gh.hip loss
gradient, dgrad GEMMs, dw_mfma, device-state Adam, hipGraph-captured), and
the achieved bytes/s of the three gh kernels on their own.

One process: two engines of the same config, one batch collected once; both
arms run update() on that same batch.  Both arms are warmed up (the fused
arm's capture happens there), then alternated (REPEATS timed windows each, a
device synchronise before every clock read); the table reports each arm's
median window and its min..max spread, in ms per update() (UPDATE_STEPS
gradient steps).

Usage: python tools/update_disc_ab.py [E ...]        (default 128 4096 65536)
       python tools/update_disc_ab.py --gh [B ...]   (default 4194304)
"""
import os, statistics, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
from dppo_amd.config import DPPOConfig
from dppo_amd.ops import require_hip_ext
from dppo_amd.parallel.comm import Comm
from dppo_amd.trainer import DPPOEngine

T = 64
REPEATS = 3
SHAPES = [("CartPole-v0", (16,), "relu"), ("LunarLander-v2", (64, 64), "tanh"),
          ("MultiLever-v0", (32,), "tanh"), ("BitFlipper-v0", (64, 64), "tanh")]
ARMS = [("autograd", "0"), ("fused", "1")]
# gh kernels alone: label, binding, P, action columns, int64 actions, nvec
GH_CASES = [("Categorical K=2", "cat", 2, 1, True, None),
            ("Categorical K=4", "cat", 4, 1, True, None),
            ("MultiCategorical (3,3,4)", "mcat", 10, 3, True, [3, 3, 4]),
            ("Bernoulli n=8", "bern", 8, 8, False, None),
            ("Bernoulli n=64", "bern", 64, 64, False, None)]


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


def update_once(eng, batch, knob):
    os.environ["DPPO_UPDATE_DISC"] = knob
    eng.update(batch, 0.9)


def updates(sizes):
    print(f"# {torch.cuda.get_device_name(0)}; T={T}, {REPEATS} alternated "
          "windows per arm; ms per update() (UPDATE_STEPS=4 steps on the same "
          "batch): median [min..max]")
    for game, hidden, act in SHAPES:
        for E in sizes:
            cfg = DPPOConfig(GAME=game, HIDDEN_SIZES=hidden, ACTIVATION=act,
                             NUM_ENVS=E, MAX_EPOCH_STEPS=T, EPOCH_MAX=10**6,
                             STOP_EPOCH=10**6, NUM_WORKERS=1,
                             LOG_FILE_PATH="/tmp/l", DEVICE="cuda")
            engs = {name: DPPOEngine(cfg, comm=Comm(device="cuda:0"))
                    for name, _ in ARMS}
            os.environ["DPPO_UPDATE_DISC"] = "1"
            assert engs["fused"]._can_fuse_update()
            engs["fused"].sync_oldpi()
            batch = engs["fused"].collect()  # views of its persistent buffers
            times, n = alternate({
                name: (lambda e=engs[name], k=knob: update_once(e, batch, k))
                for name, knob in ARMS})
            graphed = engs["fused"]._upd_graph is not None
            med = {k: statistics.median(v) for k, v in times.items()}
            worst = min(a / f for a, f in zip(times["autograd"],
                                              times["fused"]))
            print(f"{game:15s} {str(hidden):9s} {act:4s} E={E:6d}  "
                  f"{row(times, n)}  "
                  f"autograd/fused {med['autograd']/med['fused']:6.2f}x "
                  f"(worst pair {worst:5.2f}x)  "
                  f"fused arm {'graphed' if graphed else 'UNGRAPHED'}",
                  flush=True)
            del engs, batch
            torch.cuda.empty_cache()


def gh_kernels(sizes):
    ext = require_hip_ext()
    print(f"# {torch.cuda.get_device_name(0)}; gh kernels alone, {REPEATS} "
          "windows; bytes = logits + oldpi logits + actions + 4 scalars read, "
          "gh written")
    for label, fam, P, W, i64, nvec in GH_CASES:
        for B in sizes:
            lpi = torch.randn(B, P, device="cuda")
            lold = lpi + 0.1 * torch.randn(B, P, device="cuda")
            v, oldv, adv, etr = (torch.randn(B, device="cuda")
                                 for _ in range(4))
            if fam == "cat":
                a = torch.randint(0, P, (B,), device="cuda")
            elif fam == "mcat":
                a = torch.stack([torch.randint(0, k, (B,), device="cuda")
                                 for k in nvec], dim=1).contiguous()
            else:
                a = torch.randint(0, 2, (B, P), device="cuda").float()
            cd = torch.empty(0, device="cuda")
            extra = (nvec,) if fam == "mcat" else ()
            fn = getattr(ext, f"ppo_loss_{fam}_gh")
            times, n = alternate({"gh": lambda: fn(
                lpi, lold, v, oldv, a, adv, etr, *extra, 0.2, 0.01, 0.5, cd)})
            ldgh = (P + 1 + 3) & ~3
            nbytes = B * (4 * (2 * P + 4 + ldgh) + W * (8 if i64 else 4))
            t = statistics.median(times["gh"])
            print(f"{label:25s} B={B:8d} tile={ext.ppo_gh_disc_tile(P, W):3d}  "
                  f"{row(times, n)}  {nbytes/t/1e12:5.2f} TB/s", flush=True)


if __name__ == "__main__":
    if sys.argv[1:2] == ["--gh"]:
        gh_kernels([int(a) for a in sys.argv[2:]] or [4194304])
    else:
        updates([int(a) for a in sys.argv[1:]] or [128, 4096, 65536])
