"""A/B: eager physics rollout loop (DPPO_ROLLOUT_CLASSIC=0) vs the
lane-per-env classic-control rollout kernel (DPPO_ROLLOUT_CLASSIC=1).

Both arms are warmed up, then alternated in one process (REPEATS timed
windows each, a device synchronise before every clock read); the table
reports each arm's median window and its min..max spread.  Both arms include
GAE and the rollout's single host sync.

Usage: python tools/rollout_classic_ab.py [--games NAME,...] [E ...]
       (default: every game; E = 128 4096 65536)
"""
import os, statistics, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))))
from dppo_amd.config import DPPOConfig
from dppo_amd.parallel.comm import Comm
from dppo_amd.trainer import DPPOEngine

T = 64
REPEATS = 3
SHAPES = [("CartPole-v0", (16,), "relu"), ("CartPole-v0", (64, 64), "tanh"),
          ("Pendulum-v1", (16,), "relu"),
          ("Acrobot-v1", (16,), "relu"), ("Acrobot-v1", (64, 64), "tanh"),
          ("MountainCar-v0", (16,), "relu"),
          ("MountainCar-v0", (64, 64), "tanh"),
          ("MountainCarContinuous-v0", (16,), "relu")]
ARMS = [("eager", "0"), ("kernel", "1")]


def window(eng, knob, n):
    os.environ["DPPO_ROLLOUT_CLASSIC"] = knob
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        eng.rollout_once()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def main():
    argv = sys.argv[1:]
    games = None
    if argv and argv[0] == "--games":
        games, argv = argv[1].split(","), argv[2:]
    sizes = [int(a) for a in argv] or [128, 4096, 65536]
    print(f"# {torch.cuda.get_device_name(0)}; T={T}, {REPEATS} alternated "
          "windows per arm; ms per rollout_once(): median [min..max]")
    for game, hidden, act in SHAPES:
        if games is not None and game not in games:
            continue
        for E in sizes:
            cfg = DPPOConfig(GAME=game, ENV_DYNAMICS="physics",
                             HIDDEN_SIZES=hidden, ACTIVATION=act,
                             NUM_ENVS=E, MAX_EPOCH_STEPS=T, EPOCH_MAX=10**6,
                             STOP_EPOCH=10**6, NUM_WORKERS=1,
                             LOG_FILE_PATH="/tmp/l", DEVICE="cuda")
            engs = {name: DPPOEngine(cfg, comm=Comm(device="cuda:0"))
                    for name, _ in ARMS}
            assert engs["kernel"]._can_rollout_classic()
            n = {}
            for name, knob in ARMS:  # warm-up, then size the timed window
                window(engs[name], knob, 3)
                dt = window(engs[name], knob, 2)
                n[name] = max(3, min(200, int(0.25 / dt) + 1))
            assert engs["eager"].classic_rollout_launches == 0
            assert engs["kernel"].classic_rollout_launches == 5
            times = {name: [] for name, _ in ARMS}
            for _ in range(REPEATS):
                for name, knob in ARMS:
                    times[name].append(window(engs[name], knob, n[name]))
            med = {k: statistics.median(v) for k, v in times.items()}
            row = "  ".join(
                f"{k} {med[k]*1e3:8.3f} [{min(v)*1e3:8.3f}..{max(v)*1e3:8.3f}]"
                f" (n={n[k]})" for k, v in times.items())
            print(f"{game:12s} {str(hidden):9s} {act:4s} E={E:6d}  {row}  "
                  f"eager/kernel {med['eager']/med['kernel']:6.2f}x  "
                  f"kernel {E*T/med['kernel']/1e6:8.1f}M env-steps/s",
                  flush=True)
            del engs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
