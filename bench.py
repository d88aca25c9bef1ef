"""Flagship benchmark: Humanoid-shaped MLP DPPO training throughput.

Measures the BASELINE.json headline metric — env-steps/sec (whole node)
for Humanoid-shaped (obs=376, act=17) MLP DPPO on synthetic data with
random-init weights — on N GPUs of one node (weak scaling: per-GPU work
fixed as N grows).

One bench "step" = one full DPPO training round: a rollout of T env
steps on each of E device-resident envs, the GAE scan + whitening, the
cross-rank stats all-gather (Chief semantics), and UPDATE_STEPS repeated
full-batch PPO updates with flat-bucket gradient all-reduce.  env-steps
counted = E * T per rank per step.

Usage:
    python bench.py --gpus N --steps K --warmup W
For N > 1 launch via:
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
        --master-addr 127.0.0.1 bench.py --gpus N --steps K --warmup W

A plain run does only what the headline figure needs: set up, warm up,
time the K steps, print one JSON result line.  Two options add to that:

  --dump-outputs DIR   after the timed steps, rank 0 writes what the last
                       timed round produced as DIR/<name>.npy, so two
                       builds can be compared output for output (inputs
                       are seeded: same arguments, same inputs):
                         stats.npy   float64 [len(STATS_KEYS)+1]: the
                                     round's stats in STATS_KEYS order,
                                     then the stop flag
                         params.npy  float32: flat policy parameters
                                     after the round's update
                         obs.npy     float32: env observations the round
                                     left behind (input of the next one)
                       Arrays above DUMP_MAX_ELEMS elements are written
                       as a fixed, seeded sample of their elements.
  --full               secondary measurements (anything beyond the
                       headline figure belongs behind this switch).  The
                       benchmark has none at present, so a --full run
                       equals a plain one.
"""

from __future__ import annotations

import argparse
import json
import os
import time

import numpy as np
import torch

from dppo_amd.config import DPPOConfig
from dppo_amd.parallel.comm import Comm
from dppo_amd.trainer import DPPOEngine

PRESETS = {
    # BASELINE.json config 3 (the headline): Humanoid-shaped MLP DPPO
    "humanoid": dict(
        GAME="Humanoid-v4", HIDDEN_SIZES=(64, 64), ACTIVATION="tanh",
        NUM_ENVS=262144, MAX_EPOCH_STEPS=64, DTYPE="float32",
        # 262144 envs/GPU: throughput-optimal batch on 288 GB HBM3E
        # (63 GB used; 65536 -> 69.5M, 131072 -> 71.3M, 262144 -> 73.6M
        # env-steps/s) — the per-step GEMM rollout and full-batch update
        # both gain from the larger B.
    ),
    # BASELINE.json config 2: HalfCheetah-shaped, 64 envs, 1 GPU
    "halfcheetah": dict(
        GAME="HalfCheetah-v4", HIDDEN_SIZES=(64, 64), ACTIVATION="tanh",
        NUM_ENVS=64, MAX_EPOCH_STEPS=100, DTYPE="float32",
    ),
    # BASELINE.json config 5: wide MFMA-bound MLP
    # BASELINE.json config 4: Humanoid-shaped large-batch — 65k-step
    # rollouts (GAE HIP scan stress) with 4096-sample minibatched updates
    "largebatch": dict(
        GAME="Humanoid-v4", HIDDEN_SIZES=(64, 64), ACTIVATION="tanh",
        NUM_ENVS=1024, MAX_EPOCH_STEPS=65536, MINIBATCH_SIZE=4096,
        DTYPE="float32",
        # E sweep (65536-step rollouts): 64 -> 1.23M, 128 -> 2.03M,
        # 256 -> 2.68M, 1024 -> 3.53M env-steps/s — the tiny-E rollout is
        # latency-bound, so batch amortizes it; beyond ~1024 the
        # minibatch chunk loop (~260 us/4096-sample update step)
        # dominates and the curve flattens.
    ),
    # BASELINE.json config 5: wide MFMA-bound MLP, bf16 compute (as named)
    "wide4096": dict(
        GAME="Wide-4096", HIDDEN_SIZES=(4096, 4096, 4096, 4096),
        ACTIVATION="tanh", NUM_ENVS=4096, MAX_EPOCH_STEPS=16,
        DTYPE="bfloat16",
        # 4096 envs: measured optimum (1024 -> 535K, 4096 -> 573K,
        # 8192 -> 534K, 16384 -> 559K env-steps/s with the bf16 rollout).
    ),
}

# order of the train_round() stats in stats.npy (the stop flag follows)
STATS_KEYS = (
    "l_mul", "best_rank", "score", "epr_max", "epr_mean",
    "policyLoss", "entropyLoss", "valueLoss", "total_loss",
)
# per-array cap for --dump-outputs: 3 arrays x 4M x 4 B = 48 MB at most
DUMP_MAX_ELEMS = 4 * 1024 * 1024
DUMP_SAMPLE_SEED = 20240229


def _dump_array(t: torch.Tensor) -> np.ndarray:
    """float32 host copy of `t`, flattened; above DUMP_MAX_ELEMS a fixed
    seeded sample of its elements (same indices for the same numel)."""
    flat = t.detach().reshape(-1)
    if flat.numel() > DUMP_MAX_ELEMS:
        g = torch.Generator().manual_seed(DUMP_SAMPLE_SEED)
        idx = torch.randint(flat.numel(), (DUMP_MAX_ELEMS,), generator=g)
        flat = flat[idx.sort().values.to(flat.device)]
    return flat.to(device="cpu", dtype=torch.float32).numpy()


def dump_outputs(out_dir: str, engine: DPPOEngine, stats, stop: bool) -> None:
    os.makedirs(out_dir, exist_ok=True)
    missing = set(stats) ^ set(STATS_KEYS)
    assert not missing, f"train_round() stats changed: {sorted(missing)}"
    row = [float(stats[k]) for k in STATS_KEYS] + [float(stop)]
    np.save(os.path.join(out_dir, "stats.npy"), np.asarray(row, np.float64))
    np.save(os.path.join(out_dir, "params.npy"),
            _dump_array(engine.flat_pi.flat_param))
    np.save(os.path.join(out_dir, "obs.npy"), _dump_array(engine.obs))


def main() -> None:
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--preset", type=str, default="humanoid", choices=sorted(PRESETS))
    p.add_argument("--num-envs", type=int, default=None)
    p.add_argument("--rollout", type=int, default=None)
    p.add_argument("--device", type=str, default=None)
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="write the last timed round's outputs as DIR/*.npy")
    p.add_argument("--full", action="store_true",
                   help="also run the secondary measurements (none today)")
    args = p.parse_args()
    if args.steps < 1:
        p.error("--steps must be >= 1")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    n_gpus = max(args.gpus, world)

    preset = dict(PRESETS[args.preset])
    if args.num_envs:
        preset["NUM_ENVS"] = args.num_envs
    if args.rollout:
        preset["MAX_EPOCH_STEPS"] = args.rollout
    cfg = DPPOConfig(
        **preset,
        EPOCH_MAX=1_000_000, STOP_EPOCH=1_000_000,
        LEARNING_RATE=3e-4,
        NUM_WORKERS=n_gpus,
        LOG_FILE_PATH="/tmp/dppo_bench_logs",
        SEED=1234,
        DEVICE=args.device or "auto",
    )

    comm = Comm(device=args.device)
    engine = DPPOEngine(cfg, comm=comm, scope=f"Worker_N{comm.rank}")
    on_gpu = comm.device.type == "cuda"

    def sync():
        comm.barrier()
        if on_gpu:
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        engine.train_round()

    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = engine.train_round()
    sync()
    elapsed = time.perf_counter() - t0

    # MAX over ranks
    e_t = torch.tensor([elapsed], device=comm.device, dtype=torch.float64)
    if comm.distributed:
        import torch.distributed as dist

        dist.all_reduce(e_t, op=dist.ReduceOp.MAX)
    elapsed = float(e_t)

    if args.dump_outputs and comm.rank == 0:
        dump_outputs(args.dump_outputs, engine, *last)

    E, T = cfg.NUM_ENVS, cfg.MAX_EPOCH_STEPS
    env_steps = E * T * args.steps * world
    value = env_steps / elapsed
    if comm.rank == 0:
        result = {
            "metric": "env-steps/sec (whole node), Humanoid-shaped MLP DPPO at 1/2/4/8 MI355X",
            "value": value,
            "unit": "env-steps/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1000.0,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": cfg.DTYPE.replace("float32", "fp32").replace("bfloat16", "bf16"),
            "data": "synthetic",
            "config": {
                "model": f"{cfg.GAME} MLP {'x'.join(str(h) for h in cfg.HIDDEN_SIZES)} {cfg.ACTIVATION}",
                "preset": args.preset,
                "global_batch": E * T * world,
                "num_envs_per_gpu": E,
                "rollout_T": T,
                "update_steps": cfg.UPDATE_STEPS,
                "parallelism": f"dp{world}",
            },
        }
        print(json.dumps(result))
    comm.shutdown()


if __name__ == "__main__":
    main()
