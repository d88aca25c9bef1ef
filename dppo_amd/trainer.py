"""The per-rank DPPO training engine.

Implements the reference's intended Chief/Worker round protocol
 in the MI355X-native shape: one process per GPU,
each rank = one reference "Worker" with a batch of E synthetic envs;
rank 0 carries the Chief's bookkeeping; cross-rank coordination is
RCCL collectives instead of Events/deques.

One training round (reference Chief.check + Worker.work):
  1. oldpi <- pi            (sync_pis at round start; PPO.py:47, Worker.py:42)
  2. rollout MAX_EPOCH_STEPS env steps per env, with the epsilon-greedy
     exploration overlay and its linear anneal (Worker.py:140-153);
     repeat (discarding, like the partial-buffer discard rule
     Worker.py:43-47) until >=1 episode completed (push guard
     Worker.py:135), up to MAX_ROLLOUT_RETRIES.
  3. host GAE -> device GAE scan: advantages, returns, whitening
     (Worker.py:82-92; HIP segmented scan on GPU).
  4. evaluate the 4 losses pre-update for the logs vector (Worker.py:117-118)
     and build logs = [score, epr_min, epr_max, epr_mean, policyLoss,
     valueLoss, entropyLoss, totalLoss, CUR_EP] (Worker.py:123-133).
  5. all_gather [logs(9), cur_lr, valid] across ranks; the best valid
     rank by logs[2] (max episode reward — the Chief's sort key,
     Chief.py:51) supplies l_mul for everyone (Chief.py:58-63) and the
     stop decision (CUR_EP >= STOP_EPOCH, Chief.py:85-87).
  6. UPDATE_STEPS repeated full-batch updates on the SAME data
     (Chief.py:64): fwd/bwd -> flat-bucket all_reduce(AVG)
     (PPO.py:55-65 analog) -> Adam with lr = LEARNING_RATE * l_mul and
     clip = CLIP_PARAM * l_mul (PPO.py:19-20).
  7. periodic rank-0 param broadcast as drift guard (replaces the
     per-round assign broadcast Chief.py:67-70 — replicas are already
     bit-identical under all-reduced grads + identical Adam state).

A rank with no completed episode still participates in every collective
(validity flag; SURVEY.md §7 "hard parts" last bullet) so the ring never
deadlocks.
"""

from __future__ import annotations

import contextlib
import dataclasses
import math
import os
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

from .config import DPPOConfig, game_spaces
from .envs.synthetic import BatchedSyntheticEnv, make_env
from .models.mlp import PolicyValueMLP  # noqa: F401 (public engine surface)
from .ops import gae_advantages, ppo_losses, PPOLossCoeffs
from .ops.rollout_blob import rollout_blob
from .parallel.comm import Comm, FlatBuffers
from .utils.graphs import warm_and_capture
from .utils.logging import ScalarLogger
from .utils.timers import PhaseTimers
from . import spaces

STATS_DIM = 11  # logs[9] + cur_lr + valid

# RolloutBatch's per-sample tensors (leading dim T*E)
_SAMPLE_FIELDS = ("states", "actions", "adv", "etr", "oldflat", "oldv")


@dataclass
class RolloutBatch:
    states: torch.Tensor      # [T*E, obs]
    actions: torch.Tensor     # [T*E] long or [T*E, A] float
    adv: torch.Tensor         # [T*E] whitened
    etr: torch.Tensor         # [T*E]
    oldflat: torch.Tensor     # [T*E, P] pi's pd-params recorded at rollout
                              # time == oldpi outputs (oldpi==pi during the
                              # rollout, PPO.py:47 sync at round start), so
                              # the update path never re-runs oldpi.
    oldv: torch.Tensor        # [T*E] values recorded at rollout time
    cur_lr: float
    # Episode-reward moments, accumulated on-device during the rollout so
    # the hot loop never syncs to host (the reference's per-step python
    # bookkeeping, Worker.py:57-65, becomes masked tensor ops):
    ep_count: torch.Tensor    # scalar
    ep_sum: torch.Tensor
    ep_sumsq: torch.Tensor
    ep_min: torch.Tensor
    ep_max: torch.Tensor
    valid: bool

    def narrow(self, o: int, n: int) -> "RolloutBatch":
        """Rows [o, o+n) of the per-sample tensors (views); the scalars
        and episode moments are shared."""
        return dataclasses.replace(self, **{
            f: getattr(self, f).narrow(0, o, n) for f in _SAMPLE_FIELDS})


class DPPOEngine:
    def __init__(
        self,
        cfg: DPPOConfig,
        comm: Optional[Comm] = None,
        scope: str = "Worker",
        seed_offset: int = 0,
    ):
        self.cfg = cfg
        self.comm = comm if comm is not None else Comm()
        self.scope = scope
        self.device = self.comm.device
        # Rollout/batch buffers stay fp32 regardless of DTYPE;
        # DTYPE='bfloat16' switches the update-path GEMM compute to bf16
        # autocast (BASELINE config 5) with fp32 loss math.
        self.dtype = torch.float32

        # Lazily created state, declared here with its "unset" value:
        self._warned = set()            # _warn_once keys already printed
        self._wide_path = None          # WideBF16Path (ops/wide.py)
        self._sample_ctr = 0            # cat/mcat/bern_sample RNG counter
        self._rollout_counter = 0       # rollout seed counter
        # persistent rollout / GAE outputs (stable addresses for capture)
        self._rollout_out = self._adv_buf = self._etr_buf = None
        self._mw = None                 # staged MFMA weight operands
        self._wh_pad_staged = False     # last staging filled Wh_pad
        self._v3 = self._v3_key = None  # v3 rollout buffers
        self._v3_graph = self._v3_moments = None
        self._v3_graph_failed = False
        self._v3_acts_valid = False     # v3 rollout recorded activations
        self._wr = self._wr_key = None  # wide graphed rollout buffers
        self._wr_graph = None           # False once its capture failed
        self._wide_rollout_h_valid = False
        self._fwd_fused_cache = self._mid_mode_cache = None
        self.fwd_fused_launches = {}    # mlp_fwd_fused launches per use
        self.env_rows_launches = 0      # env_step_rows launches
        self.classic_rollout_launches = 0  # classic_rollout_* launches
        # real dynamics (envs/classic.py) instead of the synthetic env
        self._physics = cfg.ENV_DYNAMICS == "physics"
        self._clip_dev = None           # device clip for captured updates
        self._upd_graph = self._upd_graph_skip = None
        self._graph_failed = False
        self._mb_graphs = self._mb_key = None
        self._mb_graph_failed = False
        self._chunk_slabs = None        # chunk kernel gradient scratch

        obs_space, act_space = game_spaces(cfg.GAME)
        self.obs_space, self.act_space = obs_space, act_space
        # action-space family (make_pdtype dispatch, reference
        # distributions.py:231-243): all four are trainable end-to-end
        if isinstance(act_space, spaces.Discrete):
            self._act_kind = "discrete"
        elif isinstance(act_space, spaces.MultiDiscrete):
            self._act_kind = "multidiscrete"
        elif isinstance(act_space, spaces.MultiBinary):
            self._act_kind = "multibinary"
        else:
            self._act_kind = "box"
        self._discrete = self._act_kind == "discrete"

        seed = cfg.SEED + 1000 * (self.comm.rank + seed_offset)
        torch.manual_seed(seed)

        def build_net() -> PolicyValueMLP:
            return PolicyValueMLP(
                obs_dim=obs_space.shape[0],
                action_space=act_space,
                hidden_sizes=cfg.HIDDEN_SIZES,
                activation=cfg.ACTIVATION,
                init_std=cfg.INIT_STD,
            ).to(self.device)

        # pi / oldpi two-network scheme (PPO.py:21-22)
        self.pi = build_net()
        self.oldpi = build_net()
        self.flat_pi = FlatBuffers(self.pi)
        self.flat_old = FlatBuffers(self.oldpi)
        # initial broadcast: chief(rank0) pi AND oldpi -> everyone (main.py:48-50)
        self.comm.broadcast_(self.flat_pi.flat_param, src=0)
        self.sync_oldpi()

        # Adam moments live on every rank but stay identical (SURVEY.md §2.3
        # "parameter broadcast" row) — the reference keeps them only on the
        # Chief (PPO.py:20,53); replicated-but-identical is the DP-native form.
        # GPU: fused flat Adam HIP kernel (K10); CPU/'never': torch Adam.
        from .ops import use_hip

        if use_hip(self.device, cfg.USE_HIP_KERNELS):
            from .ops.adam import FusedFlatAdam

            self.optimizer = FusedFlatAdam(
                self.flat_pi.flat_param, self.flat_pi.flat_grad,
                lr=cfg.LEARNING_RATE,
            )
        else:
            self.optimizer = torch.optim.Adam(
                [self.flat_pi.flat_param], lr=cfg.LEARNING_RATE
            )

        self.env: BatchedSyntheticEnv = make_env(cfg, str(self.device), seed + 17)
        self.obs = self.env.reset()
        self.epr = torch.zeros(cfg.NUM_ENVS, device=self.device, dtype=torch.float32)

        self.CUR_EP = 0
        # DPPO_TIMER_SYNC=1 makes per-phase wall times attribute async GPU
        # work correctly (adds a device sync per phase boundary; off for
        # production — rocprof profiles are the ground truth either way).
        self.timers = PhaseTimers(
            cuda_sync=os.environ.get("DPPO_TIMER_SYNC", "0") == "1")
        self.logger = ScalarLogger(
            cfg.LOG_FILE_PATH, enabled=(self.comm.rank == 0), name=f"{scope}_rank0"
        )
        self._round = 0

    # ------------------------------------------------------------------
    def _warn_once(self, key: str, msg: str) -> None:
        """Rank-0 one-shot warning (graph-capture fallbacks etc. must not
        silently de-optimize production runs — VERDICT r01 weak #5)."""
        if key in self._warned:
            return
        self._warned.add(key)
        if self.comm.rank == 0:
            print(f"[dppo_amd] WARNING: {msg}", flush=True)

    @torch.no_grad()
    def sync_oldpi(self) -> None:
        """oldpi <- pi, one flat copy (sync_pis, PPO.py:47)."""
        self.flat_old.flat_param.copy_(self.flat_pi.flat_param)
        if self._wide_path is not None:
            # params may have changed since the last rollout (update,
            # drift-guard broadcast, checkpoint restore) — refresh the
            # bf16 weight copies once per round
            self._wide_path.mark_dirty()

    def _hip_path(self, act_kind: str, dtype: str = "float32") -> bool:
        """HIP kernels in use, this action family, this DTYPE: what the
        eligibility of every hand-written path opens with."""
        from .ops import use_hip

        c = self.cfg
        return (self._act_kind == act_kind and c.DTYPE == dtype
                and use_hip(self.device, c.USE_HIP_KERNELS))

    @property
    def _act_code(self) -> int:
        """Activation code of the HIP kernels: 1 tanh, 0 relu."""
        return 1 if self.cfg.ACTIVATION == "tanh" else 0

    # -- wide bf16 path (BASELINE #5) ----------------------------------
    def _can_wide_bf16(self) -> bool:
        """Eligibility for the hand-written bf16 MFMA path (ops/wide.py +
        ops/hip/bf16_gemm.hip): wide tanh MLP, Box policy, bf16 compute,
        dims in 256-multiples (the 256^2-tile GEMM's shape contract)."""
        c = self.cfg
        if os.environ.get("DPPO_WIDE") == "0":  # A/B: autocast/rocBLAS path
            return False
        if c.ACTIVATION != "tanh" or c.MINIBATCH_SIZE != 0:
            return False
        if not self._hip_path("box", "bfloat16"):
            return False
        H = c.HIDDEN_SIZES
        if self.obs_space.shape[0] % 256 or any(h % 256 for h in H):
            return False
        if len(set(H)) != 1 or c.NUM_ENVS % 256:
            return False
        return True

    def _wide(self):
        if self._wide_path is None:
            from .ops.wide import WideBF16Path

            self._wide_path = WideBF16Path(self)
        return self._wide_path

    def _policy_forward(self, obs: torch.Tensor):
        """(v, pdflat) f32 for a batch of states — hand bf16 kernels on
        the wide config, autocast/eager otherwise."""
        if self._can_wide_bf16() and obs.shape[0] % 256 == 0:
            return self._wide().forward(obs)
        with self._amp():
            v, pdflat = self.pi(obs)
        return v.float(), pdflat.float()

    def exploration_rate(self) -> float:
        """Linear epsilon anneal MAX->MIN over AC_EXP_PERCENTAGE*EPOCH_MAX
        epochs (Worker.py:140-144)."""
        c = self.cfg
        ac_exp_epoch = c.AC_EXP_PERCENTAGE * c.EPOCH_MAX
        if self.CUR_EP >= ac_exp_epoch:
            return c.MIN_AC_EXP_RATE
        return c.MAX_AC_EXP_RATE + self.CUR_EP * (
            c.MIN_AC_EXP_RATE - c.MAX_AC_EXP_RATE
        ) / ac_exp_epoch

    def current_lr_mul(self) -> float:
        """LR/clip anneal multiplier (Worker.py:77-80)."""
        c = self.cfg
        if c.SCHEDULE == "constant":
            return 1.0
        return max(1.0 - float(self.CUR_EP) / c.EPOCH_MAX, 0.0)

    # ------------------------------------------------------------------
    def _random_actions(self, n: int) -> torch.Tensor:
        """Uniform random actions for the epsilon-greedy overlay
        (Worker.py:149-152; extended to Box spaces: uniform in [low, high])."""
        if self._act_kind == "discrete":
            return torch.randint(
                self.act_space.n, (n,), device=self.device, dtype=torch.long
            )
        if self._act_kind == "multidiscrete":
            return torch.stack(
                [torch.randint(int(k), (n,), device=self.device,
                               dtype=torch.long)
                 for k in self.act_space.nvec], dim=-1)
        if self._act_kind == "multibinary":
            return torch.randint(
                2, (n, self.act_space.n), device=self.device
            ).to(self.dtype)
        low = float(self.act_space.low.flat[0])
        high = float(self.act_space.high.flat[0])
        a_dim = self.act_space.shape[0]
        return low + (high - low) * torch.rand(
            n, a_dim, device=self.device, dtype=self.dtype
        )

    def _amp(self):
        """bf16 autocast context for network forwards (BASELINE config 5:
        DTYPE='bfloat16' runs every GEMM — rollout acting, bootstrap value
        and update-path — in bf16 with fp32 loss/distribution math)."""
        if self.cfg.DTYPE == "bfloat16" and self.device.type == "cuda":
            return torch.autocast("cuda", dtype=torch.bfloat16)
        return contextlib.nullcontext()

    @torch.no_grad()
    def act_batch(self, obs: torch.Tensor, eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
        """Sample actions + values for a batch of states, with the
        epsilon-greedy overlay.  The old-policy logp of explored actions is
        NOT recorded — the ratio re-evaluates oldpi on the batch later,
        exactly the reference's formulation (Worker.py:149-152 + PPO.py:31;
        SURVEY.md §7 'hard parts')."""
        from .ops import use_hip

        v, pdflat = self._policy_forward(obs)
        pd = self.pi.pdtype.pdfromflat(pdflat)
        kind = self._act_kind
        if (((kind in ("discrete", "multidiscrete")
              and pdflat.shape[-1] <= 64) or kind == "multibinary")
                and use_hip(self.device, self.cfg.USE_HIP_KERNELS)):
            # fused sample kernels (cat_loss.hip: Gumbel-max; multi_loss.hip:
            # Gumbel-max per component, Bernoulli) — counter-based RNG, one
            # launch, no torch RNG round trips
            from .ops import hip_ext

            self._sample_ctr += 1
            seed = (self.cfg.SEED * 1_000_003
                    + self.comm.rank * 7_919) & 0x7FFFFFFF
            if kind == "discrete":
                a = hip_ext().cat_sample(pdflat, seed, self._sample_ctr)
            elif kind == "multidiscrete":
                a = hip_ext().mcat_sample(
                    pdflat, self._nvec, seed, self._sample_ctr)
            else:
                a = hip_ext().bern_sample(pdflat, seed, self._sample_ctr)
        else:
            a = pd.sample()
        if eps > 0.0:
            E = obs.shape[0]
            explore = torch.rand(E, device=self.device) < eps
            rand_a = self._random_actions(E)
            if self._discrete:
                a = torch.where(explore, rand_a, a)
            else:
                a = torch.where(explore.unsqueeze(-1), rand_a, a)
        return a, v, pdflat

    @staticmethod
    def _env_switch(name: str, default: bool) -> bool:
        """An on/off DPPO_* knob: '0' is off, any other value on, unset the
        (measured) default."""
        ov = os.environ.get(name)
        return default if ov is None else ov != "0"

    def _fits_rollout_kernel(self) -> bool:
        """The family-independent limits of rollout.hip's kernel on the
        synthetic env: 1-3 hidden layers of width <= 128, obs <= 512, env
        rank <= 32."""
        H = self.cfg.HIDDEN_SIZES
        return (1 <= len(H) <= 3 and max(H) <= 128
                and self.obs_space.shape[0] <= 512
                and self.env.Vt.size(0) <= 32)

    def _can_fuse_rollout(self) -> bool:
        """Eligibility for the fused HIP rollout kernel (rollout.hip):
        Box/DiagGaussian policy, dims within kernel limits, fp32, GPU."""
        if self._physics or not self._hip_path("box"):
            return False
        return self._fits_rollout_kernel() and self.act_space.shape[0] <= 32

    @torch.no_grad()
    def rollout_once(self) -> Tuple[RolloutBatch, Dict[str, float]]:
        if self._use_rollout_classic():
            return self._rollout_once_hip_classic()
        if self._can_rollout_v3():
            return self._rollout_once_hip_v3()
        if self._can_fuse_rollout():
            return self._rollout_once_hip()
        if self._use_rollout_cat():
            return self._rollout_once_hip_cat()
        if self._use_rollout_multi():
            return self._rollout_once_hip_multi()
        return self._rollout_once_eager()

    def _can_fuse_rollout_cat(self) -> bool:
        """Eligibility for the Categorical instantiation of the fused HIP
        rollout kernel (rollout.hip, rollout_run_cat): Discrete policy,
        dims within kernel limits, fp32, GPU.  Separate from
        _can_fuse_rollout(), which also gates the Box-only v3 rollout and
        graphed update."""
        if self._physics or not self._hip_path("discrete"):
            return False
        return self._fits_rollout_kernel() and 2 <= self.act_space.n <= 64

    def _use_rollout_cat(self) -> bool:
        """Dispatch for Discrete games: DPPO_ROLLOUT_CAT=0 forces the eager
        loop, =1 the fused kernel wherever eligible."""
        if not self._can_fuse_rollout_cat():
            return False
        # measured, T=64 (tools/rollout_cat_ab.py, profiles/r04_rollout_cat.txt):
        # CartPole (16,) eager 27.3 / 26.6 / 26.4 ms vs fused 0.42 / 0.94 /
        # 7.09 ms at E = 128 / 4096 / 65536; LunarLander (64,64) eager 27.7 /
        # 28.0 / 27.8 ms vs fused 0.54 / 1.22 / 9.78 ms; repeat spread < 1 %
        # on the fused arm.  No crossover in the measured range -> on
        # wherever eligible.
        return self._env_switch("DPPO_ROLLOUT_CAT", True)

    @property
    def _nvec(self):
        """Component sizes of a MultiDiscrete action space."""
        return [int(n) for n in self.act_space.nvec]

    def _can_fuse_rollout_multi(self) -> bool:
        """Eligibility for the MultiCategorical / Bernoulli instantiations of
        the fused HIP rollout kernel (rollout.hip, rollout_run_mcat /
        rollout_run_bern): MultiDiscrete with every n_c >= 2 and
        sum(nvec) <= 64, or MultiBinary with n <= 32; dims within kernel
        limits, fp32, GPU.  Its own function: _can_fuse_rollout_cat() stays
        False for these games."""
        if self._physics or not (self._hip_path("multidiscrete")
                                 or self._hip_path("multibinary")):
            return False
        if not self._fits_rollout_kernel():
            return False
        if self._act_kind == "multidiscrete":
            nvec = self._nvec
            return (1 <= len(nvec) <= 32 and min(nvec) >= 2
                    and sum(nvec) <= 64)
        return 1 <= self.act_space.n <= 32

    def _use_rollout_multi(self) -> bool:
        """Dispatch for MultiDiscrete / MultiBinary games:
        DPPO_ROLLOUT_MULTI=0 forces the eager loop, any other value the
        fused kernel wherever eligible."""
        if not self._can_fuse_rollout_multi():
            return False
        # measured, T=64 (tools/rollout_multi_ab.py,
        # profiles/r10_rollout_multi.txt): MultiLever (32,) eager 32.8 / 34.7 /
        # 31.9 ms vs fused 0.50 / 1.10 / 8.56 ms at E = 128 / 4096 / 65536;
        # BitFlipper (64,64) eager 30.1 / 30.4 / 32.5 ms vs fused 0.53 / 1.25 /
        # 9.92 ms; the widest min..max spread is 6.6 ms (eager) and 0.04 ms
        # (fused).  No crossover in the measured range -> on wherever
        # eligible.
        return self._env_switch("DPPO_ROLLOUT_MULTI", True)

    def _can_rollout_v3(self) -> bool:
        """Per-step GEMM rollout (v3): the T-step loop runs as pipelined
        MFMA GEMMs (MLP forward + env dynamics as [E][rank+A] @ [.][D])
        plus two small kernels (sampling, env finish).  Wins over the
        fused whole-rollout kernel at large E, where the VALU trunk/env
        phases bound it; the fused kernel keeps small-E latency."""
        if not self._can_fuse_rollout():
            return False
        if self.obs_space.shape[0] % 4 != 0:  # pipelined-GEMM staging
            return False
        # measured crossover: fused 6.8 vs v3 9.1 ms at E=16384, fused
        # 13.0 vs v3 10.3 ms at E=32768 (tools/rollout_v3_ab.py)
        return self._env_switch("DPPO_ROLLOUT_V3",
                                self.cfg.NUM_ENVS >= 32768)

    def _can_rollout_classic(self) -> bool:
        """Eligibility for the lane-per-env physics rollout
        (ops/hip/classic_rollout.hip): a physics env, fp32, GPU, and the
        kernel's trunk limits (1-2 hidden layers of width <= 64, which the
        bindings check too)."""
        H = self.cfg.HIDDEN_SIZES
        return (self._physics and self._hip_path(self._act_kind)
                and 1 <= len(H) <= 2 and max(H) <= 64)

    def _use_rollout_classic(self) -> bool:
        """Dispatch for physics envs: DPPO_ROLLOUT_CLASSIC=0 forces the
        eager loop, any other value the kernel wherever eligible."""
        if not self._can_rollout_classic():
            return False
        # measured, T=64, ms per rollout_once() (tools/rollout_classic_ab.py,
        # profiles/r12_rollout_classic.txt): CartPole (16,) eager 34.7 / 35.0 /
        # 34.6 vs kernel 0.22 / 0.23 / 0.31 at E = 128 / 4096 / 65536;
        # CartPole (64,64) 36.9 / 37.9 / 40.2 vs 1.32 / 1.34 / 1.97; Pendulum
        # (16,) 36.1 / 33.2 / 32.9 vs 0.20 / 0.21 / 0.28.  The kernel wins
        # every alternated pair (20x at the least; widest min..max spread
        # 3.9 ms eager, 0.004 ms kernel).  No crossover in the measured
        # range -> on wherever eligible.  (Measured with the moments still
        # taken by ep_moments_kernel after the rollout; the in-kernel fold
        # that replaced it drops two launches and is not re-measured.)
        # Acrobot (profiles/r13_rollout_acrobot.txt, same tool, CartPole
        # alternated in the same process): (16,) eager 88.7 / 85.7 / 76.0 vs
        # kernel 0.33 / 0.34 / 0.43; (64,64) 89.1 / 77.8 / 76.7 vs 1.61 /
        # 1.62 / 2.22.  The kernel wins every alternated pair (34x at the
        # least; widest spread 12.2 ms eager, 0.006 ms kernel) -> on wherever
        # eligible.  RK4 costs 0.11-0.18 ms per rollout over CartPole's Euler
        # step at the same shapes (0.19 / 0.19 / 0.24 and 1.48 / 1.51 / 2.03).
        # The MountainCars (profiles/r14_rollout_mountaincar.txt, same tool,
        # CartPole alternated in the same process): MountainCar-v0 (16,)
        # eager 29.2 / 29.4 / 29.1 vs kernel 0.16 / 0.17 / 0.21; (64,64)
        # 30.7 / 31.2 / 34.0 vs 1.35 / 1.37 / 1.89; MountainCarContinuous-v0
        # (16,) 31.9 / 32.0 / 31.6 vs 0.15 / 0.16 / 0.20.  The kernel wins
        # every alternated pair (18x at the least; widest spread 3.6 ms
        # eager, 0.005 ms kernel) -> on wherever eligible.  Both are faster
        # than CartPole at the same trunk and E in that run (0.18 / 0.20 /
        # 0.25 and 1.49 / 1.51 / 2.03), by more than either spread: one cosf
        # and no division per step, 2 inputs to layer 1 instead of 4.
        # classic_rollout_kernel<FAM, ENV, NH> for gfx950 (FAM 0 Box / 1
        # Categorical, ENV 0 CartPole / 1 Pendulum / 2 Acrobot / 3
        # MountainCar / 4 MountainCarContinuous, NH hidden layers), no VGPR
        # spills, scratch 0 in all ten (<1,0,2> keeps 8 SGPRs in VGPR
        # lanes):
        #   <1,0,1> VGPR  65 SGPR  91 LDS   592 B at (16,)    occ 7
        #   <1,0,2> VGPR 115 SGPR 106 LDS 35344 B at (64,64)  occ 4 (LDS: 1)
        #   <0,1,1> VGPR  65 SGPR  81 LDS   528 B at (16,)    occ 7
        #   <0,1,2> VGPR 120 SGPR 100 LDS 35088 B at (64,64)  occ 4 (LDS: 1)
        #   <1,2,1> VGPR  74 SGPR  91 LDS   720 B at (16,)    occ 6
        #   <1,2,2> VGPR 118 SGPR 104 LDS 35856 B at (64,64)  occ 4 (LDS: 1)
        #   <1,3,1> VGPR  62 SGPR  78 LDS   464 B at (16,)    occ 8
        #   <1,3,2> VGPR 115 SGPR  99 LDS 34832 B at (64,64)  occ 4 (LDS: 1)
        #   <0,4,1> VGPR  65 SGPR  83 LDS   464 B at (16,)    occ 7
        #   <0,4,2> VGPR 118 SGPR 104 LDS 34832 B at (64,64)  occ 4 (LDS: 1)
        return self._env_switch("DPPO_ROLLOUT_CLASSIC", True)

    @torch.no_grad()
    def _rollout_once_hip_classic(self) -> Tuple[RolloutBatch, Dict[str, float]]:
        """Physics rollout in a single launch, one lane per env
        (classic_rollout.hip): policy forward + sampling + epsilon overlay +
        CartPole / Pendulum / Acrobot / MountainCar / MountainCarContinuous
        step + episode bookkeeping and resets for all T steps, into the out
        blob layouts of rollout_run_cat (K = the game's action count: 2 or
        3) / rollout_run (A = 1).  The env is chosen by env.ENV_ID inside the
        family's binding."""
        return self._rollout_once_fused(
            "discrete" if self._discrete else "box", physics=True)

    @torch.no_grad()
    def _rollout_weight_blob(self):
        """Rollout weight blob: TRANSPOSED layer weights (Wt[in][out]) +
        biases + Wv[H] + Wpt[H][2A], so the rollout kernel's per-k W reads
        are coalesced.  Weights are frozen for the whole rollout; the
        transposes are a few tiny kernels per round."""
        c = self.cfg
        dims = [self.obs_space.shape[0], *c.HIDDEN_SIZES]
        parts, offsets, off = [], [], 0

        def push(t):
            nonlocal off
            flat = t.reshape(-1)
            parts.append(flat)
            offsets.append(off)
            off += flat.numel()

        for lay in self.pi.hidden:
            push(lay.weight.t().contiguous())     # Wt [in][out]
            push(lay.bias)
        push(self.pi.vf.weight.reshape(-1))       # Wv [H]
        push(self.pi.vf.bias)
        push(self.pi.pi.weight.t().contiguous())  # Wpt [H][2A]
        push(self.pi.pi.bias)
        return torch.cat(parts), offsets, dims

    @torch.no_grad()
    def _rollout_once_hip(self) -> Tuple[RolloutBatch, Dict[str, float]]:
        """One rollout iteration in a single fused kernel launch
        (ops/hip/rollout.hip): MLP forward + sampling + epsilon-greedy +
        env dynamics + episode bookkeeping for all T steps."""
        return self._rollout_once_fused("box")

    @torch.no_grad()
    def _rollout_once_hip_cat(self) -> Tuple[RolloutBatch, Dict[str, float]]:
        """Discrete-policy rollout in a single fused kernel launch (the
        Categorical instantiation of rollout.hip): MLP forward + Gumbel-max
        sampling + epsilon-greedy + env dynamics + episode bookkeeping for
        all T steps; int64 action indices come straight from the kernel."""
        return self._rollout_once_fused("discrete")

    @torch.no_grad()
    def _rollout_once_hip_multi(self) -> Tuple[RolloutBatch, Dict[str, float]]:
        """MultiDiscrete / MultiBinary rollout in a single fused kernel
        launch (the MultiCategorical / Bernoulli instantiations of
        rollout.hip): per-component Gumbel-max or Bernoulli sampling, the
        per-env epsilon overlay, a_in = sum_c B[off_c + a_c] or act @ B;
        int64 [C] or float 0/1 [n] actions come straight from the kernel."""
        return self._rollout_once_fused(self._act_kind)

    def _next_rollout_seed(self) -> int:
        """Seed of the next HIP rollout: SEED, rank and a per-engine
        rollout counter, which this bumps."""
        self._rollout_counter += 1
        return (
            self.cfg.SEED * 1_000_003
            + self.comm.rank * 7_919
            + self._rollout_counter * 104_729
        ) & 0x7FFFFFFFFFFFFFFF

    def _rollout_outputs(self, n_out: int) -> torch.Tensor:
        """Persistent rollout output blob of n_out floats (and the GAE
        outputs next to it): stable addresses let the update phase be
        hipGraph-captured once and replayed every round."""
        if self._rollout_out is None or self._rollout_out.numel() != n_out:
            B = self.cfg.MAX_EPOCH_STEPS * self.cfg.NUM_ENVS
            self._rollout_out = torch.empty(n_out, device=self.device)
            self._adv_buf = torch.empty(B, device=self.device)
            self._etr_buf = torch.empty(B, device=self.device)
        return self._rollout_out

    def _act_bounds(self) -> Tuple[float, float]:
        return (float(self.act_space.low.flat[0]),
                float(self.act_space.high.flat[0]))

    # policy kind -> (synthetic-env binding, physics-env binding, n_act of the
    # action space as the bindings take it, whether they take action bounds)
    _ROLLOUT_KINDS = {
        "discrete": ("rollout_run_cat", "classic_rollout_cat",
                     lambda sp: sp.n, False),
        "multidiscrete": ("rollout_run_mcat", None,
                          lambda sp: [int(n) for n in sp.nvec], False),
        "multibinary": ("rollout_run_bern", None, lambda sp: sp.n, False),
        "box": ("rollout_run", "classic_rollout_box",
                lambda sp: sp.shape[0], True),
    }

    def _rollout_once_fused(self, kind: str, physics: bool = False):
        """The single-launch rollout of one policy family (`kind`, an
        _act_kind): Categorical, MultiCategorical, Bernoulli or DiagGaussian,
        which also takes the action bounds; on the synthetic env
        (rollout.hip) or, with `physics`, a classic-control one
        (classic_rollout.hip).  The persistent out blob is sized by
        ops/rollout_blob.py exactly as the bindings size theirs."""
        from .ops import hip_ext

        c, E = self.cfg, self.cfg.NUM_ENVS
        T = c.MAX_EPOCH_STEPS
        eps = self.exploration_rate()
        env = self.env
        seed = self._next_rollout_seed()
        blob, offsets, dims = self._rollout_weight_blob()
        synthetic, classic, n_act_of, bounded = self._ROLLOUT_KINDS[kind]
        run = getattr(hip_ext(), classic if physics else synthetic)
        n_act = n_act_of(self.act_space)
        bounds = self._act_bounds() if bounded else ()
        out = self._rollout_outputs(
            rollout_blob(kind, T, E, self.obs_space.shape[0], n_act).numel)
        self._v3_acts_valid = False  # these kernels do not record acts
        if physics:
            self._wide_rollout_h_valid = False
            env_args, ablate = (env.ENV_ID, env.s, env.time_limit), ()
        else:
            env_args = (env.blob, env.rank_eff, env.horizons_i32,
                        float(env.NOISE))
            ablate = (0,)
        views = run(
            blob, offsets, dims, self._act_code, *env_args, *bounds,
            float(eps), env.x, env.t, self.epr, T, n_act, seed, out, *ablate,
        )
        if physics:
            self.classic_rollout_launches += 1
        self.obs = env.x  # updated in place by the kernel
        return self._finish_hip_rollout(*views, eps)

    def _finish_hip_rollout(self, states, pdflats, actions, values, rewards,
                            dones, boot_v, moments, eps):
        c = self.cfg
        adv, etr = gae_advantages(
            rewards, values, dones, boot_v,
            c.GAMMA, c.LAM, whiten=True, eps=c.ADV_EPS,
            policy=c.USE_HIP_KERNELS,
            adv_out=self._adv_buf, etr_out=self._etr_buf,
        )
        return self._make_batch(
            states, actions, adv, etr, pdflats, values, moments, eps)

    def _make_batch(self, states, actions, adv, etr, pdflats, values,
                    moments, eps):
        """(RolloutBatch, info) from the rollout's (T, E, ...) tensors and
        its five episode-reward moments."""
        B = states.shape[0] * states.shape[1]
        batch = RolloutBatch(
            states=states.reshape(B, states.shape[2]),
            # [T*E, A] float/int64 vectors or [T*E] int64 (Discrete)
            actions=actions.reshape(B, *actions.shape[2:]),
            adv=adv.reshape(B),
            etr=etr.reshape(B),
            oldflat=pdflats.reshape(B, pdflats.shape[2]),
            oldv=values.reshape(B),
            cur_lr=self.current_lr_mul(),
            ep_count=moments[0], ep_sum=moments[1], ep_sumsq=moments[2],
            ep_min=moments[3], ep_max=moments[4],
            valid=float(moments[0]) > 0,  # the rollout's single host sync
        )
        return batch, {"exploration_rate": eps}

    def _episode_moments(self, moments, r, done, donef) -> None:
        """Episode-reward bookkeeping for one env step (Worker.py:57-65),
        device-side and in place (capture-safe, no host round trip): adds
        the step rewards to epr, folds the episodes that just ended (`done`,
        `donef` its float form) into the five moments (count, sum, sum of
        squares, min, max) and resets their epr."""
        ep_count, ep_sum, ep_sumsq, ep_min, ep_max = moments
        epr = self.epr
        epr += r.float()
        ep_count += donef.sum()
        ep_sum += (epr * donef).sum()
        ep_sumsq += (epr.square() * donef).sum()
        ep_min.copy_(torch.minimum(ep_min, torch.where(
            done, epr, torch.full_like(epr, math.inf)).min()))
        ep_max.copy_(torch.maximum(ep_max, torch.where(
            done, epr, torch.full_like(epr, -math.inf)).max()))
        epr *= 1.0 - donef

    def _heads_pad(self) -> bool:
        """Padded transposed heads [H][P+2] (v at column P, a zero-weight
        pad column after it): N = P+2 a multiple of 4 routes the heads GEMM
        through the glds kernel (wt_layout 0, heads mode 2) instead of the
        pipe kernel; DPPO_HEADS_PAD=0 keeps the pipe kernel."""
        P = self.pi.pdtype.param_shape()[0]
        return (P + 2) % 4 == 0 and os.environ.get("DPPO_HEADS_PAD") != "0"

    @torch.no_grad()
    def _stage_weights(self, fwd: bool = True, dgrad: bool = False) -> dict:
        """Stage the current parameters into the persistent operand
        buffers of the MFMA kernels (copy_ only: capture-safe; the zero
        padding is written once, at allocation).  `fwd`: the forward's
        operands — transposed hidden weights `wt` and the heads, which
        `heads_pad` says are the padded and transposed `whT_pad`/`bh_pad`
        (see _heads_pad) or else the concatenated [Wp; Wv] `wh`/`bh`.
        `dgrad`: `Wh_pad`, [Wp; Wv] row-padded to gh's float4 row stride
        (zero rows: the gh pad columns multiply them and contribute
        nothing), for the per-layer backward."""
        pi = self.pi
        P, HL = pi.pi.weight.shape
        if self._mw is None:
            dev = self.device
            self._mw = dict(
                wt=[torch.empty(lay.weight.shape[1], lay.weight.shape[0],
                                device=dev) for lay in pi.hidden],
                wh=torch.empty(P + 1, HL, device=dev),
                bh=torch.empty(P + 1, device=dev),
                whT_pad=torch.zeros(HL, P + 2, device=dev),
                bh_pad=torch.zeros(P + 2, device=dev),
                Wh_pad=torch.zeros((P + 1 + 3) & ~3, HL, device=dev),
                heads_pad=False,
            )
        mw = self._mw
        heads = ((pi.pi.weight, pi.pi.bias, slice(0, P)),
                 (pi.vf.weight, pi.vf.bias, slice(P, P + 1)))
        if fwd:
            # hidden weights go in PRE-TRANSPOSED ([in][out], wt_layout 0):
            # layout-0 staging measured -16% on the big-K layer vs staging
            # the torch [out][in] layout transposed in LDS
            for wt, lay in zip(mw["wt"], pi.hidden):
                wt.copy_(lay.weight.t())
            mw["heads_pad"] = self._heads_pad()
            if mw["heads_pad"]:
                for w, b, rows in heads:
                    mw["whT_pad"][:, rows].copy_(w.t())
                    mw["bh_pad"][rows].copy_(b)
            else:
                for w, b, rows in heads:
                    mw["wh"][rows].copy_(w)
                    mw["bh"][rows].copy_(b)
        if dgrad:
            for w, _, rows in heads:
                mw["Wh_pad"][rows].copy_(w)
        self._wh_pad_staged = dgrad
        return mw

    def _v3_buffers(self):
        """Persistent device buffers for the per-step GEMM rollout."""
        c, env = self.cfg, self.env
        E, T = c.NUM_ENVS, c.MAX_EPOCH_STEPS
        D = self.obs_space.shape[0]
        A = self.act_space.shape[0]
        P = 2 * A
        H = tuple(c.HIDDEN_SIZES)
        key = (E, T, D, A, H)
        if self._v3_key == key:
            return self._v3
        dev = self.device
        r = env.rank_eff
        kw = ((r + A + 3) // 4) * 4  # concat width, padded for the GEMM
        M = torch.zeros(kw, D, device=dev)
        M[:r] = env.U
        M[r:r + A] = env.B
        B = int(E) * T
        self._v3 = dict(
            xva=torch.zeros(E, kw, device=dev), va_off=r, kw=kw,
            M=M.contiguous(), V=env.V.contiguous(),
            G=torch.empty(E, D, device=dev),
            h=[torch.empty(E, hh, device=dev) for hh in H],
            bz_r=torch.zeros(r, device=dev),
            bz_D=torch.zeros(D, device=dev),
            pd_scratch=torch.empty(E, P, device=dev),
            seed_dev=torch.zeros(1, dtype=torch.int64, device=dev),
            eps_dev=torch.zeros(1, dtype=torch.float32, device=dev),
            epr_before=torch.empty(E, device=dev),
            rsum=torch.zeros(((D + 63) // 64) * E, device=dev),
            # per-panel next-state @ V partials of the x@V fold (the fold
            # kernel is written for rank 16; other ranks keep the GEMM)
            xvp=(torch.empty(((D + 63) // 64) * E * 16, device=dev)
                 if r == 16 else None),
            empty=torch.empty(0, device=dev),
            # whole-batch activation blob in the update path's acts layout
            # ([B*H1 | B*H2 | ...]): the rollout's layer GEMMs write here
            # (same bytes they wrote to scratch before), and update step 1
            # reuses them — its forward runs on the SAME parameters
            acts=torch.empty(sum(B * hh for hh in H), device=dev),
        )
        self._v3_key = key
        return self._v3

    @staticmethod
    def _env_fused() -> bool:
        """Env transition in the G-GEMM epilogue (default);
        DPPO_ENV_FUSED=0 restores the split G-GEMM + env_finish path."""
        return os.environ.get("DPPO_ENV_FUSED", "1") != "0"

    @staticmethod
    def _xv_fold() -> bool:
        """DPPO_XV_FOLD=1: the fused env epilogue also computes the next
        step's x@V from the state tile it just finished (needs the fused
        env path).  Measured +2% at the flagship, but the reassociated
        x@V perturbs the states themselves, and after two training rounds
        the parameters sit further from the split path's than the accepted
        reward-reassociation noise (profiles/r03_rollout_env_fused.txt) —
        opt-in."""
        return os.environ.get("DPPO_XV_FOLD", "0") == "1"

    # the DPPO_ENV_ROWS default: what profiles/r09_env_rows.txt measured
    ENV_ROWS_DEFAULT = "1"

    def _env_rows(self) -> bool:
        """DPPO_ENV_ROWS=0|1: '1' runs the env step as one env_step_rows
        launch per step (one block owns all column panels of its rows: no
        rsum / env_finish2, and the next step's x@V comes out of the same
        launch in gemm_fwd's k order) where the fused env path is on, the
        fold is not selected, the env rank is 16 and D % 4 == 0; '0' keeps
        gemm_env_step + the per-step x@V gemm_fwd.  Both give bitwise-equal
        results.  Anything else is an error, not a fall-back."""
        mode = os.environ.get("DPPO_ENV_ROWS", self.ENV_ROWS_DEFAULT)
        if mode not in ("0", "1"):
            raise ValueError(f"DPPO_ENV_ROWS={mode!r}: expected '0' or '1'")
        return (mode == "1" and self._env_fused() and not self._xv_fold()
                and self.env.rank_eff == 16
                and self.obs_space.shape[0] % 4 == 0)

    # the DPPO_FWD_FUSED default: what profiles/r06_fwd_fused.txt measured
    FWD_FUSED_DEFAULT = "1"

    def _fwd_fused(self) -> bool:
        """DPPO_FWD_FUSED=0|1: '1' runs the policy forward (L1, L2, heads
        and, in the rollout, action sampling) as one mlp_fwd_fused launch
        where the shape is eligible; '0' keeps one gemm_fwd per layer plus
        rollout_sample.  Both give bitwise-equal results.  Anything else is
        an error, not a fall-back.  Resolved once per engine and value of
        the variables it depends on."""
        key = tuple(os.environ.get(k) for k in (
            "DPPO_FWD_FUSED", "DPPO_HEADS_PAD", "DPPO_GEMM_GLDS"))
        cached = self._fwd_fused_cache
        if cached is not None and cached[0] == key:
            return cached[1]
        on = self._resolve_fwd_fused(
            key[0] if key[0] is not None else self.FWD_FUSED_DEFAULT)
        self._fwd_fused_cache = (key, on)
        return on

    def _resolve_fwd_fused(self, mode: str) -> bool:
        from .ops import hip_ext

        if mode not in ("0", "1"):
            raise ValueError(f"DPPO_FWD_FUSED={mode!r}: expected '0' or '1'")
        if mode == "0":
            return False
        c = self.cfg
        if not self._hip_path("box"):
            return False
        if c.ACTIVATION not in ("tanh", "relu"):
            return False
        # the fused kernel reproduces the order of the default split chain
        # (padded heads on the glds kernel); with either switched off the
        # split chain accumulates in another order, so stay on it
        if (os.environ.get("DPPO_HEADS_PAD") == "0"
                or os.environ.get("DPPO_GEMM_GLDS", "1") == "0"):
            return False
        hs = tuple(c.HIDDEN_SIZES)
        return len(hs) == 2 and bool(hip_ext().mlp_fwd_fused_supported(
            self.obs_space.shape[0], hs[0], hs[1], self.act_space.shape[0]))

    def _count_fwd_fused(self, use: str) -> None:
        """Launch counter per use ('rollout', 'boot', 'update'): lets tests
        assert which path ran."""
        cnt = self.fwd_fused_launches
        cnt[use] = cnt.get(use, 0) + 1

    def _acts_views(self, acts: torch.Tensor, B: int):
        """Per-layer [B, H_l] views of an activation blob laid out
        [B*H1 | B*H2 | ...] (what mlp_bwd_rows and the dW GEMMs read)."""
        views, off = [], 0
        for hh in self.cfg.HIDDEN_SIZES:
            views.append(acts.narrow(0, off, B * hh).view(B, hh))
            off += B * hh
        return views

    def _v3_body(self, states, pdflats, actions, values, rewards, dones,
                 boot_v):
        """Capture-safe per-step rollout pipeline.  RNG slots match the
        fused rollout_kernel exactly (same actions/noise/resets per seed);
        seed/eps are read from device scalars."""
        from .ops import hip_ext

        ext = hip_ext()
        c, env, v3 = self.cfg, self.env, self._v3
        E, T = c.NUM_ENVS, c.MAX_EPOCH_STEPS
        act_code = self._act_code
        low, high = self._act_bounds()
        n_h = len(c.HIDDEN_SIZES)
        mw = self._stage_weights()
        wts, wh, bh = mw["wt"], mw["wh"], mw["bh"]
        whT_pad, bh_pad = mw["whT_pad"], mw["bh_pad"]
        heads_pad = mw["heads_pad"]
        v3["epr_before"].copy_(self.epr)
        states[0].reshape(-1).copy_(env.x.reshape(-1))
        # whole-batch activation views in the update acts-blob layout;
        # rollout step st writes rows [st*E, (st+1)*E) of each layer
        acts_views = self._acts_views(v3["acts"], T * E)
        fused = self._env_fused()
        rows = self._env_rows()
        fold = fused and self._xv_fold() and v3["xvp"] is not None
        no_fold = (v3["empty"], v3["empty"])
        # one launch for L1 + L2 + heads + sampling (bitwise equal to the
        # per-layer chain + rollout_sample; see mlp_fwd_fused_kernel)
        fwd_fused = heads_pad and self._fwd_fused()
        hb = [lay.bias.detach() for lay in self.pi.hidden]
        for st in range(T):
            xin = states[st]
            h = xin
            if fwd_fused:
                ext.mlp_fwd_fused(
                    xin, wts[0], hb[0], wts[1], hb[1], whT_pad, bh_pad,
                    act_code, acts_views[0].narrow(0, st * E, E),
                    acts_views[1].narrow(0, st * E, E), pdflats[st],
                    values[st], actions[st], v3["xva"], v3["seed_dev"],
                    v3["eps_dev"], st, v3["va_off"], low, high)
                self._count_fwd_fused("rollout")
            else:
                for l in range(n_h):
                    hl = acts_views[l].narrow(0, st * E, E)
                    ext.gemm_fwd(h, wts[l], hb[l], act_code, 0,
                                 hl, hl, hl, 0, 0, 0)
                    h = hl
                if heads_pad:
                    ext.gemm_fwd(h, whT_pad, bh_pad, 2, 2, pdflats[st],
                                 values[st], pdflats[st], 0, 0, 0)
                else:
                    ext.gemm_fwd(h, wh, bh, 2, 1, pdflats[st], values[st],
                                 pdflats[st], 1, 0, 0)
            # XV = x @ V into the concat buffer's first rank columns; with
            # env_step_rows or the fold, step st-1's env step already left
            # it there
            if not (fold or rows) or st == 0:
                ext.gemm_fwd(xin, v3["V"], v3["bz_r"], 2, 0, v3["xva"],
                             v3["xva"], v3["xva"], 0, 0, v3["kw"])
            if not fwd_fused:
                ext.rollout_sample(pdflats[st], actions[st], v3["xva"],
                                   v3["seed_dev"], v3["eps_dev"], st,
                                   v3["va_off"], low, high)
            # the env transition reads states[st] and writes states[st+1]
            # directly (policy input already comes from the blob) — env.x
            # only receives the FINAL state, for the bootstrap forward and
            # the next round's states[0]: one [E][D] stream per step, no
            # mirror write
            xout = states[st + 1] if st + 1 < T else env.x
            if rows:
                # the fused env step below and step st+1's x@V in one launch
                # (bitwise equal to that pair; see env_step_rows_kernel)
                ext.env_step_rows(v3["xva"], v3["M"], xin, xout, env.d,
                                  env.horizons_i32, env.t, self.epr,
                                  rewards[st], dones[st], v3["seed_dev"],
                                  float(env.NOISE), st, v3["V"])
                self.env_rows_launches += 1
            elif fused:
                # G = [XV|act] @ [U;B] with the env transition fused into
                # the GEMM epilogue: the accumulators are repacked through
                # LDS into env_finish's float4 layout (same math, RNG slots
                # and per-element work; states bitwise equal to the split
                # path), so the [E][D] G write + read never happen.  With
                # the fold the same epilogue also leaves the next step's
                # x@V in xva.
                ext.gemm_env_step(v3["xva"], v3["M"], xin, xout, env.d,
                                  env.horizons_i32, env.t, self.epr,
                                  rewards[st], dones[st], v3["rsum"],
                                  v3["seed_dev"], float(env.NOISE), st,
                                  *((v3["V"], v3["xvp"]) if fold
                                    else no_fold))
            else:
                ext.gemm_fwd(v3["xva"], v3["M"], v3["bz_D"], 2, 0, v3["G"],
                             v3["G"], v3["G"], 0, 0, 0)
                ext.rollout_env_step(xin, xout, v3["G"], env.d,
                                     env.horizons_i32, env.t, self.epr,
                                     rewards[st], dones[st], v3["seed_dev"],
                                     float(env.NOISE), st)
        # bootstrap value V(x_T)
        h = env.x
        if fwd_fused:
            ext.mlp_fwd_fused(
                h, wts[0], hb[0], wts[1], hb[1], whT_pad, bh_pad,
                act_code, v3["h"][0], v3["h"][1], v3["pd_scratch"], boot_v,
                v3["empty"], v3["empty"], v3["seed_dev"], v3["eps_dev"], 0,
                0, 0.0, 0.0)
            self._count_fwd_fused("boot")
            return ext.rollout_moments(rewards, dones, v3["epr_before"], T, E)
        for l in range(n_h):
            hl = v3["h"][l]
            ext.gemm_fwd(h, wts[l], hb[l], act_code, 0,
                         hl, hl, hl, 0, 0, 0)
            h = hl
        if heads_pad:
            ext.gemm_fwd(h, whT_pad, bh_pad, 2, 2, v3["pd_scratch"],
                         boot_v, v3["pd_scratch"], 0, 0, 0)
        else:
            ext.gemm_fwd(h, wh, bh, 2, 1, v3["pd_scratch"], boot_v,
                         v3["pd_scratch"], 1, 0, 0)
        return ext.rollout_moments(rewards, dones, v3["epr_before"], T, E)

    @torch.no_grad()
    def _rollout_once_hip_v3(self) -> Tuple[RolloutBatch, Dict[str, float]]:
        """Per-step GEMM rollout (see _can_rollout_v3), hipGraph-captured
        after warmup so replay costs one launch."""
        c, E = self.cfg, self.cfg.NUM_ENVS
        T = c.MAX_EPOCH_STEPS
        eps = self.exploration_rate()
        env = self.env
        seed = self._next_rollout_seed()
        lay = rollout_blob("box", T, E, self.obs_space.shape[0],
                           self.act_space.shape[0])
        (states, pdflats, actions, values, rewards, dones, boot_v,
         _) = lay.views(self._rollout_outputs(lay.numel))
        v3 = self._v3_buffers()
        v3["seed_dev"].fill_(seed & 0xFFFFFFFF)
        v3["eps_dev"].fill_(float(eps))
        args = (states, pdflats, actions, values, rewards, dones, boot_v)
        # unlike the update graph, the rollout graph contains NO
        # collectives — capture is safe on every rank
        graph_ok = c.USE_GRAPHS
        if not graph_ok or self._v3_graph_failed:
            moments = self._v3_body(*args)
        elif self._v3_graph is None:
            def capture_body():
                self._v3_moments = self._v3_body(*args)

            try:
                # the warmup runs the rollout for real: env/episode state
                # is restored so capture replays from the true start
                (self._v3_graph,) = warm_and_capture(
                    (env.x, env.t, self.epr),
                    lambda: self._v3_body(*args), [capture_body])
                self._v3_graph.replay()
                moments = self._v3_moments
            except Exception as exc:  # noqa: BLE001 — capture support varies
                self._warn_once(
                    "v3_graph",
                    f"rollout hipGraph capture failed ({exc!r}); "
                    "falling back to eager per-step launches",
                )
                self._v3_graph_failed = True
                self._v3_graph = None
                moments = self._v3_body(*args)
        else:
            self._v3_graph.replay()
            moments = self._v3_moments
        # step-1 of the update can reuse the recorded activations (same
        # parameters; cleared by the other rollout paths and by curation)
        self._v3_acts_valid = True
        self.obs = env.x
        return self._finish_hip_rollout(
            states, pdflats, actions, values, rewards, dones, boot_v,
            moments, eps)

    # -- wide bf16 graphed rollout -------------------------------------
    def _wide_rollout_buffers(self):
        c = self.cfg
        T, E = c.MAX_EPOCH_STEPS, c.NUM_ENVS
        D = self.obs_space.shape[0]
        A = self.act_space.shape[0]
        P = self.pi.pdtype.param_shape()[0]
        key = (T, E, D, A)
        if self._wr_key == key:
            return self._wr
        dev = self.device
        self._wr = dict(
            states=torch.empty(T, E, D, device=dev),
            pdflats=torch.empty(T, E, P, device=dev),
            actions=torch.empty(T, E, A, device=dev),
            rewards=torch.empty(T, E, device=dev),
            dones=torch.empty(T, E, device=dev),
            values=torch.empty(T, E, device=dev),
            boot_v=torch.empty(E, device=dev),
            x_env=torch.empty(E, D, device=dev),
            t_env=torch.zeros(E, device=dev, dtype=self.env.t.dtype),
            eps_moments=[torch.zeros((), device=dev) for _ in range(5)],
            eps_dev=torch.zeros((), device=dev),
        )
        self._wr_key = key
        self._wr_graph = None
        return self._wr

    @torch.no_grad()
    def _wide_rollout_body(self, b) -> None:
        """Capture-safe wide rollout: T env steps with the hand bf16
        forward, env dynamics and episode bookkeeping, reading/writing
        only persistent buffers (env state is folded back into x_env /
        t_env at the end so every replay continues from live state)."""
        c, env = self.cfg, self.env
        T, E = c.MAX_EPOCH_STEPS, c.NUM_ENVS
        eps = b["eps_dev"]
        moments = b["eps_moments"]
        for m, start in zip(moments, (0.0, 0.0, 0.0, math.inf, -math.inf)):
            m.fill_(start)
        env.x = b["x_env"]
        env.t = b["t_env"]
        obs = b["x_env"]
        wide = self._wide()
        # record activations straight into the update pipeline's buffers:
        # update step 1 runs on the same parameters and skips its forward
        u = wide._upd_bufs(T * E)
        for t in range(T):
            outs = ([u["h"][l].narrow(0, t * E, E) for l in range(len(wide.H))],
                    u["pd"].narrow(0, t * E, E), u["v"].narrow(0, t * E, E))
            # dual-write the transposed activations into the update
            # pipeline's hT buffers (column-offset views; the GEMM writes
            # CT[col][t*E + rb] through the full-B row stride), so update
            # step 1 skips its hT transposes as well as its forward
            ct = (([u["hT"][l][:, t * E:] for l in range(len(wide.H))],
                   T * E) if wide._dualw() else None)
            v, pdflat = wide.forward(obs, out=outs, ct=ct)
            pd = self.pi.pdtype.pdfromflat(pdflat)
            a = pd.sample()
            explore = torch.rand(E, device=self.device) < eps
            rand_a = self._random_actions(E)
            a = torch.where(explore.unsqueeze(-1), rand_a, a)
            b["states"][t].copy_(obs)
            b["actions"][t].copy_(a)
            b["values"][t].copy_(v)
            b["pdflats"][t].copy_(pdflat)
            obs, r, done, _ = env.step(a)
            b["rewards"][t].copy_(r.float())
            donef = done.float()
            b["dones"][t].copy_(donef)
            self._episode_moments(moments, r, done, donef)
        boot_v, _ = wide.forward(obs)
        b["boot_v"].copy_(boot_v)
        # fold live env state back into the stable buffers
        b["x_env"].copy_(obs)
        b["t_env"].copy_(env.t)
        env.x = b["x_env"]
        env.t = b["t_env"]

    @torch.no_grad()
    def _rollout_once_wide_graphed(self) -> Tuple[RolloutBatch, Dict[str, float]]:
        """Wide-config rollout as ONE hipGraph replay (the eager loop's
        ~450 small launches per round otherwise leave the GPU idle
        between kernels).  RNG (action sampling, eps overlay, env noise)
        is graph-captured via registered generator states."""
        c = self.cfg
        eps = self.exploration_rate()
        b = self._wide_rollout_buffers()
        b["eps_dev"].fill_(eps)
        if self._wr_graph is None:
            b["x_env"].copy_(self.env.x)
            b["t_env"].copy_(self.env.t)
            try:
                self._wide().refresh_weights()
                # the warmup runs the rollout for real: env/episode state
                # is restored before the capture
                (g,) = warm_and_capture(
                    (b["x_env"], b["t_env"], self.epr),
                    lambda: self._wide_rollout_body(b),
                    [lambda: self._wide_rollout_body(b)],
                    generators=[self.env._noise_gen])
                self._wr_graph = g
                g.replay()
            except Exception as exc:  # noqa: BLE001 — capture support varies
                self._warn_once(
                    "wide_rollout_graph",
                    f"wide rollout hipGraph capture failed ({exc!r}); "
                    "falling back to the eager rollout loop")
                self._wr_graph = False
                return self._rollout_once_eager_loop()
        elif self._wr_graph is False:
            return self._rollout_once_eager_loop()
        else:
            if self._weights_need_refresh_for_rollout():
                self._wide().refresh_weights()
            self._wr_graph.replay()
        # the rollout recorded h/pd/v for the whole batch into the update
        # buffers; valid for step 1 unless curation may swap batches
        self._wide_rollout_h_valid = not (
            self.cfg.BATCH_CURATION and self.comm.distributed)
        self.obs = self.env.x
        adv, etr = gae_advantages(
            b["rewards"], b["values"], b["dones"], b["boot_v"],
            c.GAMMA, c.LAM, whiten=True, eps=c.ADV_EPS,
            policy=c.USE_HIP_KERNELS,
        )
        return self._make_batch(
            b["states"], b["actions"], adv, etr, b["pdflats"], b["values"],
            b["eps_moments"], eps)

    def _weights_need_refresh_for_rollout(self) -> bool:
        w = self._wide_path
        return w is not None and w._weights_dirty

    @torch.no_grad()
    def _rollout_once_eager(self) -> Tuple[RolloutBatch, Dict[str, float]]:
        if (self._can_wide_bf16() and self.cfg.USE_GRAPHS
                and self.cfg.NUM_ENVS % 256 == 0):
            return self._rollout_once_wide_graphed()
        return self._rollout_once_eager_loop()

    @torch.no_grad()
    def _rollout_once_eager_loop(self) -> Tuple[RolloutBatch, Dict[str, float]]:
        """Collect one iteration of T = MAX_EPOCH_STEPS batched env steps
        (Worker.py:39-65), then GAE (Worker.py:82-92)."""
        self._wide_rollout_h_valid = False  # no recorded activations
        self._v3_acts_valid = False
        c, E = self.cfg, self.cfg.NUM_ENVS
        T = c.MAX_EPOCH_STEPS
        obs_dim = self.obs_space.shape[0]
        eps = self.exploration_rate()

        P = self.pi.pdtype.param_shape()[0]
        dev = self.device
        states = torch.empty(T, E, obs_dim, device=dev, dtype=self.dtype)
        pdflats = torch.empty(T, E, P, device=dev, dtype=self.dtype)
        if self._act_kind == "discrete":
            actions = torch.empty(T, E, device=dev, dtype=torch.long)
        elif self._act_kind == "multidiscrete":
            actions = torch.empty(
                T, E, len(self.act_space.nvec), device=dev, dtype=torch.long)
        else:  # box / multibinary: float vectors
            actions = torch.empty(
                T, E, self.act_space.shape[0], device=dev, dtype=self.dtype
            )
        rewards = torch.empty(T, E, device=dev, dtype=torch.float32)
        dones = torch.empty(T, E, device=dev, dtype=torch.float32)
        values = torch.empty(T, E, device=dev, dtype=torch.float32)

        # device-side episode-reward moments: the reference appends python
        # floats per done (Worker.py:62-65); here masked tensor ops keep
        # the whole loop sync-free (no host round trip per step).
        moments = [torch.full((), start, device=dev)
                   for start in (0.0, 0.0, 0.0, math.inf, -math.inf)]

        obs = self.obs
        for t in range(T):
            a, v, pdflat = self.act_batch(obs, eps)
            states[t] = obs
            actions[t] = a
            values[t] = v.float()
            pdflats[t] = pdflat
            obs, r, done, _ = self.env.step(a)
            rewards[t] = r.float()
            donef = done.float()
            dones[t] = donef
            self._episode_moments(moments, r, done, donef)
        self.obs = obs

        with torch.no_grad():
            boot_v, _ = self._policy_forward(obs)
        adv, etr = gae_advantages(
            rewards, values, dones, boot_v.float(),
            c.GAMMA, c.LAM, whiten=True, eps=c.ADV_EPS,
            policy=c.USE_HIP_KERNELS,
        )

        return self._make_batch(
            states, actions, adv, etr, pdflats, values, moments, eps)

    def collect(self) -> RolloutBatch:
        """Rollout with the push guard: retry (discarding) until at least
        one episode completed (Worker.py:135 + while-loop Worker.py:30)."""
        for _ in range(self.cfg.MAX_ROLLOUT_RETRIES):
            batch, _ = self.rollout_once()
            if batch.valid:
                return batch
        return batch  # invalid; the validity flag keeps collectives alive

    # ------------------------------------------------------------------
    def eval_losses(self, batch: RolloutBatch, l_mul: float) -> Dict[str, float]:
        """Pre-update loss evaluation for the logs vector (Worker.py:117-118).

        The reference evaluates its losses right after the rollout, when
        pi still equals oldpi (sync_pis ran at round start), so this needs
        NO forward pass: both networks' outputs on the batch are the
        recorded rollout outputs."""
        with torch.no_grad():
            losses = self._losses(batch, l_mul, recorded_pi=True)
        return {k: float(v) for k, v in losses.items()}

    def _losses(
        self, batch: RolloutBatch, l_mul: float, recorded_pi: bool = False
    ) -> Dict[str, torch.Tensor]:
        """PPO losses on a batch.  oldpi's outputs are the recorded rollout
        outputs (batch.oldflat/oldv) — bit-identical to re-running oldpi,
        which equals pi at rollout time (PPO.py:47 + Worker.py:42), without
        the 3 extra GEMMs per update step."""
        if recorded_pi:
            v, pdflat = batch.oldv, batch.oldflat
        else:
            # bf16 config (BASELINE #5): bf16 GEMMs, fp32 loss math
            with self._amp():
                v, pdflat = self.pi(batch.states)
            v, pdflat = v.float(), pdflat.float()
        pd = self.pi.pdtype.pdfromflat(pdflat)
        oldpd = self.pi.pdtype.pdfromflat(batch.oldflat)
        coeffs = PPOLossCoeffs(
            clip_param=self.cfg.CLIP_PARAM * l_mul,
            entcoeff=self.cfg.ENTCOEFF,
            vcoeff=self.cfg.VCOEFF,
        )
        return ppo_losses(
            pd, oldpd, v, batch.oldv, batch.actions, batch.adv, batch.etr,
            coeffs, policy=self.cfg.USE_HIP_KERNELS,
        )

    def stats_row(self, batch: RolloutBatch, losses: Dict[str, float]) -> torch.Tensor:
        """The 9-float logs vector + cur_lr + valid (Worker.py:123-133).

        score = epr.mean()/epr.std() is NaN-prone for a single episode
        (Worker.py:121) — computed but guarded to 0."""
        if batch.valid:
            n = float(batch.ep_count)
            mean = float(batch.ep_sum) / n
            var = max(float(batch.ep_sumsq) / n - mean * mean, 0.0)
            std = math.sqrt(var)  # population std, matching numpy's epr.std()
            score = mean / std if (n > 1 and std > 0) else 0.0
            mn, mx = float(batch.ep_min), float(batch.ep_max)
        else:
            score = 0.0
            mn = mx = mean = -math.inf  # never wins the best-rank sort
        row = torch.tensor(
            [
                score, mn, mx, mean,
                losses["policyLoss"], losses["valueLoss"],
                losses["entropyLoss"], losses["total_loss"],
                float(self.CUR_EP),
                batch.cur_lr,
                1.0 if batch.valid else 0.0,
            ],
            device=self.device, dtype=torch.float32,
        )
        assert row.numel() == STATS_DIM
        return row

    # ------------------------------------------------------------------
    def _can_fuse_update(self) -> bool:
        """Eligibility for the fused MFMA update path (mfma_gemm.hip
        forward/dgrad/dW + the family's gh kernel: ppo_loss.hip for Box,
        disc_gh.hip for Discrete, MultiDiscrete and MultiBinary).

        The three discrete families need a head within the gh kernels'
        limits (2 <= K <= 64; 1..32 components of >= 2 classes with
        sum(nvec) <= 64; n <= 64) and at least P = 2 logit columns: the
        combined-heads dW adds the (zero) gradient rows of gh's pad columns
        to the flat gradient behind the value head's row, and only from
        P = 2 on do all of them land inside the buffer.  P = 64
        (ldgh = 68) is taken: the dgrad GEMM and the dW kernel guard rows
        and columns by their runtime sizes.  DPPO_UPDATE_DISC=0 keeps these
        families on the autograd update."""
        from .ops import use_hip

        c = self.cfg
        if c.DTYPE != "float32":
            return False
        if self._act_kind != "box" and not self._use_update_disc():
            return False
        if not use_hip(self.device, c.USE_HIP_KERNELS):
            return False
        if not (1 <= len(c.HIDDEN_SIZES) <= 3) or max(c.HIDDEN_SIZES) > 128:
            return False
        if self._act_kind == "box":
            if self.act_space.shape[0] > 32:
                return False
        elif self._act_kind == "discrete":
            if not (2 <= self.act_space.n <= 64):
                return False
        elif self._act_kind == "multidiscrete":
            nvec = self._nvec
            if not (1 <= len(nvec) <= 32 and min(nvec) >= 2
                    and sum(nvec) <= 64):
                return False
        elif not (2 <= self.act_space.n <= 64):
            return False
        dims = [self.obs_space.shape[0], *c.HIDDEN_SIZES]
        P, HL = self.pi.pdtype.param_shape()[0], dims[-1]
        hsz = sum(dims[l + 1] * dims[l] for l in range(1, len(dims) - 1))
        return hsz + P * HL + HL <= 24576  # bwd staged-weight LDS budget

    @staticmethod
    def _use_update_disc() -> bool:
        """DPPO_UPDATE_DISC: '0' keeps Discrete, MultiDiscrete and
        MultiBinary policies on the autograd update loop, any other value
        takes the fused MFMA update wherever _can_fuse_update() holds;
        unset = the measured default below."""
        # measured, T=64, ms per update() of 4 steps (tools/update_disc_ab.py,
        # profiles/r11_update_disc.txt): CartPole (16,) autograd 2.02 / 5.97 /
        # 56.5 vs fused 0.31 / 0.74 / 6.22 at E = 128 / 4096 / 65536;
        # LunarLander (64,64) 2.42 / 10.9 / 97.6 vs 0.57 / 1.57 / 15.8;
        # MultiLever (32,) 1.89 / 7.08 / 65.9 vs 0.33 / 0.81 / 7.45; BitFlipper
        # (64,64) 2.39 / 9.72 / 81.5 vs 0.58 / 1.62 / 16.4.  Fused wins every
        # alternated pair (4.1x at the least; spreads < 10 % autograd, < 0.3 %
        # fused).  No crossover in the measured range -> on wherever eligible.
        return DPPOEngine._env_switch("DPPO_UPDATE_DISC", True)

    def update(self, batch: RolloutBatch, l_mul: float) -> None:
        """UPDATE_STEPS repeated full-batch steps on the same data
        (Chief.py:64), DP gradient mean across ranks each step.  The
        reference's Chief fetches only the train op (Chief.py:64), so no
        loss values are materialized here."""
        for g in self.optimizer.param_groups:
            g["lr"] = self.cfg.LEARNING_RATE * l_mul
        if self._can_wide_bf16():
            # hand bf16 MFMA path (BASELINE #5): no rocBLAS/autocast GEMMs
            self._wide().update(batch, l_mul)
            return
        if self.cfg.MINIBATCH_SIZE > 0:
            self._update_minibatched(batch, l_mul)
            return
        if self._can_fuse_update():
            # Graph capture of the RCCL all-reduce is unexercised on this
            # pool's multi-GPU boxes; keep multi-rank runs on the plain
            # fused path unless explicitly opted in (DPPO_GRAPH_DIST=1).
            graph_ok = self.cfg.USE_GRAPHS and self._batch_is_persistent() and (
                not self.comm.distributed
                or os.environ.get("DPPO_GRAPH_DIST") == "1"
            )
            if graph_ok:
                self._update_graphed(batch, l_mul)
            else:
                self._update_fused(batch, l_mul)
            return
        for _ in range(self.cfg.UPDATE_STEPS):
            self.flat_pi.zero_grad()
            losses = self._losses(batch, l_mul)
            losses["total_loss"].backward()
            self.comm.allreduce_mean_(self.flat_pi.flat_grad)
            self.optimizer.step()

    def _batch_is_persistent(self) -> bool:
        """The batch tensors are views of the persistent rollout / GAE
        buffers, as a captured update needs: what every single-launch HIP
        rollout (_rollout_once_fused, all four families, and the physics
        rollout) and the v3 rollout guarantee, and the eager rollout loop
        does not."""
        return (self._can_fuse_rollout() or self._use_rollout_cat()
                or self._use_rollout_multi() or self._use_rollout_classic())

    def _update_minibatched(self, batch: RolloutBatch, l_mul: float) -> None:
        """Minibatched update steps (BASELINE config 4): each of the
        UPDATE_STEPS epochs walks the batch in sequential MINIBATCH_SIZE
        chunks with a gradient all-reduce + Adam step per chunk.  The
        reference itself is full-batch (Chief.py:64); chunks are
        sequential (no shuffle) so every rank takes the same number of
        steps and collectives stay aligned."""
        mb = self.cfg.MINIBATCH_SIZE
        B = batch.states.shape[0]
        fuse = self._can_fuse_update()
        clip = self.cfg.CLIP_PARAM * l_mul
        if fuse and self._clip_dev is not None:
            self._clip_dev.fill_(clip)
        if (fuse and self.cfg.USE_GRAPHS
                and (not self.comm.distributed
                     or os.environ.get("DPPO_GRAPH_DIST") == "1")
                and not self._mb_graph_failed):
            # Only CAPTURE failures fall through to the uncaptured loop
            # (capture is state-safe: warmup is snapshot/restored and a
            # capture records, not executes).  A failure during replay or
            # the tail chunk has already mutated params/Adam state, so it
            # propagates instead of re-running the epochs (which would
            # double-step the round — ADVICE r01 #1).
            if self._update_minibatched_graphed(batch, l_mul):
                return
        use_ck = fuse and self._can_chunk_kernel(min(mb, B))
        if fuse:
            self.optimizer.lr_dev.fill_(self.cfg.LEARNING_RATE * l_mul)
        for _ in range(self.cfg.UPDATE_STEPS):
            for o in range(0, B, mb):
                n = min(mb, B - o)
                if use_ck:
                    self._chunk_kernel_step(batch, o, n, clip)
                    continue
                sub = batch.narrow(o, n)
                if fuse:
                    self._fused_step(sub, clip)
                    continue
                self.flat_pi.zero_grad()
                losses = self._losses(sub, l_mul)
                losses["total_loss"].backward()
                self.comm.allreduce_mean_(self.flat_pi.flat_grad)
                self.optimizer.step()

    # chunks per captured graph segment: bounds per-graph node count
    # (~11 kernels/chunk) while keeping replay overhead negligible
    _MB_SEG = 1024

    def _update_minibatched_graphed(self, batch: RolloutBatch,
                                    l_mul: float) -> bool:
        """hipGraph-captured minibatch epochs (BASELINE config 4): the
        sequential chunk walk is identical every epoch and every round —
        the rollout/GAE outputs live in persistent buffers, so chunk
        addresses are stable — and is captured ONCE in segments of
        _MB_SEG chunks, then replayed UPDATE_STEPS times per round.  The
        uncaptured loop pays ~260 us of launch/alloc overhead per
        4096-sample chunk; replay pays in-graph dispatch only.  Per-round
        scalars (clip, lr, Adam step) are device-resident as in
        _update_graphed.  A tail chunk (B % mb != 0) runs uncaptured
        after each epoch's replays, preserving chunk order; Adam state is
        fully device-side so mixing is exact."""
        c = self.cfg
        mb = c.MINIBATCH_SIZE
        B = batch.states.shape[0]
        n_full = B // mb
        tail = B - n_full * mb
        clip = c.CLIP_PARAM * l_mul
        if self._clip_dev is None:
            self._clip_dev = torch.tensor([clip], device=self.device)
        else:
            self._clip_dev.fill_(clip)
        self.optimizer.lr_dev.fill_(c.LEARNING_RATE * l_mul)
        key = (batch.states.data_ptr(), batch.actions.data_ptr(),
               batch.adv.data_ptr(), batch.etr.data_ptr(),
               batch.oldflat.data_ptr(), batch.oldv.data_ptr(), B, mb)
        if self._mb_graphs is None or self._mb_key != key:
            try:
                self._mb_capture(batch, key, n_full)
            except Exception as exc:  # noqa: BLE001 — capture support varies
                if os.environ.get("DPPO_DEBUG"):
                    import traceback

                    traceback.print_exc()
                self._warn_once(
                    "mb_graph",
                    f"minibatch hipGraph capture failed ({exc!r}); "
                    "falling back to the uncaptured chunk loop",
                )
                self._mb_graph_failed = True
                self._mb_graphs = None
                return False
        for _ in range(c.UPDATE_STEPS):
            for g in self._mb_graphs:
                g.replay()
            if tail:
                self._mb_chunk_step(batch, n_full * mb, tail)
        return True

    def _mb_chunk_step(self, batch: RolloutBatch, o: int, n: int) -> None:
        """One fused minibatch gradient step on batch[o:o+n] (capture-safe:
        clip/lr/step all come from device memory)."""
        if self._can_chunk_kernel(n):
            self._chunk_kernel_step(batch, o, n, 0.0)  # clip via _clip_dev
            return
        self._fused_step(batch.narrow(o, n), 0.0)  # clip via _clip_dev

    def _train_state(self):
        """What an update step mutates: parameters, Adam moments, step
        count.  Graph warm-ups execute real steps and restore these."""
        opt = self.optimizer
        return (self.flat_pi.flat_param, opt.exp_avg, opt.exp_avg_sq,
                opt.step_dev)

    def _mb_capture(self, batch: RolloutBatch, key, n_full: int) -> None:
        mb = self.cfg.MINIBATCH_SIZE

        def chunks(lo, hi):
            for ci in range(lo, hi):
                self._mb_chunk_step(batch, ci * mb, mb)

        # the warmup (lazy inits, allocator) is two chunks; the epoch is
        # captured in segments of _MB_SEG chunks sharing one pool
        self._mb_graphs = warm_and_capture(
            self._train_state(), lambda: chunks(0, min(2, n_full)),
            [lambda s0=s0: chunks(s0, min(n_full, s0 + self._MB_SEG))
             for s0 in range(0, n_full, self._MB_SEG)],
            pool=torch.cuda.graph_pool_handle())
        self._mb_key = key

    # Max batch routed to the fused chunk-step kernel (mlp_train.hip):
    # measured 182 us per 4096-sample chunk pair vs ~258 us for the
    # kernel chain it replaces (ladder in profiles/
    # r01_chunk_kernel_notes.md).  8192 is the largest MEASURED-faster
    # batch regime (4096-sample config-4 chunks, 6400-sample config-2
    # full batches); above it the chunk pair's serial tile loop grows
    # linearly while the MFMA GEMM path's latency is ~flat, so the
    # crossover sweep is queued (ROADMAP.md) before raising it.
    # Override via env DPPO_CHUNK_KERNEL_MAX_B (0 disables).
    CHUNK_KERNEL_MAX_B = int(
        os.environ.get("DPPO_CHUNK_KERNEL_MAX_B", "8192"))

    def _can_chunk_kernel(self, B: int) -> bool:
        """Eligibility for the fused single-kernel chunk step
        (ops/hip/mlp_train.hip): the whole fwd + PPO grad + bwd + dW +
        Adam for one (mini)batch chunk in two kernel launches."""
        from .ops import hip_ext
        from .ops.adam import FusedFlatAdam

        c = self.cfg
        if not self._hip_path("box"):
            return False
        if B > self.CHUNK_KERNEL_MAX_B:
            return False
        if not isinstance(self.optimizer, FusedFlatAdam):
            return False
        hs = c.HIDDEN_SIZES
        if len(hs) not in (1, 2) or len(set(hs)) != 1:
            return False
        return bool(hip_ext().mlp_chunk_supported(
            self.obs_space.shape[0], hs[0], self.act_space.shape[0], len(hs)))

    def _chunk_scratch(self) -> torch.Tensor:
        """Per-block gradient slab scratch (<=256 blocks x padded P)."""
        if self._chunk_slabs is None:
            ppad = (self.flat_pi.flat_param.numel() + 3) & ~3
            self._chunk_slabs = torch.zeros(
                256 * ppad, device=self.device, dtype=torch.float32)
        return self._chunk_slabs

    def _chunk_kernel_step(self, batch: RolloutBatch, o: int, n: int,
                           clip: float) -> None:
        """One fused chunk gradient+Adam step on batch[o:o+n].  Single
        rank: kernel-fused Adam (capture-safe device scalars).  Multi
        rank: the kernel writes the summed gradient, then the usual
        all-reduce + device-state Adam step run.  A live _clip_dev
        overrides `clip` inside the kernel (graphed callers pass 0)."""
        from .ops import hip_ext

        c = self.cfg
        opt = self.optimizer
        offsets = [sl.start for sl in self.flat_pi.slices]
        dims = [self.obs_space.shape[0], *c.HIDDEN_SIZES]
        fuse = not self.comm.distributed
        hip_ext().mlp_chunk_train(
            self.flat_pi.flat_param.data,
            batch.states.narrow(0, o, n), batch.actions.narrow(0, o, n),
            batch.adv.narrow(0, o, n), batch.etr.narrow(0, o, n),
            batch.oldflat.narrow(0, o, n), batch.oldv.narrow(0, o, n),
            offsets, dims, self._act_code,
            self._clip_dev_or_empty(), clip, c.ENTCOEFF, c.VCOEFF,
            self._chunk_scratch(), opt.exp_avg, opt.exp_avg_sq,
            opt.step_dev, opt.lr_dev, opt.coef,
            self.flat_pi.flat_grad, fuse,
            opt.betas[0], opt.betas[1], opt.eps)
        if not fuse:
            self.comm.allreduce_mean_(self.flat_pi.flat_grad)
            opt.step_captured()

    def _clip_dev_or_empty(self) -> torch.Tensor:
        if self._clip_dev is None:
            return torch.empty(0, device=self.device)
        return self._clip_dev

    def _update_graphed(self, batch: RolloutBatch, l_mul: float) -> None:
        """hipGraph-captured update: the whole UPDATE_STEPS pipeline
        (forward GEMMs, loss grads, dgrad chain, dW scatter, all-reduce,
        Adam) is captured ONCE and replayed each round.  Per-round scalars
        (clip = CLIP_PARAM*l_mul, lr = LEARNING_RATE*l_mul, the Adam step
        count) live in device memory, and every input tensor is a view of
        the persistent rollout/GAE buffers, so replay sees fresh data.
        Any capture failure falls back to the uncaptured fused path."""
        clip = self.cfg.CLIP_PARAM * l_mul
        lr = self.cfg.LEARNING_RATE * l_mul
        if self._graph_failed:
            self._update_fused(batch, l_mul)
            return
        if (self._upd_graph is not None
                and self._upd_graph_skip != self._v3_acts_valid):
            self._upd_graph = None  # skip-first structure changed
        if self._upd_graph is None:
            def warmup():
                for _ in range(2):
                    self._update_body(batch)

            try:
                self._clip_dev = torch.tensor([clip], device=self.device)
                self.optimizer.lr_dev.fill_(lr)
                # the warmup executes real steps: optimizer+param state is
                # restored, also when it raises (the fallback below must
                # not step the round a second time)
                (self._upd_graph,) = warm_and_capture(
                    self._train_state(), warmup,
                    [lambda: self._update_body(batch)])
                self._upd_graph_skip = self._v3_acts_valid
            except Exception as exc:  # noqa: BLE001 — capture support varies
                self._warn_once(
                    "upd_graph",
                    f"update hipGraph capture failed ({exc!r}); "
                    "falling back to uncaptured fused update",
                )
                self._graph_failed = True
                self._upd_graph = None
                self._update_fused(batch, l_mul)
                return
        self._clip_dev.fill_(clip)
        self.optimizer.lr_dev.fill_(lr)
        self._upd_graph.replay()

    def _update_body(self, batch: RolloutBatch) -> None:
        """The capture-safe UPDATE_STEPS pipeline (no host syncs, no
        host-valued scalars: clip/lr/step come from device memory)."""
        B = batch.states.shape[0]
        if self._can_chunk_kernel(B):
            for _ in range(self.cfg.UPDATE_STEPS):
                self._chunk_kernel_step(batch, 0, B, 0.0)  # clip: _clip_dev
            return
        self._fused_steps(batch, 0.0)  # clip read from _clip_dev

    def _fused_steps(self, batch: RolloutBatch, clip: float) -> None:
        """UPDATE_STEPS full-batch fused steps; step 1 reuses the v3
        rollout's recorded activations when they are valid."""
        skip1 = (self._v3_acts_valid
                 and os.environ.get("DPPO_NO_SKIP1") != "1")
        for si in range(self.cfg.UPDATE_STEPS):
            self._fused_step(batch, clip, recorded=(si == 0 and skip1))

    def _fused_step(self, batch: RolloutBatch, clip: float,
                    recorded: bool = False) -> None:
        """One fused gradient step on `batch` (a full batch or a minibatch
        chunk): MFMA forward (or, `recorded`, the rollout's activations)
        -> GEMM-shaped backward -> all-reduce -> device-state Adam, lr
        from lr_dev.  A live _clip_dev overrides `clip` inside the kernels
        (captured callers pass 0.0), so the step is capture-safe."""
        acts, a_views, v, pdflat = (
            self._recorded_acts(batch) if recorded
            else self._fused_forward(batch.states))
        self.flat_pi.zero_grad()
        self._fused_backward(
            batch.states, acts, a_views, v, pdflat,
            batch.oldflat, batch.oldv, batch.actions,
            batch.adv, batch.etr, clip,
        )
        self.comm.allreduce_mean_(self.flat_pi.flat_grad)
        self.optimizer.step_captured()

    def _recorded_acts(self, batch: RolloutBatch):
        """(acts, a_views, v, pdflat) from the v3 rollout's recorded
        activation blob — valid only for the FIRST update step of a round
        (parameters unchanged between rollout and step 1); pdflat/v are
        the recorded oldflat/oldv, making the step-1 ratio exactly 1."""
        acts = self._v3["acts"]
        a_views = self._acts_views(acts, batch.states.shape[0])
        # no forward runs: only the per-layer backward needs an operand
        # (the mid kernel reads the head weights from the flat buffer)
        self._stage_weights(fwd=False, dgrad=not self._mid_fused_mode())
        return acts, a_views, batch.oldv, batch.oldflat

    def _fused_forward(self, states: torch.Tensor):
        """MFMA forward through the MLP (gemm_fwd per layer + heads).

        Returns (acts_blob, a_views, v, pdflat): activations land in one
        contiguous blob laid out [B*H1 | B*H2 | ...] for mlp_bwd_rows.
        The weight operands are re-staged per call since params change
        every update step (<100 KB of copies); the outputs are fresh
        tensors, which callers may keep."""
        from .ops import hip_ext

        ext = hip_ext()
        c = self.cfg
        B = states.shape[0]
        act_code = self._act_code
        bs = [lay.bias.detach() for lay in self.pi.hidden]
        # the per-layer backward also wants Wh_pad; the mid kernel reads
        # the head weights from the flat buffer
        mw = self._stage_weights(dgrad=not self._mid_fused_mode())
        wts, whT_pad, bh_pad = mw["wt"], mw["whT_pad"], mw["bh_pad"]
        acts = torch.empty(B * sum(c.HIDDEN_SIZES), device=states.device,
                           dtype=states.dtype)
        a_views = self._acts_views(acts, B)
        P = self.pi.pdtype.param_shape()[0]
        pdflat = torch.empty(B, P, device=states.device, dtype=states.dtype)
        v = torch.empty(B, device=states.device, dtype=states.dtype)
        if mw["heads_pad"] and self._fwd_fused():
            # one launch: h1 / h2 are written once for the backward and
            # never read back by the forward
            empty = states.new_empty(0)
            ext.mlp_fwd_fused(states, wts[0], bs[0], wts[1], bs[1], whT_pad,
                              bh_pad, act_code, a_views[0], a_views[1],
                              pdflat, v, empty, empty, empty, empty, 0, 0,
                              0.0, 0.0)
            self._count_fwd_fused("update")
            return acts, a_views, v, pdflat
        x = states
        for l in range(len(wts)):
            ext.gemm_fwd(x, wts[l], bs[l],
                         act_code, 0, a_views[l], a_views[l], a_views[l],
                         0, 0, 0)
            x = a_views[l]
        if mw["heads_pad"]:
            ext.gemm_fwd(x, whT_pad, bh_pad, 2, 2, pdflat, v, pdflat, 0, 0, 0)
        else:
            ext.gemm_fwd(x, mw["wh"], mw["bh"], 2, 1, pdflat, v, pdflat,
                         1, 0, 0)
        return acts, a_views, v, pdflat

    # the DPPO_MID_FUSED default: what profiles/r05_update_mid_fused.txt
    # measured fastest
    MID_FUSED_DEFAULT = "load"

    def _mid_fused_mode(self) -> str:
        """DPPO_MID_FUSED=0|load: '' keeps the per-layer backward chain;
        'load' runs the fused update-middle kernel (mlp_mid.hip) where the
        shape is eligible.  Anything else is an error, not a fall-back.
        Resolved once per engine and value of the variable."""
        env = os.environ.get("DPPO_MID_FUSED", self.MID_FUSED_DEFAULT)
        cached = self._mid_mode_cache
        if cached is not None and cached[0] == env:
            return cached[1]
        mode = self._resolve_mid_mode(env)
        self._mid_mode_cache = (env, mode)
        return mode

    def _resolve_mid_mode(self, mode: str) -> str:
        from .ops import hip_ext

        if mode == "0":
            return ""
        if mode != "load":
            raise ValueError(
                f"DPPO_MID_FUSED={mode!r}: expected '0' or 'load'")
        c = self.cfg
        if not self._hip_path("box"):
            return ""
        if c.ACTIVATION not in ("tanh", "relu"):
            return ""
        hs = tuple(c.HIDDEN_SIZES)
        if len(hs) != 2 or not hip_ext().mlp_mid_supported(
                hs[0], hs[1], self.act_space.shape[0], len(hs)):
            return ""
        return mode

    def _mid_backward(self, states, a_views, v, pdflat, oldflat, oldv,
                      actions, adv, etr, clip: float) -> torch.Tensor:
        """Fused middle of the backward: (h1, h2, pdflat, v, loss inputs)
        -> dz1 plus the W2/b2/heads gradients in one kernel (gh and dz2
        stay on-chip), then dW1/db1 from dz1.  Returns dz1."""
        from .ops import hip_ext

        ext = hip_ext()
        c = self.cfg
        offsets = [sl.start for sl in self.flat_pi.slices]
        grad = self.flat_pi.flat_grad
        dz1 = torch.empty_like(a_views[0])
        ext.mlp_mid_bwd(
            self.flat_pi.flat_param.detach(), offsets, a_views[0], a_views[1],
            pdflat, v, oldflat, oldv, actions, adv, etr,
            self._act_code, self._clip_dev_or_empty(),
            clip, c.ENTCOEFF, c.VCOEFF, dz1, grad)
        ext.dw_mfma(dz1, states, grad, offsets[0], offsets[1], -1, -1, -1, 0)
        return dz1

    def _fused_backward(self, states, acts, a_views, v, pdflat,
                        oldflat, oldv, actions, adv, etr, clip: float) -> None:
        """GEMM-shaped backward into the (already zeroed) flat grad:
        wave-per-row loss grads -> dgrad GEMM chain (torch weight layouts
        ARE the needed Wt; no transposes) -> split-K dW scatter.  Eligible
        two-hidden-layer shapes take the fused middle kernel instead."""
        from .ops import hip_ext

        if self._mid_fused_mode():
            self._mid_backward(states, a_views, v, pdflat, oldflat, oldv,
                               actions, adv, etr, clip)
            return
        ext = hip_ext()
        c = self.cfg
        offsets = [sl.start for sl in self.flat_pi.slices]
        n_hidden = len(c.HIDDEN_SIZES)
        dgrad_code = 3 if c.ACTIVATION == "tanh" else 4
        P = self.pi.pdtype.param_shape()[0]
        off_wv, off_bv = offsets[2 * n_hidden], offsets[2 * n_hidden + 1]
        off_wp, off_bp = offsets[2 * n_hidden + 2], offsets[2 * n_hidden + 3]
        dummy_bias = torch.zeros(1, device=self.device)

        # the family's loss-gradient kernel; all write the same
        # [B][ldgh] operand (ops.ppo_loss.ppo_gh_ref)
        gh_fn = {
            "box": ext.ppo_loss_gauss_gh,
            "discrete": ext.ppo_loss_cat_gh,
            "multidiscrete": ext.ppo_loss_mcat_gh,
            "multibinary": ext.ppo_loss_bern_gh,
        }[self._act_kind]
        nvec = (self._nvec,) if self._act_kind == "multidiscrete" else ()
        gh = gh_fn(
            pdflat, oldflat, v, oldv, actions, adv, etr, *nvec,
            clip, c.ENTCOEFF, c.VCOEFF, self._clip_dev_or_empty(),
        )
        # the staged PADDED [Wp; Wv; 0...]: its rows are the dgrad Wt
        # matching gh's float4-padded row stride.  The forward stages it
        # unless it ran in the mid-kernel mode
        if not self._wh_pad_staged:
            self._stage_weights(fwd=False, dgrad=True)
        Wh_pad = self._mw["Wh_pad"]
        dz = [None] * n_hidden
        delta, Wt_chain = gh, Wh_pad
        for l in range(n_hidden - 1, -1, -1):
            dz_l = torch.empty_like(a_views[l])
            ext.gemm_fwd(delta, Wt_chain, dummy_bias, dgrad_code, 0,
                         dz_l, dz_l, a_views[l], 0, 0, 0)
            dz[l] = dz_l
            delta = dz_l
            Wt_chain = self.pi.hidden[l].weight.detach()
        grad = self.flat_pi.flat_grad
        ext.dw_mfma(dz[0], states, grad, offsets[0], offsets[1], -1, -1, -1, 0)
        for l in range(1, n_hidden):
            ext.dw_mfma(dz[l], a_views[l - 1], grad,
                        offsets[2 * l], offsets[2 * l + 1], -1, -1, -1, 0)
        # combined heads: rows < P -> Wp/bp, row P -> Wv/bv
        ext.dw_mfma(gh, a_views[-1], grad, off_wp, off_bp, P, off_wv, off_bv, 0)

    def _update_fused(self, batch: RolloutBatch, l_mul: float) -> None:
        """Fused MFMA update steps: gemm_fwd xL -> GEMM-shaped backward ->
        all-reduce -> fused Adam (~10 launches per step, no autograd)."""
        clip = self.cfg.CLIP_PARAM * l_mul
        # a live _clip_dev overrides the kernel's clip argument; keep it
        # coherent when falling back from the graphed path
        if self._clip_dev is not None:
            self._clip_dev.fill_(clip)
        self.optimizer.lr_dev.fill_(self.cfg.LEARNING_RATE * l_mul)
        B = batch.states.shape[0]
        if self._can_chunk_kernel(B):
            for _ in range(self.cfg.UPDATE_STEPS):
                self._chunk_kernel_step(batch, 0, B, clip)
            return
        self._fused_steps(batch, clip)

    # ------------------------------------------------------------------
    def _curate_batches(self, batch: RolloutBatch,
                        gathered: torch.Tensor) -> RolloutBatch:
        """Reference batch-curation parity (Chief.py:33-53): the Chief
        drains every worker's queue, sorts all pushed batches descending
        by best episode reward (logs[2], the Chief.py:51 sort key) and
        feeds the top-N one per tower — so a tower can train on a BETTER
        worker's batch.  Here each rank holds one batch per round; the
        sorted assignment is realized with point-to-point moves: rank i
        trains on the batch collected by rank order[i].  When fewer than
        world_size batches are valid the best batches are recycled
        (order[i % V]) so every rank still trains — the reference's full
        barrier guarantees N valid batches and never hits this case.

        Every rank executes the identical schedule (gathered stats are
        identical across ranks), so sends and recvs pair deterministically.
        """
        W = self.comm.world_size
        r = self.comm.rank
        valid = gathered[:, 10] > 0.5
        key = gathered[:, 2].clone()
        key[~valid] = -math.inf
        order = torch.argsort(key, descending=True, stable=True).tolist()
        V = int(valid.sum())
        if V == 0:
            return batch
        srcs = [order[i] if i < V else order[i % V] for i in range(W)]
        if all(s == i for i, s in enumerate(srcs)):
            return batch
        fields = _SAMPLE_FIELDS
        orig = {f: getattr(batch, f) for f in fields}
        for f in fields:
            assert orig[f].is_contiguous(), f"curation needs contiguous {f}"
        # A rank that SENDS ships a snapshot of its ORIGINAL batch
        # (assignments are of the pre-curation batches), so a receive may
        # land IN-PLACE in the persistent rollout buffers — keeping the
        # hipGraph-captured update paths (keyed on stable data_ptrs) valid.
        self._v3_acts_valid = False  # batch may be another rank's
        self._wide_rollout_h_valid = False
        sends_any = any(s == r and d != r for d, s in enumerate(srcs))
        send_copy = {f: orig[f].clone() for f in fields} if sends_any else None
        for dst, s in enumerate(srcs):
            if s == dst:
                continue
            for f in fields:
                if r == s:
                    self.comm.send(send_copy[f], dst)
                elif r == dst:
                    self.comm.recv(orig[f], s)
        return dataclasses.replace(batch, valid=True)

    def train_round(self) -> Tuple[Dict[str, float], bool]:
        """One full synchronous round. Returns (rank0-view stats, stop)."""
        c = self.cfg
        with self.timers.phase("sync_oldpi"):
            self.sync_oldpi()
        with self.timers.phase("rollout"):
            batch = self.collect()
        with self.timers.phase("eval_losses"):
            losses = self.eval_losses(batch, batch.cur_lr)
        with self.timers.phase("stats_allgather"):
            row = self.stats_row(batch, losses)
            gathered = self.comm.all_gather_rows(row)  # [W, STATS_DIM]
        # Chief semantics: best valid rank by logs[2] (max episode reward)
        valid = gathered[:, 10] > 0.5
        any_valid = bool(valid.any())
        if any_valid:
            key = gathered[:, 2].clone()
            key[~valid] = -math.inf
            best = int(torch.argmax(key))
            l_mul = float(gathered[best, 9])
            best_cur_ep = float(gathered[best, 8])
        else:
            best = -1
            l_mul = batch.cur_lr
            best_cur_ep = float(self.CUR_EP)

        if any_valid:
            if c.BATCH_CURATION and self.comm.distributed:
                with self.timers.phase("curation"):
                    batch = self._curate_batches(batch, gathered)
            with self.timers.phase("update"):
                self.update(batch, l_mul)

        self._round += 1
        if c.BROADCAST_INTERVAL > 0 and self._round % c.BROADCAST_INTERVAL == 0:
            with self.timers.phase("broadcast"):
                self.comm.broadcast_(self.flat_pi.flat_param, src=0)

        # stop rule: best rank's epoch count >= STOP_EPOCH (Chief.py:85-87)
        stop = best_cur_ep >= c.STOP_EPOCH
        self.CUR_EP += 1

        stats = {
            "l_mul": l_mul,
            "best_rank": float(best),
            "score": float(gathered[max(best, 0), 0]),
            "epr_max": float(gathered[max(best, 0), 2]),
            "epr_mean": float(gathered[max(best, 0), 3]),
            **losses,
        }
        if self.comm.rank == 0:
            self.logger.log(self.CUR_EP, stats)
        return stats, stop

    def train(self, max_rounds: Optional[int] = None) -> Dict[str, float]:
        """Run rounds until the stop rule fires (or max_rounds)."""
        n = 0
        stats: Dict[str, float] = {}
        while True:
            stats, stop = self.train_round()
            n += 1
            if stop or (max_rounds is not None and n >= max_rounds):
                break
        return stats

    # ------------------------------------------------------------------
    @torch.no_grad()
    def act(self, s) -> torch.Tensor:
        """Greedy-eval action for a single state: sample from pi with no
        epsilon overlay (Chief.act, Chief.py:89-92 — samples, not mode)."""
        s_t = torch.as_tensor(s, device=self.device, dtype=self.dtype)
        squeeze = s_t.dim() == 1
        if squeeze:
            s_t = s_t.unsqueeze(0)
        _, pdflat = self.pi(s_t)
        a = self.pi.pdtype.pdfromflat(pdflat).sample()
        return a[0] if squeeze else a
