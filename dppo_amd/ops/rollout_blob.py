"""Engine-side mirror of ops/hip/rollout_blob.h: the one float blob every
whole-rollout path writes.

  states[T][E][D] | pd params[T][E][P] | actions[T][E][actw] | values[T][E]
  | rewards[T][E] | dones[T][E] | boot[E] | moments[5]

The kinds with int64 actions (discrete, multidiscrete) have no float action
region: their int64 region, 2*T*E*actw floats wide, leads the blob.  The
engine must size its persistent blob exactly as the bindings do, or they
allocate their own and the hipGraph-captured update replays against stale
addresses; tests/test_gpu_rollout_blob.py holds the two definitions together.
"""

from __future__ import annotations

import functools
from typing import NamedTuple, Sequence, Tuple, Union

NAMES = ("states", "pd", "actions", "values", "rewards", "dones", "boot",
         "moments")


class RolloutBlob(NamedTuple):
    """`numel` floats; per region of NAMES its float offset, its shape and
    whether it holds int64."""
    numel: int
    regions: Tuple[Tuple[str, int, Tuple[int, ...], bool], ...]

    def views(self, out):
        """The eight views of the 1-D float32 blob `out`, in NAMES order (the
        order the bindings return)."""
        import torch

        res = []
        for _, off, shape, is_int in self.regions:
            n = 1
            for s in shape:
                n *= s
            if is_int:
                res.append(out.narrow(0, off, 2 * n).view(torch.int64)
                           .view(shape))
            else:
                res.append(out.narrow(0, off, n).view(shape))
        return tuple(res)


def rollout_blob(kind: str, T: int, E: int, D: int,
                 n_act: Union[int, Sequence[int]]) -> RolloutBlob:
    """Layout for a policy kind (an engine _act_kind) with n_act = the action
    count K (discrete), nvec (multidiscrete), n (multibinary) or the action
    dim A (box)."""
    if isinstance(n_act, list):
        n_act = tuple(n_act)
    return _layout(kind, T, E, D, n_act)


# the engine asks once per rollout, for the same arguments every time
@functools.lru_cache(maxsize=None)
def _layout(kind, T, E, D, n_act) -> RolloutBlob:
    if kind == "discrete":
        P, ashape, int_actions = n_act, (T, E), True
    elif kind == "multidiscrete":
        P, ashape, int_actions = sum(n_act), (T, E, len(n_act)), True
    elif kind == "multibinary":
        P, ashape, int_actions = n_act, (T, E, n_act), False
    elif kind == "box":
        P, ashape, int_actions = 2 * n_act, (T, E, n_act), False
    else:
        raise ValueError(f"no rollout blob layout for policy kind {kind!r}")
    TE = T * E
    n_a = TE * (ashape[2] if len(ashape) == 3 else 1)
    off = {}
    o = 0
    if int_actions:
        off["actions"], o = o, o + 2 * n_a
    off["states"], o = o, o + TE * D
    off["pd"], o = o, o + TE * P
    if not int_actions:
        off["actions"], o = o, o + n_a
    for name in ("values", "rewards", "dones"):
        off[name], o = o, o + TE
    boot = o
    off["boot"], off["moments"] = boot, boot + E
    shapes = {"states": (T, E, D), "pd": (T, E, P), "actions": ashape,
              "values": (T, E), "rewards": (T, E), "dones": (T, E),
              "boot": (E,), "moments": (5,)}
    return RolloutBlob(
        numel=boot + E + 5,
        regions=tuple((n, off[n], shapes[n], int_actions and n == "actions")
                      for n in NAMES))
