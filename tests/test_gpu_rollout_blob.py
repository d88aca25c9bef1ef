"""The six whole-rollout bindings against ops/rollout_blob.py, the engine's
mirror of the output blob layout (ops/hip/rollout_blob.h).

The engine sizes a persistent blob with the Python helper and the bindings
size theirs in C++; when the two differ a binding silently allocates its own
and the hipGraph-captured update replays against stale addresses.  So for each
binding: (a) a blob of the helper's numel is adopted and every returned tensor
is the helper's view of it; (b) a launch that allocates its own blob returns
the same bits; (c) a blob of another size is not adopted, and the fresh one
has the helper's size.

T = 2, hidden (8,), E = 2 (one 2-env tile) and 3 (one 8-env tile with a
tail; for the lane-per-env kernel one partly filled wave).  Episodes end at
step 2 (horizon / time limit 2), so the moments are not trivially zero.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

from dppo_amd import spaces
from dppo_amd.envs.classic import BatchedCartPole, BatchedPendulum
from dppo_amd.envs.synthetic import BatchedSyntheticEnv
from dppo_amd.models.mlp import PolicyValueMLP
from dppo_amd.ops import require_hip_ext
from dppo_amd.ops.rollout_blob import NAMES, rollout_blob

T, D, HIDDEN, SEED = 2, 5, (8,), 1234

# binding -> (blob kind, action space or classic env class, n_act)
BINDINGS = {
    "rollout_run": ("box", spaces.Box(low=-1.0, high=1.0, shape=(2,)), 2),
    "rollout_run_cat": ("discrete", spaces.Discrete(3), 3),
    "rollout_run_mcat": ("multidiscrete", spaces.MultiDiscrete([2, 3]),
                         [2, 3]),
    "rollout_run_bern": ("multibinary", spaces.MultiBinary(3), 3),
    "classic_rollout_cat": ("discrete", BatchedCartPole, 2),
    "classic_rollout_box": ("box", BatchedPendulum, 1),
}


def weight_blob(pi):
    """Wt[in][out] + b per hidden layer, Wv[H], bv, Wpt[H][P], bp."""
    parts = []
    for lay in pi.hidden:
        parts += [lay.weight.t().contiguous(), lay.bias]
    parts += [pi.vf.weight, pi.vf.bias, pi.pi.weight.t().contiguous(),
              pi.pi.bias]
    offsets, off = [], 0
    for p in parts:
        offsets.append(off)
        off += p.numel()
    with torch.no_grad():
        blob = torch.cat([p.reshape(-1) for p in parts])
    return blob, offsets, [pi.obs_dim, *pi.hidden_sizes]


def make_launcher(name, E):
    """(launch, layout): launch(out_buf) runs the binding from the same
    initial env state and seed every time."""
    kind, space, n_act = BINDINGS[name]
    classic = name.startswith("classic")
    torch.manual_seed(7)
    if classic:
        env = space(E, device="cuda", seed=3, time_limit=2)
    else:
        env = BatchedSyntheticEnv(
            spaces.Box(low=-float("inf"), high=float("inf"), shape=(D,)),
            space, E, device="cuda", seed=3, horizon=2)
    env.reset()
    pi = PolicyValueMLP(obs_dim=env.obs_dim, action_space=env.action_space,
                        hidden_sizes=HIDDEN, activation="tanh").cuda()
    blob, offsets, dims = weight_blob(pi)
    bounds = (-1.0, 1.0) if kind == "box" else ()
    run = getattr(require_hip_ext(), name)
    x0, t0 = env.x.clone(), env.t.clone()
    s0 = env.s.clone() if classic else None

    def launch(out_buf):
        x, t, epr = x0.clone(), t0.clone(), torch.zeros(E, device="cuda")
        if classic:
            env_args, ablate = (env.ENV_ID, s0.clone(), env.time_limit), ()
        else:
            env_args = (env.blob, env.rank_eff, env.horizons_i32, 0.05)
            ablate = (0,)
        return run(blob, offsets, dims, 1, *env_args, *bounds, 0.0, x, t,
                   epr, T, n_act, SEED, out_buf, *ablate)

    return launch, rollout_blob(kind, T, E, env.obs_dim, n_act)


def floats(v):
    return v.numel() * v.element_size() // 4


def storage_ptr(v):
    return v.untyped_storage().data_ptr()


@pytest.mark.parametrize("E", [2, 3])
@pytest.mark.parametrize("name", sorted(BINDINGS))
def test_binding_and_python_mirror_agree(name, E):
    launch, lay = make_launcher(name, E)

    # (a) a persistent blob of the helper's size is adopted, view for view
    blob = torch.zeros(lay.numel, device="cuda")
    got = launch(blob)
    want = lay.views(blob)
    assert len(got) == len(want) == 8
    for n, g, w in zip(NAMES, got, want):
        assert storage_ptr(g) == storage_ptr(blob), n
        assert g.data_ptr() == w.data_ptr(), n
        assert tuple(g.shape) == tuple(w.shape), n
        assert g.dtype == w.dtype, n
    kept = [g.clone() for g in got]
    assert float(kept[7][0]) == E  # every env finished one episode

    # (b) the binding's own allocation: the same bits
    own = launch(torch.empty(0, device="cuda"))
    for n, k, o in zip(NAMES, kept, own):
        assert storage_ptr(o) != storage_ptr(blob), n
        assert o.dtype == k.dtype and torch.equal(o, k), n

    # (c) a blob of another size is left alone; the fresh one has the
    # helper's size
    other = torch.full((lay.numel + 1,), 7.0, device="cuda")
    fresh = launch(other)
    assert bool((other == 7.0).all())
    for n, f in zip(NAMES, fresh):
        assert storage_ptr(f) != storage_ptr(other), n
    assert len({storage_ptr(f) for f in fresh}) == 1
    assert sum(floats(f) for f in fresh) == lay.numel
    assert fresh[0].untyped_storage().nbytes() == 4 * lay.numel
