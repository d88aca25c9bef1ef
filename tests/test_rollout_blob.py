"""ops/rollout_blob.py, the engine's mirror of the rollout output blob layout
(ops/hip/rollout_blob.h): sizes against literal formulas, and the views'
order, disjointness and coverage.  The bindings are held to the same layout
by tests/test_gpu_rollout_blob.py."""

import pytest
import torch

from dppo_amd.ops.rollout_blob import NAMES, rollout_blob

T, E, D = 2, 3, 5

# kind, n_act, expected numel (literal: not computed by the helper), pd-param
# width, actions shape, int64 actions
CASES = {
    "discrete": ("discrete", 3, T * E * (2 + D + 3 + 3) + E + 5, 3, (T, E),
                 True),
    "multidiscrete": ("multidiscrete", [2, 3],
                      T * E * (2 * 2 + D + (2 + 3) + 3) + E + 5, 5,
                      (T, E, 2), True),
    "multibinary": ("multibinary", 3, T * E * (D + 2 * 3 + 3) + E + 5, 3,
                    (T, E, 3), False),
    "box": ("box", 2, T * E * (D + 3 * 2 + 3) + E + 5, 4, (T, E, 2), False),
    "box_classic": ("box", 1, T * E * (D + 3 * 1 + 3) + E + 5, 2, (T, E, 1),
                    False),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_numel_equals_the_literal_formula(case):
    kind, n_act, numel = CASES[case][:3]
    assert rollout_blob(kind, T, E, D, n_act).numel == numel


@pytest.mark.parametrize("case", sorted(CASES))
def test_views_tile_the_blob_in_the_documented_order(case):
    kind, n_act, numel, P, ashape, int_actions = CASES[case]
    lay = rollout_blob(kind, T, E, D, n_act)
    out = torch.zeros(lay.numel)
    views = lay.views(out)
    assert tuple(r[0] for r in lay.regions) == NAMES == (
        "states", "pd", "actions", "values", "rewards", "dones", "boot",
        "moments")
    assert len(views) == 8
    shapes = [(T, E, D), (T, E, P), ashape, (T, E), (T, E), (T, E), (E,),
              (5,)]
    assert [tuple(v.shape) for v in views] == shapes
    for name, v in zip(NAMES, views):
        want = torch.int64 if (int_actions and name == "actions") \
            else torch.float32
        assert v.dtype == want and v.is_contiguous()
    # float extents [start, end) of each view inside the blob
    ext = {}
    for name, v in zip(NAMES, views):
        start = (v.data_ptr() - out.data_ptr()) // 4
        ext[name] = (start, start + v.numel() * v.element_size() // 4)
    # memory order: int64 actions lead; float actions follow pd
    order = (["actions", "states", "pd"] if int_actions
             else ["states", "pd", "actions"]) + [
        "values", "rewards", "dones", "boot", "moments"]
    pos = 0
    for name in order:  # disjoint, gap-free, covering [0, numel)
        assert ext[name][0] == pos, name
        pos = ext[name][1]
    assert pos == lay.numel == numel
    if int_actions:
        assert ext["actions"][0] == 0
    # writes through one view touch no other
    for i, v in enumerate(views):
        v.fill_(i + 1)
    for i, v in enumerate(views):
        assert bool((v == i + 1).all())


def test_unknown_kind_raises():
    with pytest.raises(ValueError):
        rollout_blob("tuple", T, E, D, 2)
