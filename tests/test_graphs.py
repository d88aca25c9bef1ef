"""utils.graphs: the snapshot-and-always-restore piece of the graph
warm-up helper, on plain CPU tensors."""

import pytest
import torch

from dppo_amd.utils.graphs import restoring


def _bits(t):
    return t.detach().contiguous().view(torch.uint8)


def _state():
    torch.manual_seed(0)
    return [torch.randn(7, 3), torch.arange(5, dtype=torch.int32),
            torch.nn.Parameter(torch.randn(11))]


def test_restoring_puts_state_back_when_the_body_raises():
    state = _state()
    want = [t.detach().clone() for t in state]
    ptrs = [t.data_ptr() for t in state]

    class Boom(RuntimeError):
        pass

    with pytest.raises(Boom):
        with restoring(state):
            with torch.no_grad():
                state[0].mul_(3.0).add_(float("nan"))
                state[1].add_(1)
                state[2].zero_()
            assert not torch.equal(state[1], want[1])
            raise Boom("after the mutation")
    for t, w, p in zip(state, want, ptrs):
        assert t.data_ptr() == p  # restored in place, not rebound
        assert t.dtype == w.dtype and torch.equal(_bits(t), _bits(w))


def test_restoring_puts_state_back_on_success_too():
    state = _state()
    want = [t.detach().clone() for t in state]
    with restoring(state):
        with torch.no_grad():
            for t in state:
                t.add_(1)
    for t, w in zip(state, want):
        assert torch.equal(_bits(t), _bits(w))
