"""hipGraph warm-up + capture, shared by every graphed path of the engine.

A graphed path warms its body up on a side stream (lazy initialisation,
allocator), which executes the body for real, then captures it.  The state
the warm-up mutated is put back before the capture — and also when the
warm-up raises, so that a caller falling back to an uncaptured path starts
from the state it had, not from a half-stepped one.
"""

from __future__ import annotations

import contextlib
from typing import Callable, Iterable, List, Sequence

import torch


@contextlib.contextmanager
def restoring(tensors: Sequence[torch.Tensor]):
    """Snapshot `tensors` on entry and copy the snapshot back on exit,
    whether the block completed or raised (the exception propagates)."""
    snap = [t.detach().clone() for t in tensors]
    try:
        yield
    finally:
        with torch.no_grad():
            for t, s in zip(tensors, snap):
                t.copy_(s)


def warm_and_capture(
    state: Sequence[torch.Tensor],
    warmup: Callable[[], None],
    bodies: Iterable[Callable[[], None]],
    generators: Iterable[torch.Generator] = (),
    pool=None,
) -> List[torch.cuda.CUDAGraph]:
    """Run `warmup` on a side stream with `state` snapshot/restored around
    it, then capture each of `bodies` into a graph of its own (all in
    `pool` when given, each with `generators` registered).  Returns the
    graphs in order; nothing is replayed."""
    side = torch.cuda.Stream()
    with restoring(state):
        try:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                warmup()
        finally:
            # also after a host exception: what the warm-up already queued
            # must finish before the restore overwrites its results
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
    graphs = []
    for body in bodies:
        g = torch.cuda.CUDAGraph()
        for gen in generators:
            g.register_generator_state(gen)
        with torch.cuda.graph(g, pool=pool):
            body()
        graphs.append(g)
    return graphs
