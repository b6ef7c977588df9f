"""The one way a replay-ring learner's host data reaches its device: ``Staging``, a group of named host buffers that are written and
copied together (a step's transition, a step's observations, a batch's indices).  DESIGN.md section 3.20 states the rule."""
from __future__ import annotations

import torch


class Staging:
    """``Staging(device, name=(shape, dtype), ...)``.

    On a GPU the buffers are pinned and have device mirrors.  A stream orders the asynchronous copies it is given, but nothing orders the
    HOST's next write to a pinned buffer behind a copy still reading it, and the loops here store and update many times back to back
    with no synchronisation (every step before ``learning_starts``, an offline phase that logs every 100th update).  So there are two
    host sets used in turn, each with an event recorded behind its copies: ``begin`` waits for the set that comes round again, which
    leaves the host one transfer ahead of the device.  On the CPU there is one plain set and ``push`` returns it: the twins read it in
    place."""

    def __init__(self, device, **specs):
        self.device = torch.device(device)
        cuda = self.device.type == "cuda"
        make = lambda **kw: {k: torch.zeros(shape, dtype=dtype, **kw) for k, (shape, dtype) in specs.items()}  # noqa: E731
        self.sets = [make(pin_memory=cuda) for _ in range(2 if cuda else 1)]
        self.events = [torch.cuda.Event() for _ in self.sets] if cuda else []
        self.mirror = make(device=self.device) if cuda else None
        self.turn = 0

    def begin(self) -> dict:
        """The host set to write now, once the copies of its last ``push`` have left it."""
        self.turn = (self.turn + 1) % len(self.sets)
        if self.events:
            self.events[self.turn].synchronize()
        return self.sets[self.turn]

    def push(self) -> dict:
        """The set just written, where the kernels read it: copied to the mirrors on the current stream (GPU), or itself (CPU)."""
        host = self.sets[self.turn]
        if not self.events:
            return host
        for k, t in host.items():
            self.mirror[k].copy_(t, non_blocking=True)
        self.events[self.turn].record(torch.cuda.current_stream(self.device))
        return self.mirror
