"""Guard-band arena: every tensor a kernel (or a host twin) is handed lies inside ONE allocation that the test owns, between
bands of sentinel words.  A write past a tensor lands in a band and is reported; a read of a word that nobody wrote returns the
sentinel and shows up in the result's bits.  Nothing leaves the arena, so an overrun here is a finding, never a fault.

The convention is the one of ``test_conv1q_forward_writes_nothing_past_its_tensors`` and
``test_kernel_rb_is_kernel_z_bit_for_bit_and_writes_nothing_past_its_tensor``: int32 storage filled with a sentinel, tensors carved
as views, at least ``1 << 16`` sentinel words on either side.  Two sentinels, the project's own:

* ``0x7FC0DEAD`` -- a NaN as f32: a stale read poisons whatever is computed from it;
* ``0x5A5A5A5A`` -- a large finite f32 (1.5e16): ``fmaxf`` / ``fminf`` / compare-select paths swallow a NaN, a stale read that
  passes through one of them is caught by this one.

A case is run with both; its results must not depend on which.
"""
from __future__ import annotations

import contextlib
import sys

import torch

NAN_SENTINEL = 0x7FC0DEAD
FINITE_SENTINEL = 0x5A5A5A5A
SENTINELS = (NAN_SENTINEL, FINITE_SENTINEL)
GUARD_WORDS = 1 << 16
ALIGN = 256                    # a carved tensor's start (torch's allocators give no less)
WORKSPACE_ALIGN = 16           # a carved workspace's start: the least the C ABI asks of a workspace pointer


def _up(x: int, a: int) -> int:
    return (x + a - 1) // a * a


class Arena:
    """One int32 tensor on ``device`` filled with ``sentinel``; ``carve`` hands out views of it, ``assert_guards_intact`` checks
    every word that was never handed out."""

    def __init__(self, device, sentinel: int = NAN_SENTINEL, words: int = 1 << 23):
        self.device = torch.device(device)
        self.sentinel = int(sentinel)
        self.buf = torch.full((int(words),), self.sentinel, dtype=torch.int32, device=self.device)
        self.bytes = self.buf.view(torch.uint8)
        self.carves: list = []                       # (name, first byte, byte count), in address order
        self._free = GUARD_WORDS * 4                 # the first byte the next carve may start at
        self.stage = ""                              # a prefix for the names of the carves that follow (the entry point being run)

    # ---------------------------------------------------------------------------------------------- carving
    def carve(self, shape, dtype=torch.float32, name: str | None = None, align: int = ALIGN) -> torch.Tensor:
        """A sentinel-filled tensor of ``shape`` / ``dtype``: starts at a multiple of ``align`` bytes, ends exactly at its last
        element, at least ``GUARD_WORDS`` untouched words on both sides."""
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        item = torch.empty((), dtype=dtype).element_size()
        numel = 1
        for s in shape:
            numel *= s
        nbytes = numel * item
        base = self.buf.data_ptr()
        start = _up(base + self._free, max(align, item)) - base
        end = start + nbytes
        if end + GUARD_WORDS * 4 > self.bytes.numel():
            raise MemoryError(f"arena of {self.buf.numel()} words cannot hold {name or shape} ({nbytes} bytes) and its guard: give the case more words")
        self.carves.append((name or f"carve#{len(self.carves)}", start, nbytes))
        self._free = end + GUARD_WORDS * 4
        return self.bytes[start:end].view(dtype).view(shape)

    def input(self, data: torch.Tensor, name: str | None = None, align: int = ALIGN) -> torch.Tensor:
        """``data`` copied into a carve of its own shape: a read past its last element sees the sentinel."""
        t = self.carve(data.shape, data.dtype, name, align)
        t.copy_(data)
        return t

    # ---------------------------------------------------------------------------------------------- checking
    def _gaps(self):
        """(first byte, end byte, carve before | None, carve after | None) of every guard band."""
        lo, before = 0, None
        for c in self.carves:
            yield lo, c[1], before, c
            lo, before = c[1] + c[2], c
        yield lo, self.bytes.numel(), before, None

    def _expected_byte(self, b: int) -> int:
        return (self.sentinel >> (8 * (b % 4))) & 0xFF             # little endian

    def first_touched(self):
        """None, or (guard number, byte offset in the arena, message) of the first guard byte that lost its sentinel."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        flags = []
        for lo, hi, _, _ in self._gaps():
            flags.append((self.buf[_up(lo, 4) // 4:hi // 4] != self.sentinel).any())
        dirty = torch.stack(flags).cpu().tolist()
        for g, (lo, hi, before, after) in enumerate(self._gaps()):
            off = None
            edge = list(range(lo, min(_up(lo, 4), hi))) + list(range(max(hi // 4 * 4, lo), hi))
            for b in edge[:3]:                                      # the bytes of a word that a tensor ends inside
                if int(self.bytes[b].item()) != self._expected_byte(b):
                    off = b
                    break
            if off is None and dirty[g]:
                w0 = _up(lo, 4) // 4
                off = 4 * (w0 + int((self.buf[w0:hi // 4] != self.sentinel).nonzero()[0].item()))
            if off is None:
                continue
            past = None if before is None else off - (before[1] + before[2])
            ahead = None if after is None else after[1] - off
            if ahead is None or (past is not None and past <= ahead):
                where = f"{past} bytes past the end of carve '{before[0]}' ({before[2]} bytes)"
            else:
                where = f"{ahead} bytes before the start of carve '{after[0]}' ({after[2]} bytes)"
            word = int(self.buf[off // 4].item()) & 0xFFFFFFFF
            return g, off, f"guard {g} was touched at arena byte {off} (word {off // 4} = 0x{word:08X}, sentinel 0x{self.sentinel:08X}): {where}"
        return None

    def assert_guards_intact(self):
        hit = self.first_touched()
        assert hit is None, hit[2]


# -------------------------------------------------------------------------------------------------- the library on the arena
def _workspace_bindings():
    """Every module of the package that binds ``ops._workspace`` under that name (``cleanrl_amd.ops`` defines it,
    ``cleanrl_amd.cnn`` imports it)."""
    import cleanrl_amd.cnn  # noqa: F401  (binds the name on import)
    import cleanrl_amd.ops as ops

    real = ops._workspace
    return real, [m for n, m in sorted(sys.modules.items())
                  if n.startswith("cleanrl_amd") and m is not None and getattr(m, "_workspace", None) is real]


@contextlib.contextmanager
def exact_workspaces(monkeypatch, arena: Arena):
    """Inside the context every ``_workspace(dev, nbytes)`` of the package returns a FRESH carve of exactly ``nbytes`` bytes
    (one byte for a request of 0), sentinel-filled, 16-byte aligned.  Yields the list of sizes requested."""
    _, mods = _workspace_bindings()
    requested: list = []

    def carved(dev, nbytes):
        nbytes = int(nbytes)
        requested.append(nbytes)
        return arena.carve((max(nbytes, 1),), torch.uint8, f"{arena.stage}workspace #{len(requested)} ({nbytes} bytes)", align=WORKSPACE_ALIGN)

    with monkeypatch.context() as m:
        for mod in mods:
            m.setattr(mod, "_workspace", carved)
        yield requested


class _CarvingTorch:
    """``torch`` as a wrapper module sees it inside ``carved_allocations``: ``empty`` / ``empty_like`` / ``zeros`` / ``full`` for the
    arena's device come out of the arena at exactly their size, every other attribute is torch's."""

    def __init__(self, arena: Arena):
        self._arena, self._n = arena, 0

    def __getattr__(self, name):
        return getattr(torch, name)

    def _mine(self, device):
        return device is None and self._arena.device.type == "cpu" or device is not None and torch.device(device).type == self._arena.device.type

    def _carve(self, shape, dtype, what):
        self._n += 1
        return self._arena.carve(shape, dtype or torch.float32, f"{self._arena.stage}wrapper's own #{self._n}: {what}{tuple(shape)}")

    def empty(self, *size, dtype=None, device=None, **kw):
        shape = size[0] if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else size
        if not self._mine(device):
            return torch.empty(*size, dtype=dtype, device=device, **kw)
        return self._carve(shape, dtype, "empty")

    def empty_like(self, t, dtype=None, **kw):
        if t.device.type != self._arena.device.type:
            return torch.empty_like(t, dtype=dtype, **kw)
        return self._carve(t.shape, dtype or t.dtype, "empty_like")

    def zeros(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.zeros(*size, dtype=dtype, device=device, **kw)
        return self.empty(*size, dtype=dtype, device=device).zero_()

    def full(self, size, fill_value, dtype=None, device=None, **kw):
        if not self._mine(device):
            return torch.full(size, fill_value, dtype=dtype, device=device, **kw)
        dtype = dtype or (torch.float32 if isinstance(fill_value, float) else torch.int64)
        return self.empty(size, dtype=dtype, device=device).fill_(fill_value)


@contextlib.contextmanager
def carved_allocations(monkeypatch, arena: Arena, *modules):
    """Inside the context the buffers that the wrappers of ``modules`` allocate themselves (outputs without an ``out=`` parameter,
    ``impala_forward``'s ``saved`` / ``argmax`` / workspace, the backward's auxiliary rows) are carves of exactly the size the
    wrapper asks torch for -- the advertised one -- instead of blocks that the caching allocator rounds up."""
    proxy = _CarvingTorch(arena)
    with monkeypatch.context() as m:
        for mod in modules:
            m.setattr(mod, "torch", proxy)
        yield proxy


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit equality with NaN positions compared as ``offpolicy_cases.same`` does; integer tensors by value."""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.is_floating_point():
        return torch.equal(a, b)
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
