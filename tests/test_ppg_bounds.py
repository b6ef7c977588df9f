"""Guard bands around the PPG auxiliary-phase host twins: every tensor of every entry point carved from an arena of sentinel words
(tests/guard_arena.py), outputs pre-filled with the sentinel, once per sentinel.  No guard word may change, and the results must
be the bits of the ordinary run -- a read of memory nobody wrote would show in them.  The device side of the same cases, with
exact workspaces, is tests/test_gpu_ppg.py."""
import pytest
import torch

import guard_arena as GA
import ppg_cases as P
from cleanrl_amd import host_ops

CPU = torch.device("cpu")


def run_guarded(mod, dev, monkeypatch, sentinel):
    arena = GA.Arena(dev, sentinel, words=1 << 24)
    put, out_of = P.carved(arena)
    with GA.exact_workspaces(monkeypatch, arena) as requested:
        out = P.every_entry_point(mod, put, out_of, stage=lambda name: setattr(arena, "stage", name + ": "))
    return out, arena, requested


@pytest.mark.parametrize("sentinel", GA.SENTINELS, ids=[f"0x{s:08X}" for s in GA.SENTINELS])
def test_twins_stay_inside_their_tensors_and_read_only_what_was_written(sentinel, monkeypatch):
    ref = P.every_entry_point(host_ops, *P.plain(CPU))
    out, arena, _ = run_guarded(host_ops, CPU, monkeypatch, sentinel)
    arena.assert_guards_intact()
    assert set(out) == set(ref) and len(out) >= 60
    for k, v in ref.items():
        assert GA.same_bits(out[k], v), f"sentinel 0x{sentinel:08X}: output '{k}' differs from the ordinary run"
