"""The guard-band cases (tests/bounds_cases.py) on the host twins -- C code that can overrun like a kernel -- with every tensor
carved from a CPU arena, and the self-tests of the arena itself (tests/guard_arena.py)."""
import pytest
import torch

import bounds_cases as BC
import guard_arena as GA
from cleanrl_amd import host_ops

CPU = torch.device("cpu")


@pytest.mark.parametrize("case", BC.TWIN_CASES, ids=[c.name for c in BC.TWIN_CASES])
def test_twin_stays_inside_its_tensors_and_reads_only_what_was_written(case, monkeypatch):
    BC.check(case, host_ops, CPU, monkeypatch)


def test_case_names_are_unique_and_every_family_is_in_the_table():
    names = [c.name for c in BC.CASES]
    assert len(set(names)) == len(names)
    for family in ("offpolicy", "sac", "pqn ", "pqn_lstm_act", "pqn_lstm_td", "optim", "lstm", "trxl", "impala ", "impala_maxpool", "gae", "categorical",
                   "normal", "loss_categorical", "loss_normal", "obs", "mlp", "synth N", "synth_atari", "cnn conv_wgrad", "cnn fc/heads", "cnn nature"):
        assert any(n.startswith(family) for n in names), family


# ---------------------------------------------------------------------------------------------------- the arena itself
@pytest.mark.parametrize("sentinel", GA.SENTINELS)
def test_carves_are_aligned_end_at_their_last_element_and_keep_their_guards(sentinel):
    a = GA.Arena(CPU, sentinel, words=1 << 19)
    shapes = [((3, 5), torch.float32), ((7,), torch.uint8), ((1,), torch.int64), ((2, 3), torch.uint8)]
    ts = [a.carve(s, d, f"t{i}") for i, (s, d) in enumerate(shapes)]
    ws = a.carve((33,), torch.uint8, "ws", align=GA.WORKSPACE_ALIGN)
    base, prev_end = a.buf.data_ptr(), a.buf.data_ptr()
    for t, (s, d) in zip(ts, shapes):
        assert tuple(t.shape) == s and t.dtype == d and t.is_contiguous()
        assert t.data_ptr() % GA.ALIGN == 0
        assert t.data_ptr() - prev_end >= 4 * GA.GUARD_WORDS                      # the guard in front of it
        prev_end = t.data_ptr() + t.numel() * t.element_size()
    assert ws.data_ptr() % GA.WORKSPACE_ALIGN == 0 and ws.data_ptr() - prev_end >= 4 * GA.GUARD_WORDS
    assert base + 4 * a.buf.numel() - (ws.data_ptr() + 33) >= 4 * GA.GUARD_WORDS   # the last guard runs to the arena's end
    # a fresh carve holds the sentinel; the element after a tensor's last one is the sentinel too (here: seen as bytes)
    assert ts[0].view(torch.int32).eq(sentinel).all()
    end = ts[1].data_ptr() - base + 7
    assert int(a.bytes[end]) == (sentinel >> (8 * (end % 4))) & 0xFF
    x = a.input(torch.arange(6, dtype=torch.float32).reshape(2, 3), "x")
    assert torch.equal(x, torch.arange(6, dtype=torch.float32).reshape(2, 3))
    after = (x.data_ptr() - base) // 4 + 6
    assert int(a.buf[after]) == sentinel
    for t in ts + [ws, x]:                                                     # writing every element of every carve touches no guard
        t.fill_(1)
    a.assert_guards_intact()


def test_a_word_written_into_each_guard_is_reported_with_its_carve():
    a = GA.Arena(CPU, GA.NAN_SENTINEL, words=1 << 19)
    t0, t1 = a.carve((5,), torch.float32, "first"), a.carve((3,), torch.uint8, "second")
    base = a.buf.data_ptr()
    s0, s1 = (t0.data_ptr() - base) // 4, t1.data_ptr() - base
    spots = [(s0 - 1, "4 bytes before the start of carve 'first'", 0), (s0 + 5, "0 bytes past the end of carve 'first'", 1),
             (s0 + 5 + 100, "400 bytes past the end of carve 'first'", 1), (s1 // 4 - 2, "8 bytes before the start of carve 'second'", 1),
             (s1 // 4 + 1, "1 bytes past the end of carve 'second'", 2), (a.buf.numel() - 1, "past the end of carve 'second'", 2)]
    for word, text, guard in spots:
        a.buf[word] = 0
        hit = a.first_touched()
        assert hit is not None and hit[0] == guard and hit[1] == 4 * word and text in hit[2], (word, hit)
        with pytest.raises(AssertionError, match="guard"):
            a.assert_guards_intact()
        a.buf[word] = GA.NAN_SENTINEL
        a.assert_guards_intact()
    # the byte right behind a tensor that ends inside a word
    a.bytes[s1 + 3] = 0
    hit = a.first_touched()
    assert hit[0] == 2 and hit[1] == s1 + 3 and "0 bytes past the end of carve 'second'" in hit[2]


def test_an_arena_that_is_too_small_refuses_the_carve():
    a = GA.Arena(CPU, GA.FINITE_SENTINEL, words=3 * GA.GUARD_WORDS)
    a.carve((GA.GUARD_WORDS // 2,), torch.float32)
    with pytest.raises(MemoryError):
        a.carve((GA.GUARD_WORDS,), torch.float32)


def test_exact_workspaces_rebinds_every_binding_and_restores_it(monkeypatch):
    from cleanrl_amd import cnn, ops

    real = ops._workspace
    assert cnn._workspace is real
    a = GA.Arena(CPU, GA.NAN_SENTINEL, words=1 << 19)
    with GA.exact_workspaces(monkeypatch, a) as requested:
        assert ops._workspace is not real and cnn._workspace is ops._workspace
        ws = ops._workspace(CPU, 100)
        w0 = cnn._workspace(CPU, 0)
        assert ws.numel() == 100 and ws.dtype == torch.uint8 and ws.data_ptr() % GA.WORKSPACE_ALIGN == 0 and w0.numel() == 1
        assert ws.data_ptr() != w0.data_ptr() and requested == [100, 0]
        assert ws.eq(GA.NAN_SENTINEL & 0xFF).sum() == 25                          # sentinel-filled (0xAD, once per word)
    assert ops._workspace is real and cnn._workspace is real
    with GA.carved_allocations(monkeypatch, a, host_ops) as proxy:
        assert host_ops.torch is proxy
        t = host_ops.torch.empty((2, 3))
        z = host_ops.torch.zeros(4, dtype=torch.int32)
        assert t.shape == (2, 3) and a.buf.data_ptr() < t.data_ptr() < a.buf.data_ptr() + 4 * a.buf.numel() and not z.any()
        assert host_ops.torch.float32 is torch.float32
    assert host_ops.torch is torch
    a.assert_guards_intact()
