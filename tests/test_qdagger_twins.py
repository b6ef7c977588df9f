"""The QDagger head's host twins (mi355ppo_qdagger_head_*_cpu, the device kernels' arithmetic compiled for the host) against the
reference's own lines: argmax and td_target bit for bit, the loss scalars and gradients against float64 autograd, the structure of
the dense dq, and the C ABI's refusals.  No GPU."""
import ctypes

import pytest
import torch

import qdagger_cases as Q
from cleanrl_amd import _lib, ops
from cleanrl_amd import host_ops as H

CPU = torch.device("cpu")


@pytest.mark.parametrize("M,n", Q.HEAD_GRID)
@pytest.mark.parametrize("T", Q.TEMPS)
@pytest.mark.parametrize("coeff", Q.COEFFS)
def test_head_twin_against_the_reference_lines(M, n, T, coeff):
    c = Q.make_head_case(M, n, temperature=T, coeff=coeff)
    got = Q.run_heads(H, c, CPU)
    r64, r32 = Q.reference_head(c, torch.float64), Q.reference_head(c, torch.float32)
    # bit for bit: the greedy action, the target network's values and td_target (d = 0 and d = 1 rows are in every case with M >= 2)
    assert torch.equal(got["act"], r32["act"])
    for k in ("q", "target_q"):
        assert Q.within_bar(got[k], r64[k], r32[k])[0]
    mx = got["target_q"].max(dim=1).values
    assert torch.equal(got["td_target"], c.rewards + c.gamma * mx * (1 - c.dones))
    for k in ("scalars", "dh", "dw", "db"):
        ok, err, own = Q.within_bar(got[k], r64[k], r32[k])
        assert ok, (k, err, own)
    if coeff == 0.0 and n > 2:                                     # the last action is never taken: nothing but the KL reaches it
        assert not got["dw"][n - 1].any() and not got["db"][n - 1].any()
        untaken = [j for j in range(n) if not (c.actions == j).any()]
        assert all(not got["dw"][j].any() for j in untaken)


def test_argmax_ties_and_nan_follow_torch():
    c = Q.make_head_case(5, 6, tie=True)
    c.h[2, 7] = float("nan")                                        # a NaN row: every q is NaN, torch.argmax returns index 0
    c.b[4] = float("nan")                                           # and NaN is the maximum of the other rows
    got = Q.run_heads(H, c, CPU)
    want = torch.argmax(torch.nn.functional.linear(c.h, c.w, c.b), dim=1)
    assert torch.equal(got["act"], want)
    assert got["act"][2] == 0 and (got["act"][[0, 1, 3, 4]] == 4).all()
    c = Q.make_head_case(5, 6, tie=True)                            # exact ties go to the lowest index
    got = Q.run_heads(H, c, CPU)
    assert torch.equal(got["act"], torch.argmax(torch.nn.functional.linear(c.h, c.w, c.b), dim=1)) and not (got["act"] == 1).any()
    assert torch.equal(got["q"][:, 0], got["q"][:, 1])


def test_each_row_has_its_own_td_part_over_m_and_its_own_kl_part():
    """dq[r] = (2 / M) (q - y) e_a + (c / T) (softmax(s) - softmax(t)): the TD part of the row alone scales with 1 / M, the KL part does
    not (the KL is summed over the batch).  Row r alone at coeff 0 gives the TD part x M, at coeff c the TD part x M plus the KL part."""
    c = Q.make_head_case(32, 6, temperature=0.7, coeff=0.37)
    full = Q.run_heads(H, c, CPU)
    for r in (0, 1, 31):
        one = Q.make_head_case(1, 6, temperature=0.7, coeff=0.37)
        for k in ("h", "h_next", "teacher_q", "actions", "rewards", "dones"):
            setattr(one, k, getattr(c, k)[r:r + 1].clone())
        for k in ("w", "b", "wt", "bt"):
            setattr(one, k, getattr(c, k))
        both = Q.run_heads(H, one, CPU)["dh"][0].double()
        one.coeff = 0.0
        td = Q.run_heads(H, one, CPU)["dh"][0].double()
        want = td / 32 + (both - td)
        scale = max(both.abs().max().item(), td.abs().max().item())
        # f32 sums of <= 6 products per element on both sides: a few ulps of the larger operand
        assert (full["dh"][r].double() - want).abs().max().item() <= 8 * 2.0 ** -24 * scale
        assert torch.equal(full["td_target"][r], Q.run_heads(H, one, CPU)["td_target"][0])


def test_out_of_limit_sizes_are_refused_and_leave_the_outputs_untouched():
    lib = _lib.load()
    c = Q.make_head_case(2, 6)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    wide = torch.zeros((19, 256))
    dh, dw, db, sc = torch.full((2, 256), 7.0), torch.full((19, 256), 7.0), torch.full((19,), 7.0), torch.full((4,), 7.0)
    act = torch.full((2,), 9, dtype=torch.int64)
    nets = [ptr(c.h), ptr(c.h_next), ptr(wide), ptr(wide), ptr(wide), ptr(wide), ptr(wide)]
    batch = [ptr(c.actions), ptr(c.rewards), ptr(c.dones)]
    outs = [ptr(dh), ptr(dw), ptr(db), ptr(sc), None, None]
    for M, hidden, n in ((2, 512, 6), (2, 256, 1), (2, 256, 19), (0, 256, 6), (1025, 256, 6)):
        assert lib.mi355ppo_qdagger_head_fwd_bwd_f32_cpu(*nets, *batch, 0.99, 1.0, 1.0, *outs, M, hidden, n) == -1
        assert lib.mi355ppo_qdagger_head_fwd_bwd_f32(*nets, *batch, 0.99, 1.0, 1.0, *outs, M, hidden, n, ptr(wide), 1 << 30, None) == -1
        assert lib.mi355ppo_qdagger_head_act_f32_cpu(ptr(c.h), ptr(wide), ptr(wide), ptr(act), None, M, hidden, n) == -1
        assert lib.mi355ppo_qdagger_head_act_f32(ptr(c.h), ptr(wide), ptr(wide), ptr(act), None, M, hidden, n, ptr(wide), 1 << 30, None) == -1
        assert lib.mi355ppo_qdagger_head_workspace_bytes(M, n) == 0 or hidden != 256
        assert ops.qdagger_head_limits_ok(n, M, hidden) is False
    assert lib.mi355ppo_qdagger_head_fwd_bwd_f32_cpu(*nets, *batch, 0.99, 0.0, 1.0, *outs, 2, 256, 6) == -1      # temperature
    assert b"temperature" in lib.mi355ppo_last_error()
    assert ops.qdagger_head_limits_ok(6, 32) and ops.qdagger_head_limits_ok(18, 1024) and ops.qdagger_head_limits_ok(2, 1)
    assert (dh == 7.0).all() and (dw == 7.0).all() and (db == 7.0).all() and (sc == 7.0).all() and (act == 9).all()
