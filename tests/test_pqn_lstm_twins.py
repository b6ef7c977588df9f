"""The recurrent PQN tail on the host twins (csrc/pqn_lstm.hip's row functions compiled for the host; no GPU): argument checks of
the four entry points, the act twin against the scan twin (bits) and the reference's float64 step (bar rule of lstm_cases),
e-greedy equal to the reference's on the twin's own q, the TD twin against float64 autograd (bar rule of pqn_cases)."""
import ctypes

import pytest
import torch

import lstm_cases as L
import pqn_cases as P
import pqn_lstm_cases as C
from cleanrl_amd import _lib
from cleanrl_amd import host_ops as H


def test_argument_checks_return_their_codes_before_any_launch():
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for name, tail in (("mi355ppo_pqn_lstm_act_f32", (None,)), ("mi355ppo_pqn_lstm_act_f32_cpu", ())):
        act = getattr(lib, name)
        full = lambda N=2, Hh=128, A=4, gx=p, h_out=p, c_out=p, q=p, a=p, v=p, rnd=p: act(  # noqa: E731
            gx, p, p, p, p, p, p, rnd, p, 0.1, h_out, c_out, q, a, v, p, p, N, Hh, A, *tail)
        assert full(gx=None) == -1 and b"null" in lib.mi355ppo_last_error()
        assert full(Hh=64) == -1 and b"H=64" in lib.mi355ppo_last_error()
        assert full(A=0) == -1 and full(A=19) == -1 and b"1 <= A <= 18" in lib.mi355ppo_last_error()
        assert full(N=0) == -1
        assert full(c_out=None) == -1                       # h_out without c_out
        assert full(v=None) == -1 and full(rnd=None) == -1  # actions_out without values_out / without the draws
        assert act(p, p, p, p, p, p, p, None, None, 0.1, None, None, None, None, None, None, None, 2, 128, 4, *tail) == -1   # no output
    for name, tail in (("mi355ppo_pqn_lstm_td_fwd_bwd_f32", (p, 1 << 20, None)), ("mi355ppo_pqn_lstm_td_fwd_bwd_f32_cpu", ())):
        td = getattr(lib, name)
        full = lambda M=2, Hh=128, A=4, B=8, h=p, dwq=p: td(h, p, p, p, p, p, p, dwq, p, p, M, Hh, A, B, *tail)  # noqa: E731
        assert full(h=None) == -1 and full(dwq=None) == -1 and b"null" in lib.mi355ppo_last_error()
        assert full(Hh=256) == -1 and b"H=256" in lib.mi355ppo_last_error()
        assert full(A=0) == -1 and full(A=19) == -1
        assert full(M=0) == -1 and full(B=0) == -1
    td = lib.mi355ppo_pqn_lstm_td_fwd_bwd_f32
    need = lib.mi355ppo_pqn_lstm_td_workspace_bytes(300, 4)
    assert need == (2 * 320 + 2 * (4 * 128 + 4)) * 4                   # old | sq padded to 64 rows, two 256-row partials of (dwq | dbq)
    assert lib.mi355ppo_pqn_lstm_td_workspace_bytes(0, 4) == 0
    assert td(p, p, p, p, p, p, p, p, p, p, 300, 128, 4, 600, None, 0, None) == -4
    assert td(p, p, p, p, p, p, p, p, p, p, 300, 128, 4, 600, p, need - 4, None) == -4 and b"workspace" in lib.mi355ppo_last_error()


def test_wrappers_are_reachable_through_ops_twins():
    from cleanrl_amd import ops

    g = ops.twins(torch.device("cpu"))
    assert g.pqn_lstm_act is H.pqn_lstm_act and g.pqn_lstm_td_fwd_bwd is H.pqn_lstm_td_fwd_bwd
    x = torch.zeros(2, 512)
    with pytest.raises(TypeError, match="CUDA/HIP"):
        ops.pqn_lstm_act(x, torch.zeros(512, 128), x[:, :128], x[:, :128], x[:, 0], torch.zeros(4, 128), torch.zeros(4), q_out=torch.zeros(2, 4))
    with pytest.raises(TypeError, match="CUDA/HIP"):
        ops.pqn_lstm_td_fwd_bwd(x[:, :128], torch.zeros(2, dtype=torch.int64), x[:, 0], x[:, 0], torch.zeros(4, 128), torch.zeros(4),
                                torch.zeros(4, 128), torch.zeros(4))


@pytest.mark.parametrize("A", C.ACT_A)
@pytest.mark.parametrize("N", C.ACT_N)
@pytest.mark.parametrize("pattern", L.DONE_PATTERNS)
def test_act_twin(pattern, N, A):
    c = C.make_act_case(N, A, pattern, seed=1)
    out = C.run_act(H, c)
    # the state: the scan twin's bits at T = 1
    _, hT, cT, _ = H.lstm_seq_forward(c["gx"][None].contiguous(), c["w_hh"], c["h0"], c["c0"], c["done"])
    assert torch.equal(out["h"], hT) and torch.equal(out["c"], cT)
    # state and q against the reference's step in float64, at the bar of the f32 reference
    r64, r32 = C.reference_act(c, torch.float64), C.reference_act(c, torch.float32)
    for name, got, a64, a32 in zip(("h", "c", "q"), (out["h"], out["c"], out["q"]), r64, r32):
        L.assert_bar(name, L.max_err(got, a64), L.max_err(a32, a64), L.FWD_FLOOR)
    # e-greedy on the twin's own q, at several epsilons, and with NaN / inf planted through the bias
    C.check_egreedy(out, c, 0.3)
    for eps in (0.0, 1.0, float(c["u"][0])):
        C.check_egreedy(C.run_act(H, c, eps=eps), c, eps)
    planted = C.run_act(H, c, bq=C.planted_bias(c))
    assert planted["q"].isnan().any()
    C.check_egreedy(planted, c, 0.3)
    # the bootstrap form writes q only (the state it read is untouched); aliased state in / out equals the separate buffers
    boot = C.run_act(H, c, bootstrap=True)
    assert torch.equal(boot["q"], out["q"]) and torch.equal(boot["h_in"], c["h0"]) and torch.equal(boot["c_in"], c["c0"])
    al = C.run_act(H, c, alias=True)
    assert all(torch.equal(al[k], out[k]) for k in out)


TD_CASES = [(1, None), (256, None), (256, (32, 16, [3, 0, 9, 5, 1, 15, 2, 8])), (4096 + 3, None)]


@pytest.mark.parametrize("M,envwise", TD_CASES)
def test_td_twin(M, envwise):
    assert {m for m, _ in TD_CASES} == set(C.TD_M)
    A = 6
    c = C.make_td_case(M, A, seed=2, envwise=envwise, actions=(0, 2, 3))
    got = C.run_td(H, c)
    r64, r32 = C.reference_td_head(c, torch.float64), C.reference_td_head(c, torch.float32)
    for k in ("loss", "mean_old", "dh", "dwq", "dbq"):             # mean_old: old enters the outputs through its mean and the loss
        ok, err, own = P.within_bar(got[k], r64[k], r32[k])
        assert ok, (k, err, own)
    never = [1, 4, 5]
    assert int(torch.count_nonzero(got["dwq"][never])) == 0 and int(torch.count_nonzero(got["dbq"][never])) == 0
    assert int(torch.count_nonzero(got["dwq"])) > 0
    # a permutation of the rows permutes dh's rows bit for bit (a row depends on the others only through 2 / M)
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(M))
    assert torch.equal(C.run_td(H, c, perm=perm)["dh"], got["dh"][perm])
    # every action in range: the clamp leaves them alone; out-of-range ones take the nearest action
    c2 = dict(c, b_actions=c["b_actions"].clone())
    c2["b_actions"][c["mb"][0]] = 99.0
    c3 = dict(c, b_actions=c2["b_actions"].clone())
    c3["b_actions"][c["mb"][0]] = float(A - 1)
    assert all(torch.equal(a, b) for a, b in zip(C.run_td(H, c2).values(), C.run_td(H, c3).values()))
