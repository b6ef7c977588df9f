"""The done-masked LSTM sequence scans (csrc/lstm.hip) on the MI355X: against float64 autograd of the reference's loop at the bars of
tests/lstm_cases.py, against their host twins, deterministic and batch-invariant, the T = 1 forward under graph capture, the
``LSTMSeq`` gradients, and the recurrent learner / script with ``MI355PPO_LSTM=fused``."""
import pytest
import torch

from cleanrl_amd import host_ops, ops
from lstm_cases import (DONE_PATTERNS, FWD_FLOOR, GRAD_FLOOR, H, assert_bar, check_lstmseq_autograd, check_scan, gx_of, make_case, max_err,
                        reference_loop)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(c):
    return {k: v.to(DEV) for k, v in c.items()}


@pytest.mark.parametrize("pattern", DONE_PATTERNS)
@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("T", [1, 2, 17, 128])
def test_device_scan_against_float64(T, B, pattern):
    check_scan(make_case(T, B, pattern), ops.lstm_seq_forward, ops.lstm_seq_backward, DEV)


@pytest.mark.parametrize("B", [64, 257, 1024])
def test_device_scan_against_float64_at_update_sizes(B):
    check_scan(make_case(128, B, "random20"), ops.lstm_seq_forward, ops.lstm_seq_backward, DEV)


def _run(c, gx=None):
    gx = (gx_of(c) if gx is None else gx).contiguous()
    h, hT, cT, rec = ops.lstm_seq_forward(gx.to(DEV), c["w_hh"].to(DEV), c["h0"].to(DEV), c["c0"].to(DEV), c["done"].to(DEV), record=True)
    dgx, dh0, dc0 = ops.lstm_seq_backward(c["dh"].to(DEV), c["dhT"].to(DEV), c["dcT"].to(DEV), rec, c["w_hh"].to(DEV), c["done"].to(DEV))
    torch.cuda.synchronize()
    return [t.cpu() for t in (h, hT, cT, rec, dgx, dh0, dc0)]


def test_deterministic_and_batch_invariant():
    """Two calls give the same bits; each env of a B = 257 batch (two envs per workgroup) is bit-equal to the same env run
    alone (one per workgroup) -- and so to any other B."""
    T, B = 128, 257
    c = make_case(T, B, "random20")
    a, b = _run(c), _run(c)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    h, hT, cT, rec, dgx, dh0, dc0 = a
    gx = gx_of(c)                   # the scan's input sliced, not recomputed: the host GEMM forming gx is not batch-invariant
    for env in (0, 1, 128, 255, 256):
        one = {k: (v[:, env:env + 1] if k in ("x", "done", "dh") else v[env:env + 1] if k in ("h0", "c0", "dhT", "dcT") else v)
               for k, v in c.items()}
        h1, hT1, cT1, _, dgx1, dh01, dc01 = _run(one, gx[:, env:env + 1])
        assert torch.equal(h1[:, 0], h[:, env]) and torch.equal(hT1[0], hT[env]) and torch.equal(cT1[0], cT[env])
        assert torch.equal(dgx1[:, 0], dgx[:, env]) and torch.equal(dh01[0], dh0[env]) and torch.equal(dc01[0], dc0[env])


@pytest.mark.parametrize("T,B,pattern", [(1, 3, "random20"), (17, 8, "nonbinary"), (128, 8, "random20")])
def test_device_against_host_twin(T, B, pattern):
    c = make_case(T, B, pattern)
    dev = _run(c)
    gx = gx_of(c).contiguous()
    h, hT, cT, rec = host_ops.lstm_seq_forward(gx, c["w_hh"], c["h0"], c["c0"], c["done"], record=True)
    dgx, dh0, dc0 = host_ops.lstm_seq_backward(c["dh"], c["dhT"], c["dcT"], rec, c["w_hh"], c["done"])
    (h64, hT64, cT64), g64 = reference_loop(c, torch.float64, on_gx=True)
    (h32, hT32, cT32), g32 = reference_loop(c, torch.float32, on_gx=True)
    for name, d, t, r32, r64, floor in (("h", dev[0], h, h32, h64, FWD_FLOOR), ("hT", dev[1], hT, hT32, hT64, FWD_FLOOR),
                                        ("cT", dev[2], cT, cT32, cT64, FWD_FLOOR), ("dgx", dev[4], dgx, g32["gx"], g64["gx"], GRAD_FLOOR),
                                        ("dh0", dev[5], dh0, g32["h0"], g64["h0"], GRAD_FLOOR),
                                        ("dc0", dev[6], dc0, g32["c0"], g64["c0"], GRAD_FLOOR)):
        assert_bar(f"{name} device vs host twin", max_err(d, t.double()), max_err(r32, r64), floor)


@pytest.mark.parametrize("T,B,pattern", [(1, 2, "random20"), (128, 2, "random20"), (128, 64, "nonbinary")])
def test_lstmseq_gradients_on_device_against_float64(T, B, pattern):
    check_lstmseq_autograd(make_case(T, B, pattern, seed=1), ops.LSTMSeq.apply, DEV)


def test_t1_forward_graph_capture_replays_bit_identical():
    c = _dev(make_case(1, 8, "random20"))
    gx = gx_of(c).contiguous()
    eager = ops.lstm_seq_forward(gx, c["w_hh"], c["h0"], c["c0"], c["done"])[:3]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.lstm_seq_forward(gx, c["w_hh"], c["h0"], c["c0"], c["done"])
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.lstm_seq_forward(gx, c["w_hh"], c["h0"], c["c0"], c["done"])[:3]
    for _ in range(2):
        g.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, eager):
            assert torch.equal(a, b)


def _count_scans(monkeypatch):
    calls = []
    real = ops.lstm_seq

    def counting(*a):
        calls.append(tuple(a[0].shape))
        return real(*a)

    monkeypatch.setattr(ops, "lstm_seq", counting)
    return calls


def test_lstm_golden_teacher_forced_with_fused_scan(monkeypatch):
    """The lstm_T8_N4 golden (the reference iteration's own outputs), teacher-forced exactly as in test_zz_gpu_new_scripts.py and
    at its tolerances, with the agent on the scan."""
    import test_zz_gpu_new_scripts as Z

    monkeypatch.setenv("MI355PPO_LSTM", "fused")
    calls = _count_scans(monkeypatch)
    Z.test_lstm_hip_path_teacher_forced_against_reference_iteration()
    assert (1, 4, 4 * H) in calls and (8, 2, 4 * H) in calls       # rollout / bootstrap steps and the update's minibatches


def test_ppo_atari_lstm_script_runs_with_fused_scan(monkeypatch):
    import test_zz_gpu_new_scripts as Z

    monkeypatch.setenv("MI355PPO_LSTM", "fused")
    calls = _count_scans(monkeypatch)
    Z.test_ppo_atari_lstm_script_runs_on_gpu()
    assert (1, 8, 4 * H) in calls and (16, 2, 4 * H) in calls
