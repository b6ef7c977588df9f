"""The done-masked LSTM sequence scans of ppo_atari_lstm.py (include/mi355ppo.h: mi355ppo_lstm_seq_fwd_f32 / _bwd_f32) through their
host-pointer twins, the ``LSTMSeq`` autograd Function on CPU tensors, the agent's ``MI355PPO_LSTM`` switch and one rollout + update
of the recurrent learner with the scan in place of the per-step loop.  Bars: tests/lstm_cases.py (relative to the reference's own
f32 loop against float64)."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cleanrl_amd import _lib, envs as E, host_ops, ops
from cleanrl_amd.agents import AtariLSTMAgent
from cleanrl_amd.learner_lstm import LSTMPPOLearner
from cleanrl_amd.learner_smoke import default_args
from lstm_cases import DONE_PATTERNS, H, check_lstmseq_autograd, check_scan, make_case
from test_hip_branches_on_fake_ops import _drive, _episode_streams, _frames, _params


@pytest.mark.parametrize("pattern", DONE_PATTERNS)
@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("T", [1, 2, 17, 128])
def test_twins_against_float64_reference_loop(T, B, pattern):
    check_scan(make_case(T, B, pattern), host_ops.lstm_seq_forward, host_ops.lstm_seq_backward)


def test_twin_inference_form_matches_recording_form():
    c = make_case(17, 3, "random20")
    gx = torch.nn.functional.linear(c["x"], c["w_ih"], c["b_ih"] + c["b_hh"])
    a = host_ops.lstm_seq_forward(gx, c["w_hh"], c["h0"], c["c0"], c["done"], record=False)
    b = host_ops.lstm_seq_forward(gx, c["w_hh"], c["h0"], c["c0"], c["done"], record=True)
    assert a[3] is None and b[3].numel() == 7 * 17 * 3 * H
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("pattern", ["random20", "nonbinary"])
@pytest.mark.parametrize("T,B", [(1, 2), (17, 3), (128, 2)])
def test_lstmseq_autograd_on_cpu_against_float64(T, B, pattern):
    check_lstmseq_autograd(make_case(T, B, pattern, seed=1), ops.LSTMSeq.apply, "cpu")


def test_lstm_seq_without_grad_is_the_inference_scan():
    c = make_case(5, 2, "random20")
    w = c["w_hh"].clone().requires_grad_(True)
    gx = torch.nn.functional.linear(c["x"], c["w_ih"], c["b_ih"] + c["b_hh"])
    with torch.no_grad():
        h, hT, cT = ops.lstm_seq(gx, w, c["h0"], c["c0"], c["done"])
    assert h.grad_fn is None
    h2, hT2, cT2 = ops.lstm_seq(gx, w, c["h0"], c["c0"], c["done"])
    assert h2.grad_fn is not None and torch.equal(h, h2.detach()) and torch.equal(cT, cT2.detach())


def _buf(n):
    return (ctypes.c_float * n)()


@pytest.mark.parametrize("suffix", ["_cpu", ""])
def test_refusals(suffix):
    """Null pointers, H != 128, T < 1, B < 1 -> MI355PPO_EINVAL before any work (the device entry points before any HIP call,
    so this holds on a box without a GPU)."""
    lib = _lib.load()
    fwd = getattr(lib, "mi355ppo_lstm_seq_fwd_f32" + suffix)
    bwd = getattr(lib, "mi355ppo_lstm_seq_bwd_f32" + suffix)
    extra = [] if suffix else [None]
    p = ctypes.cast(_buf(16), ctypes.c_void_p)
    ok_f = [p] * 9
    ok_b = [p] * 9
    for i in range(8):                                      # every required pointer of the forward (record is optional)
        args = list(ok_f)
        args[i] = None
        assert fwd(*args, 2, 2, H, *extra) == -1
    for i in (0, 3, 4, 5, 6):                               # dh, record, w_hh, done, dgx (dhT, dcT, dh0, dc0 are optional)
        args = list(ok_b)
        args[i] = None
        assert bwd(*args, 2, 2, H, *extra) == -1
    for T, B, h in ((2, 2, 64), (2, 2, 256), (0, 2, H), (2, 0, H), (-1, 2, H)):
        assert fwd(*ok_f, T, B, h, *extra) == -1
        assert bwd(*ok_b, T, B, h, *extra) == -1
    assert b"must be positive" in lib.mi355ppo_last_error() or b"H=" in lib.mi355ppo_last_error()


def test_python_wrappers_refuse_cpu_tensors_and_bad_shapes():
    c = make_case(2, 2, "none")
    gx = torch.zeros(2, 2, 4 * H)
    with pytest.raises(TypeError):
        ops.lstm_seq_forward(gx, c["w_hh"], c["h0"], c["c0"], c["done"])
    with pytest.raises(ValueError):
        ops.lstm_seq_forward(torch.zeros(2, 2, 4 * H + 1), c["w_hh"], c["h0"], c["c0"], c["done"])


_ENVS = SimpleNamespace(single_observation_space=E.Box(0, 255, (1, 84, 84), np.uint8), single_action_space=E.Discrete(4))


def test_switch(monkeypatch):
    monkeypatch.delenv("MI355PPO_LSTM", raising=False)
    assert AtariLSTMAgent(_ENVS).lstm_backend == "torch"
    monkeypatch.setenv("MI355PPO_LSTM", "torch")
    assert AtariLSTMAgent(_ENVS).lstm_backend == "torch"
    monkeypatch.setenv("MI355PPO_LSTM", "fused")
    assert AtariLSTMAgent(_ENVS).lstm_backend == "fused"
    monkeypatch.setenv("MI355PPO_LSTM", "cudnn")
    with pytest.raises(ValueError, match="MI355PPO_LSTM"):
        AtariLSTMAgent(_ENVS)


def test_fused_agent_matches_the_loop():
    torch.manual_seed(0)
    agent = AtariLSTMAgent(_ENVS)
    T, B = 9, 3
    feats = torch.relu(torch.randn(T * B, 512))
    done = (torch.rand(T * B) < 0.3).float()
    state = (0.3 * torch.randn(1, B, H), torch.randn(1, B, H))
    agent.lstm_backend = "torch"
    h_ref, (hT_ref, cT_ref) = agent.states_from_features(feats, state, done)
    (h_ref.sum() + hT_ref.sum()).backward()
    g_ref = [p.grad.clone() for p in agent.lstm.parameters()]
    agent.zero_grad()
    agent.lstm_backend = "fused"
    h, (hT, cT) = agent.states_from_features(feats, state, done)
    assert h.shape == h_ref.shape and hT.shape == hT_ref.shape == (1, B, H)
    torch.testing.assert_close(h, h_ref, rtol=0, atol=2e-6)
    torch.testing.assert_close(cT, cT_ref, rtol=0, atol=2e-6)
    (h.sum() + hT.sum()).backward()
    for p, g in zip(agent.lstm.parameters(), g_ref):
        assert ((p.grad - g).norm() / g.norm()).item() < 1e-5


def test_learner_rollout_and_update_fused_against_torch_loop():
    """One rollout + one update of LSTMPPOLearner on CPU: the scan (host twins through LSTMSeq) against the reference's
    per-step loop, at the bars of test_hip_branches_on_fake_ops._compare_rollout_and_update."""
    T, N = 6, 4
    args = lambda: default_args(num_steps=T, num_minibatches=2, update_epochs=2)  # noqa: E731

    def make(backend):
        torch.manual_seed(0)
        agent = AtariLSTMAgent(_ENVS)
        agent.lstm_backend = backend
        return LSTMPPOLearner(agent, args(), _ENVS.single_observation_space, _ENVS.single_action_space, N, torch.device("cpu"))

    loop, fused = make("torch"), make("fused")
    rs = np.random.RandomState(1)
    dones, rewards = _episode_streams(rs, T, N)
    frames = _frames(rs, T, N, (1, 84, 84))
    _drive(loop, frames, dones, rewards, 11, False)
    _drive(fused, frames, dones, rewards, 11, False)
    for name in ("actions", "logprobs", "values", "dones", "rewards", "advantages", "returns"):
        assert torch.allclose(getattr(loop, name), getattr(fused, name), rtol=1e-6, atol=1e-6), name
    lr, metrics = 2.5e-4, []
    for L in (loop, fused):
        np.random.seed(3)
        torch.manual_seed(3)
        metrics.append(L.update(lr))
    mh, mf = metrics
    assert mh["num_updates"] == mf["num_updates"]
    for k in ("loss", "policy_loss", "value_loss", "entropy", "approx_kl", "clipfrac"):
        assert abs(mh[k] - mf[k]) <= 1e-5 * max(1.0, abs(mh[k])), (k, mh[k], mf[k])
    d = (_params([loop.agent]) - _params([fused.agent])).abs()
    assert (d <= 2e-5).float().mean().item() >= 1.0 - 1e-5 and d.max().item() <= 2.5 * lr, \
        f"parameters diverge between the loop and the scan: max {d.max().item()}, {(d > 2e-5).sum().item()} above 2e-5"
    assert torch.allclose(loop.next_lstm_state[0], fused.next_lstm_state[0], atol=1e-6)
    assert torch.allclose(loop.next_lstm_state[1], fused.next_lstm_state[1], atol=1e-6)
