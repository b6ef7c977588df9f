"""The host twin of kernel Q1's ReLU forward (mi355ppo_cnn_conv1q1_fwd_cpu, csrc/ma_atari_twins.hip) -- conv1 of ppo_atari_lstm.py's network
on one uint8 frame -- against float64, against the pre-activation twin, its mask words and amax record; the MI355PPO_LSTM_TRUNK switch; the
new C ABI symbols.  Runs without a GPU.

The one-frame family of ``cnn.NatureTrunkFn`` is not run here: layers 2 / 3 and the FC layer have no host twins (the node runs on device
tensors only), so its arithmetic is covered on the GPU (tests/test_gpu_lstm_trunk.py) and its dispatch on CPU stand-ins
(tests/test_hip_branches_on_fake_ops.py)."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pqn_trunk_cases as PC
from cleanrl_amd import _lib, envs as E, host_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mi355ppo_cnn_conv1q1_fwd_bits", "mi355ppo_cnn_conv1q1_fwd_amax", "mi355ppo_cnn_conv1q1_fwd_cpu"]
CASES = [(1, None), (3, [3, 0, 3]), (70, None)]


def case(stored, seed=0):
    g = torch.Generator().manual_seed(8000 + seed)
    frames = torch.randint(0, 256, (stored, 84, 84), generator=g, dtype=torch.uint8)
    return frames, 0.05 * torch.randn((32, 1, 8, 8), generator=g), 0.5 * torch.randn(32, generator=g)


_RUNS = {}


def run(images, inds):
    """(frames, W, b, inds, out, bits, record) of one case, computed once and shared (nobody writes to it)."""
    key = (images, None if inds is None else tuple(inds))
    if key not in _RUNS:
        frames, W, b = case(images if inds is None else 4, seed=images)
        ii = None if inds is None else torch.tensor(inds, dtype=torch.int64)
        bits, rec = torch.full((images * 400,), -1, dtype=torch.int32), torch.zeros(PC.AMAX_WORDS, dtype=torch.int32)
        out = host_ops.conv1q1_fwd(frames, host_ops.conv1q1_pack(W), b, ii, bits=bits, amax=rec)
        _RUNS[key] = (frames, W, b, ii, out, bits, rec)
    return _RUNS[key]


@pytest.mark.parametrize("images,inds", CASES)
def test_forward_twin_is_within_the_bar_of_float64(images, inds):
    frames, W, b, ii, out, _, _ = run(images, inds)
    x = (frames if ii is None else frames[ii]).unsqueeze(1)
    ref64 = F.conv2d(x.double() / 255.0, W.double(), b.double(), stride=4).relu().permute(0, 2, 3, 1)
    ref32 = F.conv2d(x.float() / 255.0, W, b, stride=4).relu().permute(0, 2, 3, 1)
    assert out.shape == (images, 20, 20, 32)
    PC.bar(f"a1 ({images} images)", out, ref64, ref32)
    assert (out == 0).any() and (out > 0).any() and not (out < 0).any()
    if inds is not None:
        assert torch.equal(out[0], out[2])


@pytest.mark.parametrize("images,inds", CASES)
def test_forward_twin_is_the_clamped_pre_activation_with_its_bits_and_amax(images, inds):
    frames, W, b, ii, out, bits, rec = run(images, inds)
    pre = host_ops.conv1q1_pre_fwd(frames, host_ops.conv1q1_pack(W), b, ii)
    assert torch.equal(out, pre.clamp_min(0))
    assert torch.equal(bits, PC.packed_bits(out))
    assert PC.amax_value(rec) == out.max().item() and int((rec.view(-1)[1:] != 0).sum()) == 0
    assert torch.equal(host_ops.conv1q1_fwd(frames, host_ops.conv1q1_pack(W), b, ii), out)             # neither bits nor a record


def test_the_record_is_folded_not_overwritten_and_bad_arguments_are_refused():
    frames, W, b, _, out, _, _ = run(1, None)
    pack = host_ops.conv1q1_pack(W)
    rec = torch.zeros(PC.AMAX_WORDS, dtype=torch.int32)
    rec[0] = torch.tensor(1e6).view(torch.int32)
    host_ops.conv1q1_fwd(frames, pack, b, amax=rec)
    assert PC.amax_value(rec) == 1e6
    with pytest.raises(ValueError, match="uint8 frames"):
        host_ops.conv1q1_fwd(torch.zeros((2, 84, 84, 4), dtype=torch.uint8), pack, b)
    with pytest.raises(ValueError, match="out of range"):
        host_ops.conv1q1_fwd(frames, pack, b, torch.tensor([1]))
    with pytest.raises(ValueError, match="bits"):
        host_ops.conv1q1_fwd(frames, pack, b, bits=torch.zeros(399, dtype=torch.int32))
    with pytest.raises(TypeError, match="amax"):
        host_ops.conv1q1_fwd(frames, pack, b, amax=torch.zeros(PC.AMAX_WORDS))


# ------------------------------------------------------------------------------------------------------------ the switch
def test_the_trunk_switch_defaults_to_torch_and_refuses_other_values(monkeypatch):
    from cleanrl_amd.agents import lstm_trunk_backend_from_env

    monkeypatch.delenv("MI355PPO_LSTM_TRUNK", raising=False)
    assert lstm_trunk_backend_from_env() == "torch"
    for v in ("torch", "fused"):
        monkeypatch.setenv("MI355PPO_LSTM_TRUNK", v)
        assert lstm_trunk_backend_from_env() == v
    monkeypatch.setenv("MI355PPO_LSTM_TRUNK", "miopen")
    with pytest.raises(ValueError, match="MI355PPO_LSTM_TRUNK='miopen'"):
        lstm_trunk_backend_from_env()


def _cpu_learner():
    from cleanrl_amd.agents import AtariLSTMAgent
    from cleanrl_amd.learner_lstm import LSTMPPOLearner
    from cleanrl_amd.learner_smoke import default_args

    envs = SimpleNamespace(single_observation_space=E.Box(0, 255, (1, 84, 84), np.uint8), single_action_space=E.Discrete(4))
    args = default_args(num_steps=4, num_minibatches=2, update_epochs=1)
    return LSTMPPOLearner(AtariLSTMAgent(envs), args, envs.single_observation_space, envs.single_action_space, 2, torch.device("cpu"))


def test_the_recurrent_learner_defaults_to_the_torch_trunk_and_refuses_the_fused_one_on_the_cpu(monkeypatch):
    monkeypatch.delenv("MI355PPO_LSTM_TRUNK", raising=False)
    L = _cpu_learner()
    assert L.trunk == "torch" and not L.fused_trunk and not L.fused_cnn and L.agent._trunk is None
    monkeypatch.setenv("MI355PPO_LSTM_TRUNK", "fused")
    with pytest.raises(ValueError, match="HIP kernels only"):
        _cpu_learner()
    monkeypatch.setenv("MI355PPO_LSTM_TRUNK", "both")
    with pytest.raises(ValueError, match="expected torch or fused"):
        _cpu_learner()


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_c_abi_declares_binds_and_exports_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "mi355ppo.h")).read()
    declared = set(re.findall(r"MI355PPO_API\s+[\w\s\*]+?\b(mi355ppo_\w+)\s*\(", header))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and getattr(lib, name) is not None, name
    import ctypes

    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.mi355ppo_cnn_conv1q1_fwd_bits(p, None, p, p, p, None, 1, None) == -1              # refusals precede any launch
    assert b"null" in lib.mi355ppo_last_error()
    assert lib.mi355ppo_cnn_conv1q1_fwd_amax(p, None, p, p, p, None, 1, None, None) == -1
    assert b"amax record" in lib.mi355ppo_last_error()
    assert lib.mi355ppo_cnn_conv1q1_fwd_cpu(p, None, p, p, p, None, None, 0) == -1
