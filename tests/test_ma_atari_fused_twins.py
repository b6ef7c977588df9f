"""MI355PPO_MA_ATARI=fused without a GPU: the host twins of the new entry points (csrc/ma_atari_twins.hip, csrc/ma_atari_rows.h) against
numpy, and the plumbing -- C ABI, the switch, the learner's flag check.

The twins of kernel Q's pack and forward (``mi355ppo_cnn_conv1q_pack_cpu`` / ``mi355ppo_cnn_conv1q_fwd_cpu``) are new with this
backend: they are what "the existing pack / forward" means on a box without a device, and the GPU tests hold the kernels to them bit
for bit (tests/test_gpu_ma_atari_fused.py)."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cleanrl_amd import _lib
from cleanrl_amd import envs as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACK_BYTES = 33408
NEW = ["mi355ppo_ma_atari_split_u8", "mi355ppo_ma_atari_conv1_pack_f32", "mi355ppo_ma_atari_conv1_fwd_bits", "mi355ppo_ma_atari_conv1_fwd_amax",
       "mi355ppo_ma_atari_conv1_wgrad_fold_f32"]
INDICATORS = [(1, 0), (0, 1), (3, 250)]


def P(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def call(name, *args):
    _lib.call(name, *args)


def frames6(n, seed, indicators=INDICATORS):
    rs = np.random.RandomState(seed)
    f = rs.randint(0, 256, size=(n, 84, 84, 6)).astype(np.uint8)
    for i in range(n):
        f[i, :, :, 4], f[i, :, :, 5] = indicators[i % len(indicators)]
    return f


def split(f, flag=None):
    n = f.shape[0]
    rows, ind = np.full((n, 84, 84, 4), 7, np.uint8), np.full((n, 2), 7, np.uint8)
    flag = np.zeros(1, np.uint32) if flag is None else flag
    call("mi355ppo_ma_atari_split_u8_cpu", P(f), P(rows), P(ind), P(flag), n)
    return rows, ind, flag


def weights6(seed):
    g = torch.Generator().manual_seed(seed)
    W = (torch.randn(32, 6, 8, 8, generator=g) * (1.0 / np.sqrt(6 * 64))).numpy()
    b = (torch.randn(32, generator=g) * 0.1).numpy()
    return np.ascontiguousarray(W), b


def pack6(W6):
    pack, tapsum = np.zeros(PACK_BYTES, np.uint8), np.zeros(64, np.float32)
    call("mi355ppo_ma_atari_conv1_pack_f32_cpu", P(W6), P(pack), P(tapsum))
    return pack, tapsum


def conv1_float64(rows_u8, ind, inds, W6, b):
    """relu(conv1) of the six-channel observations whose planes 4 / 5 hold ``ind`` everywhere, in float64; (M, 20, 20, 32)."""
    sel = np.arange(rows_u8.shape[0]) if inds is None else inds
    x = np.concatenate([rows_u8[sel].astype(np.float64) / 255.0,
                        np.broadcast_to(ind[sel].astype(np.float64)[:, None, None, :], (len(sel), 84, 84, 2))], axis=-1)
    y = torch.nn.functional.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(W6).double(), torch.from_numpy(b).double(), stride=4)
    return torch.relu(y).permute(0, 2, 3, 1).numpy()


def test_split_twin_rows_indicator_bytes_and_the_sticky_flag():
    f = frames6(3, 1)
    rows, ind, flag = split(f)
    assert np.array_equal(rows, f[..., :4]) and np.array_equal(ind, np.array(INDICATORS, np.uint8)) and flag[0] == 0
    bad = f.copy()
    bad[2, 83, 83, 5] ^= 1
    rows_b, ind_b, flag_b = split(bad)
    assert flag_b[0] != 0 and np.array_equal(rows_b, rows) and np.array_equal(ind_b, ind)
    _, _, kept = split(f, flag_b)                                   # a clean store leaves a set flag alone
    assert kept[0] != 0
    bad = f.copy()
    bad[1, 0, 1, 4] = 9
    assert split(bad)[2][0] != 0
    assert split(f)[2][0] == 0


def test_pack_twin_is_the_four_channel_pack_and_the_float64_tap_sums():
    W6, _ = weights6(4)
    W6[5] = 0.0
    W6[9, :4] *= 1e-3                                               # channels 4 / 5 must not enter a channel's scale
    pack, tapsum = pack6(W6)
    want = np.zeros(PACK_BYTES, np.uint8)
    W4 = np.ascontiguousarray(W6[:, :4])                            # (kept alive across the call: P holds an address only)
    call("mi355ppo_cnn_conv1q_pack_cpu", P(W4), P(want))
    assert np.array_equal(pack, want)
    sums = W6[:, 4:].astype(np.float64).reshape(32, 2, 64).sum(-1).astype(np.float32)
    assert np.array_equal(tapsum.reshape(32, 2), sums)


@pytest.mark.parametrize("M", [1, 3, 33])
def test_forward_and_fold_twins_against_float64(M):
    """The row-bias forward at kernel Q's bar against float64 (tests/test_gpu_cnn.py::_close: 2e-5 of the result's scale), the fold at the
    weight-gradient kernels' bar (the same) per channel group; a permuted ``inds``; all-zero indicators are the plain twin's bits."""
    rs = np.random.RandomState(M)
    R = M + 2
    f = frames6(R, 10 + M, INDICATORS + [(0, 0)])
    rows, ind, _ = split(f)
    inds = rs.permutation(R)[:M].astype(np.int64)
    W6, b = weights6(2)
    pack, tapsum = pack6(W6)
    out, bits = np.zeros((M, 20, 20, 32), np.float32), np.zeros(M * 400, np.uint32)
    call("mi355ppo_ma_atari_conv1_fwd_cpu", P(rows), P(inds), P(ind), P(pack), P(tapsum), P(b), P(out), P(bits), M)
    ref = conv1_float64(rows, ind, inds, W6, b)
    err, scale = np.abs(out - ref).max(), np.abs(ref).max()
    print(f"row-bias forward twin, M={M}: max err {err:.3e}, scale {scale:.3e}")
    assert err <= 2e-5 * scale
    assert np.array_equal(bits.reshape(M, 400), ((out > 0).reshape(M, 400, 32) << np.arange(32)).sum(-1).astype(np.uint32))
    zero = np.zeros_like(ind)
    a, c = np.zeros_like(out), np.zeros_like(out)
    call("mi355ppo_ma_atari_conv1_fwd_cpu", P(rows), P(inds), P(zero), P(pack), P(tapsum), P(b), P(a), None, M)
    call("mi355ppo_cnn_conv1q_fwd_cpu", P(rows), P(inds), P(pack), P(b), P(c), None, M)
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))
    # the fold: channels 0 - 3 copied, every tap of channel 4 + j = sum_i v_j(i) sum_p dz1[i][p][n]
    dz = rs.standard_normal((M, 20, 20, 32)).astype(np.float32)
    dW4 = rs.standard_normal((32, 4, 8, 8)).astype(np.float32)
    dW6 = np.full((32, 6, 8, 8), np.nan, np.float32)
    call("mi355ppo_ma_atari_conv1_wgrad_fold_f32_cpu", P(dz), P(inds), P(ind), P(dW4), P(dW6), M)
    assert np.array_equal(dW6[:, :4], dW4)
    g = np.einsum("ij,in->nj", ind[inds].astype(np.float64), dz.astype(np.float64).sum((1, 2)))
    assert np.array_equal(dW6[:, 4:], np.broadcast_to(dW6[:, 4:, :1, :1], (32, 2, 8, 8)))
    err, scale = np.abs(dW6[:, 4:, 0, 0] - g).max(), np.abs(g).max()
    print(f"fold twin, M={M}: max err {err:.3e}, scale {scale:.3e}")
    assert err <= 2e-5 * scale
    again = np.zeros_like(dW6)
    call("mi355ppo_ma_atari_conv1_wgrad_fold_f32_cpu", P(dz), P(inds), P(ind), P(dW4), P(again), M)
    assert np.array_equal(again.view(np.uint32), dW6.view(np.uint32))


def test_c_abi_declares_binds_and_exports_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "mi355ppo.h")).read()
    declared = set(re.findall(r"MI355PPO_API\s+[\w\s\*]+?\b(mi355ppo_\w+)\s*\(", header))
    lib = _lib.load()
    names = NEW + [n + "_cpu" for n in NEW if not n.endswith(("_bits", "_amax"))] + [
        "mi355ppo_ma_atari_conv1_fwd_cpu", "mi355ppo_cnn_conv1q_pack_cpu", "mi355ppo_cnn_conv1q_fwd_cpu",
        "mi355ppo_ma_atari_conv1_wgrad_fold_workspace_bytes"]
    for name in names:
        assert name in declared and name in _lib.SIGNATURES and getattr(lib, name) is not None, name
    assert lib.mi355ppo_ma_atari_conv1_wgrad_fold_workspace_bytes(0) == 0
    assert lib.mi355ppo_ma_atari_conv1_wgrad_fold_workspace_bytes(33) == 9 * 64 * 8          # four images per partial, 64 doubles each
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.mi355ppo_ma_atari_split_u8(p, p, p, None, 1, None) == -1                      # refusals precede any launch
    assert lib.mi355ppo_ma_atari_conv1_fwd_bits(p, None, None, p, p, p, p, p, 1, None) == -1
    assert lib.mi355ppo_ma_atari_conv1_wgrad_fold_f32(p, None, p, p, p, 8, p, 16, None) == -4
    assert b"workspace" in lib.mi355ppo_last_error()


def _cpu_learner():
    from cleanrl_amd.agents import MAAtariAgent
    from cleanrl_amd.learner import PPOLearner
    from cleanrl_amd.learner_smoke import default_args

    envs = SimpleNamespace(single_observation_space=E.Box(0, 255, (84, 84, 6), np.uint8), single_action_space=E.Discrete(6))
    return PPOLearner(MAAtariAgent(envs), default_args(num_steps=2, num_minibatches=2, update_epochs=1), envs.single_observation_space,
                      envs.single_action_space, 2, torch.device("cpu"))


def test_switch_accepts_torch_and_fused_only(monkeypatch):
    from cleanrl_amd.agents import ma_atari_backend

    monkeypatch.delenv("MI355PPO_MA_ATARI", raising=False)
    assert ma_atari_backend() == "torch"
    L = _cpu_learner()
    assert not L.ma_fused and L.partial_scale and tuple(L.obs.shape[2:]) == (84, 84, 6)
    monkeypatch.setenv("MI355PPO_MA_ATARI", "fused")
    assert ma_atari_backend() == "fused"
    assert not _cpu_learner().ma_fused                              # HIP learner only: the host learner keeps the reference's ops
    monkeypatch.setenv("MI355PPO_MA_ATARI", "mfma")
    with pytest.raises(ValueError, match="MI355PPO_MA_ATARI"):
        _cpu_learner()


def test_learner_raises_when_the_diagnostics_carry_a_set_flag(monkeypatch):
    """The flag word travels with an update's diagnostics; ``PendingMetrics.result`` runs the learner's check once they arrived.  A stand-in
    for the device side in the manner of tests/test_hip_branches_on_fake_ops.py: the host copies the HIP branch would have made."""
    from cleanrl_amd.learner import PendingMetrics

    monkeypatch.delenv("MI355PPO_MA_ATARI", raising=False)
    L = _cpu_learner()
    values, returns, scalars = torch.zeros(4), torch.arange(4.0), torch.zeros(2, 7)
    pm = PendingMetrics(None, values, returns, scalars, None, 2)
    pm.after_sync = L._ma_flag_check(torch.zeros(1, dtype=torch.int32))
    assert pm.result()["num_updates"] == 2
    pm = PendingMetrics(None, values, returns, scalars, None, 2)
    pm.after_sync = L._ma_flag_check(torch.ones(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="not constant") as exc:
        pm.result()
    assert "MI355PPO_MA_ATARI" in str(exc.value) and "unset" in str(exc.value)
