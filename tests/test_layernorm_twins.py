"""The host twins of the LayerNorm + ReLU kernels (csrc/layernorm_twins.hip) and of kernel Q's pre-activation instance against torch,
their guard bands, and the validation of PQNLearner's MI355PPO_PQN_TRUNK switch.  Everything here runs without a GPU."""
import numpy as np
import pytest
import torch

import guard_arena as GA
import pqn_trunk_cases as PC
from cleanrl_amd import _lib, envs as E, host_ops

CPU = torch.device("cpu")


@pytest.mark.parametrize("rows,C,HW", PC.FWD_SHAPES)
def test_forward_twin_is_within_the_bar_of_torch_layer_norm(rows, C, HW):
    z, gamma, beta, _ = PC.inputs(rows, C, HW)
    a, mean, rstd = host_ops.layernorm_relu_fwd(z, gamma, beta, C, HW, PC.EPS)
    ref64, ref32 = PC.reference_fwd(z, gamma, beta, torch.float64), PC.reference_fwd(z, gamma, beta, torch.float32)
    PC.bar(f"a ({rows}, {C}, {HW})", a, ref64, ref32)
    zn = PC.nchw(z, rows, C, HW).double().reshape(rows, -1)
    assert torch.allclose(mean.double(), zn.mean(1), rtol=0, atol=1e-6)
    assert torch.allclose(rstd.double(), 1.0 / torch.sqrt(zn.var(1, unbiased=False) + PC.EPS), rtol=1e-6, atol=0)


def test_a_constant_row_gives_relu_of_beta_exactly():
    rows, C, HW = 3, 64, 49
    z, gamma, beta, _ = PC.inputs(rows, C, HW, constant_row=True)
    a, mean, rstd = host_ops.layernorm_relu_fwd(z, gamma, beta, C, HW, PC.EPS)
    assert mean[1].item() == np.float32(1.7) and rstd[1].item() == 1.0 / np.sqrt(np.float32(0.0) + np.float32(PC.EPS), dtype=np.float32)
    assert torch.equal(a[1], torch.relu(beta).t().contiguous())      # var = 0: (z - mean) = 0 exactly


@pytest.mark.parametrize("rows,C,HW", PC.BWD_SHAPES)
def test_backward_twin_is_within_the_bar_of_float64_autograd(rows, C, HW):
    act_mask = (rows, C, HW) == (257, 512, 1)
    z, gamma, beta, dy = PC.inputs(rows, C, HW, seed=1)
    a, mean, rstd = host_ops.layernorm_relu_fwd(z, gamma, beta, C, HW, PC.EPS)
    if not act_mask:
        dy = dy * (a > 0)                                              # what the data-gradient kernels hand over
    rec = torch.zeros(PC.AMAX_WORDS, dtype=torch.int32)
    dz, dg, db = host_ops.layernorm_relu_bwd(dy, z, mean, rstd, gamma, C, HW, act=a if act_mask else None, amax=rec)
    r64, r32 = (PC.reference_bwd(z, gamma, beta, dy, t, act_mask) for t in (torch.float64, torch.float32))
    for name, got, x64, x32 in zip(("dz", "dgamma", "dbeta"), (dz, dg, db), r64, r32):
        PC.bar(f"{name} ({rows}, {C}, {HW})", got, x64, x32)
    assert PC.amax_value(rec) == dz.abs().max().item()
    # the same call again: the same bits
    dz2, dg2, db2 = host_ops.layernorm_relu_bwd(dy, z, mean, rstd, gamma, C, HW, act=a if act_mask else None)
    assert torch.equal(dz, dz2) and torch.equal(dg, dg2) and torch.equal(db, db2)


@pytest.mark.parametrize("rows,C,HW", PC.FWD_SHAPES)
def test_mask_bits_and_the_amax_record_of_the_forward(rows, C, HW):
    z, gamma, beta, _ = PC.inputs(rows, C, HW, seed=2)
    bits, rec = torch.full((rows * C * HW // 32,), -1, dtype=torch.int32), torch.zeros(PC.AMAX_WORDS, dtype=torch.int32)
    a, _, _ = host_ops.layernorm_relu_fwd(z, gamma, beta, C, HW, PC.EPS, bits=bits, amax=rec)
    assert torch.equal(bits, PC.packed_bits(a))
    assert PC.amax_value(rec) == a.max().item() > 0


def test_layernorm_twins_refuse_what_the_kernels_do_not_take():
    z = torch.zeros((2, 6))
    with pytest.raises(_lib.Mi355PpoError):
        host_ops.layernorm_relu_fwd(z, torch.ones(6), torch.zeros(6), 6, 1)                  # C % 4
    z = torch.zeros((1, 4 * 5000))
    with pytest.raises(_lib.Mi355PpoError):
        host_ops.layernorm_relu_fwd(z, torch.ones(20000), torch.zeros(20000), 20000, 1)     # D > 16,384
    z = torch.zeros((1, 8))
    with pytest.raises(_lib.Mi355PpoError):
        host_ops.layernorm_relu_fwd(z, torch.ones(8), torch.zeros(8), 8, 1, bits=torch.zeros(8, dtype=torch.int32))     # bits: D % 32


@pytest.mark.parametrize("images,with_inds", [(3, False), (3, True), (70, False), (70, True)])
def test_relu_of_the_kernel_q_pre_twin_is_the_relu_forward_twin(images, with_inds):
    g = torch.Generator().manual_seed(images)
    rows = images + 5 if with_inds else images
    frames = torch.randint(0, 256, (rows, 84, 84, 4), generator=g, dtype=torch.uint8)
    inds = torch.randperm(rows, generator=g)[:images].contiguous() if with_inds else None
    W, b = 0.05 * torch.randn((32, 4, 8, 8), generator=g), 0.5 * torch.randn(32, generator=g)
    pack = host_ops.conv1q_pack(W)
    pre = host_ops.conv1q_pre_fwd(frames, pack, b, inds)
    act = torch.empty((images, 20, 20, 32))
    _lib.call("mi355ppo_cnn_conv1q_fwd_cpu", frames.data_ptr(), None if inds is None else inds.data_ptr(), pack.data_ptr(), b.data_ptr(),
              act.data_ptr(), None, images)
    assert (pre < 0).any() and torch.equal(torch.relu(pre), act)
    src = frames if inds is None else frames[inds]
    ref = torch.nn.functional.conv2d(src.permute(0, 3, 1, 2).double() / 255.0, W.double(), b.double(), stride=4).permute(0, 2, 3, 1)
    assert (pre.double() - ref).abs().max().item() < 1e-5


# ------------------------------------------------------------------------------------------------------------ guard bands
@pytest.mark.parametrize("sentinel", GA.SENTINELS)
@pytest.mark.parametrize("rows,C,HW,act_mask", [(1, 512, 1, True), (3, 64, 49, False), (5, 32, 400, False), (70, 64, 81, False), (257, 512, 1, True)])
def test_layernorm_twins_stay_inside_their_tensors(rows, C, HW, act_mask, sentinel, monkeypatch):
    got = PC.run_guarded_layernorm(host_ops, CPU, sentinel, rows, C, HW, act_mask, monkeypatch)
    other = PC.run_guarded_layernorm(host_ops, CPU, GA.SENTINELS[1 - GA.SENTINELS.index(sentinel)], rows, C, HW, act_mask, monkeypatch)
    for x, y in zip(got[:7], other[:7]):
        assert GA.same_bits(x, y)                                      # nothing read that was not written
    assert got[7:] == other[7:] and all(torch.isfinite(t).all() for t in got[:3] + got[4:7])


@pytest.mark.parametrize("sentinel", GA.SENTINELS)
def test_kernel_q_pre_twin_stays_inside_its_tensors(sentinel):
    arena = GA.Arena(CPU, sentinel, words=1 << 21)
    g = torch.Generator().manual_seed(5)
    frames = arena.input(torch.randint(0, 256, (4, 84, 84, 4), generator=g, dtype=torch.uint8), "frames")
    inds = arena.input(torch.tensor([3, 0, 3], dtype=torch.int64), "inds")
    pack = arena.input(host_ops.conv1q_pack(0.05 * torch.randn((32, 4, 8, 8), generator=g)), "pack")
    bias = arena.input(torch.randn(32, generator=g), "bias")
    out = arena.carve((3, 20, 20, 32), name="pre")
    host_ops.conv1q_pre_fwd(frames, pack, bias, inds, out)
    arena.assert_guards_intact()
    assert torch.isfinite(out).all() and torch.equal(out[0], out[2])


# ------------------------------------------------------------------------------------------------------------ the learner's switch
def _learner(monkeypatch, env=None, **kw):
    from cleanrl_amd.agents import AtariQNetwork
    from cleanrl_amd.learner_pqn import PQNLearner
    from cleanrl_amd.pqn_atari_envpool import Args

    if env is not None:
        monkeypatch.setenv("MI355PPO_PQN_TRUNK", env)
    else:
        monkeypatch.delenv("MI355PPO_PQN_TRUNK", raising=False)
    args = Args(num_envs=2, num_steps=4)
    envs = E.SyntheticAtariVecEnv(2, seed=1, n_actions=4, api="gym")
    kw.setdefault("obs_space", envs.single_observation_space)
    return PQNLearner(AtariQNetwork(envs), args, envs.single_observation_space.shape, 4, 2, "cpu", mlp=False, **kw)


def test_the_trunk_switch_defaults_to_torch(monkeypatch):
    learner = _learner(monkeypatch, backend="fused")
    assert learner.trunk == "torch" and not learner.fused_trunk and learner.obs.dtype == torch.float32 and learner.obs.shape == (4, 2, 4, 84, 84)


def test_the_fused_trunk_is_refused_on_the_cpu(monkeypatch):
    with pytest.raises(ValueError, match="HIP kernels only"):
        _learner(monkeypatch, env="fused", backend="fused")
    with pytest.raises(ValueError, match="HIP kernels only"):
        _learner(monkeypatch, backend="fused", trunk="fused")


def test_the_fused_trunk_is_refused_with_the_torch_backend(monkeypatch):
    with pytest.raises(ValueError, match="needs MI355PPO_PQN=fused"):
        _learner(monkeypatch, env="fused", backend="torch")


def test_the_fused_trunk_is_refused_for_a_non_uint8_observation_space(monkeypatch):
    with pytest.raises(ValueError, match="uint8 frame stacks"):
        _learner(monkeypatch, env="fused", backend="fused", obs_space=E.Box(0.0, 1.0, (4, 84, 84)))


def test_an_unknown_trunk_is_refused_and_the_mlp_ignores_the_variable(monkeypatch):
    with pytest.raises(ValueError, match="MI355PPO_PQN_TRUNK"):
        _learner(monkeypatch, env="hip", backend="fused")
    from cleanrl_amd.agents import QNetwork
    from cleanrl_amd.learner_pqn import PQNLearner
    from cleanrl_amd.pqn import Args

    monkeypatch.setenv("MI355PPO_PQN_TRUNK", "fused")
    envs = E.CartPoleVecEnv(2, seed=1)
    learner = PQNLearner(QNetwork(envs), Args(num_envs=2, num_steps=4), envs.single_observation_space.shape, 2, 2, "cpu", backend="fused")
    assert learner.trunk == "torch"
    with pytest.raises(ValueError, match="has no trunk"):
        PQNLearner(QNetwork(envs), Args(num_envs=2, num_steps=4), envs.single_observation_space.shape, 2, 2, "cpu", backend="fused", trunk="fused")
