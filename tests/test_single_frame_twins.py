"""The host twins of the one-frame conv1 kernels (kernel Q1's pack and pre-activation forward, csrc/ma_atari_twins.hip) against an integer
reference written here, their guard bands, and the validation of LSTMPQNLearner's MI355PPO_PQN_TRUNK switch.  Runs without a GPU."""
import pytest
import torch
import torch.nn.functional as F

import guard_arena as GA
import pqn_trunk_cases as PC
from cleanrl_amd import envs as E, host_ops

CPU = torch.device("cpu")


def case(stored, seed=0):
    g = torch.Generator().manual_seed(7000 + seed)
    frames = torch.randint(0, 256, (stored, 84, 84), generator=g, dtype=torch.uint8)
    return frames, 0.05 * torch.randn((32, 1, 8, 8), generator=g), 0.5 * torch.randn(32, generator=g)


def integer_reference(frames, W, b):
    """Kernel Q's arithmetic contract restated with torch int64: each weight rounded once to 31-bit fixed point on its output channel's
    scale (q = rint(w * 2^(30 - E_n)), 2^(E_n - 1) <= max |w[n]| < 2^E_n), four signed radix-256 digits, an exact integer convolution of the
    bytes with every digit plane, the Horner chain over the four digit sums in float32, * 2^(E_n - 6) / 255, + bias."""
    m = frames.shape[0]
    Wd = W.double().reshape(32, 64)
    E_n = torch.frexp(Wd.abs().max(1).values)[1].to(torch.int64)              # max = f * 2^E, f in [0.5, 1)
    q = torch.round(Wd * torch.pow(torch.tensor(2.0, dtype=torch.float64), (30 - E_n).double()).unsqueeze(1)).to(torch.int64)   # (ties: none at 2^-30 of a randn)
    digits = []
    for _ in range(4):                                                       # least significant first
        lo = ((q + 128) & 255) - 128
        digits.append(lo)
        q = (q - lo) >> 8
    assert (q == 0).all()
    d3, d2, d1, d0 = digits                                                  # q = d0 2^24 + d1 2^16 + d2 2^8 + d3
    patches = F.unfold(frames.double().unsqueeze(1), 8, stride=4).to(torch.int64)          # (m, 64, 400): taps in (kh, kw) order
    D = [torch.einsum("nk,mkp->mpn", d, patches) for d in (d0, d1, d2, d3)]   # exact int64 sums, (m, 400, 32)
    assert all(x.abs().max().item() <= 64 * 128 * 255 for x in D)
    f = lambda x: x.to(torch.float32)      # noqa: E731  (exact: |D| < 2^24)
    k = torch.tensor(0.00390625, dtype=torch.float32)
    t = f(D[3])
    for j in (2, 1, 0):                                                      # fmaf(t, 2^-8, D_j): t * 2^-8 is exact, one rounding per step
        t = (t.double() * k.double() + D[j].double()).to(torch.float32)
    scale = (torch.pow(torch.tensor(2.0, dtype=torch.float64), (E_n - 6).double()) / 255.0).to(torch.float32)
    return ((t * scale) + b.to(torch.float32)).view(m, 20, 20, 32)


@pytest.mark.parametrize("stored,inds", [(1, None), (4, [3, 0, 3])])
def test_forward_twin_equals_the_integer_reference_bit_for_bit(stored, inds):
    frames, W, b = case(stored, seed=stored)
    ii = None if inds is None else torch.tensor(inds, dtype=torch.int64)
    z1 = host_ops.conv1q1_pre_fwd(frames, host_ops.conv1q1_pack(W), b, ii)
    src = frames if ii is None else frames[ii]
    assert z1.shape == (src.shape[0], 20, 20, 32)
    ref = integer_reference(src, W, b)
    assert torch.equal(z1, ref), (z1.double() - ref.double()).abs().max().item()
    assert (z1 < 0).any()
    if inds is not None:
        assert torch.equal(z1[0], z1[2])
    x = src.unsqueeze(1)
    ref64 = F.conv2d(x.double() / 255.0, W.double(), b.double(), stride=4).permute(0, 2, 3, 1)
    ref32 = F.conv2d(x.float() / 255.0, W, b, stride=4).permute(0, 2, 3, 1)
    PC.bar(f"z1 ({src.shape[0]} images)", z1, ref64, ref32)


def test_the_three_frame_layouts_are_the_same_bytes():
    frames, W, b = case(2, seed=9)
    pack = host_ops.conv1q1_pack(W)
    z = host_ops.conv1q1_pre_fwd(frames, pack, b)
    assert torch.equal(z, host_ops.conv1q1_pre_fwd(frames.view(2, 1, 84, 84), pack, b))
    assert torch.equal(z, host_ops.conv1q1_pre_fwd(frames.view(2, 84, 84, 1), pack, b))
    with pytest.raises(ValueError, match="uint8 frames"):
        host_ops.conv1q1_pre_fwd(torch.zeros((2, 84, 84, 4), dtype=torch.uint8), pack, b)
    with pytest.raises(ValueError, match="out of range"):
        host_ops.conv1q1_pre_fwd(frames, pack, b, torch.tensor([2]))


# ------------------------------------------------------------------------------------------------------------ guard bands
@pytest.mark.parametrize("sentinel", GA.SENTINELS)
def test_one_frame_twins_stay_inside_their_tensors(sentinel):
    arena = GA.Arena(CPU, sentinel, words=1 << 21)
    frames_, W_, b_ = case(4, seed=5)
    frames = arena.input(frames_, "frames")                                   # exactly 4 x 7,056 bytes
    inds = arena.input(torch.tensor([3, 0, 3], dtype=torch.int64), "inds")
    W = arena.input(W_, "W")
    pack = arena.carve((host_ops.conv1q1_pack(W_).numel(),), name="pack")
    host_ops.conv1q1_pack(W, pack)
    bias = arena.input(b_, "bias")
    out = arena.carve((3, 20, 20, 32), name="z1")
    host_ops.conv1q1_pre_fwd(frames, pack, bias, inds, out)
    arena.assert_guards_intact()
    assert torch.equal(pack.view(torch.int32), host_ops.conv1q1_pack(W_).view(torch.int32))      # (digit bytes as f32 storage: compare the words)
    assert torch.isfinite(out).all() and torch.equal(out[0], out[2]) and torch.equal(out, host_ops.conv1q1_pre_fwd(frames_, pack.clone(), b_, inds.clone()))


# ------------------------------------------------------------------------------------------------------------ the learner's switch
T, N = 4, 2


def _learner(monkeypatch, env=None, **kw):
    from cleanrl_amd.agents import AtariLSTMQNetwork
    from cleanrl_amd.learner_pqn_lstm import LSTMPQNLearner
    from cleanrl_amd.pqn_atari_envpool_lstm import Args

    if env is not None:
        monkeypatch.setenv("MI355PPO_PQN_TRUNK", env)
    else:
        monkeypatch.delenv("MI355PPO_PQN_TRUNK", raising=False)
    args = Args(num_envs=N, num_steps=T, num_minibatches=1)
    envs = E.SyntheticAtariVecEnv(N, seed=1, n_actions=4, api="gym", frames=1)
    assert envs.single_observation_space.shape == (1, 84, 84)
    kw.setdefault("obs_space", envs.single_observation_space)
    return LSTMPQNLearner(AtariLSTMQNetwork(envs), args, envs.single_observation_space.shape, 4, N, "cpu", **kw)


def test_the_recurrent_learner_defaults_to_the_torch_trunk(monkeypatch):
    learner = _learner(monkeypatch, backend="fused")
    assert learner.trunk == "torch" and not learner.fused_trunk
    assert learner.obs.dtype == torch.float32 and learner.obs.shape == (T, N, 1, 84, 84)


def test_the_fused_trunk_is_refused_on_the_cpu(monkeypatch):
    with pytest.raises(ValueError, match="HIP kernels only"):
        _learner(monkeypatch, backend="fused", trunk="fused")
    with pytest.raises(ValueError, match="HIP kernels only"):
        _learner(monkeypatch, env="fused", backend="fused")


def test_the_fused_trunk_is_refused_with_the_torch_backend(monkeypatch):
    with pytest.raises(ValueError, match="needs MI355PPO_PQN=fused"):
        _learner(monkeypatch, backend="torch", trunk="fused")


def test_the_fused_trunk_is_refused_for_a_non_uint8_observation_space(monkeypatch):
    with pytest.raises(ValueError, match="uint8 frame stacks"):
        _learner(monkeypatch, backend="fused", trunk="fused", obs_space=E.Box(0.0, 1.0, (1, 84, 84)))


def test_each_learner_refuses_the_other_ones_frame_count(monkeypatch):
    from cleanrl_amd.agents import AtariLSTMQNetwork, AtariQNetwork
    from cleanrl_amd.learner_pqn import PQNLearner
    from cleanrl_amd.learner_pqn_lstm import LSTMPQNLearner
    from cleanrl_amd.pqn_atari_envpool import Args
    from cleanrl_amd.pqn_atari_envpool_lstm import Args as LstmArgs

    monkeypatch.delenv("MI355PPO_PQN_TRUNK", raising=False)
    one = E.SyntheticAtariVecEnv(N, seed=1, n_actions=4, api="gym", frames=1)
    four = E.SyntheticAtariVecEnv(N, seed=1, n_actions=4, api="gym")
    with pytest.raises(ValueError, match="uint8 frame stacks"):
        PQNLearner(AtariQNetwork(four), Args(num_envs=N, num_steps=T), (1, 84, 84), 4, N, "cpu", mlp=False, backend="fused", trunk="fused",
                   obs_space=one.single_observation_space)
    with pytest.raises(ValueError, match="uint8 frame stacks"):
        LSTMPQNLearner(AtariLSTMQNetwork(one), LstmArgs(num_envs=N, num_steps=T, num_minibatches=1), (4, 84, 84), 4, N, "cpu", backend="fused",
                       trunk="fused", obs_space=four.single_observation_space)
