"""``MI355PPO_RND_TRUNK`` off the GPU: the LeakyReLU host twins (csrc/leaky_twins.hip) against torch's own ``leaky_relu`` and its autograd
gradient bit for bit, the switch's values and its dependence on ``MI355PPO_RND=fused``, and the host learner, which ignores it."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cleanrl_amd import envs as E
from cleanrl_amd import host_ops as H
from cleanrl_amd.rnd_ops import LEAKY_SLOPE

SUB = float(np.float32(2.0 ** -149))          # the smallest f32 subnormal
# +-0, the smallest subnormals (their product with 0.01f underflows to +-0), the smallest normal, a value whose product is subnormal
EDGE = [0.0, -0.0, SUB, -SUB, -2.0 * SUB, float(np.float32(2.0 ** -126)), -float(np.float32(2.0 ** -126)), -1e-36, -3.0e-38, 1.0, -1.0,
        3.0e38, -3.0e38]
SIZES = (1, 13, 32, 33, 1000)                 # one element; less than a word; a word; one past it; no multiple of 32 or of 4 x 256


def leaky_case(n: int):
    g = torch.Generator().manual_seed(400 + n)
    z = torch.randn(n, generator=g) * torch.exp2(torch.randint(-20, 20, (n,), generator=g).float())
    k = min(n, len(EDGE))
    z[:k] = torch.tensor(EDGE[:k])
    if n == 1:
        z[0] = -SUB
    da = torch.randn(n, generator=g)
    da[:k] = torch.tensor(EDGE[::-1][:k])
    return z, da


def _bits_of(mask: torch.Tensor) -> torch.Tensor:
    n = mask.numel()
    m = F.pad(mask.reshape(-1).to(torch.int64), (0, (-n) % 32)).reshape(-1, 32)
    w = (m << torch.arange(32, dtype=torch.int64)).sum(1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _record(rec):
    """The value of an amax record: the largest of its slots (bit patterns of non-negative floats order like the floats)."""
    return float(rec.max().reshape(1).view(torch.float32))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("in_place", [False, True])
def test_leaky_twins_equal_torch_bit_for_bit(n, in_place):
    z, da = leaky_case(n)
    zt = z.clone().requires_grad_(True)
    want = F.leaky_relu(zt, LEAKY_SLOPE)
    want.backward(da)
    words = (n + 31) // 32
    bits, rec = torch.full((words,), 0x5A5A5A5A, dtype=torch.int32), torch.zeros(256, dtype=torch.int32)
    src = z.clone()
    a = H.leaky_relu_fwd(src, out=src if in_place else None, bits=bits, amax=rec)
    assert _same(a, want.detach()), "forward differs from torch.nn.functional.leaky_relu"
    assert torch.equal(bits, _bits_of(z > 0)), "mask bits are not z > 0 (bits past n must be zero)"
    assert _record(rec) == float(want.detach().abs().max()), "the amax record is not max |a|"
    rec2 = torch.zeros(256, dtype=torch.int32)
    g = da.clone()
    dz = H.leaky_relu_bwd(g, bits, out=g if in_place else None, amax=rec2)
    assert _same(dz, zt.grad), "backward differs from torch's autograd gradient"
    assert _record(rec2) == float(zt.grad.abs().max())
    # without the optional outputs: the same values
    assert _same(H.leaky_relu_fwd(z.clone()), want.detach())


def test_leaky_operators_refuse_what_they_cannot_take():
    z = torch.zeros(40)
    with pytest.raises(ValueError):
        H.leaky_relu_fwd(z, bits=torch.zeros(1, dtype=torch.int32))          # 40 elements need two words
    with pytest.raises(TypeError):
        H.leaky_relu_fwd(z.double())
    with pytest.raises(TypeError):
        H.leaky_relu_bwd(z, None)
    with pytest.raises(ValueError):
        H.leaky_relu_fwd(torch.zeros(0))


# ---------------------------------------------------------------------------------------------- the switch
def test_the_trunk_switch_takes_torch_and_fused_only(monkeypatch):
    from cleanrl_amd import learner_rnd

    monkeypatch.delenv("MI355PPO_RND_TRUNK", raising=False)
    assert learner_rnd.rnd_trunk_backend() == "torch"
    monkeypatch.setenv("MI355PPO_RND_TRUNK", "Fused ")
    assert learner_rnd.rnd_trunk_backend() == "fused"
    monkeypatch.setenv("MI355PPO_RND_TRUNK", "hip")
    with pytest.raises(ValueError, match="MI355PPO_RND_TRUNK"):
        learner_rnd.rnd_trunk_backend()


def _host_learner():
    from cleanrl_amd.agents import RNDAgent, RNDModel
    from cleanrl_amd.learner_rnd import RNDPPOLearner
    from cleanrl_amd.learner_smoke import default_args

    envs = SimpleNamespace(single_observation_space=E.Box(0, 255, (4, 84, 84), np.uint8), single_action_space=E.Discrete(6))
    args = default_args(num_steps=4, num_minibatches=2, update_epochs=1, gamma=0.999, int_gamma=0.99, clip_coef=0.1, ent_coef=0.001,
                        update_proportion=0.25, int_coef=1.0, ext_coef=2.0, learning_rate=1e-4)
    return RNDPPOLearner(RNDAgent(envs), RNDModel(4, 6), args, envs.single_observation_space, envs.single_action_space, 2, torch.device("cpu"))


def test_fused_trunk_on_the_hip_learner_needs_the_fused_rnd_backend(monkeypatch):
    monkeypatch.setenv("MI355PPO_RND_TRUNK", "fused")
    monkeypatch.delenv("MI355PPO_RND", raising=False)
    L = _host_learner()                               # the host learner ignores the switch ...
    assert not L.hip and not L.rnd_trunk_fused and not L.rnd_fused
    L.hip = True                                      # ... the HIP learner without MI355PPO_RND=fused refuses it
    with pytest.raises(ValueError, match="MI355PPO_RND=fused"):
        L.select_rnd_trunk()
    monkeypatch.setenv("MI355PPO_RND_TRUNK", "both")
    with pytest.raises(ValueError, match="MI355PPO_RND_TRUNK"):
        L.select_rnd_trunk()
    L.hip = False
    L.select_rnd_trunk()                              # a bad value on the host learner is not even read, as MI355PPO_RND's


def test_rnd_agent_has_the_trunk_seam_and_stays_off_the_plain_fused_cnn_path():
    from cleanrl_amd.agents import RNDAgent, _NatureTrunkMixin

    assert issubclass(RNDAgent, _NatureTrunkMixin) and hasattr(RNDAgent, "heads3_u8")
    assert not hasattr(RNDAgent, "heads_u8")          # PPOLearner.fused_cnn keys on that name: RND's default path is unchanged


def test_the_host_learner_ignores_the_switch_bit_for_bit(monkeypatch):
    """tests/test_rnd_script.py's iteration against the reference's lines, with both switches set: the same bits as without them."""
    import test_rnd_script as S

    monkeypatch.setenv("MI355PPO_RND_TRUNK", "fused")
    monkeypatch.setenv("MI355PPO_RND", "fused")
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        S.test_rnd_iteration_matches_the_reference_lines(None)      # (its fixture only sets one thread, as done here)
    finally:
        torch.set_num_threads(n)
