"""cleanrl_amd/replay_ops.py: one definition per replay-ring operator, bound once to the device side (``ops``) and once to the host
side (``host_ops``).  The ABI rule that makes this possible, the bindings, and for one operator per family which side refuses what,
which symbol is called with how many arguments, and that every refusal precedes the C call."""
import ctypes
import inspect

import pytest
import torch

from cleanrl_amd import _lib, host_ops, ops
from cleanrl_amd.replay_ops import ATARI_FRAME, OPERATORS, dqn_counts, offpolicy_counts, sac_actor_count

SYMBOLS = {
    "replay_add": "mi355ppo_replay_add_f32", "ddpg_act": "mi355ppo_ddpg_act_f32", "td3_target": "mi355ppo_td3_target_f32",
    "td3_critic_fwd_bwd": "mi355ppo_td3_critic_fwd_bwd_f32", "td3_actor_fwd_bwd": "mi355ppo_td3_actor_fwd_bwd_f32", "polyak_": "mi355ppo_polyak_f32",
    "sac_policy": "mi355ppo_sac_policy_f32", "sac_target": "mi355ppo_sac_target_f32", "sac_actor_fwd_bwd": "mi355ppo_sac_actor_fwd_bwd_f32",
    "sac_alpha_": "mi355ppo_sac_alpha_f32",
    "dqn_act": "mi355ppo_dqn_act_f32", "dqn_td_fwd_bwd": "mi355ppo_dqn_td_fwd_bwd_f32", "c51_fwd_bwd": "mi355ppo_c51_fwd_bwd_f32",
    "replay_add_u8": "mi355ppo_replay_add_u8", "replay_gather_u8": "mi355ppo_replay_gather_u8", "dqn_head_act": "mi355ppo_dqn_head_act_f32",
    "dqn_head_td_fwd_bwd": "mi355ppo_dqn_head_td_fwd_bwd_f32", "c51_head_fwd_bwd": "mi355ppo_c51_head_fwd_bwd_f32",
    "qdagger_head_act": "mi355ppo_qdagger_head_act_f32", "qdagger_head_fwd_bwd": "mi355ppo_qdagger_head_fwd_bwd_f32",
    "rainbow_per_add_u8": "mi355ppo_rainbow_per_add_u8", "rainbow_per_sample": "mi355ppo_rainbow_per_sample",
    "rainbow_per_gather_u8": "mi355ppo_rainbow_per_gather_u8", "rainbow_per_update": "mi355ppo_rainbow_per_update",
    "rainbow_noisy_compose": "mi355ppo_rainbow_noisy_compose_f32", "rainbow_noisy_grad": "mi355ppo_rainbow_noisy_grad_f32",
    "rainbow_head_act": "mi355ppo_rainbow_head_act_f32", "rainbow_head_fwd_bwd": "mi355ppo_rainbow_head_fwd_bwd_f32",
    "replay_add2_u8": "mi355ppo_replay_add2_u8", "replay_gather2_u8": "mi355ppo_replay_gather2_u8", "sacd_head_act": "mi355ppo_sacd_head_act_f32",
    "sacd_critic_fwd_bwd": "mi355ppo_sacd_critic_fwd_bwd_f32", "sacd_actor_fwd_bwd": "mi355ppo_sacd_actor_fwd_bwd_f32",
}
P, Z = ctypes.c_void_p, ctypes.c_size_t


def test_the_33_operators_are_the_issue_s_list():
    assert len(OPERATORS) == 33 and set(OPERATORS) == set(SYMBOLS)


@pytest.mark.parametrize("op", sorted(SYMBOLS))
def test_twin_takes_the_device_arguments_minus_workspace_and_stream(op):
    name = SYMBOLS[op]
    dev_args, cpu_args = _lib.SIGNATURES[name][1], _lib.SIGNATURES[name + "_cpu"][1]
    if name == "mi355ppo_sac_alpha_f32":                                  # the one exception: sched2 sits before the two outputs
        assert dev_args[-1] is P and dev_args[-4] is P and dev_args[:-4] + dev_args[-3:-1] == cpu_args
        return
    tail = dev_args[len(cpu_args):]
    assert dev_args[:len(cpu_args)] == cpu_args and tail in ([P], [P, Z, P])


@pytest.mark.parametrize("op", sorted(SYMBOLS))
def test_both_modules_bind_the_one_definition(op):
    d, h = getattr(ops, op), getattr(host_ops, op)
    assert d is not h and d.__func__ is h.__func__ and d.__self__ is not h.__self__
    assert inspect.signature(d) == inspect.signature(h) and d.__doc__ and h.__doc__ and d.__name__ == op
    assert op in ops.__all__


# ---------------------------------------------------------------------------------------------- one operator per family
def _mlp_ring(dev, act_width=2):
    """slots 4, 2 envs, obs 3, act 2 (1 for the DQN ring); batch 4."""
    z = lambda *s: torch.zeros(s, device=dev)  # noqa: E731
    ring = (z(4, 2, 3), z(4, 2, 3), z(4, 2, act_width), z(4, 2), z(4, 2))
    return ring, torch.tensor([0, 1, 2, 3], device=dev), torch.tensor([0, 1, 0, 1], device=dev)


def _td3_target(dev, out):
    ring, bi, ei = _mlp_ring(dev)
    pa, pq = offpolicy_counts(3, 2)
    z = lambda *s: torch.zeros(s, device=dev)  # noqa: E731
    return (ring, bi, ei, z(pa), z(2 * pq), 2, z(2), z(2), z(4, 2), 0.2, 0.5, -1.0, 1.0, 0.99, out)


def _sac_target(dev, out):
    ring, bi, ei = _mlp_ring(dev)
    z = lambda *s: torch.zeros(s, device=dev)  # noqa: E731
    return (ring, bi, ei, z(sac_actor_count(3, 2)), z(2 * offpolicy_counts(3, 2)[1]), z(2), z(2), z(4, 2), z(1), 0.99, out)


def _dqn_td(dev, out):
    ring, bi, ei = _mlp_ring(dev, 1)
    n = dqn_counts(3, 2)
    return (ring, bi, ei, torch.zeros(n, device=dev), torch.zeros(n, device=dev), 2, 0.99, torch.zeros(n, device=dev), out)


def _gather_u8(dev, out):
    """slots 3, 1 env, batch 2."""
    ring = (torch.zeros((3, 1) + ATARI_FRAME, dtype=torch.uint8, device=dev), torch.zeros(3, 1, dtype=torch.int64, device=dev),
            torch.zeros(3, 1, device=dev), torch.zeros(3, 1, device=dev))
    inds = torch.tensor([0, 2], device=dev)
    return (ring, inds, torch.zeros_like(inds), torch.zeros((4,) + ATARI_FRAME, dtype=torch.uint8, device=dev),
            torch.zeros(2, dtype=torch.int64, device=dev), out, torch.zeros(2, device=dev))


def _head_act(hidden):
    def args(dev, out):
        return (torch.zeros(2, hidden, device=dev), torch.zeros(2, hidden, device=dev), torch.zeros(2, device=dev), out)
    return args


def _rainbow_head_act(dev, out):
    """2 actions, 2 atoms: (2 + 1) * 2 output rows."""
    return (torch.zeros(2, 1024, device=dev), torch.zeros(6, 512, device=dev), torch.zeros(6, device=dev), torch.zeros(2, device=dev), 2, out)


def _sacd_head_act(dev, out):
    return _head_act(512)(dev, torch.zeros(2, 2, device=dev)) + (out,)


# family: (operator, its arguments given the output under test, that output's shape and dtype)
FAMILIES = {
    "td3": ("td3_target", _td3_target, (4,), torch.float32),
    "sac": ("sac_target", _sac_target, (4,), torch.float32),
    "dqn": ("dqn_td_fwd_bwd", _dqn_td, (2,), torch.float32),
    "dqn_atari": ("replay_gather_u8", _gather_u8, (2,), torch.float32),
    "rainbow": ("rainbow_head_act", _rainbow_head_act, (2,), torch.int64),
    "sac_atari": ("sacd_head_act", _sacd_head_act, (2,), torch.int64),
    "qdagger": ("qdagger_head_act", _head_act(256), (2,), torch.int64),
}
SENTINEL = 7


@pytest.fixture
def calls(monkeypatch):
    seen = []
    monkeypatch.setattr(_lib, "call", lambda name, *args: seen.append((name, args)))
    return seen


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_device_side_refuses_cpu_tensors_and_the_host_side_calls_the_twin_once(family, calls):
    op, make, shape, dtype = FAMILIES[family]
    args = make("cpu", torch.full(shape, SENTINEL, dtype=dtype))
    with pytest.raises(TypeError, match="CUDA/HIP tensor"):
        getattr(ops, op)(*args)
    assert calls == []
    getattr(host_ops, op)(*args)
    assert [name for name, _ in calls] == [SYMBOLS[op] + "_cpu"]
    assert len(calls[0][1]) == len(_lib.SIGNATURES[SYMBOLS[op] + "_cpu"][1])


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_host_side_refuses_a_bad_output_before_the_call(family, calls):
    op, make, shape, dtype = FAMILIES[family]
    (rows,) = shape
    other = torch.int64 if dtype != torch.int64 else torch.float32
    bad = ((TypeError, torch.full(shape, SENTINEL, dtype=other)),
           (ValueError, torch.full((2 * rows,), SENTINEL, dtype=dtype)[::2]),
           (ValueError, torch.full((rows - 1,), SENTINEL, dtype=dtype)))
    for error, out in bad:
        with pytest.raises(error):
            getattr(host_ops, op)(*make("cpu", out))
        assert calls == [] and bool((out == SENTINEL).all())


@pytest.mark.gpu
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_the_host_side_refuses_cuda_tensors(family, calls):
    op, make, shape, dtype = FAMILIES[family]
    with pytest.raises(TypeError, match="CPU tensors only"):
        getattr(host_ops, op)(*make("cuda", torch.full(shape, SENTINEL, dtype=dtype, device="cuda")))
    assert calls == []
