"""The IMPALA-CNN trunk's host twins (mi355ppo_impala_*_cpu, the device kernels' arithmetic compiled for the host) against
float64 autograd of the reference's modules, the max pool alone against torch bit for bit, ``ops.ImpalaTrunk`` on CPU tensors
through the procgen_update and ppg_phase goldens, the MI355PPO_IMPALA switch and the C ABI's refusals.  No GPU."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import impala_cases as C
from conftest import load_golden
from cleanrl_amd import _lib, agents, host_ops, ops
from cleanrl_amd import envs as E
from cleanrl_amd.learner import PPOLearner
from cleanrl_amd.learner_ppg import PPGLearner
from cleanrl_amd.learner_smoke import default_args


@pytest.fixture
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)          # as when the goldens were minted
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("init", C.INITS)
@pytest.mark.parametrize("frames", C.FRAMES)
def test_twins_against_float64(B, init, frames):
    agent = C.make_agent(init, seed=B)
    x, dy = C.make_frames(frames, B, seed=B), C.upstream(B, seed=B + 7)
    params = C.trunk_params(agent)
    y, saved, arg = host_ops.impala_forward(x, params)
    grads = host_ops.impala_backward(x, params, saved, arg, dy)
    args = C.argmax_planes(arg, B)
    C.check_argmax(agent, x, args)
    C.check_against_f64(agent, x, dy, y, grads, args)


@pytest.mark.parametrize("B,H,Cc", [(2, 64, 16), (3, 32, 32), (1, 16, 32)])
@pytest.mark.parametrize("kind", ["noise", "ties", "neg"])
def test_maxpool_twin_equals_torch_bit_for_bit(B, H, Cc, kind):
    g = torch.Generator().manual_seed(H + B)
    if kind == "noise":
        x = torch.randn((B, H, H, Cc), generator=g)
    elif kind == "ties":                                           # flat blocks and a quantised palette: exact ties everywhere
        x = torch.randint(0, 3, (B, H // 4, H // 4, Cc), generator=g).float().repeat_interleave(4, 1).repeat_interleave(4, 2)
        x = x + (torch.rand((B, H, H, Cc), generator=g) < 0.05).float()
    else:                                                          # all negative, ties at the borders and corners
        x = -torch.randint(1, 3, (B, H, H, Cc), generator=g).float()
    y, arg = host_ops.impala_maxpool_forward(x)
    ty, idx = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
    assert torch.equal(y, ty.permute(0, 2, 3, 1))
    Ho = H // 2
    a = arg.permute(0, 3, 1, 2).long()
    oy, ox = torch.arange(Ho).view(1, 1, Ho, 1), torch.arange(Ho).view(1, 1, 1, Ho)
    assert torch.equal((2 * oy - 1 + a // 3) * H + (2 * ox - 1 + a % 3), idx)
    dy = torch.randn((B, Ho, Ho, Cc), generator=g)
    dx = host_ops.impala_maxpool_backward(dy, arg)
    xr = x.permute(0, 3, 1, 2).clone().requires_grad_(True)
    F.max_pool2d(xr, 3, 2, 1).backward(dy.permute(0, 3, 1, 2))
    assert torch.equal(dx, xr.grad.permute(0, 2, 3, 1))          # same adds in the same (row-major output) order as ATen's CPU kernel


def test_impala_trunk_autograd_on_cpu_accumulates_into_grad():
    agent = C.make_agent("ppg", seed=3)
    agent.impala_backend = "fused"
    x = C.make_frames("noise", 2, seed=3)
    params = C.trunk_params(agent)
    dy = C.upstream(2, seed=4)
    y = ops.ImpalaTrunk.apply(x, *params)
    assert y.shape == (2, 8, 8, 32)
    y.backward(dy)
    first = [p.grad.clone() for p in params]
    _, saved, arg = host_ops.impala_forward(x, params)
    direct = host_ops.impala_backward(x, params, saved, arg, dy)
    assert all(torch.equal(a, b) for a, b in zip(first, direct))
    ops.ImpalaTrunk.apply(x, *params).backward(dy)                 # autograd accumulates, as PPG's gradient accumulation needs
    assert all(torch.equal(p.grad, a + a) for p, a in zip(params, first))
    with torch.no_grad():
        assert torch.equal(ops.impala_trunk(x, params), y.detach())


def _flat(agent):
    return torch.cat([p.detach().reshape(-1) for p in agent.parameters()])


def test_procgen_golden_through_the_fused_twin(one_thread, monkeypatch):
    monkeypatch.setenv("MI355PPO_IMPALA", "fused")
    g = load_golden("procgen_update")["impala_2steps"]
    envs = SimpleNamespace(single_observation_space=E.Box(0, 255, (64, 64, 3), np.uint8), single_action_space=E.Discrete(15))
    torch.manual_seed(int(g["init_seed"]))
    agent = agents.ProcgenAgent(envs)
    assert agent.impala_backend == "fused"
    stride = int(g["stride"])
    # same seed -> same weights up to the last bits of torch's CPU kernels (the default init's vectorised ops round per CPU
    # capability); the fused path is not the yardstick of the initialisation
    np.testing.assert_allclose(_flat(agent)[::stride].numpy(), g["init_params_sub"], rtol=1e-6, atol=1e-8)
    B = g["b_actions"].shape[0]
    args = default_args(num_steps=B // 4, num_minibatches=3, clip_coef=0.2)
    L = PPOLearner(agent, args, envs.single_observation_space, envs.single_action_space, 4, torch.device("cpu"))
    b_obs = torch.from_numpy(g["b_obs_u8"]).float()
    with torch.no_grad():
        _, lp, _, v = agent.get_action_and_value(b_obs, torch.from_numpy(g["b_actions"]).long())
    np.testing.assert_allclose(lp.numpy(), g["logprob_all"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(v.view(-1).numpy(), g["value_all"], rtol=1e-5, atol=2e-6)
    T = lambda k: torch.from_numpy(g[k])
    M = 16
    for k in range(2):
        sc = L._minibatch_host(g["perm"][k * M:(k + 1) * M], b_obs, T("b_actions"), T("b_logprobs"), T("b_advantages"),
                               T("b_returns"), T("b_values"), float(g["lr"]))
        assert abs(sc[0].item() - float(g["losses"][k])) <= 1e-5 * max(1.0, abs(float(g["losses"][k])))
        got = _flat(agent)[::stride]
        assert (got - T(f"params_sub_after_{k + 1}")).abs().max().item() <= 4e-6
    assert abs(_flat(agent).double().sum().item() - float(g["final_checksum"])) <= 1e-3


def test_ppg_phase_through_the_fused_twin(one_thread, monkeypatch, capsys):
    monkeypatch.setenv("MI355PPO_IMPALA", "fused")
    g = load_golden("ppg_phase")["ppg_T8_N4"]
    T, N = g["rewards"].shape
    envs = SimpleNamespace(single_observation_space=E.Box(0, 255, (64, 64, 3), np.uint8), single_action_space=E.Discrete(15))
    torch.manual_seed(int(g["init_seed"]))
    agent = agents.PPGAgent(envs)
    assert agent.impala_backend == "fused"
    stride = int(g["stride"])
    args = default_args(num_steps=T, num_minibatches=2, gamma=0.999, clip_coef=0.2, adv_norm_fullbatch=True, e_policy=1,
                        e_auxiliary=2, beta_clone=1.0, num_aux_rollouts=2, n_aux_grad_accum=1, aux_batch_rollouts=N, n_iteration=1,
                        learning_rate=5e-4)
    L = PPGLearner(agent, args, envs.single_observation_space, envs.single_action_space, N, torch.device("cpu"))
    frames, step_done = g["frames_u8"], g["step_done"]
    L.observe(0, frames[0], step_done[0])
    torch.manual_seed(int(g["sample_seed"]))
    for step in range(T):
        L.act(step)
        L.store_reward(step, g["rewards"][step])
        L.observe(step + 1, frames[step + 1], step_done[step + 1])
    assert torch.equal(L.actions, torch.from_numpy(g["actions"]))
    np.testing.assert_allclose(L.values.numpy(), g["values"], rtol=1e-5, atol=2e-6)
    L.values.copy_(torch.from_numpy(g["values"]))                 # teacher-forced, as the GPU golden test does
    L.logprobs.copy_(torch.from_numpy(g["logprobs"]))
    L.finish_rollout()
    np.random.seed(int(g["shuffle_seed"]))
    m = L.update(float(g["lr"]))
    assert (_flat(agent)[::stride] - torch.from_numpy(g["policy_params_sub"])).abs().max().item() <= 2e-5
    assert abs(m["loss"] - float(g["policy_loss"])) <= 1e-5 * max(1.0, abs(float(g["policy_loss"])))
    aux = L.aux_phase()
    assert "aux epoch 2" in capsys.readouterr().out
    assert (_flat(agent)[::stride] - torch.from_numpy(g["final_params_sub"])).abs().max().item() <= 4e-5
    for key in ("kl_loss", "aux_value_loss", "real_value_loss"):
        ref = float(g[key])
        assert abs(aux[key] - ref) <= 1e-4 * max(1.0, abs(ref)), (key, aux[key], ref)


def test_switch(monkeypatch):
    envs = SimpleNamespace(single_observation_space=E.Box(0, 255, (64, 64, 3), np.uint8), single_action_space=E.Discrete(15))
    monkeypatch.delenv("MI355PPO_IMPALA", raising=False)
    assert agents.impala_backend_from_env() == "torch"
    ref = agents.ProcgenAgent(envs)
    assert ref.impala_backend == "torch"
    monkeypatch.setenv("MI355PPO_IMPALA", "hip")
    with pytest.raises(ValueError):
        agents.impala_backend_from_env()
    with pytest.raises(ValueError):
        agents.PPGAgent(envs)
    monkeypatch.setenv("MI355PPO_IMPALA", "fused")
    for cls in (agents.ProcgenAgent, agents.PPGAgent):
        a = cls(envs)
        assert a.impala_backend == "fused"
    a = agents.ProcgenAgent(envs)
    assert sum(p.numel() for p in a.parameters()) == 626256
    assert list(a.state_dict().keys()) == list(ref.state_dict().keys())


def test_refusals_leave_outputs_untouched():
    lib = _lib.load()
    B = 1
    x = torch.rand((B, 64, 64, 3))
    params = C.trunk_params(C.make_agent("procgen"))
    P = (ctypes.c_void_p * 30)(*[p.data_ptr() for p in params])
    y = torch.full((B, 8, 8, 32), 7.0)
    saved = torch.full((int(lib.mi355ppo_impala_saved_floats(B)),), 7.0)
    arg = torch.full((int(lib.mi355ppo_impala_argmax_bytes(B)),), 9, dtype=torch.uint8)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    for shape, ch in (((64, 64, 4), (16, 32, 32)), ((84, 84, 3), (16, 32, 32)), ((64, 32, 3), (16, 32, 32)),
                      ((64, 64, 3), (16, 32, 64)), ((64, 64, 3), (32, 32, 32))):
        assert lib.mi355ppo_impala_fwd_f32_cpu(ptr(x), P, ptr(y), ptr(saved), ptr(arg), B, *shape, *ch) == -1
        assert lib.mi355ppo_impala_fwd_f32(ptr(x), P, ptr(y), ptr(saved), ptr(arg), B, *shape, *ch, ptr(saved), 1 << 40, None) == -1
    assert lib.mi355ppo_impala_fwd_f32_cpu(ptr(x), P, ptr(y), ptr(saved), ptr(arg), 0, 64, 64, 3, 16, 32, 32) == -1
    assert lib.mi355ppo_impala_fwd_f32(ptr(x), P, ptr(y), ptr(saved), ptr(arg), B, 64, 64, 3, 16, 32, 32, None, 0, None) == -4
    assert b"workspace" in lib.mi355ppo_last_error()
    assert lib.mi355ppo_impala_maxpool_fwd_f32_cpu(ptr(x), ptr(y), ptr(arg), B, 64, 64, 3) == -1
    assert lib.mi355ppo_impala_maxpool_bwd_f32(ptr(y), ptr(arg), ptr(x), B, 8, 8, 32, None) == -1
    assert (y == 7.0).all() and (saved == 7.0).all() and (arg == 9).all()
    with pytest.raises(ValueError):                               # the Python seam refuses other shapes / channel lists first
        ops.ImpalaTrunk.apply(torch.rand((1, 84, 84, 3)), *params)
    with pytest.raises(ValueError):
        ops.ImpalaTrunk.apply(x, *params[:-2])
