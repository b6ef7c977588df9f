"""The DQN / C51 host twins (csrc/host_twins.hip over csrc/dqn_rows.h) on the CPU: the bit-equal pieces (ring, argmax, TD target,
projection) against the reference's ops, the parity bars of DESIGN.md section 3.15 against float64 autograd, the clamp's dead
gradient, Adam with c51.py's eps, index clamping, refusals."""
import ctypes
import math

import numpy as np
import pytest
import torch

import dqn_cases as D
import offpolicy_cases as C
from cleanrl_amd import _lib
from cleanrl_amd import host_ops as H

CPU = torch.device("cpu")


def test_symbols_are_bound():
    for n in ("dqn_act", "dqn_td_fwd_bwd", "c51_fwd_bwd"):
        assert f"mi355ppo_{n}_f32" in _lib.SIGNATURES and f"mi355ppo_{n}_f32_cpu" in _lib.SIGNATURES
    assert "mi355ppo_dqn_td_workspace_bytes" in _lib.SIGNATURES and "mi355ppo_c51_workspace_bytes" in _lib.SIGNATURES


def test_ring_add_and_gather_with_the_integer_action():
    N, O, slots = 2, 4, 5
    ring = tuple(torch.zeros(s) for s in ((slots, N, O), (slots, N, O), (slots, N, 1), (slots, N), (slots, N)))
    model = C.NumpyRing(slots * N, N, O, 1)
    g = torch.Generator().manual_seed(0)
    for step in range(12):
        data = [torch.randn((N, O), generator=g), torch.randn((N, O), generator=g), torch.randint(0, 18, (N, 1), generator=g).float(),
                torch.randn(N, generator=g), (torch.rand(N, generator=g) < 0.5).float()]
        H.replay_add(ring, model.pos, *data)
        model.add(*[t.numpy() for t in data])
    assert model.full and all(torch.equal(a, torch.from_numpy(b)) for a, b in zip(ring, model.arr))
    assert torch.equal(ring[2].long().float(), ring[2])


def test_argmax_including_exact_ties():
    c = D.make_case(4, 3, 1, 8)
    with torch.no_grad():                                        # a last layer of zeros: q = bias, ties are exact
        w = list(c.nets.online.parameters())
        w[4].zero_()
        for bias, want in (([1.0, 1.0, 0.5], 0), ([0.5, 1.0, 1.0], 1), ([2.0, 2.0, 2.0], 0), ([0.0, -0.0, 0.0], 0), ([1.0, 2.0, 3.0], 2)):
            w[5].copy_(torch.tensor(bias))
            acts, q = torch.zeros(8, dtype=torch.int64), torch.zeros((8, 3))
            H.dqn_act(torch.randn(8, 4), D.flat(c.nets.online), 3, acts, q_out=q)
            assert torch.equal(acts, torch.argmax(q, dim=1)) and acts.tolist() == [want] * 8
    for O, n, na, M in ((4, 2, 1, 37), (8, 18, 1, 37), (4, 2, 51, 37), (8, 5, 101, 9)):
        c = D.make_case(O, n, na, M)
        out = D.run_entry_points(H, c, CPU)
        assert torch.equal(out["act"], torch.argmax(out["q"], dim=1))


@pytest.mark.parametrize("O,n,M", [(4, 2, 37), (8, 18, 128), (65, 3, 1)])
def test_td_target_given_the_target_networks_output(O, n, M):
    c = D.make_case(O, n, 1, M)
    out = D.run_entry_points(H, c, CPU)
    obs, act, nxt, done, rew = D.batch(c, torch.float32)
    target_max, _ = out["aux_a"].max(dim=1)
    assert torch.equal(out["aux_b"], rew.flatten() + c.gamma * target_max * (1 - done.flatten()))
    assert done.sum() > 0 or M == 1


def _projection_case(na, v_min, v_max, rewards, dones, gamma=0.99):
    """A ring whose rewards / dones are the given lists (slot m, env 0) and a batch that reads them in order."""
    M = len(rewards)
    c = D.make_case(4, 2, na, M, N=1, slots=M, v_min=v_min, v_max=v_max, gamma=gamma)
    c.ring[3][:, 0] = torch.tensor(rewards)
    c.ring[4][:, 0] = torch.tensor(dones)
    c.bi, c.ei = torch.arange(M), torch.zeros(M, dtype=torch.int64)
    return c


@pytest.mark.parametrize("na,v_min,v_max,gamma", [(5, -2.0, 2.0, 0.99), (5, -2.0, 2.0, 0.5), (101, -100.0, 100.0, 0.99), (51, -10.0, 10.0, 0.99)])
def test_projection_given_next_pmfs_is_the_references_bit_for_bit(na, v_min, v_max, gamma):
    """Rewards on atoms (b integral, the l == u branch), at both ends (b = 0 and n_atoms - 1), past both clamps, between atoms; done = 1
    puts all mass on one atom or splits it over two."""
    dz = (v_max - v_min) / (na - 1)
    rewards = [0.0, dz, -dz, v_min, v_max, v_min - 5.0, v_max + 5.0, 1.0, 0.3 * dz, -1.7 * dz, 2 * dz, v_max - dz, 1e-3, -1e-3]
    dones = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    rewards, dones = rewards + rewards, dones + [1.0 - d for d in dones]
    c = _projection_case(na, v_min, v_max, rewards, dones, gamma)
    out = D.run_entry_points(H, c, CPU)
    obs, act, nxt, done, rew = D.batch(c, torch.float32)
    want = D.projection(out["aux_a"], rew, done, c.atoms, c.gamma, c.v_min, c.v_max)
    assert torch.equal(out["aux_b"], want)
    b = ((rew + c.gamma * c.atoms * (1 - done)).clamp(v_min, v_max) - v_min) / (c.atoms[1] - c.atoms[0])
    assert (b == b.floor()).any() and (b == 0).any() and (b >= na - 1).any() and (b != b.floor()).any()      # the inputs hit the branches
    torch.testing.assert_close(want.sum(1), torch.ones(len(rewards)), rtol=0, atol=1e-5)


@pytest.mark.parametrize("O,n,na,M", [(4, 2, 1, 128), (65, 18, 1, 37), (4, 2, 101, 128), (8, 3, 51, 37), (65, 18, 28, 5), (8, 2, 5, 1)])
def test_forwards_losses_and_gradients_within_the_f32_references_bar(O, n, na, M):
    """Bar (DESIGN.md sections 3.11 / 3.13): within twice the f32 torch reference's own error against float64 autograd, plus 2e-6."""
    c = D.make_case(O, n, na, M)
    out = D.run_entry_points(H, c, CPU)
    ref = D.reference_c51 if na > 1 else D.reference_dqn
    r64, r32 = ref(c, torch.float64), ref(c, torch.float32)
    Nr = min(M, 11)
    obs = c.ring[0][c.bi[:Nr], c.ei[:Nr]]
    r64["q"], r32["q"] = D.reference_act(c, obs, torch.float64), D.reference_act(c, obs, torch.float32)
    for k in ("q", "aux_a", "aux_b", "scalars", "grads"):
        ok, err, own = D.within_bar(out[k], r64[k], r32[k])
        print(k, f"{err:.3e} (f32 reference {own:.3e})")
        assert ok, (k, err, own)


def test_the_clamps_dead_gradient():
    """A row whose taken-action pmf has atoms below 1e-5 and one above 1 - 1e-5: those atoms pass no gradient, as clamp's backward."""
    c = D.make_case(4, 2, 5, 3, N=1, slots=3)
    with torch.no_grad():
        w = list(c.nets.online.parameters())
        w[5].copy_(torch.tensor([30.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, -1.0, 0.5]))      # action 0: one atom takes (almost) all the mass
        w[4].mul_(0.01)
    c.online = D.flat(c.nets.online)
    c.ring[2][:, 0, 0] = torch.tensor([0.0, 1.0, 0.0])
    c.bi, c.ei = torch.arange(3), torch.zeros(3, dtype=torch.int64)
    out = D.run_entry_points(H, c, CPU)
    r64, r32 = D.reference_c51(c, torch.float64), D.reference_c51(c, torch.float32)
    n64 = D.copies(c, torch.float64)
    obs, act, nxt, done, rew = D.batch(c, torch.float64)
    _, old = n64.online.get_action(obs, act.flatten())
    assert (old[0] < 1e-5).sum() == 4 and (old[0] > 1 - 1e-5).sum() == 1 and ((old[1] > 1e-5) & (old[1] < 1 - 1e-5)).all()
    for k in ("scalars", "grads"):
        ok, err, own = D.within_bar(out[k], r64[k], r32[k])
        assert ok, (k, err, own)
    # rows 0 and 2 are dead: the whole gradient is row 1's
    c.M, c.bi, c.ei = 1, torch.tensor([1]), torch.zeros(1, dtype=torch.int64)
    alone = D.run_entry_points(H, c, CPU)
    torch.testing.assert_close(out["grads"] * 3, alone["grads"], rtol=1e-5, atol=1e-9)


def test_adam_with_c51s_eps_against_torch():
    g = torch.Generator().manual_seed(3)
    n = 10007
    eps = 0.01 / 128
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * 0.1 for _ in range(C.ADAM_STEPS)]
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([p], lr=2.5e-4, eps=eps)
    for gr in grads:
        p.grad = gr.clone()
        opt.step()
    hp, hm, hv = p0.clone(), torch.zeros(n), torch.zeros(n)
    for i, gr in enumerate(grads):
        H.clip_adam_(hp, gr.clone(), hm, hv, i + 1, 2.5e-4, math.inf, 1.0, eps=eps)
    torch.testing.assert_close(hp, p.detach(), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("na", [1, 5])
def test_out_of_range_indices_clamp_into_the_ring(na):
    c = D.make_case(4, 2, na, 6)
    c.bi = torch.tensor([-5, 0, c.slots - 1, c.slots, 10 ** 12, -(2 ** 40)])
    c.ei = torch.tensor([-1, 0, c.N - 1, c.N, 2 ** 33, -7])
    got = D.run_entry_points(H, c, CPU)
    c.bi, c.ei = c.bi.clamp(0, c.slots - 1), c.ei.clamp(0, c.N - 1)
    want = D.run_entry_points(H, c, CPU)
    assert all(D.same(got[k], want[k]) for k in want)


@pytest.mark.parametrize("shape", D.GUARD_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_twins_stay_inside_their_outputs(shape, monkeypatch):
    """Every output carved from a sentinel arena at its exact size: the guards are intact and the bits do not depend on the sentinel."""
    import bounds_cases as B

    B.check(D.bounds_case(*shape), H, CPU, monkeypatch)


def test_limits_are_refused_with_einval_before_any_launch():
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    for O, n, na in ((0, 2, 1), (513, 2, 1), (4, 1, 1), (4, 19, 1), (4, 2, 0), (4, 2, 102), (4, 6, 101), (4, 18, 29)):
        assert lib.mi355ppo_dqn_act_f32(p, p, p, p, None, 1, O, n, na, None) == -1
        assert b"n_actions" in lib.mi355ppo_last_error()
        assert lib.mi355ppo_dqn_act_f32_cpu(p, p, p, p, None, 1, O, n, na) == -1
        assert lib.mi355ppo_c51_fwd_bwd_f32(p, p, p, p, p, p, p, 4, 1, p, p, p, 0.99, -1.0, 1.0, p, p, None, None, 4, O, n, na, p, 1 << 30, None) == -1
        assert lib.mi355ppo_c51_fwd_bwd_f32_cpu(p, p, p, p, p, p, p, 4, 1, p, p, p, 0.99, -1.0, 1.0, p, p, None, None, 4, O, n, na) == -1
        assert lib.mi355ppo_c51_workspace_bytes(4, O, n, na) == 0
        if na == 1:
            assert lib.mi355ppo_dqn_td_fwd_bwd_f32(p, p, p, p, p, p, p, 4, 1, p, p, 0.99, p, p, None, None, 4, O, n, p, 1 << 30, None) == -1
            assert lib.mi355ppo_dqn_td_fwd_bwd_f32_cpu(p, p, p, p, p, p, p, 4, 1, p, p, 0.99, p, p, None, None, 4, O, n) == -1
            assert lib.mi355ppo_dqn_td_workspace_bytes(4, O, n) == 0
    assert lib.mi355ppo_c51_fwd_bwd_f32(p, p, p, p, p, p, p, 4, 1, p, p, p, 0.99, -1.0, 1.0, p, p, None, None, 4, 4, 2, 1, p, 1 << 30, None) == -1
    assert lib.mi355ppo_dqn_td_fwd_bwd_f32(p, p, p, p, p, p, p, 4, 1, p, p, 0.99, p, p, None, None, 4, 4, 2, p, 8, None) == -4
    assert lib.mi355ppo_dqn_td_workspace_bytes(128, 4, 2) == (2 * 128 + 16 * (120 * 4 + 120 + 84 * 120 + 84 + 2 * 84 + 2)) * 4


def test_the_learner_names_the_torch_backend_when_a_shape_is_outside_the_limits():
    from types import SimpleNamespace

    from cleanrl_amd.agents import C51Network
    from cleanrl_amd.learner_dqn import DQNLearner

    env = D.fake_env(4, 6)
    args = SimpleNamespace(buffer_size=16, batch_size=4, learning_rate=1e-3, n_atoms=101, v_min=-1, v_max=1, gamma=0.99)
    with pytest.raises(ValueError, match="MI355PPO_OFFPOLICY=torch"):
        DQNLearner(C51Network(env), C51Network(env), args, env, CPU, c51=True, backend="fused")


def test_the_host_replay_buffer_keeps_float_actions_for_its_existing_callers():
    from cleanrl_amd.learner_offpolicy import HostReplayBuffer

    assert HostReplayBuffer(8, 3, 2, CPU).actions.dtype == np.float32
    assert HostReplayBuffer(8, 3, 1, CPU, act_dtype=np.int64).actions.dtype == np.int64
