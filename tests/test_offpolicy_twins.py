"""The DDPG / TD3 host twins (csrc/host_twins.hip over csrc/offpolicy_rows.h) on the CPU: the parity bars of DESIGN.md section 3.13,
refusals, and the ring's wrap-around against a numpy model."""
import math

import numpy as np
import pytest
import torch

import offpolicy_cases as C
from cleanrl_amd import _lib
from cleanrl_amd import host_ops as H

CPU = torch.device("cpu")


def test_abi_version_and_symbols():
    assert _lib.ABI_VERSION // 10 == 27 and _lib.load().mi355ppo_version() // 10 == 27
    for n in ("replay_add", "ddpg_act", "td3_target", "td3_critic_fwd_bwd", "td3_actor_fwd_bwd", "polyak"):
        assert f"mi355ppo_{n}_f32" in _lib.SIGNATURES and f"mi355ppo_{n}_f32_cpu" in _lib.SIGNATURES


def test_ring_add_and_gather_follow_the_numpy_model():
    N, O, A, buffer_size = 2, 5, 3, 14                       # 7 slots: 17 adds wrap twice
    model = C.NumpyRing(buffer_size, N, O, A)
    ring = tuple(torch.zeros(a.shape) for a in model.arr)
    pos, full = 0, False
    rs = np.random.RandomState(0)
    for step in range(17):
        data = [rs.standard_normal((N, O)).astype(np.float32), rs.standard_normal((N, O)).astype(np.float32),
                rs.standard_normal((N, A)).astype(np.float32), rs.standard_normal(N).astype(np.float32), (rs.rand(N) < 0.5).astype(np.float32)]
        model.add(*data)
        H.replay_add(ring, pos, *[torch.from_numpy(d) for d in data])
        pos += 1
        if pos == model.slots:
            pos, full = 0, True
        assert (pos, full) == (model.pos, model.full)
        for t, a in zip(ring, model.arr):
            assert torch.equal(t, torch.from_numpy(a))
    with pytest.raises(_lib.Mi355PpoError, match="pos"):
        H.replay_add(ring, model.slots, *[torch.from_numpy(d) for d in data])


def test_polyak_is_bit_equal_to_the_reference_loop():
    g = torch.Generator().manual_seed(0)
    p, t = torch.randn(100003, generator=g), torch.randn(100003, generator=g)
    for tau in (0.005, 0.3, 1.0):
        want = tau * p + (1 - tau) * t
        assert torch.equal(H.polyak_(p, t.clone(), tau), want)


def test_td_target_is_bit_equal_given_the_target_outputs():
    """A critic whose first two layers are zero returns its last bias: q' is known exactly, so the target's arithmetic is isolated."""
    c = C.make_case(6, 3, 65, n_critics=2)
    P = c.target_critics.numel() // 2
    tc = torch.zeros_like(c.target_critics)
    tc[P - 1], tc[2 * P - 1] = 0.75, -1.25
    y = torch.zeros(c.M)
    H.td3_target(c.ring, c.bi, c.ei, c.target_actor, tc, 2, c.scale, c.bias, c.noise, 0.2, 0.5, -1.0, 1.0, 0.99, y)
    r, d = c.ring[3][c.bi, c.ei], c.ring[4][c.bi, c.ei]
    mq = torch.min(torch.full((c.M, 1), 0.75), torch.full((c.M, 1), -1.25))
    assert torch.equal(y, r.flatten() + (1 - d.flatten()) * 0.99 * mq.view(-1))


@pytest.mark.parametrize("O,A,M,n_critics,use_noise", [(17, 6, 256, 2, True), (17, 6, 32, 1, False), (3, 1, 1, 2, True), (40, 20, 70, 2, True)])
def test_twins_within_the_float64_bar(O, A, M, n_critics, use_noise):
    c = C.make_case(O, A, M, n_critics=n_critics, low=-2.0, high=2.0)
    got = C.run_entry_points(H, c, CPU, use_noise)
    y64, na64, _ = C.reference_target(c, torch.float64, use_noise)
    y32, na32, _ = C.reference_target(c, torch.float32, use_noise)
    checks = [("y", got["y"], y64, y32), ("next_actions", got["next_actions"], na64, na32)]
    g64, s64 = C.reference_critic(c, got["y"], torch.float64)
    g32, s32 = C.reference_critic(c, got["y"], torch.float32)
    checks += [("critic_grads", got["critic_grads"], g64, g32), ("critic_scalars", got["critic_scalars"], s64, s32)]
    a64, a32 = C.reference_actor(c, torch.float64), C.reference_actor(c, torch.float32)
    checks += [(nm, got[nm], r64, r32) for nm, r64, r32 in zip(("actor_grads", "actor_loss", "dq_daction"), a64, a32)]
    for nm, g, r64, r32 in checks:
        ok, err, own = C.within_bar(g.reshape(r64.shape), r64, r32)
        print(f"{nm}: err {err:.3e} reference's own {own:.3e}")
        assert ok, (nm, err, own)


def test_act_matches_the_reference_ops():
    c = C.make_case(17, 6, 16)
    x = c.ring[0][:, 0].contiguous()[:9]
    nz = torch.randn(6) * 0.1
    lo, hi = torch.full((6,), -0.5), torch.full((6,), 0.5)
    out = H.ddpg_act(x, c.actor, c.scale, c.bias, nz, lo, hi, torch.zeros(9, 6))
    with torch.no_grad():
        want64 = (c.nets.actor.double()(x.double()) + nz.double()).numpy().clip(-0.5, 0.5)
        c.nets.actor.float()
        want32 = (c.nets.actor(x) + nz).numpy().clip(-0.5, 0.5)
    ok, err, own = C.within_bar(out, torch.from_numpy(want64), torch.from_numpy(want32))
    assert ok, (err, own)
    assert out.min() >= -0.5 and out.max() <= 0.5


def test_adam_through_clip_adam_with_infinite_norm():
    """max_grad_norm = inf gives a clip coefficient of exactly 1: torch.optim.Adam (eps 1e-8) at rtol 1e-5 / atol 1e-7 over 12 steps."""
    g = torch.Generator().manual_seed(3)
    n = 70001
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * 10 ** float(torch.randint(-3, 2, (1,), generator=g)) for _ in range(C.ADAM_STEPS)]
    want = C.adam_reference(p0, grads)
    p, m, v = p0.clone(), torch.zeros(n), torch.zeros(n)
    for i, gr in enumerate(grads):
        gb = gr.clone()
        H.clip_adam_(p, gb, m, v, i + 1, 3e-4, math.inf, 1.0, eps=1e-8)
        assert not gb.any()
    torch.testing.assert_close(p, want, rtol=1e-5, atol=1e-7)


def test_twins_are_deterministic():
    c = C.make_case(11, 4, 100)
    a, b = C.run_entry_points(H, c, CPU), C.run_entry_points(H, c, CPU)
    assert all(C.same(a[k], b[k]) for k in a)


@pytest.mark.parametrize("O,A", [(513, 6), (17, 21), (0, 3)])
def test_width_limits_are_einval(O, A):
    lib = _lib.load()
    buf = torch.zeros(8)
    p = buf.data_ptr()
    rc = lib.mi355ppo_ddpg_act_f32_cpu(p, p, p, p, None, p, p, p, 1, O, A)
    assert rc != 0 and b"obs_dim" in lib.mi355ppo_last_error()
    rc = lib.mi355ppo_td3_critic_fwd_bwd_f32_cpu(p, p, p, p, 4, 1, p, 2, p, p, p, 1, O, A)
    assert rc != 0 and b"obs_dim" in lib.mi355ppo_last_error()
    assert not buf.any()


def test_refusals_leave_outputs_untouched():
    c = C.make_case(5, 2, 8, n_critics=1)
    args = lambda y: (c.ring, c.bi, c.ei, c.target_actor, c.target_critics, 1, c.scale, c.bias, None, 0.2, 0.5, -1.0, 1.0, 0.99, y)  # noqa: E731
    y64 = torch.full((8,), 7.0, dtype=torch.float64)
    with pytest.raises(TypeError):
        H.td3_target(*args(y64))
    assert (y64 == 7).all()
    ync = torch.full((8, 2), 7.0)[:, 0]
    with pytest.raises(ValueError):
        H.td3_target(*args(ync))
    short = torch.full((7,), 7.0)
    with pytest.raises(ValueError):
        H.td3_target(*args(short))
    assert (ync == 7).all() and (short == 7).all()
    g = torch.full((c.critics.numel() - 1,), 7.0)
    with pytest.raises(ValueError):
        H.td3_critic_fwd_bwd(c.ring, c.bi, c.ei, c.critics, 1, torch.zeros(8), g, torch.zeros(2))
    assert (g == 7).all()
    with pytest.raises(_lib.Mi355PpoError, match="n_critics"):
        H.td3_critic_fwd_bwd(c.ring, c.bi, c.ei, torch.zeros(3 * c.critics.numel()), 3, torch.zeros(8), torch.zeros(3 * c.critics.numel()),
                             torch.zeros(6))


def test_learner_refuses_wide_shapes_naming_the_switch():
    from types import SimpleNamespace

    from cleanrl_amd.learner_offpolicy import OffPolicyLearner

    env = C.fake_env(17, 21)
    c = C.make_case(17, 21, 4, n_critics=1)
    args = SimpleNamespace(buffer_size=8, batch_size=4, learning_rate=3e-4)
    with pytest.raises(ValueError, match="MI355PPO_OFFPOLICY=torch"):
        OffPolicyLearner(c.nets.actor, c.nets.qfs, c.nets.target_actor, c.nets.qf_targets, args, env, CPU, td3=False, backend="fused")
