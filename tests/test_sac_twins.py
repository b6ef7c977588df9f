"""The SAC host twins (csrc/host_twins.hip over csrc/sac_rows.h) on the CPU: op_exp / op_log against float64, the parity bars of
DESIGN.md section 3.14 against float64 autograd of the reference's ops, the min backward on a tie, the bit-equal pieces, refusals."""
import numpy as np
import pytest
import torch

import offpolicy_cases as C
import sac_cases as S
from cleanrl_amd import _lib
from cleanrl_amd import host_ops as H

CPU = torch.device("cpu")
ENTRY_POINTS = ("sac_policy", "sac_target", "sac_actor_fwd_bwd", "sac_alpha")


def test_abi_version_and_symbols():
    assert _lib.ABI_VERSION == 271 and _lib.load().mi355ppo_version() == 271
    for n in ENTRY_POINTS:
        assert f"mi355ppo_{n}_f32" in _lib.SIGNATURES and f"mi355ppo_{n}_f32_cpu" in _lib.SIGNATURES


def _max_rel(got, want64):
    return ((got.double() - want64).abs() / want64.abs()).max().item()


def test_op_exp_and_op_log_against_float64():
    """Bar: the maximum relative error against float64 is at most twice torch float32's own on the same grid plus one f32 ulp."""
    xe = torch.linspace(-20.0, 5.0, 2_000_001, dtype=torch.float64).float()
    xl = torch.cat([torch.logspace(-6, 3, 2_000_001, dtype=torch.float64).float(), 1.0 + torch.arange(-2000, 2001) * 2.0 ** -23])
    xl = xl[(xl >= 1e-6) & (xl <= 1e3) & (xl != 1.0)]                       # log(1) = 0 has no relative error
    e, _ = H.sac_exp_log(xe)
    _, l = H.sac_exp_log(xl)
    ee, own_e = _max_rel(e, xe.double().exp()), _max_rel(xe.exp(), xe.double().exp())
    el, own_l = _max_rel(l, xl.double().log()), _max_rel(xl.log(), xl.double().log())
    print(f"op_exp: {ee:.3e} (torch f32 {own_e:.3e})   op_log: {el:.3e} (torch f32 {own_l:.3e})")
    assert ee <= 2 * own_e + 1.2e-7, (ee, own_e)
    assert el <= 2 * own_l + 1.2e-7, (el, own_l)
    one = torch.tensor([1.0, float("nan"), 0.0])
    e, l = H.sac_exp_log(one)
    assert l[0] == 0.0 and e[2] == 1.0 and e[1].isnan() and l[1].isnan()


@pytest.mark.parametrize("O,A,M", S.SHAPES)
def test_twins_within_the_float64_bar(O, A, M):
    c = S.make_case(O, A, M)
    got = S.run_entry_points(H, c, CPU)
    r64, r32 = S.reference(c, torch.float64), S.reference(c, torch.float32)
    for nm in ("y", "next_actions", "next_log_pi", "log_pi", "pi", "actor_grads", "actor_loss", "dmean", "du", "log_pi2", "alpha_loss",
               "log_alpha"):
        ok, err, own = C.within_bar(got[nm].reshape(r64[nm].shape), r64[nm], r32[nm])
        print(f"{nm}: err {err:.3e} reference's own {own:.3e}")
        assert ok, (nm, err, own)
    # the other flat gradient: the critic step (n_critics = 2) on the twin's own SAC target, as DESIGN 3.13 does for TD3's
    (g64, s64), (g32, s32) = S.reference_critic(c, got["y"], torch.float64), S.reference_critic(c, got["y"], torch.float32)
    for nm, r64c, r32c in (("critic_grads", g64, g32), ("critic_scalars", s64, s32)):
        ok, err, own = C.within_bar(got[nm], r64c, r32c)
        print(f"{nm}: err {err:.3e} reference's own {own:.3e}")
        assert ok, (nm, err, own)
    assert torch.equal(got["log_pi"], got["log_pi_policy"]) and torch.equal(got["pi"], got["pi_dense"])
    assert torch.equal(got["alpha"], H.sac_exp_log(got["log_alpha"])[0])
    # saturated entries: y is exactly +-1, so the action is the bound, log(1e-6) enters log_pi and the head gradient at mean is zero
    assert len(c.sat) >= 2 or M == 1
    for r, a, v in c.sat:
        assert got["pi"][r, a] == (S.HIGH if v > 0 else S.LOW) and abs(r64["y_t"][r, a]) == 1, (r, a, v)
        assert got["dmean"][r, a] == 0 and got["du"][r, a] != 0, (r, a, v)
    assert torch.isfinite(got["log_pi"]).all() and torch.isfinite(got["actor_grads"]).all()


def test_a_nan_eps_stays_in_its_row():
    c, ref = S.make_case(17, 6, 70, nan_row=13), S.make_case(17, 6, 70)
    got, want = S.run_entry_points(H, c, CPU), S.run_entry_points(H, ref, CPU)
    rows = torch.arange(70) != 13
    for nm in ("y", "next_actions", "next_log_pi", "log_pi", "pi", "dmean", "du", "log_pi2"):
        assert got[nm][13].isnan().any(), nm
        assert torch.equal(got[nm][rows], want[nm][rows]), nm


def test_min_backward_splits_a_tie_half_and_half():
    """Both critics with the same parameters: q1 == q2 in every row, so d loss / d action is 0.5 of each critic's -- the gradients
    equal those of the untied formula on one critic, and torch's autograd of torch.min agrees."""
    c = S.make_case(17, 6, 70, tie_row=0, saturate=False)
    got = S.run_entry_points(H, c, CPU)
    r64, r32 = S.reference(c, torch.float64), S.reference(c, torch.float32)
    for nm in ("dmean", "du", "actor_grads", "actor_loss"):
        ok, err, own = C.within_bar(got[nm].reshape(r64[nm].shape), r64[nm], r32[nm])
        assert ok, (nm, err, own)
    a, b = torch.tensor([1.0, 2.0, 3.0], requires_grad=True), torch.tensor([1.0, 3.0, 2.0], requires_grad=True)
    torch.min(a, b).sum().backward()
    assert a.grad.tolist() == [0.5, 1.0, 0.0] and b.grad.tolist() == [0.5, 0.0, 1.0]


def test_min_weights_on_a_forced_tie_between_distinct_critics():
    """Two different critics whose q agree bit for bit in row 0 (the second's last bias is set to q1 minus its own pre-bias value)
    and differ in row 1.  With (qf_a, qf_a) the kernel's gradient at mean is qf_a's own, with (qf_b, qf_b) qf_b's; with (qf_a, qf_b)
    row 0 must be their half-and-half mean, which differs from either, and row 1 must be the smaller critic's, bit for bit."""
    c = S.make_case(17, 6, 2, saturate=False)
    Pq = c.critics.numel() // 2
    qa, qb = c.critics[:Pq].clone(), c.critics[Pq:].clone()
    pi = torch.zeros(2, 6)
    H.sac_policy(c.ring[0], c.actor, c.scale, c.bias, c.eps[1], actions_out=pi, batch_inds=c.bi, env_inds=c.ei)
    ring = tuple(t.clone() for t in c.ring)
    ring[2][c.bi, c.ei] = pi                                   # the critic step then evaluates q(obs, pi) in the actor kernel's order

    def q_of(critics, row):                                    # a one-row batch: the scalars' means are that row's q, exactly
        sc = torch.zeros(4)
        H.td3_critic_fwd_bwd(ring, c.bi[row:row + 1].clone(), c.ei[row:row + 1].clone(), critics, 2, torch.zeros(1), torch.zeros(2 * Pq), sc)
        return sc[0].item(), sc[2].item()

    assert (c.bi[0], c.ei[0]) != (c.bi[1], c.ei[1])
    qb[-1] = 0.0
    q1, pre = q_of(torch.cat([qa, qb]), 0)
    b = np.float32(q1) - np.float32(pre)
    for _ in range(8):                                         # pre + b == q1 in float32, nudging b by an ulp if the sum rounds away
        tot = np.float32(pre) + b
        if tot == np.float32(q1):
            break
        b = np.nextafter(b, np.float32(np.inf) if tot < np.float32(q1) else np.float32(-np.inf))
    qb[-1] = float(b)
    t0, t1 = q_of(torch.cat([qa, qb]), 0), q_of(torch.cat([qa, qb]), 1)
    assert t0[0] == t0[1] and t1[0] != t1[1]

    def dmean(critics):
        g, l, dm = torch.zeros(c.actor.numel()), torch.zeros(1), torch.zeros(2, 6)
        H.sac_actor_fwd_bwd(c.ring, c.bi, c.ei, c.actor, critics, c.scale, c.bias, c.eps[1], c.alpha, g, l, None, dm, None)
        return dm

    da, db, dt = dmean(torch.cat([qa, qa])), dmean(torch.cat([qb, qb])), dmean(torch.cat([qa, qb]))
    gap = (da[0] - db[0]).abs().max().item()
    half = (dt[0] - 0.5 * (da[0] + db[0])).abs().max().item()
    print(f"row 0: |d_a - d_b| {gap:.3e}, |d_tie - mean| {half:.3e}")
    # d mean is a few float32 operations on the two gradients: the mean is met to rounding (1e-6 relative), far below the gap
    assert half <= 1e-6 * max(da[0].abs().max().item(), db[0].abs().max().item()) and gap > 1e3 * max(half, 1e-12)
    assert torch.equal(dt[1], da[1] if t1[0] < t1[1] else db[1])


def test_td_target_is_bit_equal_given_min_q_log_pi_and_alpha():
    """Target critics whose first two layers are zero return their last bias: min_q is known exactly, log_pi is the twin's own."""
    c = S.make_case(6, 3, 65)
    P = c.target_critics.numel() // 2
    tc = torch.zeros_like(c.target_critics)
    tc[P - 1], tc[2 * P - 1] = 0.75, -1.25
    y, lp = torch.zeros(c.M), torch.zeros(c.M)
    H.sac_target(c.ring, c.bi, c.ei, c.actor, tc, c.scale, c.bias, c.eps[0], c.alpha, S.GAMMA, y, None, lp)
    r, d = c.ring[3][c.bi, c.ei], c.ring[4][c.bi, c.ei]
    alpha = c.alpha.item()
    mq = torch.min(torch.full((c.M, 1), 0.75), torch.full((c.M, 1), -1.25)) - alpha * lp.view(-1, 1)
    assert torch.equal(y, r.flatten() + (1 - d.flatten()) * S.GAMMA * mq.view(-1))


def test_polyak_over_the_critics_segment_and_the_gather_are_bit_equal():
    c = S.make_case(17, 6, 33)
    tgt = c.target_critics.clone()
    want = 0.005 * c.critics + (1 - 0.005) * tgt
    assert torch.equal(H.polyak_(c.critics, tgt, 0.005), want)
    # the ring gather: a network-free check through the dense and the gathered forms of the policy entry point
    dense = c.ring[0][c.bi, c.ei].contiguous()
    a, b = torch.zeros(33, 6), torch.zeros(33, 6)
    H.sac_policy(dense, c.actor, c.scale, c.bias, c.eps[0], actions_out=a)
    H.sac_policy(c.ring[0], c.actor, c.scale, c.bias, c.eps[0], actions_out=b, batch_inds=c.bi, env_inds=c.ei)
    assert torch.equal(a, b)


def test_twins_are_deterministic():
    c = S.make_case(11, 4, 100)
    a, b = S.run_entry_points(H, c, CPU), S.run_entry_points(H, c, CPU)
    assert all(C.same(a[k], b[k]) for k in a)


def test_scalar_adam_of_the_alpha_step_against_torch():
    """12 steps on one element against torch.optim.Adam at the optimizer bar of DESIGN.md section 3.13 (rtol 1e-5 / atol 1e-7)."""
    g = torch.Generator().manual_seed(1)
    lps = [torch.randn(50, generator=g) * 3 - 4 for _ in range(C.ADAM_STEPS)]
    te = -6.0
    log_alpha = torch.zeros(1, requires_grad=True)
    opt = torch.optim.Adam([log_alpha], lr=1e-3)
    st = torch.zeros(5)
    s = [st[i:i + 1] for i in range(5)]
    for i, lp in enumerate(lps):
        loss = (-log_alpha.exp() * (lp.view(-1, 1) + te)).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        H.sac_alpha_(lp, te, s[0], s[1], s[2], i + 1, 1e-3, s[3], s[4])
        torch.testing.assert_close(s[4], loss.detach().reshape(1), rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(s[0], log_alpha.detach(), rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(s[3], log_alpha.detach().exp(), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("O,A,M", [(513, 6, 4), (17, 21, 4), (17, 6, 0)])
def test_limits_are_einval_and_leave_outputs_untouched(O, A, M):
    lib = _lib.load()
    buf, idx = torch.zeros(64), torch.zeros(8, dtype=torch.int64)
    p, q = buf.data_ptr(), idx.data_ptr()
    calls = [lambda: lib.mi355ppo_sac_policy_f32_cpu(p, None, None, 0, 0, p, p, p, p, p, p, M, O, A),
             lambda: lib.mi355ppo_sac_target_f32_cpu(p, p, p, q, q, 4, 1, p, p, p, p, p, p, 0.99, p, None, None, M, O, A),
             lambda: lib.mi355ppo_sac_actor_fwd_bwd_f32_cpu(p, q, q, 4, 1, p, p, p, p, p, p, p, p, None, None, None, M, O, A)]
    for call in calls:
        assert call() == -1 and b"obs_dim" in lib.mi355ppo_last_error()
    assert lib.mi355ppo_sac_alpha_f32_cpu(p, 0, -6.0, p, p, p, 1e-3, 0.9, 0.999, 1e-8, 1, p, p) == -1
    assert not buf.any()


def test_null_pointers_are_einval():
    lib = _lib.load()
    buf, idx = torch.zeros(64), torch.zeros(8, dtype=torch.int64)
    p, q = buf.data_ptr(), idx.data_ptr()
    assert lib.mi355ppo_sac_policy_f32_cpu(p, None, None, 0, 0, p, p, p, p, None, None, 4, 3, 2) == -1
    assert lib.mi355ppo_sac_policy_f32_cpu(p, q, None, 4, 1, p, p, p, p, p, p, 4, 3, 2) == -1
    assert lib.mi355ppo_sac_target_f32_cpu(p, p, p, q, q, 4, 1, p, p, p, p, p, None, 0.99, p, None, None, 4, 3, 2) == -1
    assert lib.mi355ppo_sac_actor_fwd_bwd_f32_cpu(p, q, q, 4, 1, p, p, p, p, None, p, p, p, None, None, None, 4, 3, 2) == -1
    assert lib.mi355ppo_sac_alpha_f32_cpu(p, 4, -6.0, None, p, p, 1e-3, 0.9, 0.999, 1e-8, 1, p, p) == -1
    assert lib.mi355ppo_sac_exp_log_f32_cpu(p, None, None, 4) == -1
    assert b"null" in lib.mi355ppo_last_error() and not buf.any()


def test_learner_refuses_wide_shapes_naming_the_switch():
    from types import SimpleNamespace

    from cleanrl_amd.agents import ActionValueNetwork, SoftActor
    from cleanrl_amd.learner_sac import SACLearner

    env = C.fake_env(17, 21)
    args = SimpleNamespace(buffer_size=8, batch_size=4, q_lr=1e-3, policy_lr=3e-4, autotune=True, alpha=0.2)
    nets = [SoftActor(env)] + [ActionValueNetwork(env) for _ in range(4)]
    with pytest.raises(ValueError, match="MI355PPO_OFFPOLICY=torch"):
        SACLearner(*nets, args, env, CPU, backend="fused")
    assert np.prod(env.single_action_space.shape) == 21
