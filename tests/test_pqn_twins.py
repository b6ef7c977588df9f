"""PQN host twins (csrc/pqn.hip's row math on the CPU, cleanrl_amd/host_ops.py) against the reference's lines: Q(lambda) and
e-greedy bit for bit against torch on the CPU, the TD loss and the LayerNorm MLP against float64 autograd at the f32 reference's
bar, clip + RAdam against torch.optim.RAdam + clip_grad_norm_."""
import numpy as np
import pytest
import torch

import pqn_cases as C
from cleanrl_amd import host_ops as H

NAN, INF = float("nan"), float("inf")


def _same(a, b):
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def _qlambda_inputs(T, N, A, seed):
    g = torch.Generator().manual_seed(seed)
    r = torch.randn((T, N), generator=g)
    d = (torch.rand((T, N), generator=g) < 0.2).float()
    v = torch.randn((T, N), generator=g) * 3
    nd = (torch.rand((N,), generator=g) < 0.5).float()
    nq = torch.randn((N, A), generator=g)
    return r, d, v, nd, nq


@pytest.mark.parametrize("T,N,A", [(16, 4, 2), (1, 3, 4), (128, 65, 6), (7, 130, 18), (33, 1, 1)])
@pytest.mark.parametrize("gamma,lam", [(0.99, 0.65), (0.9, 0.0), (0.999, 1.0), (0.97, 0.3)])
def test_qlambda_twin_bit_exact(T, N, A, gamma, lam):
    r, d, v, nd, nq = _qlambda_inputs(T, N, A, seed=T * 131 + N)
    d[0] = 1.0                                   # dones at t = 0 and at T - 1
    d[-1, : N // 2 + 1] = 1.0
    ref = C.reference_qlambda(r, d, v, nd, nq, gamma, lam)
    assert _same(H.pqn_qlambda(r, d, v, nd, nq, gamma, lam), ref)


def test_qlambda_twin_nan_and_inf_in_next_q():
    T, N, A = 9, 70, 5
    r, d, v, nd, nq = _qlambda_inputs(T, N, A, seed=7)
    nq[0, 2] = NAN
    nq[1, :] = NAN
    nq[2, 0], nq[2, 3] = NAN, INF
    nq[3, 1] = INF
    nq[4, :] = -INF
    nq[5, 4] = -INF
    nd[:] = 0.0
    nd[6] = 1.0
    ref = C.reference_qlambda(r, d, v, nd, nq, 0.99, 0.65)
    out = H.pqn_qlambda(r, d, v, nd, nq, 0.99, 0.65)
    assert _same(out, ref)
    assert out[:, :3].isnan().any() and out[-1, 3].isinf()


def _egreedy(q, rnd, u, eps):
    N = q.shape[0]
    act, val, a64 = torch.empty(N), torch.empty(N), torch.empty(N, dtype=torch.int64)
    H.pqn_egreedy(q, rnd, u, eps, act, val, a64)
    return act, val, a64


@pytest.mark.parametrize("A", [1, 2, 4, 18])
def test_egreedy_twin_bit_exact(A):
    N = 300
    g = torch.Generator().manual_seed(A)
    q = torch.randint(-2, 3, (N, A), generator=g).float()            # many ties
    q[0] = 1.0                                                           # an all-equal row
    q[1, -1] = NAN
    q[2, :] = NAN
    q[3, 0] = -INF
    q[4, :] = -INF
    if A > 2:
        q[5, 1], q[5, 2] = NAN, INF
        q[6, 2], q[6, 1] = NAN, NAN
    rnd = torch.randint(0, A, (N,), generator=g)
    u = torch.rand((N,), generator=g)
    for eps in (0.0, 1.0, 0.37, float(u[7]), float(np.nextafter(np.float32(u[8]), np.float32(1))) + 1e-12):
        ref_a, ref_v = C.reference_egreedy(q, rnd, u, eps)
        act, val, a64 = _egreedy(q, rnd, u, eps)
        assert torch.equal(a64, ref_a) and torch.equal(act, ref_a.float()), eps
        assert _same(val, ref_v), eps


def test_egreedy_compares_against_f32_epsilon():
    """torch rounds the Python epsilon to f32 before ``u < epsilon``: with u == f32(eps) and eps slightly above u in double the
    result is False."""
    u = torch.tensor([0.3], dtype=torch.float32)
    eps = float(u[0]) + 1e-12
    assert float(np.float32(eps)) == float(u[0])
    ref = (u < eps)
    act, _, a64 = _egreedy(torch.tensor([[0.0, 1.0]]), torch.tensor([0]), u, eps)
    assert not bool(ref[0]) and int(a64[0]) == 1


@pytest.mark.parametrize("M,A,B", [(1, 2, 8), (63, 3, 100), (65, 18, 512), (512, 6, 2048)])
def test_td_loss_twin_within_the_f32_bar(M, A, B):
    g = torch.Generator().manual_seed(M + A)
    q = torch.randn((M, A), generator=g) * 4
    mb = torch.randperm(B, generator=g)[:M]
    b_actions = torch.randint(0, A, (B,), generator=g).float()
    b_returns = torch.randn((B,), generator=g) * 5
    l64, m64, dq64 = C.reference_td(q.double(), mb, b_actions, b_returns.double())
    l32, m32, dq32 = C.reference_td(q, mb, b_actions, b_returns)
    dq, sc = H.pqn_td_loss(q, mb, b_actions, b_returns)
    for got, r64, r32 in ((dq, dq64, dq32), (sc[0:1], l64.reshape(1), l32.reshape(1)), (sc[1:2], m64.reshape(1), m32.reshape(1))):
        ok, err, own = C.within_bar(got, r64, r32)
        assert ok, (err, own)
    assert torch.equal((dq != 0).sum(1) <= 1, torch.ones(M, dtype=torch.bool))


MLP_SHAPES = [(4, 2, 1), (6, 3, 63), (8, 18, 65), (64, 2, 512), (4, 18, 512), (64, 3, 63)]


@pytest.mark.parametrize("O,A,M", MLP_SHAPES)
def test_mlp_twin_within_the_f32_bar(O, A, M):
    params = C.random_mlp_params(O, A, seed=O * 7 + A)
    B = M + 17
    g = torch.Generator().manual_seed(M)
    b_obs = torch.randn((B, O), generator=g) * 2
    mb = torch.randperm(B, generator=g)[:M]
    b_actions = torch.randint(0, A, (B,), generator=g).float()
    b_returns = torch.randn((B,), generator=g) * 3
    q64, l64, m64, g64 = C.reference_mlp_td(params, O, A, b_obs, mb, b_actions, b_returns, torch.float64)
    q32, l32, m32, g32 = C.reference_mlp_td(params, O, A, b_obs, mb, b_actions, b_returns, torch.float32)
    q = H.pqn_mlp_forward(b_obs[mb].contiguous(), params, A)
    ok, err, own = C.within_bar(q, q64, q32)
    assert ok, ("q", err, own)
    grads = torch.empty_like(params)
    sc = H.pqn_mlp_td_fwd_bwd(b_obs, mb, params, b_actions, b_returns, grads, A)
    ok, err, own = C.within_bar(grads, g64, g32)
    assert ok, ("grads", err, own)
    for got, r64, r32 in ((sc[0:1], l64.reshape(1), l32.reshape(1)), (sc[1:2], m64.reshape(1), m32.reshape(1))):
        ok, err, own = C.within_bar(got, r64, r32)
        assert ok, ("scalars", err, own)
    # act = forward + e-greedy of the same rows
    N = M
    rnd = torch.randint(0, A, (N,), generator=g)
    u = torch.rand((N,), generator=g)
    act, val, a64 = torch.empty(N), torch.empty(N), torch.empty(N, dtype=torch.int64)
    obs_row_out, dstore, din = torch.empty((N, O)), torch.empty(N), torch.rand(N, generator=g)
    x = b_obs[mb].contiguous()
    H.pqn_mlp_act(x, params, A, rnd, u, 0.25, act, val, a64, obs_row_out=obs_row_out, done_in=din, done_row_out=dstore)
    ref_a, ref_v = C.reference_egreedy(q, rnd, u, 0.25)
    assert torch.equal(a64, ref_a) and torch.equal(val, ref_v)
    assert torch.equal(obs_row_out, x) and torch.equal(dstore, din)


def test_mlp_refuses_unsupported_shapes():
    with pytest.raises(Exception, match="obs_dim"):
        H.pqn_mlp_forward(torch.zeros((2, 65)), torch.zeros(H.pqn_param_count(65, 2)), 2)
    with pytest.raises(Exception, match="n_actions"):
        H.pqn_mlp_forward(torch.zeros((2, 4)), torch.zeros(H.pqn_param_count(4, 19)), 19)


def test_clip_radam_twin_against_torch():
    """12 steps (1 - 5 unrectified, 6 on rectified) with one hard-clipped step, against optim.RAdam + clip_grad_norm_ on the CPU."""
    torch.manual_seed(0)
    shapes = [(120, 4), (120,), (120,), (120,), (84, 120), (84,), (3, 84), (3,)]
    ps = [torch.randn(s) * 0.3 for s in shapes]
    ref = [torch.nn.Parameter(p.clone()) for p in ps]
    opt = torch.optim.RAdam(ref, lr=2.5e-4)
    flat = torch.cat([p.reshape(-1) for p in ps])
    m, v, grads = torch.zeros_like(flat), torch.zeros_like(flat), torch.zeros_like(flat)
    for step in range(1, 13):
        lr = 2.5e-4 * (1.0 - (step - 1) / 12)
        scale = 50.0 if step == 7 else 0.05
        gs = [torch.randn(s) * scale for s in shapes]
        for p, gg in zip(ref, gs):
            p.grad = gg.clone()
        opt.param_groups[0]["lr"] = lr
        tn = torch.nn.utils.clip_grad_norm_(ref, 10.0)
        opt.step()
        grads.copy_(torch.cat([gg.reshape(-1) for gg in gs]))
        total = H.clip_radam_(flat, grads, m, v, step, lr, 10.0)
        assert abs(float(total) - float(tn)) <= 1e-5 * float(tn)
        assert torch.count_nonzero(grads) == 0
        want = torch.cat([p.detach().reshape(-1) for p in ref])
        np.testing.assert_allclose(flat.numpy(), want.numpy(), rtol=1e-5, atol=1e-7)
    assert float(tn) < 10.0  # the last steps are not clipped; step 7 was
    sched = [H.radam_schedule(2.5e-4, s)[4] for s in range(1, 8)]
    assert sched == [0.0] * 5 + [1.0, 1.0]


# ------------------------------------------------------------------------------------------- caller-owned outputs
def _bad_outputs(good):
    """``good`` (a contiguous CPU tensor a twin writes) -> its float64 copy, a non-contiguous view of the same shape and a tensor one
    element short, each with the exception the wrapper owes."""
    wide = torch.zeros(tuple(good.shape[:-1]) + (2 * good.shape[-1],), dtype=good.dtype)[..., ::2]
    assert wide.shape == good.shape and (good.numel() == 1 or not wide.is_contiguous())      # (one element is always contiguous)
    other = torch.float64 if good.dtype == torch.float32 else torch.int32
    return [(torch.zeros(good.shape, dtype=other), TypeError), (torch.zeros(good.numel() - 1, dtype=good.dtype), ValueError)] + \
        [(wide, ValueError)] * (good.numel() > 1)


def _refuses(call, outputs):
    """``call(**outputs)`` is fine; with any one output swapped for a bad one it raises and no output is written."""
    call(**{k: v.clone() for k, v in outputs.items()})
    for name, good in outputs.items():
        for bad, exc in _bad_outputs(good):
            kw = {k: torch.full(v.shape, 7, dtype=v.dtype) for k, v in outputs.items()}
            kw[name] = bad.fill_(7) if bad.is_contiguous() else bad.copy_(torch.full(bad.shape, 7, dtype=bad.dtype))
            with pytest.raises(exc):
                call(**kw)
            assert all(bool((v == 7).all()) for v in kw.values()), (name, exc)


def test_twins_refuse_caller_owned_outputs_they_would_overrun():
    N, O, A, T = 5, 4, 3, 6
    g = torch.Generator().manual_seed(3)
    obs, q = torch.randn((N, O), generator=g), torch.randn((N, A), generator=g)
    params = torch.randn(H.pqn_param_count(O, A), generator=g) * 0.1
    rnd, u = torch.randint(0, A, (N,), generator=g), torch.rand(N, generator=g)
    f, i64 = (lambda *s: torch.zeros(s)), (lambda *s: torch.zeros(s, dtype=torch.int64))
    _refuses(lambda **o: H.pqn_egreedy(q, rnd, u, 0.1, **o), dict(actions_out=f(N), values_out=f(N), action_i64_out=i64(N)))
    _refuses(lambda **o: H.pqn_mlp_act(obs, params, A, rnd, u, 0.1, done_in=torch.zeros(N), **o),
             dict(actions_out=f(N), values_out=f(N), action_i64_out=i64(N), obs_row_out=f(N, O), done_row_out=f(N)))
    r, d, v, nd, nq = _qlambda_inputs(T, N, A, seed=5)
    _refuses(lambda **o: H.pqn_qlambda(r, d, v, nd, nq, 0.99, 0.65, **o), dict(returns=f(T, N)))
    inds, ba, br = torch.tensor([3, 0, 4, 1, 2]), torch.randint(0, A, (N,)).float(), torch.randn(N, generator=g)
    _refuses(lambda **o: H.pqn_td_loss(q, inds, ba, br, **o), dict(dq=f(N, A), scalars=f(2)))
    _refuses(lambda **o: H.pqn_mlp_forward(obs, params, A, **o), dict(q_out=f(N, A)))
    _refuses(lambda **o: H.pqn_mlp_td_fwd_bwd(obs, inds, params, ba, br, n_actions=A, **o), dict(grads=f(params.numel()), scalars=f(2)))
    n = 16
    # (params defines n: a shorter one is a smaller update, so it is tried for dtype and layout only)
    _refuses(lambda **o: H.clip_radam_(torch.ones(n), step=1, lr=1e-3, max_grad_norm=0.5, **o),
             dict(grads=torch.ones(n), exp_avg=f(n), exp_avg_sq=f(n), total_norm_out=f(1)))
    for bad, exc in _bad_outputs(torch.ones(n))[::2]:
        with pytest.raises(exc):
            H.clip_radam_(bad, torch.ones(n), f(n), f(n), step=1, lr=1e-3, max_grad_norm=0.5)
