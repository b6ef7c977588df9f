"""The distribution kernels (K2 / K2': Categorical and Normal log-prob / entropy, forward and backward), the Normal and the
Categorical K3 loss and the advantage statistics against float64 autograd of the reference's lines, at the C ABI and through the ``ops`` wrappers and the agents.

One reference everywhere: the f32 inputs cast up to float64 and run through oracle/torch_oracle.py (pinned to the reference-line
goldens by tests/test_oracle_golden.py), on the device so the large sizes stay fast.  Cases and bars live in tests/dist_cases.py,
shared with the host twins' float64 tests (tests/test_host_twins_float64.py).  Values only: every call here is a valid call or
one the library refuses before it launches anything."""
import copy
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dist_cases as C
from cleanrl_amd import _lib, agents, envs as E, ops
from oracle import torch_oracle as TO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -1          # MI355PPO_EINVAL (include/mi355ppo.h)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cat_bwd_abi(logits, a64, af, g_lp, g_ent, A=None):
    """mi355ppo_categorical_logprob_entropy_bwd_f32 straight through ctypes (null g pointers allowed) -> (status, dlogits)."""
    B = logits.shape[0]
    A = logits.shape[1] if A is None else A
    out = torch.full((B, logits.shape[1]), 7.0, device=DEV)
    st = _lib.load().mi355ppo_categorical_logprob_entropy_bwd_f32(_p(logits), _p(a64), _p(af), _p(g_lp), _p(g_ent), _p(out), B, A,
                                                                  _stream())
    return st, out


def _normal_bwd_abi(mean, logstd, action, g_lp, g_ent):
    B, D = mean.shape
    dmean, drows = torch.empty_like(mean), torch.empty_like(mean)
    st = _lib.load().mi355ppo_normal_logprob_entropy_bwd_f32(_p(mean), _p(logstd), _p(action), _p(g_lp), _p(g_ent), _p(dmean),
                                                             _p(drows), B, D, _stream())
    _lib.check(st, "mi355ppo_normal_logprob_entropy_bwd_f32")
    return dmean, drows


# ======================================================================= K2  Categorical forward + backward
def _cat_small():
    for A in C.CAT_A:
        for regime in C.REGIMES:
            if regime == "masked" and A == 1:
                continue              # a one-action row with its only entry masked has no distribution (float64 gives NaN)
            for B in (1, 63, 257):
                yield B, A, regime


def _cat_large():
    for B in (65535, 65536, 65537, 300007):             # block_for switches from 64 to 256 lanes at 65,536 rows
        for A in (4, 9, 19, 64):
            for regime in C.REGIMES:
                yield B, A, regime


def _check_categorical(B, A, regime):
    logits, action, g_lp, g_ent = C.categorical_case(B, A, regime, seed=B, device=DEV)
    ref_lp, ref_ent, lse, ref_d = C.categorical_ref(logits, action, g_lp, g_ent)
    what = f"B={B} A={A} {regime}"
    # forward at the ABI (ops.categorical_logprob_entropy is a thin ctypes call) ...
    lp, ent = ops.categorical_logprob_entropy(logits, action)
    C.check_categorical_forward(lp, ent, ref_lp, ref_ent, lse, what)
    # ... and forward + backward through the autograd Function that Agent.get_action_and_value uses
    x = logits.clone().requires_grad_(True)
    lp2, ent2 = ops.CategoricalLogProbEntropy.apply(x, action)
    assert torch.equal(lp2, lp) and torch.equal(ent2, ent)
    (lp2 * g_lp + ent2 * g_ent).sum().backward()
    C.check_categorical_backward(x.grad, ref_d, g_lp, g_ent, what)
    # the f32 action storage of the reference's rollout buffer gives the same bits
    af = action.float()
    lp3, ent3 = ops.categorical_logprob_entropy(logits, af)
    st, d3 = _cat_bwd_abi(logits, None, af, g_lp, g_ent)
    assert st == 0 and torch.equal(lp3, lp) and torch.equal(ent3, ent) and torch.equal(d3, x.grad)


@pytest.mark.parametrize("B,A,regime", list(_cat_small()))
def test_categorical_fwd_bwd_float64_small(B, A, regime):
    _check_categorical(B, A, regime)


@pytest.mark.parametrize("B,A,regime", list(_cat_large()))
def test_categorical_fwd_bwd_float64_large(B, A, regime):
    _check_categorical(B, A, regime)


@pytest.mark.parametrize("A", [4, 18, 64])
def test_categorical_rows_are_independent_of_batch_geometry_and_repeatable(A):
    """A row's results do not depend on the batch around it (64- and 256-lane blocks, any position), a second call gives the
    same bits, and absent upstream gradients (null pointers) are zeros."""
    B = 65537
    logits, action, g_lp, g_ent = C.categorical_case(B, A, "randn", seed=5, device=DEV)
    lp, ent = ops.categorical_logprob_entropy(logits, action)
    st, d = _cat_bwd_abi(logits, action, None, g_lp, g_ent)
    assert st == 0
    for lo, hi in ((0, 63), (65500, 65537), (65536, 65537), (1000, 1001)):
        lp_s, ent_s = ops.categorical_logprob_entropy(logits[lo:hi].contiguous(), action[lo:hi].contiguous())
        st, d_s = _cat_bwd_abi(logits[lo:hi].contiguous(), action[lo:hi].contiguous(), None, g_lp[lo:hi].contiguous(),
                               g_ent[lo:hi].contiguous())
        assert st == 0
        assert torch.equal(lp_s, lp[lo:hi]) and torch.equal(ent_s, ent[lo:hi]) and torch.equal(d_s, d[lo:hi]), (lo, hi)
    lp2, ent2 = ops.categorical_logprob_entropy(logits, action)
    st, d2 = _cat_bwd_abi(logits, action, None, g_lp, g_ent)
    assert st == 0 and torch.equal(lp2, lp) and torch.equal(ent2, ent) and torch.equal(d2, d)
    zero = torch.zeros_like(g_lp)
    for gl, ge, zl, ze in ((None, g_ent, zero, g_ent), (g_lp, None, g_lp, zero), (None, None, zero, zero)):
        st1, d_null = _cat_bwd_abi(logits, action, None, gl, ge)
        st2, d_zero = _cat_bwd_abi(logits, action, None, zl, ze)
        assert st1 == 0 and st2 == 0 and torch.equal(d_null, d_zero)
    assert not d_zero.any()


def test_categorical_misaligned_rows_take_the_scalar_path_with_the_same_bits():
    """At A = 4 load_row reads a row as one float4 when it is 16-byte aligned; a base at storage offset 1 (4-byte aligned only)
    takes the scalar loads.  Both give the same bits, forward and backward."""
    B, A = 70001, 4
    logits, action, g_lp, g_ent = C.categorical_case(B, A, "randn", seed=11, device=DEV)
    buf = torch.empty(B * A + 1, device=DEV)
    buf[1:] = logits.reshape(-1)
    view = buf[1:].view(B, A)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and logits.data_ptr() % 16 == 0
    lp_a, ent_a = ops.categorical_logprob_entropy(logits, action)
    lp_m, ent_m = ops.categorical_logprob_entropy(view, action)
    assert torch.equal(lp_m, lp_a) and torch.equal(ent_m, ent_a)
    st1, d_a = _cat_bwd_abi(logits, action, None, g_lp, g_ent)
    st2, d_m = _cat_bwd_abi(view, action, None, g_lp, g_ent)
    assert st1 == 0 and st2 == 0 and torch.equal(d_m, d_a)
    ref_lp, ref_ent, lse, ref_d = C.categorical_ref(logits, action, g_lp, g_ent)
    C.check_categorical_forward(lp_m, ent_m, ref_lp, ref_ent, lse, "misaligned")
    C.check_categorical_backward(d_m, ref_d, g_lp, g_ent, "misaligned")


def test_categorical_refuses_65_actions():
    B, A = 8, 65
    logits = torch.randn(B, A, device=DEV)
    action = torch.zeros(B, dtype=torch.int64, device=DEV)
    out = torch.full((B,), 7.0, device=DEV)
    lib = _lib.load()
    assert lib.mi355ppo_categorical_logprob_entropy_f32(_p(logits), _p(action), None, _p(out), _p(out), B, A, _stream()) == EINVAL
    st, d = _cat_bwd_abi(logits, action, None, out, out)
    assert st == EINVAL
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (d == 7.0).all()                  # refused before any launch: outputs untouched
    with pytest.raises(_lib.Mi355PpoError):
        ops.categorical_logprob_entropy(logits, action)


# ============================================================================ K2'  Normal forward + backward
@pytest.mark.parametrize("far", [False, True])
@pytest.mark.parametrize("B", [257, 65535, 65536, 65537])
@pytest.mark.parametrize("D", C.NORMAL_D)
def test_normal_fwd_bwd_float64(D, B, far):
    mean, logstd, action, g_lp, g_ent = C.normal_case(B, D, far=far, seed=B, device=DEV)
    ref_lp, ref_ent, ref_dm, ref_dls, mag_lp, mag_ent, mag_rows = C.normal_ref(mean, logstd, action, g_lp, g_ent)
    what = f"B={B} D={D} far={far}"
    lp, ent = ops.normal_logprob_entropy(mean, logstd, action)
    C.check_normal_forward(lp, ent, ref_lp, ref_ent, mag_lp, mag_ent, D, what)
    dmean, drows = _normal_bwd_abi(mean, logstd, action, g_lp, g_ent)
    C.check_normal_backward(dmean, drows, ref_dm, mag_rows, g_lp, g_ent, mean, logstd, action, what)
    # through the autograd Function of ContinuousAgent.get_action_and_value: dlogstd is the wrapper's f32 drows.sum(0)
    mu = mean.clone().requires_grad_(True)
    ls = logstd.reshape(1, D).clone().requires_grad_(True)
    lp2, ent2 = ops.NormalLogProbEntropy.apply(mu, ls, action)
    assert torch.equal(lp2, lp) and torch.equal(ent2, ent)
    (lp2 * g_lp + ent2 * g_ent).sum().backward()
    assert torch.equal(mu.grad, dmean) and ls.grad.shape == (1, D)
    # (an f32 tree sum of B terms: log2(B) u of the sum of their magnitudes, < 1e-6 of it; the bar is 1e-5)
    err = (ls.grad.reshape(-1).double() - ref_dls).abs()
    assert (err <= 1e-5 * mag_rows.sum(0)).all(), f"{what} dlogstd: worst err/mag {float((err / mag_rows.sum(0)).max()):.3g}"
    # repeatable, and null upstream gradients are zeros
    dmean2, drows2 = _normal_bwd_abi(mean, logstd, action, g_lp, g_ent)
    assert torch.equal(dmean2, dmean) and torch.equal(drows2, drows)
    dm0, dr0 = _normal_bwd_abi(mean, logstd, action, None, g_ent)
    dmz, drz = _normal_bwd_abi(mean, logstd, action, torch.zeros_like(g_lp), g_ent)
    assert torch.equal(dm0, dmz) and torch.equal(dr0, drz)


# ===================================================================== through the agents (reference update step)
def _ref_update_grads(agent64, x, act, mb):
    """ppo.py:250-288 on a float64 CPU copy of the agent: torch.distributions (the reference's own Agent code path)."""
    _, lp, ent, v = agent64.get_action_and_value(x, act)
    out = TO.ppo_loss(lp, ent, v, mb["logprobs"], mb["adv"], mb["ret"], mb["values"], 0.2, 0.01, 0.5, True, True)
    out["loss"].backward()
    return out["loss"].item()


def _minibatch(M, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(logprobs=torch.randn(M, generator=g) * 0.3 - 1.5, adv=torch.randn(M, generator=g), ret=torch.randn(M, generator=g),
                values=torch.randn(M, generator=g))


def _compare_agents(agent, agent64, x, act, mb, perturb=None):
    dev_mb = {k: v.to(DEV) for k, v in mb.items()}
    if perturb is not None:
        torch.cuda.manual_seed(perturb)
    _, lp, ent, v = agent.get_action_and_value(x.to(DEV), act.to(DEV))
    out = TO.ppo_loss(lp, ent, v, dev_mb["logprobs"], dev_mb["adv"], dev_mb["ret"], dev_mb["values"], 0.2, 0.01, 0.5, True, True)
    out["loss"].backward()
    loss64 = _ref_update_grads(agent64, x.double(), act if act.dtype == torch.int64 else act.double(),
                               {k: v.double() for k, v in mb.items()})
    np.testing.assert_allclose(out["loss"].item(), loss64, rtol=1e-5)
    n = 0
    for (name, p), p64 in zip(agent.named_parameters(), agent64.parameters()):
        ref = p64.grad.numpy()
        np.testing.assert_allclose(p.grad.double().cpu().numpy(), ref, rtol=1e-4, atol=1e-5 * np.abs(ref).max(), err_msg=name)
        n += 1
    assert n == len(list(agent64.parameters()))


def test_discrete_agent_update_step_matches_float64_torch_distributions():
    torch.manual_seed(0)
    envs = SimpleNamespace(single_observation_space=E.Box(-np.inf, np.inf, (8,)), single_action_space=E.Discrete(5))
    agent = agents.MlpAgent(envs)
    agent64 = copy.deepcopy(agent).double()
    agent.to(DEV)
    M = 512
    x = torch.randn(M, 8)
    act = torch.randint(0, 5, (M,))
    _compare_agents(agent, agent64, x, act, _minibatch(M, 1))


@pytest.mark.parametrize("rpo_alpha", [None, 0.5])
def test_continuous_agent_update_step_matches_float64_torch_distributions(rpo_alpha):
    """ContinuousAgent (ppo_continuous_action.py) and, with rpo_alpha, RPO's perturbed mean (rpo_continuous_action.py:138-142):
    the device draw of the perturbation is replayed from the same seed and added to the float64 mean."""
    torch.manual_seed(1)
    D, O, M = 3, 11, 512
    envs = SimpleNamespace(single_observation_space=E.Box(-np.inf, np.inf, (O,)), single_action_space=E.Box(-1.0, 1.0, (D,)))
    agent = agents.ContinuousAgent(envs, rpo_alpha=rpo_alpha)
    with torch.no_grad():
        agent.actor_logstd.copy_(torch.linspace(-1.0, 0.5, D)[None])
    agent64 = copy.deepcopy(agent).double()
    agent.to(DEV)
    x = torch.randn(M, O)
    act = torch.randn(M, D)
    seed = None
    if rpo_alpha is not None:
        seed = 1234
        torch.cuda.manual_seed(seed)
        u = torch.empty(M, D, device=DEV).uniform_(-rpo_alpha, rpo_alpha).double().cpu()
        agent64.perturb_mean = lambda mean: mean + u
    _compare_agents(agent, agent64, x, act, _minibatch(M, 2), perturb=seed)


# ============================================================================== K3  Normal loss
LOSS_M = [1, 2, 255, 256, 257, 1025, 4096, 32768, 524288, 524289, 1048577, 1200007]
FLAGS = [(True, True), (True, False), (False, True), (False, False)]


def _loss_cases():
    for M in LOSS_M:
        for D in (1, 6, 17, 64):
            if D == 64 and M > 32768:
                continue                                 # bounds memory and time
            for norm_adv, clip_vloss in FLAGS:
                if norm_adv and M == 1:
                    continue                             # one row has no unbiased std (the library refuses it, as torch gives NaN:
                    #                                      test_losses_refuse_norm_adv_on_one_row)
                yield M, D, norm_adv, clip_vloss


def _loss_args(c):
    return (c["new_mean"], c["logstd"], c["new_value"], c["mb_inds"], c["b_actions"], c["b_logprobs"], c["b_advantages"],
            c["b_returns"], c["b_values"])


@pytest.mark.parametrize("ent_coef", [0.0, 0.01])
@pytest.mark.parametrize("M,D,norm_adv,clip_vloss", list(_loss_cases()))
def test_loss_normal_float64(M, D, norm_adv, clip_vloss, ent_coef):
    """Sizes cross one workgroup (256 rows), the statistics' second partial (1,024) and their cap of 1,024 blocks (1,048,576),
    and the persistent pass's second sweep (2,048 x 256 = 524,288 rows)."""
    c = C.loss_normal_case(M, D, seed=3, device=DEV)
    ref = C.loss_normal_ref(c, ent_coef, norm_adv, clip_vloss)
    sc, dmean, dlogstd, dvalue = ops.ppo_loss_normal(*_loss_args(c), C.CLIP, ent_coef, C.VF, norm_adv, clip_vloss)
    C.check_loss_normal(sc, dmean, dlogstd, dvalue, ref, M, D, f"M={M} D={D}")


@pytest.mark.parametrize("M", LOSS_M[1:])
def test_loss_normal_stats_identity_and_determinism(M):
    """Caller-supplied (mean, std + 1e-8) from ops.adv_stats meets the same float64 bar; a second call gives the same bits;
    identity indices (null mb_inds) give the bits of an explicit arange."""
    D, kw = 6, dict(clip_coef=C.CLIP, ent_coef=0.01, vf_coef=C.VF, norm_adv=True, clip_vloss=True)
    c = C.loss_normal_case(M, D, seed=4, device=DEV)
    ref = C.loss_normal_ref(c, 0.01, True, True)
    args = _loss_args(c)
    out = ops.ppo_loss_normal(*args, **kw)
    out2 = ops.ppo_loss_normal(*args, **kw)
    assert all(torch.equal(a, b) for a, b in zip(out, out2))
    md = ops.adv_stats(c["b_advantages"], c["mb_inds"], M)
    assert md.shape == (1, 2)
    out3 = ops.ppo_loss_normal(*args, adv_mean_den=md[0], **kw)
    C.check_loss_normal(*out3, ref, M, D, f"M={M} adv_mean_den")
    ident = list(args)
    ident[3] = None
    ar = list(args)
    ar[3] = torch.arange(M, device=DEV)
    o_id, o_ar = ops.ppo_loss_normal(*ident, **kw), ops.ppo_loss_normal(*ar, **kw)
    assert all(torch.equal(a, b) for a, b in zip(o_id, o_ar))
    c_ar = dict(c, mb_inds=torch.arange(M, device=DEV))
    C.check_loss_normal(*o_ar, C.loss_normal_ref(c_ar, 0.01, True, True), M, D, f"M={M} identity")


@pytest.mark.parametrize("D", [0, 65])
def test_loss_normal_refuses_D_outside_1_to_64(D):
    M = 300
    lib = _lib.load()
    f = lambda *s: torch.full(s, 7.0, device=DEV)       # noqa: E731
    mean, logstd, value, acts = f(M, max(D, 1)), f(max(D, 1)), f(M), f(M, max(D, 1))
    b = f(M)
    scalars, dmean, dlogstd, dvalue = f(7), f(M, max(D, 1)), f(max(D, 1)), f(M)
    ws = torch.zeros(lib.mi355ppo_loss_workspace_bytes(M, 64), dtype=torch.uint8, device=DEV)
    st = lib.mi355ppo_loss_normal_fwd_bwd_f32(_p(mean), _p(logstd), _p(value), None, _p(acts), _p(b), _p(b), _p(b), _p(b), M, D,
                                              0.2, 0.01, 0.5, 1, 1, None, _p(scalars), _p(dmean), _p(dlogstd), _p(dvalue), _p(ws),
                                              ws.numel(), _stream())
    assert st == EINVAL
    if D > 64:
        assert lib.mi355ppo_loss_workspace_bytes(M, D) == 0
    torch.cuda.synchronize()
    for t in (scalars, dmean, dlogstd, dvalue):
        assert (t == 7.0).all()                                     # refused before any launch
    with pytest.raises(_lib.Mi355PpoError):
        ops.ppo_loss_normal(torch.zeros(M, D, device=DEV), torch.zeros(D, device=DEV), b, None, torch.zeros(M, D, device=DEV), b, b,
                            b, b, 0.2, 0.01, 0.5)


def test_loss_normal_autograd_function_matches_float64_autograd_under_a_network():
    """PPOLossNormal under a tiny network == the reference's continuous loss lines differentiated by float64 autograd."""
    torch.manual_seed(0)
    M, D, Bf, O = 512, 3, 2048, 16
    net = torch.nn.Linear(O, D + 1).to(DEV)
    logstd = torch.nn.Parameter(torch.linspace(-1.0, 0.5, D, device=DEV)[None])
    x = torch.randn(M, O, device=DEV)
    inds = torch.randperm(Bf, device=DEV)[:M]
    b_actions = torch.randn(Bf, D, device=DEV)
    b_logprobs = -3.0 + 0.5 * torch.randn(Bf, device=DEV)
    b_adv = torch.randn(Bf, device=DEV)
    b_val = torch.randn(Bf, device=DEV)
    b_ret = b_val + b_adv
    out = net(x)
    loss, _ = ops.PPOLossNormal.apply(out[:, :D].contiguous(), logstd, out[:, D].contiguous(), inds, b_actions, b_logprobs, b_adv,
                                      b_ret, b_val, 0.2, 0.01, 0.5, True, True)
    loss.backward()
    net64 = copy.deepcopy(net).double()
    net64.zero_grad(set_to_none=True)
    ls64 = logstd.detach().double().clone().requires_grad_(True)
    o = net64(x.double())
    lp, ent = TO.normal_logprob_entropy(o[:, :D], ls64, b_actions.double()[inds])
    ref = TO.ppo_loss(lp, ent, o[:, D], b_logprobs.double()[inds], b_adv.double()[inds], b_ret.double()[inds], b_val.double()[inds],
                      0.2, 0.01, 0.5, True, True)
    ref["loss"].backward()
    np.testing.assert_allclose(loss.item(), ref["loss"].item(), rtol=1e-5)
    for got, want, name in ((net.weight.grad, net64.weight.grad, "weight"), (net.bias.grad, net64.bias.grad, "bias"),
                            (logstd.grad, ls64.grad, "logstd")):
        w = want.cpu().numpy()
        np.testing.assert_allclose(got.double().cpu().numpy(), w, rtol=1e-4, atol=1e-5 * np.abs(w).max(), err_msg=name)


# ============================================================================== K3  Categorical loss
def _cat_loss_args(c):
    return tuple(c[k] for k in C.LOSS_CAT_KEYS)


def _cat_loss_small():
    for regime in C.REGIMES:
        for A in C.LOSS_CAT_A:
            if regime == "masked" and A == 1:
                continue                                 # no distribution (see _cat_small)
            yield regime, A


@pytest.mark.parametrize("regime,A", list(_cat_loss_small()))
def test_loss_categorical_float64(regime, A):
    """Every logit regime x both sides of every A bucket of the dispatch (4 / 8 / 18 / 64) x M in {1, 2, 255, 257, 1025} (one
    lane, one workgroup +- 1, the statistics' second partial) x the four flag pairs x ent_coef in {0, 0.01}."""
    for M in (1, 2, 255, 257, 1025):
        c = C.loss_categorical_case(M, A, regime, seed=1, device=DEV)
        for norm_adv, clip_vloss in FLAGS:
            if norm_adv and M == 1:
                continue                                 # refused: test_losses_refuse_norm_adv_on_one_row
            for ent_coef in (0.0, 0.01):
                ref = C.loss_categorical_ref(c, ent_coef, norm_adv, clip_vloss)
                out = ops.ppo_loss_categorical(*_cat_loss_args(c), C.CLIP, ent_coef, C.VF, norm_adv, clip_vloss)
                C.check_loss_categorical(*out, ref, f"{regime} A={A} M={M} flags=({norm_adv}, {clip_vloss}) ent={ent_coef}")


@pytest.mark.parametrize("A", [4, 18])
@pytest.mark.parametrize("regime", ["randn", "masked"])
@pytest.mark.parametrize("M", [524288, 524289, 1048577, 1200007])
def test_loss_categorical_float64_large(M, regime, A):
    """Across the second sweep of the persistent pass (2,048 x 256 rows) and the 1,024-partial cap of the statistics."""
    c = C.loss_categorical_case(M, A, regime, seed=2, device=DEV)
    ref = C.loss_categorical_ref(c, 0.01, True, True)
    out = ops.ppo_loss_categorical(*_cat_loss_args(c), C.CLIP, 0.01, C.VF, True, True)
    C.check_loss_categorical(*out, ref, f"{regime} A={A} M={M}")


@pytest.mark.parametrize("regime", ["masked", "randn_x40"])
@pytest.mark.parametrize("M,A", [(257, 4), (1025, 4), (1025, 9), (300, 19)])
def test_loss_categorical_every_route_meets_the_float64_bar(M, A, regime):
    """The five-array call, the packed call (batch_pack + adv_stats_packed), a caller-supplied adv_mean_den, the deferred fold
    through LossSlots at a non-zero slot and, at A = 4, logits and dlogits on views at storage offset 1 (4-byte aligned: the
    scalar route instead of the float4 one): each meets the float64 bar, and all give the same bits."""
    c = C.loss_categorical_case(M, A, regime, seed=3, device=DEV)
    ref = C.loss_categorical_ref(c, 0.01, True, True)
    args, kw = _cat_loss_args(c), dict(clip_coef=C.CLIP, ent_coef=0.01, vf_coef=C.VF, norm_adv=True, clip_vloss=True)
    base = ops.ppo_loss_categorical(*args, **kw)
    routes = {"five arrays": base}
    pack = ops.batch_pack(*args[3:])
    md = ops.adv_stats(c["b_advantages"], c["mb_inds"], M)
    mdp = ops.adv_stats_packed(pack, c["mb_inds"], M)
    assert torch.equal(md, mdp)
    routes["packed"] = ops.ppo_loss_categorical_packed(*args[:3], pack, adv_mean_den=mdp[0], **kw)
    routes["packed, own statistics"] = ops.ppo_loss_categorical_packed(*args[:3], pack, **kw)
    routes["adv_mean_den"] = ops.ppo_loss_categorical(*args, adv_mean_den=md[0], **kw)
    slots = ops.LossSlots(3, torch.device(DEV))
    none, dl_s, dv_s = ops.ppo_loss_categorical(*args, slot=(slots, 2), **kw)
    table = torch.zeros(3, 7, device=DEV)
    slots.fold(1, table, first=2)
    assert none is None and not table[:2].any()
    routes["deferred fold"] = (table[2], dl_s, dv_s)
    if A == 4:
        buf, obuf = torch.empty(M * A + 1, device=DEV), torch.empty(M * A + 1, device=DEV)
        buf[1:] = c["new_logits"].reshape(-1)
        view, oview = buf[1:].view(M, A), obuf[1:].view(M, A)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4 and c["new_logits"].data_ptr() % 16 == 0
        routes["misaligned"] = ops.ppo_loss_categorical(view, *args[1:], dlogits_out=oview, **kw)
    for name, out in routes.items():
        C.check_loss_categorical(*out, ref, f"{regime} A={A} M={M} {name}")
        assert all(torch.equal(a, b) for a, b in zip(out, base)), name


def _device_loss(clip, norm_adv, clip_vloss):
    def run(c, ent_coef=0.0):
        return ops.ppo_loss_categorical(*_cat_loss_args(c), clip, ent_coef, C.VF, norm_adv, clip_vloss)
    return run


@pytest.mark.parametrize("clip_vloss", [True, False])
def test_loss_categorical_exact_convention_rows(clip_vloss):
    """dist_cases.EXACT_ROWS: dv == +-clip (torch.clamp passes gradient on the closed interval), u == c inside and outside the
    clip (torch.max splits a tie 1/2 + 1/2), a zero gradient, an advantage of exactly 0.  Every value-loss quantity is dyadic:
    dvalue and v_loss are bit-equal to float64 autograd rounded to f32."""
    C.check_exact_rows(_device_loss(C.EXACT_CLIP, False, clip_vloss), DEV, clip_vloss)


def test_loss_categorical_policy_tie_rows_device_equals_twin():
    """The policy-side tie pg1 == pg2 cannot be placed exactly against float64 on a general row: the f32 and the float64
    log-probability differ, so one of the two runs is off the tie.  It is pinned on the rows of dist_cases.loss_tie_case, whose
    exp / log are exact in every arithmetic, with clip_coef = 0 and b_logprobs = the kernel's own categorical_logprob_entropy
    output: the device and the twin give the same bits, which are the bits of float64 autograd."""
    from cleanrl_amd import host_ops as H
    dev = C.check_tie_rows(_device_loss(0.0, False, True), ops.categorical_logprob_entropy, DEV)

    def twin(c):
        lg, vl = c["new_logits"].clone().requires_grad_(True), c["new_value"].clone().requires_grad_(True)
        loss, sc = H.ppo_loss_categorical(lg, vl, *(c[k] for k in C.LOSS_CAT_KEYS[2:]), 0.0, 0.0, C.VF, False, True)
        loss.backward()
        return sc, lg.grad, vl.grad
    host = C.check_tie_rows(twin, H.categorical_logprob_entropy, "cpu")
    assert all(torch.equal(a, b) for a, b in zip(dev, host))


def test_loss_categorical_autograd_function_matches_float64_autograd_under_a_network():
    """PPOLossCategorical under a tiny network == the reference's discrete loss lines differentiated by float64 autograd."""
    torch.manual_seed(0)
    M, A, Bf, O = 512, 6, 2048, 16
    net = torch.nn.Linear(O, A + 1).to(DEV)
    x = torch.randn(M, O, device=DEV)
    inds = torch.randperm(Bf, device=DEV)[:M]
    b_actions = torch.randint(0, A, (Bf,), device=DEV).float()
    b_logprobs = -np.log(A) + 0.3 * torch.randn(Bf, device=DEV)
    b_adv = torch.randn(Bf, device=DEV)
    b_val = torch.randn(Bf, device=DEV)
    b_ret = b_val + b_adv
    out = net(x)
    loss, _ = ops.PPOLossCategorical.apply(out[:, :A].contiguous(), out[:, A].contiguous(), inds, b_actions, b_logprobs, b_adv,
                                           b_ret, b_val, 0.2, 0.01, 0.5, True, True)
    loss.backward()
    net64 = copy.deepcopy(net).double()
    net64.zero_grad(set_to_none=True)
    o = net64(x.double())
    lp, ent = TO.categorical_logprob_entropy(o[:, :A], b_actions.long()[inds])
    ref = TO.ppo_loss(lp, ent, o[:, A], b_logprobs.double()[inds], b_adv.double()[inds], b_ret.double()[inds], b_val.double()[inds],
                      0.2, 0.01, 0.5, True, True)
    ref["loss"].backward()
    np.testing.assert_allclose(loss.item(), ref["loss"].item(), rtol=1e-5)
    for got, want, name in ((net.weight.grad, net64.weight.grad, "weight"), (net.bias.grad, net64.bias.grad, "bias")):
        w = want.cpu().numpy()
        np.testing.assert_allclose(got.double().cpu().numpy(), w, rtol=1e-4, atol=1e-5 * np.abs(w).max(), err_msg=name)


def test_losses_refuse_norm_adv_on_one_row():
    """One row has no unbiased std (torch gives NaN): norm_adv with M == 1 and no caller-supplied adv_mean_den is refused with
    MI355PPO_EINVAL before anything is launched, by the five-array, the packed and the Normal entry points and by their ops
    wrappers, as by the twins; with adv_mean_den the call is valid."""
    lib = _lib.load()
    c = C.loss_categorical_case(1, 4, "randn", seed=2, device=DEV)
    args = _cat_loss_args(c)
    f = lambda *s: torch.full(s, 7.0, device=DEV)       # noqa: E731
    sc, dl, dv, dm, dls = f(7), f(1, 4), f(1), f(1, 4), f(4)
    ws = torch.zeros(lib.mi355ppo_loss_workspace_bytes(1, 4), dtype=torch.uint8, device=DEV)
    pack = ops.batch_pack(*args[3:])
    hp = (C.CLIP, 0.01, C.VF, 1, 1)
    tail = (_p(ws), ws.numel(), _stream())
    md = torch.tensor([0.25, 2.0], device=DEV)

    def five(given):
        return lib.mi355ppo_loss_categorical_fwd_bwd_f32(*(_p(t) for t in args), 1, 4, *hp, _p(given), _p(sc), _p(dl), _p(dv), *tail)

    def packed(given):
        return lib.mi355ppo_loss_categorical_packed_fwd_bwd_f32(*(_p(t) for t in args[:3]), _p(pack), 1, 4, *hp, _p(given), _p(sc),
                                                                _p(dl), _p(dv), *tail)
    cn = C.loss_normal_case(1, 4, seed=5, device=DEV)
    nargs = _loss_args(cn)

    def normal(given):
        return lib.mi355ppo_loss_normal_fwd_bwd_f32(*(_p(t) for t in nargs), 1, 4, *hp, _p(given), _p(sc), _p(dm), _p(dls), _p(dv),
                                                    *tail)
    for call in (five, packed, normal):
        assert call(None) == EINVAL
        assert b"norm_adv needs M > 1" in lib.mi355ppo_last_error()
    torch.cuda.synchronize()
    for t in (sc, dl, dv, dm, dls):
        assert (t == 7.0).all()                                     # refused before any launch
    kw = dict(clip_coef=C.CLIP, ent_coef=0.01, vf_coef=C.VF, norm_adv=True, clip_vloss=True)
    with pytest.raises(_lib.Mi355PpoError, match="norm_adv needs M > 1"):
        ops.ppo_loss_categorical(*args, **kw)
    with pytest.raises(_lib.Mi355PpoError, match="norm_adv needs M > 1"):
        ops.ppo_loss_categorical_packed(*args[:3], pack, **kw)
    with pytest.raises(_lib.Mi355PpoError, match="norm_adv needs M > 1"):
        ops.ppo_loss_normal(*nargs, **kw)
    # with the statistics supplied the one-row call is valid: == the un-normalised loss of the advantage (a - 0.25) / 2
    c2 = dict(c, b_advantages=(c["b_advantages"] - 0.25) / 2.0)
    ref = C.loss_categorical_ref(c2, 0.01, False, True)
    assert five(md) == 0
    C.check_loss_categorical(sc, dl, dv, ref, "five arrays, given statistics")
    out = ops.ppo_loss_categorical_packed(*args[:3], pack, adv_mean_den=md, **kw)
    C.check_loss_categorical(*out, ref, "packed, given statistics")
    cn2 = dict(cn, b_advantages=(cn["b_advantages"] - 0.25) / 2.0)
    assert normal(md) == 0
    C.check_loss_normal(sc, dm, dls, dv, C.loss_normal_ref(cn2, 0.01, False, True), 1, 4, "Normal, given statistics")


# ============================================================================== advantage statistics
@pytest.mark.parametrize("kind", C.ADV_KINDS)
@pytest.mark.parametrize("total,M", C.ADV_SEGMENTS + [(64, 2)])
def test_adv_stats_float64(total, M, kind):
    """Every minibatch of an epoch in one call: more than one segment, a ragged last one (of two rows, and of ONE row at
    (2049, 1024): NaN, as torch), more than one partial per segment above M = 1,024 and their cap of 1,024; well conditioned,
    a large mean with a small spread (the one-pass variance) and a constant (the variance is exactly 0); with a permutation
    and with identity indices; packed and unpacked routes give the same bits."""
    adv = C.adv_values(total, kind, seed=1, device=DEV)
    perm = torch.randperm(adv.numel(), device=DEV)[:total]
    zeros = torch.zeros_like(adv)
    pack = ops.batch_pack(zeros, zeros, adv, zeros, zeros)
    for inds, flat, rows in ((perm, adv, pack), (None, adv[:total].contiguous(), pack[:total])):
        got = ops.adv_stats(flat, inds, M)
        C.check_adv_stats(got, flat, inds, M, f"total={total} M={M} {kind} {'perm' if inds is not None else 'identity'}")
        packed = ops.adv_stats_packed(rows, inds, M)
        assert torch.equal(torch.isnan(packed), torch.isnan(got)) and torch.equal(packed.nan_to_num(), got.nan_to_num())


def test_adv_stats_constant_segments_clamp_a_negative_variance_residue():
    """Constant advantages that are not dyadic: s = n a and mu = a are exact, but n a^2 outgrows 53 bits and rounds, so the
    one-pass ss - s mu is a rounding residue of either sign where float64's two-pass variance is exactly 0.  Every segment's
    den stays inside [1e-8f, 1e-8 + sqrt(E)] -- a negative residue clamps to exactly 1e-8f instead of a NaN.  Over three
    constants x segments of 900, 1,024, 1,025 and 1,200,007 rows (thirteen independent residues; the reductions run in a fixed
    order, so each sign is the same on every run) at least one is negative or zero: the clamp is on the path."""
    clamped = 0
    for a in C.ADV_CONSTANTS:
        for total, M in C.ADV_SEGMENTS[1:]:
            adv = C.adv_values(total, a, device=DEV)
            got = ops.adv_stats(adv[:total].contiguous(), None, M)
            clamped += C.check_adv_stats(got, adv[:total], None, M, f"constant {a} total={total} M={M}", exact_constant=False)
    assert clamped > 0


def test_adv_stats_of_one_row_minibatches_is_the_row_and_nan():
    """M == 1 as a whole call: every row of the table is (that advantage, NaN), as torch.std of one element; not refused."""
    adv = C.adv_values(5, "n(0.5,2)", seed=3, device=DEV)
    perm = torch.randperm(adv.numel(), device=DEV)[:5]
    got = ops.adv_stats(adv, perm, 1)
    assert got.shape == (5, 2) and torch.equal(got[:, 0], adv[perm]) and torch.isnan(got[:, 1]).all()
    C.check_adv_stats(got, adv, perm, 1, "M=1")
    zeros = torch.zeros_like(adv)
    packed = ops.adv_stats_packed(ops.batch_pack(zeros, zeros, adv, zeros, zeros), perm, 1)
    assert torch.equal(packed[:, 0], got[:, 0]) and torch.isnan(packed[:, 1]).all()
