"""Case generators shared by the float64 tests of the distribution kernels (K2 / K2' forward and backward) and of the Normal
K3 loss: tests/test_gpu_distributions.py (device) and tests/test_host_twins_float64.py (the ``*_cpu`` twins).

Every generator returns float32 tensors on the requested device; the reference is float64 autograd on the same values cast up
(``oracle/torch_oracle.py``, pinned to the reference-line goldens).  Plain module, not a conftest: import it as ``dist_cases``.
"""
from __future__ import annotations

import math

import torch

from oracle import torch_oracle as TO

# capacities of MI355_DISPATCH_AMAX (distributions.hip) are 4 / 8 / 18 / 64: both sides of every bucket edge
CAT_A = [1, 2, 3, 4, 5, 7, 8, 9, 17, 18, 19, 33, 63, 64]
NORMAL_D = [1, 2, 3, 4, 5, 6, 8, 17, 21, 64, 100]
REGIMES = ["randn", "randn_x40", "constant", "offset_1e4", "masked"]
U32 = 2.0 ** -24          # unit roundoff of float32


def _gen(seed, device):
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    return g


def categorical_case(B, A, regime, seed=0, device="cpu"):
    """(logits (B, A) f32, action (B,) int64, g_lp (B,), g_ent (B,)) for one logit regime.

    * randn       N(0, 1)
    * randn_x40   N(0, 1) * 40: most probabilities underflow in f32
    * constant    every entry of a row equal (H = log A); rows differ
    * offset_1e4  N(0, 1) + 1e4: only the max subtraction keeps exp finite
    * masked      N(0, 1) with one entry of each row at -inf (a masked action); the action is never the masked one.
                  Needs A >= 2: at A = 1 the row would be all -inf and the float64 reference is NaN (no distribution).
    Upstream gradients lie in [-1, 1]: at the masked entry float64 autograd multiplies finfo(float64).min by them, which stays
    finite only there.
    """
    g = _gen(seed * 131 + A * 7 + REGIMES.index(regime), device)
    x = torch.randn(B, A, generator=g, device=device)
    if regime == "randn_x40":
        x = x * 40.0
    elif regime == "constant":
        x = (torch.rand(B, 1, generator=g, device=device) * 20.0 - 10.0).expand(B, A).contiguous()
    elif regime == "offset_1e4":
        x = x + 1e4
    action = torch.randint(0, A, (B,), generator=g, device=device)
    if regime == "masked":
        assert A >= 2, "the masked regime needs two actions"
        shift = torch.randint(1, A, (B,), generator=g, device=device)
        masked = (action + shift) % A                                   # never the taken action
        x.scatter_(1, masked[:, None], float("-inf"))
    g_lp = torch.rand(B, generator=g, device=device) * 2.0 - 1.0
    g_ent = torch.rand(B, generator=g, device=device) * 2.0 - 1.0
    return x.contiguous(), action, g_lp, g_ent


def categorical_ref(logits, action, g_lp, g_ent):
    """float64 autograd of the reference's Categorical lines: (logprob, entropy, lse, dlogits) as float64."""
    x = logits.double().detach().clone().requires_grad_(True)
    lp, ent = TO.categorical_logprob_entropy(x, action)
    (lp * g_lp.double() + ent * g_ent.double()).sum().backward()
    lse = logits.double().logsumexp(-1)
    return lp.detach(), ent.detach(), lse, x.grad


def f32_ulp(t):
    """Spacing of float32 at |t| (t float64)."""
    a = t.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 23)


def check_categorical_forward(lp, ent, ref_lp, ref_ent, lse, what=""):
    """The K2 bar, rtol 2e-6 and atol 2e-6 * max(1, |ref|), plus one f32 ulp of the row's logsumexp: the reference's own
    ``logits - logits.logsumexp(-1)`` (categorical.py) rounds the logsumexp to float32 before the subtraction, and every
    log-probability of the row (hence the entropy) carries that rounding.  Below |lse| = 16 the extra term is < 2e-6."""
    for got, ref, name in ((lp, ref_lp, "logprob"), (ent, ref_ent, "entropy")):
        got = got.double().to(ref.device)
        tol = 2e-6 * ref.abs() + 2e-6 * ref.abs().clamp_min(1.0) + f32_ulp(lse)
        err = (got - ref).abs()
        bad = ~(err <= tol)
        assert not bad.any(), (f"{what} {name}: {int(bad.sum())} rows off, worst err {float(err.max()):.3g} "
                               f"(row {int(torch.argmax(err - tol))}), got {got[bad][:4].tolist()} ref {ref[bad][:4].tolist()}")


def check_categorical_backward(dlogits, ref, g_lp, g_ent, what=""):
    """Per row: |d - ref| <= 1e-5 * max_j |ref_row| + 2e-7 * (|g_lp| + |g_ent|).  The floor is the f32 rounding of a
    probability next to 1 (1 - p of a near one-hot row); the logsumexp rounding cancels in p_j and in lp_j + H."""
    got = dlogits.double().to(ref.device)
    err = (got - ref).abs()
    tol = 1e-5 * ref.abs().amax(1, keepdim=True) + 2e-7 * (g_lp.double().abs() + g_ent.double().abs()).to(ref.device)[:, None]
    bad = ~(err <= tol)
    assert not bad.any(), (f"{what} dlogits: {int(bad.any(1).sum())} rows off, worst err {float(err.max()):.3g}, "
                           f"first row {int(bad.any(1).nonzero()[0])}")


def normal_case(B, D, far=False, seed=0, device="cpu"):
    """(mean (B, D), logstd (D,), action (B, D), g_lp (B,), g_ent (B,)), f32.  logstd spread over [-5, 2]; the action at
    mean + std * z, or with ``far`` at |a - mean| = 10 whatever the std (10 / e^-5 ~ 1.5e3 standard deviations)."""
    g = _gen(seed * 977 + D * 13 + int(far), device)
    mean = torch.randn(B, D, generator=g, device=device) * 2.0
    logstd = torch.rand(D, generator=g, device=device) * 7.0 - 5.0
    if far:
        sign = torch.where(torch.rand(B, D, generator=g, device=device) < 0.5, -1.0, 1.0)
        action = mean + 10.0 * sign
    else:
        action = mean + torch.exp(logstd) * torch.randn(B, D, generator=g, device=device)
    g_lp = torch.rand(B, generator=g, device=device) * 2.0 - 1.0
    g_ent = torch.rand(B, generator=g, device=device) * 2.0 - 1.0
    return mean, logstd, action, g_lp, g_ent


def normal_ref(mean, logstd, action, g_lp, g_ent):
    """float64 autograd of the reference's Normal lines: (logprob_sum, entropy_sum, dmean, dlogstd, mag_lp, mag_ent, mag_dls)
    where the mag_* are the sums of absolute values of the summed terms (the condition of each sum: what its f32 rounding
    error is relative to)."""
    mu = mean.double().detach().clone().requires_grad_(True)
    ls = logstd.double().detach().clone().reshape(1, -1).requires_grad_(True)
    a = action.double()
    lp, ent = TO.normal_logprob_entropy(mu, ls, a)
    (lp * g_lp.double() + ent * g_ent.double()).sum().backward()
    var = torch.exp(2.0 * ls.detach())
    q = (a - mu.detach()) ** 2 / var
    mag_lp = (0.5 * q + ls.detach().abs() + math.log(math.sqrt(2 * math.pi))).sum(1)
    mag_ent = (ls.detach().abs() + 0.5 + 0.5 * math.log(2 * math.pi)).expand_as(q).sum(1)
    mag_rows = g_lp.double().abs()[:, None] * (q + 1.0) + g_ent.double().abs()[:, None]    # |per-row dlogstd terms|
    return lp.detach(), ent.detach(), mu.grad, ls.grad.reshape(-1), mag_lp, mag_ent, mag_rows


def normal_sum_rtol(D):
    """Relative bound of an f32 sum of D row terms, each good to a few ulp: the K2' bar 2e-6 up to D ~ 24, the recursive
    summation bound (D + 8) u above."""
    return max(2e-6, (D + 8) * U32)


def check_normal_forward(lp, ent, ref_lp, ref_ent, mag_lp, mag_ent, D, what=""):
    r = normal_sum_rtol(D)
    for got, ref, mag, name in ((lp, ref_lp, mag_lp, "logprob"), (ent, ref_ent, mag_ent, "entropy")):
        err = (got.double().to(ref.device) - ref).abs()
        tol = r * mag.clamp_min(1.0)
        assert (err <= tol).all(), f"{what} {name}: worst err/tol {float((err / tol).max()):.3g}"


def check_normal_backward(dmean, drows, ref_dmean, mag_rows, g_lp, g_ent, ref_mean, ref_logstd, ref_action, what=""):
    """dmean elementwise (a quotient and two products of rounded values: rtol 2e-6); the per-row dlogstd terms
    g_lp * ((a - mu)^2 / var - 1) + g_ent against float64 at 2e-6 of their magnitude."""
    err = (dmean.double().to(ref_dmean.device) - ref_dmean).abs()
    assert (err <= 2e-6 * ref_dmean.abs() + 1e-30).all(), f"{what} dmean: worst rel err {float((err / ref_dmean.abs().clamp_min(1e-30)).max()):.3g}"
    if drows is None:
        return
    mu, a = ref_mean.double(), ref_action.double()
    var = torch.exp(2.0 * ref_logstd.double())[None]
    rows = g_lp.double()[:, None] * ((a - mu) ** 2 / var - 1.0) + g_ent.double()[:, None]
    err = (drows.double().to(rows.device) - rows).abs()
    assert (err <= 2e-6 * mag_rows).all(), f"{what} dlogstd rows: worst err/mag {float((err / mag_rows).max()):.3g}"


# ------------------------------------------------------------------------------------------------ Normal K3 loss
CLIP, VF = 0.2, 0.5


def loss_normal_case(M, D, seed=0, device="cpu"):
    """One minibatch of the continuous-action loss: M rows drawn from a flat batch of Bf = 4 M behaviour rows.

    The inputs keep every row away from the loss's kinks, where f32 and float64 may take different branches and the
    gradient of a row jumps: the log-ratio stays >= 1e-3 from log(1 +- clip) and |newvalue - old value| >= 1e-3 from clip.
    Returns a dict of f32 tensors (mb_inds int64)."""
    g = _gen(seed * 7919 + M * 3 + D, device)
    Bf = 4 * M
    logstd = torch.rand(D, generator=g, device=device) * 1.5 - 1.0
    std = torch.exp(logstd)
    inds = torch.randperm(Bf, generator=g, device=device)[:M]
    b_actions = torch.randn(Bf, D, generator=g, device=device)
    new_mean = b_actions[inds] - std * torch.randn(M, D, generator=g, device=device)
    # new log-probability in float64, then the behaviour log-probability at a log-ratio spread over both clip edges
    lp64, _ = TO.normal_logprob_entropy(new_mean.double(), logstd.double().reshape(1, -1), b_actions[inds].double())
    r = torch.randn(M, generator=g, device=device, dtype=torch.float64) * 0.25
    for edge in (math.log(1.0 + CLIP), math.log(1.0 - CLIP)):
        near = (r - edge).abs() < 2e-3
        r = torch.where(near, edge + 4e-3 * torch.sign(r - edge + 1e-12), r)
    b_logprobs = torch.randn(Bf, generator=g, device=device) - 3.0 * D
    b_logprobs[inds] = (lp64 - r).float()
    b_adv = torch.randn(Bf, generator=g, device=device) * 2.0 + 0.5
    b_values = torch.randn(Bf, generator=g, device=device)
    b_returns = b_values + b_adv
    dv = torch.randn(M, generator=g, device=device) * 0.3
    near = (dv.abs() - CLIP).abs() < 2e-3
    dv = torch.where(near, dv + 4e-3 * torch.sign(dv), dv)
    new_value = b_values[inds] + dv
    return dict(new_mean=new_mean.contiguous(), logstd=logstd, new_value=new_value, mb_inds=inds, b_actions=b_actions,
                b_logprobs=b_logprobs, b_advantages=b_adv, b_returns=b_returns, b_values=b_values)


def loss_normal_ref(c, ent_coef, norm_adv, clip_vloss):
    """float64 autograd of ppo_continuous_action.py:265-300 (the lines of oracle/torch_oracle.loss_normal_seam) on the case's
    values cast up.  Also ``dlogstd_mag`` = sum_m |g_lp_m| ((a - mu)^2 / var + 1) + ent_coef per component: the sum of the
    absolute values of the M row terms that make up dlogstd, i.e. what the rounding of that sum is relative to."""
    d = {k: (v if k == "mb_inds" else v.double()) for k, v in c.items()}
    idx = c["mb_inds"]
    mean = d["new_mean"].clone().requires_grad_(True)
    ls = d["logstd"].clone().requires_grad_(True)
    value = d["new_value"].clone().requires_grad_(True)
    act = d["b_actions"][idx]
    lp, ent = TO.normal_logprob_entropy(mean, ls.reshape(1, -1), act)
    lp.retain_grad()
    out = TO.ppo_loss(lp, ent, value, d["b_logprobs"][idx], d["b_advantages"][idx], d["b_returns"][idx], d["b_values"][idx],
                      CLIP, ent_coef, VF, norm_adv, clip_vloss)
    out["loss"].backward()
    res = {k: v.detach() for k, v in out.items()}
    res["dmean"], res["dlogstd"], res["dvalue"] = mean.grad, ls.grad, value.grad
    q = (act - mean.detach()) ** 2 / torch.exp(2.0 * ls.detach())[None]
    res["dlogstd_mag"] = (lp.grad.abs()[:, None] * (q + 1.0)).sum(0) + ent_coef
    return res


LOSS_SCALARS = ("loss", "pg_loss", "v_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac")


def loss_bar(D):
    """The Normal-loss bar against float64.  Base: the K3 bars of the goldens (scalars rtol 2e-5 / atol 2e-6, gradients 2e-5 of
    max |ref|).  It grows with D above 16 because every row's new log-probability is an f32 sum of D terms of one sign (|lp| up
    to ~2 D here), and its rounding -- which float64 does not have -- enters each ratio, hence each row's gradient and each
    scalar, as a relative error; measured at D = 64 on the twins: 1.6e-5 of max |ref| in dmean, 1.3e-6 absolute in old_approx_kl."""
    return 2e-5 * max(1.0, D / 16.0)


def check_loss_normal(sc, dmean, dlogstd, dvalue, ref, M, D, what=""):
    """Seven scalars (rtol 2e-5, atol loss_bar(D) / 10); dmean and dvalue per element against max |ref| at loss_bar(D); dlogstd
    -- a sum of M row terms per component, up to 1.2 M of them, with cancellation -- at loss_bar(D) of the sum of the terms'
    absolute values (dlogstd_mag), which is at most ~ M / sqrt(M) times max |ref| for terms of random sign."""
    bar = loss_bar(D)
    sc = sc.detach().double().to(ref["loss"].device)
    for i, k in enumerate(LOSS_SCALARS):
        err = float((sc[i] - ref[k]).abs())
        assert err <= 2e-5 * float(ref[k].abs()) + bar / 10, f"{what} {k}: got {float(sc[i])!r} ref {float(ref[k])!r}"
    for got, k in ((dmean, "dmean"), (dvalue, "dvalue")):
        r = ref[k].reshape(got.shape)
        err = (got.detach().double().to(r.device) - r).abs().max()
        assert err <= bar * r.abs().max(), f"{what} {k}: worst err {float(err):.3g} vs max |ref| {float(r.abs().max()):.3g}"
    err = (dlogstd.detach().double().reshape(-1).to(ref["dlogstd"].device) - ref["dlogstd"]).abs()
    assert (err <= bar * ref["dlogstd_mag"]).all(), f"{what} dlogstd: worst err / mag {float((err / ref['dlogstd_mag']).max()):.3g}"
