"""Case generators shared by the float64 tests of the distribution kernels (K2 / K2' forward and backward), of the Normal and
Categorical K3 losses and of the advantage statistics: tests/test_gpu_distributions.py (device) and
tests/test_host_twins_float64.py (the ``*_cpu`` twins).

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


# ------------------------------------------------------------------------------------------------ Categorical K3 loss
LOSS_CAT_A = [1, 2, 4, 5, 8, 9, 18, 19, 63, 64]      # both sides of every bucket edge of the K3 dispatch (4 / 8 / 18 / 64)
KINK = 4e-3                                          # every row of a generated case is at least this far from every kink
_PUSH = 1.25                                         # rows are pushed to _PUSH * margin; the margin itself is then asserted


def loss_categorical_case(M, A, regime, seed=0, device="cpu", clip=CLIP):
    """One minibatch of the discrete-action loss: M rows out of a flat batch of Bf = 4 M behaviour rows (``mb_inds`` is the head
    of a permutation); logits and taken action from ``categorical_case(M, A, regime)``.

    CONDITION (asserted below on the float64 values of the f32 tensors that are returned, so the reference alone guarantees
    it): no row lies within ``margin`` of a kink of the loss, where f32 and float64 may take different branches and a row's
    gradient jumps --
      * |logratio - log(1 +- clip)| >= margin       (the ratio clamp, the pg1 / pg2 choice and clipfrac),
      * ||newvalue - old value| - clip| >= margin   (the value clamp),
      * |ret - (v + v_clipped) / 2| >= margin / 4 on the rows outside the value clip, where the unclipped and the clipped
        value loss tie (there |u - c| = 2 |v - v_clipped| |ret - mid| >= 2 margin^2 / 4, five orders above the f32 rounding
        of u and c at these magnitudes).
    ``margin`` is KINK = 4e-3, or four f32 ulps of the largest logsumexp where that is more: the reference's own
    ``logits - logsumexp`` rounds the logsumexp to f32 (offset_1e4: ulp = 2^-10 ~ 1e-3), which moves the f32 log-ratio of a row
    by that much against float64.  Returns a dict of f32 tensors (mb_inds int64) plus ``margin``."""
    logits, action, _, _ = categorical_case(M, A, regime, seed=seed * 31 + M, device=device)
    g = _gen(seed * 6151 + M * 5 + A * 3 + REGIMES.index(regime), device)
    Bf = 4 * M
    inds = torch.randperm(Bf, generator=g, device=device)[:M]
    b_actions = torch.randint(0, A, (Bf,), generator=g, device=device).float()
    b_actions[inds] = action.float()
    lp64, _ = TO.categorical_logprob_entropy(logits.double(), action)
    lse = logits.double().logsumexp(-1)
    margin = max(KINK, 4.0 * float(f32_ulp(lse).max()))
    edges = (math.log(1.0 + clip), math.log(1.0 - clip)) if clip > 0 else (0.0,)
    r = torch.randn(M, generator=g, device=device, dtype=torch.float64) * 0.25
    for edge in edges:
        near = (r - edge).abs() < _PUSH * margin
        r = torch.where(near, edge + _PUSH * margin * torch.sign(r - edge + 1e-12), r)
    b_logprobs = torch.randn(Bf, generator=g, device=device) * 0.3 - math.log(A)
    b_logprobs[inds] = (lp64 - r).float()
    b_adv = torch.randn(Bf, generator=g, device=device) * 2.0 + 0.5
    b_values = torch.randn(Bf, generator=g, device=device)
    b_returns = b_values + b_adv
    dv = torch.randn(M, generator=g, device=device) * 0.3
    near = (dv.abs() - clip).abs() < _PUSH * margin
    dv = torch.where(near, torch.sign(dv + 1e-12) * (clip + _PUSH * margin), dv)
    new_value = b_values[inds] + dv
    # the value-loss tie: outside the clip, u == c where the return is midway between v and the clipped v
    v, ov, ret = new_value.double(), b_values[inds].double(), b_returns[inds].double()
    mid = 0.5 * (v + ov + (v - ov).clamp(-clip, clip))
    near = (ret - mid).abs() < _PUSH * margin / 4
    b_returns[inds] = torch.where(near, mid + _PUSH * margin / 4 * torch.sign(ret - mid + 1e-12), ret).float()
    c = dict(new_logits=logits, new_value=new_value, mb_inds=inds, b_actions=b_actions, b_logprobs=b_logprobs,
             b_advantages=b_adv, b_returns=b_returns, b_values=b_values, margin=margin, regime=regime)
    assert_away_from_kinks(c, clip)
    return c


def assert_away_from_kinks(c, clip=CLIP):
    """The condition of ``loss_categorical_case`` on the float64 values of the case's f32 tensors."""
    idx, margin = c["mb_inds"], c["margin"]
    act = c["b_actions"][idx].long()
    lp64, _ = TO.categorical_logprob_entropy(c["new_logits"].double(), act)
    assert torch.isfinite(lp64).all(), "a taken action is masked"
    logratio = lp64 - c["b_logprobs"][idx].double()
    for edge in ((math.log(1.0 + clip), math.log(1.0 - clip)) if clip > 0 else (0.0,)):
        assert ((logratio - edge).abs() >= margin).all(), "a row's ratio lies within the margin of a clip edge"
    v, ov, ret = c["new_value"].double(), c["b_values"][idx].double(), c["b_returns"][idx].double()
    dv = v - ov
    assert ((dv.abs() - clip).abs() >= margin).all(), "a row's value step lies within the margin of the value clip"
    mid = 0.5 * (v + ov + dv.clamp(-clip, clip))
    outside = dv.abs() > clip
    assert ((ret - mid).abs()[outside] >= margin / 4).all(), "a row outside the value clip lies on the u == c tie"


LOSS_CAT_KEYS = ("new_logits", "new_value", "mb_inds", "b_actions", "b_logprobs", "b_advantages", "b_returns", "b_values")


def loss_categorical_ref(c, ent_coef, norm_adv, clip_vloss, clip=CLIP, vf=VF):
    """float64 autograd of ``oracle/torch_oracle.loss_categorical_seam`` (ppo_atari_multigpu.py:320-355) on the case's f32 values
    cast up: the seven scalars, ``dlogits``, ``dvalue``.  Also, for the bars of ``check_loss_categorical``: ``g_lp`` (d loss / d
    newlogprob per row), and ``lp_ulp`` = f32_ulp(logsumexp) + f32_ulp(newlogprob) per row -- the two f32 roundings (one ulp
    bounds both halves) that the reference's own ``(logits - logsumexp)[action]`` puts into a row's new log-probability, hence
    into its ratio as a relative error -- and ``lp_ulp_w`` = mean_m lp_ulp_m max(1, |A_m| ratio_m), what those roundings can move
    a scalar of the loss by to first order (|d pg / d lp| = |A| ratio, |d entropy / d lse| = |d old_approx_kl / d lp| = 1)."""
    idx = c["mb_inds"]
    args = [c[k] if k == "mb_inds" else c[k].double() for k in LOSS_CAT_KEYS]
    res = TO.loss_categorical_seam(*args, clip, ent_coef, vf, norm_adv, clip_vloss)
    act = c["b_actions"][idx].long()
    lp, ent = TO.categorical_logprob_entropy(c["new_logits"].double(), act)
    lp = lp.clone().requires_grad_(True)
    adv = c["b_advantages"][idx].double()
    out = TO.ppo_loss(lp, ent, c["new_value"].double(), c["b_logprobs"][idx].double(), adv, c["b_returns"][idx].double(),
                      c["b_values"][idx].double(), clip, ent_coef, vf, norm_adv, clip_vloss)
    out["pg_loss"].backward()
    res["g_lp"] = lp.grad
    ratio = (lp.detach() - c["b_logprobs"][idx].double()).exp()
    res["g_lp_abs"] = torch.zeros_like(ratio)
    if norm_adv:
        res["g_lp_abs"] = (f32_ulp(adv.mean()) + f32_ulp(adv)) / (adv.std() + 1e-8) * ratio / lp.numel()
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    res["lp_ulp"] = f32_ulp(c["new_logits"].double().logsumexp(-1)) + f32_ulp(lp.detach())
    res["lp_ulp_w"] = (res["lp_ulp"] * (adv.abs() * ratio).clamp_min(1.0)).mean()
    res["g_ent"] = ent_coef / lp.numel()
    res["regime"] = c["regime"]
    return res


LOSS_CAT_BAR = 5e-6          # a quarter of loss_bar(1), the Normal-loss bar
LOSS_CAT_DV = 5e-7           # dvalue: eight f32 roundings, no exp / log
FLAT_REGIMES = ("randn", "constant", "masked")       # their bars never exceed the Normal bar loss_bar(1)


def loss_categorical_fractions(sc, dlogits, dvalue, ref):
    """error / tolerance of every quantity that ``check_loss_categorical`` bounds -> {name: (fraction, message)}; see there."""
    dev = ref["loss"].device
    flat = ref["regime"] in FLAT_REGIMES
    sc = sc.detach().double().to(dev)
    res = {}
    for i, k in enumerate(LOSS_SCALARS):
        err, mag = float((sc[i] - ref[k]).abs()), float(ref[k].abs())
        tol = LOSS_CAT_BAR * mag + LOSS_CAT_BAR / 10 + float(ref["lp_ulp_w"])
        if flat:
            tol = min(tol, loss_bar(1) * mag + loss_bar(1) / 10)
        if k == "clipfrac":
            tol = 6e-8
        res[k] = (err / tol, f"{k}: got {float(sc[i])!r} ref {float(ref[k])!r} err {err:.3g} tol {tol:.3g}")
    r = ref["dvalue"]
    err = (dvalue.detach().double().to(dev) - r).abs().max()
    res["dvalue"] = (float(err / (LOSS_CAT_DV * r.abs().max())) if err > 0 else 0.0, f"dvalue: worst err {float(err):.3g} vs max |ref| {float(r.abs().max()):.3g}")
    r = ref["dlogits"]
    err = (dlogits.detach().double().to(dev) - r).abs()
    rel = 2e-7 if flat else 2e-7 + ref["lp_ulp"]
    floors = ((rel * ref["g_lp"].abs() + ref["g_lp_abs"])[:, None] + 2e-7 * ref["g_ent"]).expand_as(err)
    tol = LOSS_CAT_BAR * r.abs().amax(1, keepdim=True) + floors
    frac = torch.where(err > 0, err / tol, torch.zeros_like(err))
    res["dlogits rows"] = (float(frac.max()), f"dlogits: {int((frac > 1).any(1).sum())} rows off, worst err / tol {float(frac.max()):.3g} "
                           f"in row {int(frac.amax(1).argmax())}")
    if flat:
        tol = LOSS_CAT_BAR * r.abs().max() + floors.max()
        res["dlogits"] = (float(err.max() / tol) if err.max() > 0 else 0.0, f"dlogits: worst err {float(err.max()):.3g} vs max |ref| {float(r.abs().max()):.3g}")
    return res


def check_loss_categorical(sc, dlogits, dvalue, ref, what=""):
    """The categorical K3 bar against float64 (``ref`` from ``loss_categorical_ref``).

    * six scalars: |err| <= 5e-6 |ref| + 5e-7 + lp_ulp_w -- a flat bar plus the first-order bound of what the reference's own
      f32 log-probability roundings move a scalar by (docstring of ``loss_categorical_ref``: ~3e-5 at randn_x40, where a
      taken log-probability reaches -300, ~2e-3 at offset_1e4; up to 5e-6 in the other regimes, at M = 1 and 2 where one
      row's weight max(1, |A| ratio) is the whole mean).  In randn, constant and masked (FLAT_REGIMES, by name) the tolerance
      is capped at the Normal bar ``loss_bar(1)``, 2e-5 |ref| + 2e-6.  clipfrac to 6e-8 (the f32 rounding of count / M:
      exact, since no row of a case is near a clip edge).
    * dvalue: 5e-7 of max |ref| (independent of the logits).
    * dlogits, per row: |err| <= 5e-6 max_j |ref_mj| + 2e-7 |g_lp_m| + the two floors below; outside the flat regimes
      (2e-7 + lp_ulp_m) |g_lp_m|.  A row's policy gradient g_lp (onehot - p) is proportional to its ratio, so the row's lp_ulp
      enters relative to |g_lp| (not to the row's net gradient: the policy and the entropy term may cancel); 2e-7 |g_lp| is
      the f32 rounding of a probability next to 1 (1 - p of a near one-hot row), as in ``check_categorical_backward``.  In the
      flat regimes the whole gradient also meets 5e-6 of the global max |ref| plus the largest floor of the case.
    * the two floors, both roundings that the reference's own f32 run has as well: 2e-7 ent_coef / M for the entropy gradient
      p (lp + H) of a row whose two terms cancel (``check_categorical_backward``'s g_ent floor), and with norm_adv
      (ulp(mean) + ulp(adv_m)) / den * ratio_m / M (``g_lp_abs``) for a row whose advantage lies next to the minibatch mean,
      where adv - mean cancels.

    Worst error / tolerance measured over the small grid (regimes x LOSS_CAT_A x M in {1, 2, 255, 257, 1025} x flags x
    ent_coef), the ``*_cpu`` twin | the device kernels:
      randn        scalars 0.25 | 0.50   dvalue 0.25 | 0.25   dlogits rows 0.28 | 0.32   whole dlogits 0.11 | 0.18
      constant     scalars 0.16 | 0.50   dvalue 0.22 | 0.28   dlogits rows 0.20 | 0.20   whole dlogits 0.19 | 0.15
      masked       scalars 0.25 | 0.50   dvalue 0.23 | 0.23   dlogits rows 0.28 | 0.26   whole dlogits 0.10 | 0.15
      randn_x40    scalars 0.44 | 0.50   dvalue 0.25 | 0.25   dlogits rows 0.41 | 0.43
      offset_1e4   scalars 0.45 | 0.50   dvalue 0.28 | 0.25   dlogits rows 0.50 | 0.49
    (the generators draw other values on the device than on the host, so the two columns are not the same cases; the device's
    0.50 of the scalars is clipfrac at M = 255 in every regime: 2^-25 / 6e-8, the half ulp of a count / M in [0.5, 1).)  In absolute terms the twin's worst cases are 3.1e-6 of |ref| + 0.1 in a scalar and 6.0e-7 of
    max |ref| in dlogits in the flat regimes, 2.1e-5 (randn_x40, M = 2) and 3.3e-3 (offset_1e4) in a scalar, 4.8e-4 of max |ref|
    in dlogits at offset_1e4.
    The base bars (5e-6, dvalue 5e-7) are a quarter of the Normal bar and two to four times the twin's worst case; the
    regimes whose bar is the f32 log-probability rounding sit at half of that bound, as a rounding is half an ulp."""
    for frac, msg in loss_categorical_fractions(sc, dlogits, dvalue, ref).values():
        assert frac <= 1.0, f"{what} {msg}"


# the exact-convention rows: (old value, new value, return), all dyadic, for clip_coef = 0.25, vf_coef = 0.5, M = 8
EXACT_CLIP = 0.25
EXACT_ROWS = [
    (0.0, 0.25, 1.0),        # dv == +clip: torch.clamp passes gradient on the closed interval; u == c
    (0.0, -0.25, 1.0),       # dv == -clip
    (0.0, 0.75, 0.5),        # u == c outside the clip: torch.max splits 1/2 + 1/2, the clamp passes nothing -> 1/2 * 2 du
    (0.0, -0.75, -0.5),      # the same on the other side
    (0.5, 0.5, 2.0),         # u == c inside the clip -> 2 du
    (1.0, 3.0, 0.0),         # plain row, u > c
    (0.0, 0.25, 0.25),       # dv == clip and du == 0: zero gradient
    (-1.0, -0.5, 0.5),       # c > u outside the clip: zero gradient; this row's advantage is exactly 0
]
# d max(u, c) / d v per row by torch's conventions, worked out by hand (the tests compare float64 autograd with it too)
EXACT_GV = [-1.5, -2.5, 0.25, -0.25, -3.0, 6.0, 0.0, 0.0]


def loss_categorical_exact_case(A=5, device="cpu"):
    """M = 8 rows landing on the subgradient conventions of the value loss (EXACT_ROWS), norm_adv off: every value-loss
    quantity is a dyadic number that f32 and float64 hold exactly, so ``dvalue`` and ``v_loss`` must be BIT-equal to the
    float64 reference rounded to f32.  The policy side comes from ``loss_categorical_case`` (away from its kinks); the last
    row's advantage is exactly 0."""
    c = loss_categorical_case(8, A, "randn", seed=77, device=device, clip=EXACT_CLIP)
    idx = c["mb_inds"]
    rows = torch.tensor(EXACT_ROWS, device=device)
    c["b_values"][idx], c["new_value"], c["b_returns"][idx] = rows[:, 0], rows[:, 1].clone(), rows[:, 2]
    c["b_advantages"][idx[7]] = 0.0
    return c


def loss_tie_case(device="cpu"):
    """Rows on the POLICY tie pg1 == pg2 with ratio == lo == hi == 1 (clip_coef = 0 and the behaviour log-probability equal
    to the new one).  A general row cannot be placed there against float64 -- its f32 and float64 log-probabilities differ --
    and is not bit-equal between the device and the twin either (their expf / logf differ in the last bit).  These rows are: one
    logit is 0 and the others are -150, -200 or -inf, so every exp is exactly 1 or underflows to exactly 0 and every log is
    log(1) = 0 in f32 (whatever the libm) and in float64 alike: log-probabilities == logits, probabilities one-hot, ratio == 1.
    M = 8 and dyadic advantages of both signs (and 0) keep g_lp = -A / M exact.  Returns (case dict, the exact new
    log-probabilities)."""
    ninf = float("-inf")
    logits = torch.tensor([[0.0, -200.0, ninf, -150.0], [-200.0, 0.0, -150.0, ninf], [0.0, -200.0, ninf, -150.0],
                           [-150.0, ninf, 0.0, -200.0], [ninf, -150.0, -200.0, 0.0], [0.0, -150.0, -200.0, ninf],
                           [-200.0, -150.0, 0.0, -150.0], [0.0, ninf, -200.0, -200.0]], device=device)
    action = torch.tensor([1, 0, 0, 3, 1, 2, 2, 3], device=device)
    lp = logits.gather(1, action[:, None]).squeeze(1)
    M, Bf = 8, 32
    inds = torch.arange(3, 3 + 4 * M, 4, device=device)
    b_actions = torch.zeros(Bf, device=device)
    b_actions[inds] = action.float()
    b_logprobs = torch.full((Bf,), -1.0, device=device)
    b_logprobs[inds] = lp
    b_adv = torch.zeros(Bf, device=device)
    b_adv[inds] = torch.tensor([1.0, -2.0, 0.5, 0.0, -0.25, 3.0, -1.5, 4.0], device=device)
    b_values = torch.arange(Bf, device=device) / 16.0 - 1.0        # dyadic: the value loss is exact as well
    new_value = b_values[inds] + 0.125
    b_returns = b_values + 1.0
    return dict(new_logits=logits, new_value=new_value, mb_inds=inds, b_actions=b_actions, b_logprobs=b_logprobs,
                b_advantages=b_adv, b_returns=b_returns, b_values=b_values, regime="masked"), lp


# ------------------------------------------------------------------------------------------------ advantage statistics
ADV_SEGMENTS = [(10, 4), (2049, 1024), (5000, 1025), (4 * 1200007, 1200007)]       # (total, M): ragged last segments, of two
#                                          rows and of ONE row; per_seg > 1 above M = 1024 and at its cap of 1024 partials
ADV_KINDS = ["n(0.5,2)", "n(1e3,1e-2)", "constant"]
ADV_CONSTANTS = [1000.1, 0.3, -7.3]                  # not dyadic: n a^2 rounds in f64 once n a^2 outgrows 53 bits


def adv_values(total, kind, seed=0, device="cpu"):
    """The flat advantages that a permutation's head of ``total`` indices draws from: 4 x total values (total itself above 10^6).
    The constant of kind "constant" is dyadic, so that every f64 sum of the kernels is exact; a float ``kind`` is that constant."""
    n = 4 * total if total < 10 ** 6 else total
    if not isinstance(kind, str):
        return torch.full((n,), float(kind), device=device)
    if kind == "constant":
        return torch.full((n,), 1000.0, device=device)
    z = torch.randn(n, generator=_gen(seed * 271 + total % 9973 + ADV_KINDS.index(kind), device), device=device)
    return z * 2.0 + 0.5 if kind == "n(0.5,2)" else z * 1e-2 + 1e3


def check_adv_stats(got, adv, inds, M, what="", exact_constant=True):
    """Every row of ``got`` (nseg, 2) against float64 ``mean`` and ``std(unbiased) + 1e-8`` of the segment's gathered advantages.

    * mean: one f32 ulp (the f64 sum of n f32 values is good to n 2^-53 relative to sum |a|; its rounding to f32 is half an ulp).
    * den: the kernel's one-pass variance (ss - s mu) / (n - 1) from f64 sums carries an absolute error of up to
      E = n 2^-53 (mean^2 + var) n / (n - 1), so |den - ref| <= sqrt(var + E) - sqrt(var) + 2^-23 ref: relative
      ~ 2^-54 n (1 + (mean / std)^2) where var >> E, plus the two f32 roundings (of the square root and of the + 1e-8f).
    * a one-row segment: (that row, NaN), as torch.std of one element is NaN.
    * a constant segment: with ``exact_constant`` (a dyadic value: every sum is exact) the variance is exactly 0 and den ==
      float32(1e-8).  Otherwise n a^2 rounds, the computed ss - s mu is a rounding residue of either sign, and den lies in
      [float32(1e-8), 1e-8 + sqrt(E)]: a negative residue is clamped to 0 (den == float32(1e-8) exactly), never a NaN.
    Returns the number of constant segments with den == float32(1e-8)."""
    total = adv.numel() if inds is None else inds.numel()
    gathered = (adv if inds is None else adv[inds]).double()
    nseg = (total + M - 1) // M
    assert got.shape == (nseg, 2)
    got = got.double().cpu()
    eps32 = float(torch.tensor(1e-8, dtype=torch.float32))
    at_eps = 0
    for j in range(nseg):
        seg = gathered[j * M:min((j + 1) * M, total)]
        n = seg.numel()
        mean = float(seg.mean())
        assert abs(float(got[j, 0]) - mean) <= float(f32_ulp(torch.tensor(mean, dtype=torch.float64))), \
            f"{what} segment {j}: mean {float(got[j, 0])!r} vs {mean!r}"
        if n == 1:
            assert torch.isnan(got[j, 1]), f"{what} segment {j}: one row must give NaN, got {float(got[j, 1])!r}"
            continue
        var = float(seg.var())
        ref = math.sqrt(var) + 1e-8
        E = n * 2.0 ** -53 * (mean * mean + var) * n / (n - 1)
        den = float(got[j, 1])
        if var == 0.0:
            at_eps += den == eps32
            if exact_constant:
                assert den == eps32, f"{what} segment {j}: constant, den {den!r}"
            else:
                assert eps32 <= den <= 1e-8 + math.sqrt(E) + 2.0 ** -23 * ref, f"{what} segment {j} (n={n}): constant, den {den!r}"
            continue
        tol = math.sqrt(var + E) - math.sqrt(var) + 2.0 ** -23 * ref
        assert abs(den - ref) <= tol, f"{what} segment {j} (n={n}): den {den!r} vs {ref!r}, tol {tol:.3g}"
    return at_eps


def check_exact_rows(run, device, clip_vloss):
    """``run(case, ent_coef) -> (scalars7, dlogits, dvalue)`` on ``loss_categorical_exact_case``: see the tests that call it."""
    c = loss_categorical_exact_case(device=device)
    for ent_coef in (0.0, 0.01):
        ref = loss_categorical_ref(c, ent_coef, False, clip_vloss, clip=EXACT_CLIP)
        sc, dl, dv = run(c, ent_coef)
        gv = torch.tensor(EXACT_GV if clip_vloss else [2.0 * (v - r) for _, v, r in EXACT_ROWS], dtype=torch.float64, device=ref["dvalue"].device)
        assert torch.equal(ref["dvalue"], VF * 0.5 / 8.0 * gv), "float64 autograd against the hand-worked subgradients"
        assert torch.equal(dv.detach().cpu(), ref["dvalue"].float().cpu()), f"dvalue {dv.tolist()} vs {ref['dvalue'].tolist()}"
        assert float(sc[2]) == float(ref["v_loss"].float()), f"v_loss {float(sc[2])!r} vs {float(ref['v_loss'])!r}"
        check_loss_categorical(sc, dl, dv, ref, f"exact rows ent_coef={ent_coef}")
        if ent_coef == 0.0:
            assert not dl[7].any() and not ref["dlogits"][7].any(), "advantage 0: no policy gradient"
            assert dl[:7].any()


def check_tie_rows(run, logprob_entropy, device):
    """``run(case) -> (scalars7, dlogits, dvalue)`` on ``loss_tie_case`` with clip_coef = 0, ent_coef = 0, norm_adv off.  The
    behaviour log-probabilities are the kernel's own (``logprob_entropy``) and equal the logits of the taken actions; pg1 ==
    pg2 and ratio == lo == hi on every row, where torch.max splits 1/2 + 1/2 and torch.clamp passes on the closed interval:
    the whole gradient passes, g_lp = -A / M, and dlogits is exactly g_lp (onehot - onehot of the 0 logit).  Returns the
    outputs, for a bit-comparison of the device with the twin."""
    c, lp = loss_tie_case(device)
    act = c["b_actions"][c["mb_inds"]].long()
    own_lp, own_ent = logprob_entropy(c["new_logits"], act)
    assert torch.equal(own_lp, lp) and not own_ent.any()
    c["b_logprobs"][c["mb_inds"]] = own_lp
    ref = loss_categorical_ref(c, 0.0, False, True, clip=0.0)
    sc, dl, dv = run(c)
    adv = c["b_advantages"][c["mb_inds"]]
    want = torch.zeros_like(c["new_logits"])
    want.scatter_(1, act[:, None], (-adv / 8.0)[:, None])
    want.scatter_add_(1, c["new_logits"].argmax(1, keepdim=True), (adv / 8.0)[:, None])
    assert torch.equal(ref["dlogits"].float(), want), "float64 autograd: the tie passes the whole gradient"
    assert torch.equal(dl.detach(), want), f"dlogits {dl.tolist()}"
    assert torch.equal(sc.detach().cpu(), torch.stack([ref[k] for k in LOSS_SCALARS]).float().cpu()), f"scalars {sc.tolist()}"
    assert float(sc[6]) == 0.0 and float(sc[4]) == 0.0 and float(sc[5]) == 0.0
    return sc.detach().cpu(), dl.detach().cpu(), dv.detach().cpu()
