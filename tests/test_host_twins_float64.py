"""The ``*_cpu`` twins of the distribution entry points (K2 / K2' forward and backward) and of the Normal and Categorical K3
losses against float64 autograd of the reference's lines, on the A / D / logit-regime grid of tests/dist_cases.py at small batch sizes.  The
device kernels are held to the same references and bars in tests/test_gpu_distributions.py.  CPU only."""
import pytest
import torch

import dist_cases as C
from cleanrl_amd import host_ops as H

SMALL_B = [1, 63, 257]


def _cat_params():
    for A in C.CAT_A:
        for regime in C.REGIMES:
            if regime == "masked" and A == 1:
                continue                      # a one-action row with its only entry masked has no distribution (NaN in float64)
            yield A, regime


@pytest.mark.parametrize("B", SMALL_B)
@pytest.mark.parametrize("A,regime", list(_cat_params()))
def test_categorical_twins_match_float64(A, regime, B):
    logits, action, g_lp, g_ent = C.categorical_case(B, A, regime, seed=B)
    ref_lp, ref_ent, lse, ref_d = C.categorical_ref(logits, action, g_lp, g_ent)
    lp, ent = H.categorical_logprob_entropy(logits, action)
    C.check_categorical_forward(lp, ent, ref_lp, ref_ent, lse, f"A={A} {regime}")
    d = H.categorical_logprob_entropy_bwd(logits, action, g_lp, g_ent)
    C.check_categorical_backward(d, ref_d, g_lp, g_ent, f"A={A} {regime}")
    # one upstream gradient at a time: g_lp and g_ent enter the kernel through different terms
    zero = torch.zeros_like(g_lp)
    for gl, ge in ((g_lp, zero), (zero, g_ent)):
        d1 = H.categorical_logprob_entropy_bwd(logits, action, gl, ge)
        C.check_categorical_backward(d1, C.categorical_ref(logits, action, gl, ge)[3], gl, ge, f"A={A} {regime} split")
    # absent upstream gradients are zeros
    assert torch.equal(H.categorical_logprob_entropy_bwd(logits, action, g_lp, None),
                       H.categorical_logprob_entropy_bwd(logits, action, g_lp, zero))
    assert torch.equal(H.categorical_logprob_entropy_bwd(logits, action, None, g_ent),
                       H.categorical_logprob_entropy_bwd(logits, action, zero, g_ent))


@pytest.mark.parametrize("far", [False, True])
@pytest.mark.parametrize("D", C.NORMAL_D)
def test_normal_twins_match_float64(D, far):
    B = 257
    mean, logstd, action, g_lp, g_ent = C.normal_case(B, D, far=far, seed=D)
    ref_lp, ref_ent, ref_dm, ref_dls, mag_lp, mag_ent, mag_rows = C.normal_ref(mean, logstd, action, g_lp, g_ent)
    lp, ent = H.normal_logprob_entropy(mean, logstd, action)
    C.check_normal_forward(lp, ent, ref_lp, ref_ent, mag_lp, mag_ent, D, f"D={D}")
    dmean, drows = H.normal_logprob_entropy_bwd(mean, logstd, action, g_lp, g_ent)
    C.check_normal_backward(dmean, drows, ref_dm, mag_rows, g_lp, g_ent, mean, logstd, action, f"D={D}")
    err = (drows.double().sum(0) - ref_dls).abs()
    assert (err <= 2e-6 * mag_rows.sum(0)).all(), f"dlogstd: worst err/mag {float((err / mag_rows.sum(0)).max()):.3g}"


LOSS_FLAGS = [(True, True), (True, False), (False, True), (False, False)]


@pytest.mark.parametrize("ent_coef", [0.0, 0.01])
@pytest.mark.parametrize("norm_adv,clip_vloss", LOSS_FLAGS)
@pytest.mark.parametrize("M,D", [(2, 1), (255, 6), (257, 17), (1025, 64), (64, 3)])
def test_loss_normal_twin_matches_float64(M, D, norm_adv, clip_vloss, ent_coef):
    c = C.loss_normal_case(M, D, seed=1)
    ref = C.loss_normal_ref(c, ent_coef, norm_adv, clip_vloss)
    mean = c["new_mean"].clone().requires_grad_(True)
    logstd = c["logstd"].clone().requires_grad_(True)
    value = c["new_value"].clone().requires_grad_(True)
    loss, sc = H.ppo_loss_normal(mean, logstd, value, c["mb_inds"], c["b_actions"], c["b_logprobs"], c["b_advantages"],
                                 c["b_returns"], c["b_values"], C.CLIP, ent_coef, C.VF, norm_adv, clip_vloss)
    loss.backward()
    C.check_loss_normal(sc, mean.grad, logstd.grad, value.grad, ref, M, D)


# ---------------------------------------------------------------------------------------------- Categorical K3 loss
def _twin_loss_categorical(c, clip, ent_coef, norm_adv, clip_vloss):
    lg = c["new_logits"].clone().requires_grad_(True)
    vl = c["new_value"].clone().requires_grad_(True)
    loss, sc = H.ppo_loss_categorical(lg, vl, c["mb_inds"], c["b_actions"], c["b_logprobs"], c["b_advantages"], c["b_returns"],
                                      c["b_values"], clip, ent_coef, C.VF, norm_adv, clip_vloss)
    loss.backward()
    assert float(loss.detach()) == float(sc[0])
    return sc, lg.grad, vl.grad


def _loss_cat_params():
    for regime in C.REGIMES:
        for A in C.LOSS_CAT_A:
            if regime == "masked" and A == 1:
                continue                      # no distribution (see _cat_params)
            yield regime, A


@pytest.mark.parametrize("regime,A", list(_loss_cat_params()))
def test_loss_categorical_twin_matches_float64(regime, A):
    """Every logit regime x both sides of every A bucket of the device dispatch x M in {1, 2, 255, 257, 1025} x the four flag
    pairs x ent_coef in {0, 0.01}; norm_adv needs two rows."""
    for M in (1, 2, 255, 257, 1025):
        c = C.loss_categorical_case(M, A, regime, seed=1)
        for norm_adv, clip_vloss in LOSS_FLAGS:
            if norm_adv and M == 1:
                continue
            for ent_coef in (0.0, 0.01):
                ref = C.loss_categorical_ref(c, ent_coef, norm_adv, clip_vloss)
                sc, dl, dv = _twin_loss_categorical(c, C.CLIP, ent_coef, norm_adv, clip_vloss)
                C.check_loss_categorical(sc, dl, dv, ref, f"{regime} A={A} M={M} flags=({norm_adv}, {clip_vloss}) ent={ent_coef}")


@pytest.mark.parametrize("clip_vloss", [True, False])
def test_loss_categorical_twin_exact_convention_rows(clip_vloss):
    """The rows of dist_cases.EXACT_ROWS land on dv == +-clip, on u == c inside and outside the clip and on a zero gradient:
    dvalue and v_loss are bit-equal to float64 autograd rounded to f32 (torch.max splits a tie 1/2 + 1/2, torch.clamp passes
    gradient on the closed interval), float64 autograd agrees with the hand-worked EXACT_GV, and the row whose advantage is
    exactly 0 has an exactly zero policy gradient."""
    C.check_exact_rows(lambda c, ent: _twin_loss_categorical(c, C.EXACT_CLIP, ent, False, clip_vloss), "cpu", clip_vloss)


def test_loss_categorical_twin_policy_tie_rows():
    C.check_tie_rows(lambda c: _twin_loss_categorical(c, 0.0, 0.0, False, True), H.categorical_logprob_entropy, "cpu")


def test_loss_twins_take_one_row_with_caller_supplied_statistics_only():
    """norm_adv on a one-row minibatch has no unbiased std: refused (-1, outputs untouched) unless the caller supplies
    (mean, std + 1e-8), exactly as the device entry points."""
    import ctypes
    from cleanrl_amd import _lib
    lib = _lib.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())       # noqa: E731
    c = C.loss_categorical_case(1, 4, "randn", seed=2)
    b = [c[k] for k in ("b_actions", "b_logprobs", "b_advantages", "b_returns", "b_values")]
    sc, dl, dv = torch.full((7,), 7.0), torch.full((1, 4), 7.0), torch.full((1,), 7.0)
    args = (p(c["new_logits"]), p(c["new_value"]), p(c["mb_inds"]), *(p(t) for t in b), 1, 4, C.CLIP, 0.01, C.VF, 1, 1)
    assert lib.mi355ppo_loss_categorical_fwd_bwd_f32_cpu(*args, None, p(sc), p(dl), p(dv)) == -1
    assert b"norm_adv needs M > 1" in lib.mi355ppo_last_error()
    assert (sc == 7.0).all() and (dl == 7.0).all() and (dv == 7.0).all()
    md = torch.tensor([0.25, 2.0])
    assert lib.mi355ppo_loss_categorical_fwd_bwd_f32_cpu(*args, p(md), p(sc), p(dl), p(dv)) == 0
    # == the un-normalised loss of the advantage (a - 0.25) / 2
    c2 = dict(c, b_advantages=(c["b_advantages"] - 0.25) / 2.0)
    C.check_loss_categorical(sc, dl, dv, C.loss_categorical_ref(c2, 0.01, False, True), "given statistics")
