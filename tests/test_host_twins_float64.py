"""The ``*_cpu`` twins of the distribution entry points (K2 / K2' forward and backward) and of the Normal K3 loss against
float64 autograd of the reference's lines, on the A / D / logit-regime grid of tests/dist_cases.py at small batch sizes.  The
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
