"""The RND host twins (csrc/rnd.hip over csrc/rnd_rows.h) on the CPU against independent restatements of the reference's lines
(tests/rnd_cases.py): the bit-equal pieces (normalisation in float64, integer moments, the env-axis filter, the scaled rewards),
the bars of the float pieces, refusals, and the fused branch of ``RNDPPOLearner`` driven on the CPU."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rnd_cases as R
from offpolicy_cases import within_bar
from cleanrl_amd import _lib, ops
from cleanrl_amd import host_ops as H

CPU = torch.device("cpu")
PUT, OUT = R.plain(CPU)
ENTRY_POINTS = ("rnd_normalize_u8_f32", "rnd_obs_moments_u8", "rnd_intrinsic_reward_f32", "rnd_reward_filter_f32", "rnd_loss_fwd_bwd_f32")


def test_symbols_are_bound_on_both_sides():
    for n in ENTRY_POINTS:
        assert f"mi355ppo_{n}" in _lib.SIGNATURES and f"mi355ppo_{n}_cpu" in _lib.SIGNATURES
    assert "mi355ppo_rnd_obs_moments_workspace_bytes" in _lib.SIGNATURES and "mi355ppo_rnd_loss_workspace_bytes" in _lib.SIGNATURES
    for name in ("rnd_normalize", "rnd_obs_moments", "rnd_intrinsic_reward", "rnd_reward_filter_", "rnd_loss_fwd_bwd", "rnd_mean_var"):
        assert callable(getattr(ops, name)) and callable(getattr(H, name)) and name in ops.__all__
    with pytest.raises(TypeError, match="CUDA/HIP"):
        ops.rnd_intrinsic_reward(torch.zeros(2, 512), torch.zeros(2, 512))


# ---------------------------------------------------------------------------------------------- a
@pytest.mark.parametrize("M", R.NORMALIZE_M)
@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("nhwc", [True, False])
def test_normalize_is_the_float64_expression_bit_for_bit(M, gather, nhwc):
    c = R.normalize_case(M, gather)
    got = R.run_normalize(H, c, nhwc, PUT, OUT)
    assert got.dtype == torch.float32 and torch.equal(got, c["want"])
    # the case reaches what it is for: both clips, and values landing exactly on the bounds
    assert (c["preclip"] > 5).any() and (c["preclip"] < -5).any() and (c["preclip"] == 5).any() and (c["preclip"] == -5).any()
    if gather and M >= 3:
        assert c["idx"][0] == c["idx"][2] and c["idx"][1] < c["idx"][0] and torch.equal(got[0], got[2])


# ---------------------------------------------------------------------------------------------- b
@pytest.mark.parametrize("B,nhwc", R.MOMENT_CASES)
def test_moments_are_the_exact_integer_sums(B, nhwc):
    c = R.moments_case(B)
    sums = R.run_moments(H, c, nhwc, PUT, OUT)                   # the output starts as garbage
    got = sums.numpy().astype(np.uint64)
    assert np.array_equal(got[0], c["S1"]) and np.array_equal(got[1], c["S2"])
    mean, var = H.rnd_mean_var(sums, B)
    x = c["rows"][:, 3].reshape(B, -1).numpy().astype(np.float64)
    np.testing.assert_allclose(mean, x.mean(0), rtol=1e-12, atol=0)
    np.testing.assert_allclose(var, x.var(0), rtol=1e-12, atol=0)


def test_moments_reproduce_the_references_observation_statistics():
    """The golden's update: obs_rms (mean0, var0, count0) + the 32 newest frames of the rollout -> (mean1, var1), which the
    reference formed with f32 numpy statistics (2.6e-7 relative from float64 on these frames); the bar is 1e-6 relative."""
    from cleanrl_amd.learner_rnd import RunningMeanStd

    g = R.golden()
    T, N = g["rewards"].shape
    rows = torch.from_numpy(g["frames_u8"][:T].reshape(T * N, 4, 84, 84))
    mean, var = H.rnd_mean_var(H.rnd_obs_moments(R.to_nhwc(rows)), T * N)
    x = rows[:, 3].reshape(T * N, -1).numpy().astype(np.float64)
    assert np.array_equal(mean, x.mean(0))
    np.testing.assert_allclose(var, x.var(0), rtol=1e-12, atol=0)
    rms = RunningMeanStd(shape=(1, 1, 84, 84))
    rms.mean, rms.var, rms.count = g["obs_mean0"].copy(), g["obs_var0"].copy(), float(g["obs_count0"])
    rms.update_from_moments(mean.reshape(1, 1, 84, 84), var.reshape(1, 1, 84, 84), T * N)
    np.testing.assert_allclose(rms.mean, g["obs_mean1"], rtol=1e-6, atol=0)
    np.testing.assert_allclose(rms.var, g["obs_var1"], rtol=1e-6, atol=0)


def test_mean_and_variance_round_once_at_every_batch_size():
    """Numerators of 2^53 and more (B from about 372,000 on) do not fit float64: the variance must still be the exact quotient
    rounded once, as ``Fraction`` rounds it; B >= 2^24 is refused."""
    from fractions import Fraction

    B = (1 << 24) - 1
    k = np.array([1, B // 3 + 1, B // 2, B - 1, 12345, 0] + [7] * (R.P - 6), dtype=np.int64)      # rows holding 255, the others 0
    sums = torch.from_numpy(np.stack([255 * k, 65025 * k]))
    mean, var = H.rnd_mean_var(sums, B)
    nums = [B * int(s2) - int(s1) ** 2 for s1, s2 in zip(sums[0].tolist(), sums[1].tolist())]
    assert max(nums) >= 1 << 53 and min(nums) == 0
    assert var.tolist() == [float(Fraction(n, B * B)) for n in nums]
    assert mean.tolist() == [float(Fraction(int(s1), B)) for s1 in sums[0].tolist()]
    with pytest.raises(ValueError, match="2\\^24"):
        H.rnd_mean_var(sums, 1 << 24)


# ---------------------------------------------------------------------------------------------- c
@pytest.mark.parametrize("N", R.INTRINSIC_N)
def test_intrinsic_reward_within_the_bound_of_512_f32_additions(N):
    """512 f32 additions of non-negative terms: at most 512 * 2^-24 = 3.1e-5 relative; asserted at 1e-4."""
    c = R.intrinsic_case(N)
    got = R.run_intrinsic(H, c, PUT, OUT)
    rel = ((got.double() - c["want64"]).abs() / c["want64"]).max().item()
    print(f"N={N}: max relative error {rel:.3e}")
    assert rel <= 1e-4
    np.testing.assert_allclose(got.numpy(), c["want64"].numpy(), rtol=2e-3, atol=1e-5)      # the bar of raw_curiosity in the GPU test


# ---------------------------------------------------------------------------------------------- d
def _check_filter(steps, outs):
    for s, (scaled, filtered, rewems, stats) in zip(steps, outs):
        assert np.array_equal(filtered.numpy(), s["filtered"]) and np.array_equal(rewems.numpy(), s["rewems"])      # the Python loop's bits
        np.testing.assert_allclose(stats.numpy(), np.array(s["stats"]), rtol=1e-11, atol=0)
        assert stats[2].item() == s["stats"][2]                                                                      # the count is N, as len()
        # f32 division by the f32-rounded divisor: what `tensor /= np.sqrt(var)` does
        assert torch.equal(scaled, torch.from_numpy(s["raw"]) / np.float32(np.sqrt(stats[1].item())))
        np.testing.assert_allclose(scaled.numpy(), s["scaled"].numpy(), rtol=1e-6, atol=0)


def test_reward_filter_on_the_golden_rollout():
    g = R.golden()
    steps = R.filter_case(8, 4, golden_raw=True)
    outs = R.run_filter(H, steps, PUT, OUT)
    _check_filter(steps, outs)
    scaled, _, _, stats = outs[0]
    assert abs(stats[1].item() - float(g["reward_var"])) <= 1e-6 * float(g["reward_var"])
    assert np.array_equal(scaled.numpy(), g["scaled_curiosity"])                     # bit-equal to what the reference stored


@pytest.mark.parametrize("T,N", R.FILTER_SHAPES)
def test_reward_filter_runs_along_the_env_axis_and_carries_its_state(T, N):
    steps = R.filter_case(T, N)
    _check_filter(steps, R.run_filter(H, steps, PUT, OUT))
    if N > 1:                                                                        # the quirk: env n + 1 sees env n's reward of the same step
        raw = steps[0]["raw"]
        assert steps[0]["filtered"][0, 1] == np.float32(np.float32(raw[0, 0] * np.float32(0.99)) + raw[0, 1])


# ---------------------------------------------------------------------------------------------- e
@pytest.mark.parametrize("M", R.LOSS_M)
@pytest.mark.parametrize("mask", [m for m, _ in R.LOSS_MASKS])
def test_loss_scalars_and_gradients_within_the_f32_references_bar(M, mask):
    """Bar (tests/test_dqn_twins.py): within twice the f32 torch reference's own error against float64 autograd, plus 2e-6."""
    c = R.loss_case(M, mask)
    out = R.run_loss(H, c, PUT, OUT)
    n_on = int((c["u"] < c["proportion"]).sum())
    assert {"none": n_on == 0, "all": n_on == M, "quarter": True}[mask]
    if mask == "none":
        assert not out["d_predict"].any() and out["scalars"][1].item() == 0.0      # divisor 1, no gradient
    for k in ("scalars", "d_predict", "d_v_int"):
        ok, err, own = within_bar(out[k], c["ref64"][k], c["ref32"][k])
        print(k, f"{err:.3e} (f32 reference {own:.3e})")
        assert ok, (k, err, own)


# ---------------------------------------------------------------------------------------------- refusals
def test_argument_validation_is_loud_and_precedes_any_launch():
    lib = _lib.load()
    buf = (ctypes.c_double * 16384)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    mis = ctypes.c_void_p(p.value + 2)
    RB = 4 * R.P
    err = lambda: lib.mi355ppo_last_error()                                                               # noqa: E731
    for sfx, tail in (("", (None,)), ("_cpu", ())):
        norm, mom = getattr(lib, "mi355ppo_rnd_normalize_u8_f32" + sfx), getattr(lib, "mi355ppo_rnd_obs_moments_u8" + sfx)
        intr, filt = getattr(lib, "mi355ppo_rnd_intrinsic_reward_f32" + sfx), getattr(lib, "mi355ppo_rnd_reward_filter_f32" + sfx)
        loss = getattr(lib, "mi355ppo_rnd_loss_fwd_bwd_f32" + sfx)
        ws = (p, 1 << 30) if not sfx else ()
        assert norm(None, 4, RB, 4, 3, None, p, p, p, 2, *tail) == -1 and b"null" in err()
        assert norm(mis, 4, RB, 4, 3, None, p, p, p, 2, *tail) == -2
        assert norm(p, 4, RB, 2, 3, None, p, p, p, 2, *tail) == -1 and b"pixel_stride" in err()
        assert norm(p, 4, RB, 4, 4, None, p, p, p, 2, *tail) == -1                                      # no such byte in a 4-byte pixel
        assert norm(p, 4, RB, 1, 3 * R.P + 1, None, p, p, p, 2, *tail) == -1                            # the frame leaves the row
        assert norm(p, 4, RB, 4, 3, None, p, p, p, 5, *tail) == -1                                      # M > B without an index
        assert mom(None, 4, RB, 4, 3, p, *ws, *tail) == -1 and b"null" in err()
        assert mom(p, 4, RB, 4, 3, mis, *ws, *tail) == -2
        assert mom(p, 1 << 24, RB, 4, 3, p, *ws, *tail) == -1 and b"2^24" in err()
        assert intr(p, None, p, 4, 512, *tail) == -1 and b"null" in err()
        assert intr(mis, p, p, 4, 512, *tail) == -2
        assert intr(p, p, p, 4, 256, *tail) == -1 and b"512 features" in err()
        assert filt(p, None, p, None, 4, 4, 0.99, *tail) == -1 and b"null" in err()
        assert filt(p, p, mis, None, 4, 4, 0.99, *tail) == -2
        assert filt(p, p, p, None, 1025, 4, 0.99, *tail) == -1 and b"1024" in err()
        assert filt(p, p, p, p, 4, 4, 0.99, *tail) == -1 and b"alias" in err()
        assert loss(p, p, p, 0.25, p, p, None, 8, 0.5, p, p, p, 4, 512, *ws, *tail) == -1 and b"null" in err()
        assert loss(p, mis, p, 0.25, p, p, p, 8, 0.5, p, p, p, 4, 512, *ws, *tail) == -2
        assert loss(p, p, p, 0.25, p, p, p, 8, 0.5, p, p, p, 4, 511, *ws, *tail) == -1 and b"512 features" in err()
    # missing / short workspaces (device entry points only: a twin takes none)
    assert lib.mi355ppo_rnd_obs_moments_u8(p, 4, RB, 4, 3, p, None, 0, None) == -4 and b"workspace" in err()
    assert lib.mi355ppo_rnd_obs_moments_u8(p, 257, RB, 4, 3, p, p, 2 * 2 * R.P * 4 - 1, None) == -4
    assert lib.mi355ppo_rnd_loss_fwd_bwd_f32(p, p, p, 0.25, p, p, p, 8, 0.5, p, p, p, 4, 512, None, 0, None) == -4 and b"workspace" in err()
    assert lib.mi355ppo_rnd_loss_fwd_bwd_f32(p, p, p, 0.25, p, p, p, 8, 0.5, p, p, p, 4, 512, p, 15, None) == -4
    assert lib.mi355ppo_rnd_obs_moments_workspace_bytes(257) == 2 * 2 * R.P * 4 and lib.mi355ppo_rnd_obs_moments_workspace_bytes(1 << 24) == 0
    assert lib.mi355ppo_rnd_loss_workspace_bytes(4096) == 16 + 4096 * 4          # the mask count's 16-byte head, then M floats
    # the wrappers refuse before the C call
    with pytest.raises(_lib.Mi355PpoError, match="512 features"):
        H.rnd_intrinsic_reward(torch.zeros(2, 256), torch.zeros(2, 256))
    with pytest.raises(TypeError):
        H.rnd_normalize(torch.zeros((2, 84, 84, 4)), torch.zeros(R.P, dtype=torch.float64), torch.ones(R.P, dtype=torch.float64))
    with pytest.raises(ValueError):
        H.rnd_obs_moments(torch.zeros((2, 84, 84, 3), dtype=torch.uint8))


# ---------------------------------------------------------------------------------------------- the learner's fused branch on the CPU
def test_the_switch_is_read_when_a_learner_is_built(monkeypatch):
    from cleanrl_amd import learner_rnd

    monkeypatch.delenv("MI355PPO_RND", raising=False)
    assert learner_rnd.rnd_backend() == "torch"
    monkeypatch.setenv("MI355PPO_RND", "fused")
    assert learner_rnd.rnd_backend() == "fused"
    monkeypatch.setenv("MI355PPO_RND", "hip")
    with pytest.raises(ValueError, match="MI355PPO_RND"):
        learner_rnd.rnd_backend()


def test_fused_branch_of_the_learner_on_the_goldens_rollout_against_the_host_learner(monkeypatch):
    """``RNDPPOLearner``'s fused branch with ``host_ops`` standing in for ``ops`` (tests/test_hip_branches_on_fake_ops.py's harness),
    through the golden's frames, dones and rewards and one update, against the host learner at that file's bars."""
    from test_hip_branches_on_fake_ops import FakeOps, _compare_rollout_and_update, _pair

    from cleanrl_amd import envs as E
    from cleanrl_amd.agents import RNDAgent, RNDModel
    from cleanrl_amd.learner_rnd import DeviceRunningMeanStd, RNDPPOLearner, _Combined
    from cleanrl_amd.learner_smoke import default_args

    class FusedOps(FakeOps):
        rnd_normalize, rnd_obs_moments, rnd_intrinsic_reward = H.rnd_normalize, H.rnd_obs_moments, H.rnd_intrinsic_reward
        rnd_reward_filter_, rnd_loss_fwd_bwd = H.rnd_reward_filter_, H.rnd_loss_fwd_bwd

    g = R.golden()
    T, N = g["rewards"].shape
    A = int(g["n_actions"])
    envs = SimpleNamespace(single_observation_space=E.Box(0, 255, (4, 84, 84), np.uint8), single_action_space=E.Discrete(A))
    args = lambda: default_args(num_steps=T, num_minibatches=2, update_epochs=1, gamma=0.999, int_gamma=0.99, clip_coef=0.1,      # noqa: E731
                                ent_coef=0.001, update_proportion=0.25, int_coef=1.0, ext_coef=2.0, learning_rate=1e-4)
    monkeypatch.delenv("MI355PPO_RND", raising=False)

    def make(ag):
        return RNDPPOLearner(ag, RNDModel(4, A), args(), envs.single_observation_space, envs.single_action_space, N, CPU)

    host, fake = _pair(lambda: RNDAgent(envs), make, flat_module=lambda L: _Combined(L.agent, L.rnd_model.predictor))
    assert not host.rnd_fused and not fake.rnd_fused
    fake._extra = torch.zeros((2, 2))
    fake._zeros_TN, fake._zeros_N = torch.zeros((T, N)), torch.zeros(N)
    fake.ops = FusedOps
    for L in (host, fake):
        L.obs_rms.mean, L.obs_rms.var, L.obs_rms.count = g["obs_mean0"].copy(), g["obs_var0"].copy(), float(g["obs_count0"])
    fake.init_rnd_fused()
    assert fake.rnd_fused and isinstance(fake.reward_rms, DeviceRunningMeanStd)
    mh, mf = _compare_rollout_and_update(host, fake, g["frames_u8"], g["step_done"], g["rewards"], [host.agent, host.rnd_model.predictor],
                                         [fake.agent, fake.rnd_model.predictor], lr=1e-4, extra_step=lambda L, step: L.curiosity(step))
    assert torch.allclose(host.int_returns, fake.int_returns, rtol=1e-5, atol=1e-6) and host.int_returns.abs().sum() > 0
    assert torch.allclose(host.curiosity_rewards, fake.curiosity_rewards, rtol=1e-5, atol=1e-7)
    assert abs(mh["fwd_loss"] - mf["fwd_loss"]) <= 1e-5 * max(1.0, abs(mh["fwd_loss"]))
    assert np.allclose(host.obs_rms.mean, fake.obs_rms.mean, atol=1e-4) and np.allclose(host.obs_rms.var, fake.obs_rms.var, rtol=1e-5)
    assert abs(host.reward_rms.var - fake.reward_rms.var) <= 1e-6 * host.reward_rms.var
    assert torch.count_nonzero(fake._rnd_rewems) == T                                # the filter state lives in the fused branch's tensor
    fake.reward_rms.var = 2.0                                                        # assigning still works
    assert fake.reward_rms.var == 2.0 and fake.reward_rms.stats[1].item() == 2.0
