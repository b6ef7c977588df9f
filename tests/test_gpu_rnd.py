"""The RND kernels (csrc/rnd.hip) on the MI355X: every entry point bit-equal to its host twin on the cases of tests/rnd_cases.py,
the guard-band cases on device tensors with exact workspaces, a non-default stream, and ``MI355PPO_RND=fused`` in the learner --
teacher-forced against the reference's iteration, the script, and no device-to-host copy in ``finish_rollout``."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import guard_arena as GA
import rnd_cases as R
from conftest import load_golden
from cleanrl_amd import envs as E
from cleanrl_amd import host_ops as H
from cleanrl_amd import ops
from cleanrl_amd.learner_smoke import default_args
from test_rnd_bounds import run_guarded

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CPU = torch.device("cpu")


def _same(a, b, what):
    assert GA.same_bits(a, b), f"{what}: the device differs from its twin"


@pytest.mark.parametrize("M", R.NORMALIZE_M)
@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("nhwc", [True, False])
def test_normalize_equals_its_twin_and_the_float64_expression(M, gather, nhwc):
    c = R.normalize_case(M, gather)
    got = R.run_normalize(ops, c, nhwc, *R.plain(DEV))
    _same(got, R.run_normalize(H, c, nhwc, *R.plain(CPU)), "normalize")
    assert torch.equal(got.cpu(), c["want"])


@pytest.mark.parametrize("B,nhwc", R.MOMENT_CASES)
def test_moments_equal_their_twin_and_the_integer_sums(B, nhwc):
    c = R.moments_case(B)
    got = R.run_moments(ops, c, nhwc, *R.plain(DEV)).cpu().numpy().astype(np.uint64)
    assert np.array_equal(got[0], c["S1"]) and np.array_equal(got[1], c["S2"])


@pytest.mark.parametrize("N", R.INTRINSIC_N)
def test_intrinsic_reward_equals_its_twin(N):
    c = R.intrinsic_case(N)
    got = R.run_intrinsic(ops, c, *R.plain(DEV))
    _same(got, R.run_intrinsic(H, c, *R.plain(CPU)), "intrinsic reward")
    assert ((got.cpu().double() - c["want64"]).abs() / c["want64"]).max().item() <= 1e-4


@pytest.mark.parametrize("T,N,golden_raw", [(8, 4, True)] + [s + (False,) for s in R.FILTER_SHAPES])
def test_reward_filter_equals_its_twin_over_two_rollouts(T, N, golden_raw):
    steps = R.filter_case(T, N, golden_raw)
    dev, host = R.run_filter(ops, steps, *R.plain(DEV)), R.run_filter(H, steps, *R.plain(CPU))
    for k, (d, h) in enumerate(zip(dev, host)):
        for name, a, b in zip(("scaled", "filtered", "rewems", "stats"), d, h):
            _same(a, b, f"rollout {k} {name}")
    if golden_raw:
        assert np.array_equal(dev[0][0].cpu().numpy(), R.golden()["scaled_curiosity"])


@pytest.mark.parametrize("M", R.LOSS_M)
@pytest.mark.parametrize("mask", [m for m, _ in R.LOSS_MASKS])
def test_loss_equals_its_twin(M, mask):
    c = R.loss_case(M, mask)
    dev, host = R.run_loss(ops, c, *R.plain(DEV)), R.run_loss(H, c, *R.plain(CPU))
    for k in host:
        _same(dev[k], host[k], f"loss {k}")


@pytest.mark.parametrize("sentinel", GA.SENTINELS, ids=[f"0x{s:08X}" for s in GA.SENTINELS])
def test_kernels_stay_inside_their_tensors_and_exact_workspaces(sentinel, monkeypatch):
    ref = R.every_entry_point(H, *R.plain(CPU))
    out, arena, requested = run_guarded(ops, DEV, monkeypatch, sentinel)
    arena.assert_guards_intact()
    assert requested and max(requested) > 0
    for k, v in ref.items():
        _same(out[k], v, f"sentinel 0x{sentinel:08X}, {k}")


def test_a_non_default_stream_gives_the_same_bits():
    ref = R.every_entry_point(ops, *R.plain(DEV))
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        out = R.every_entry_point(ops, *R.plain(DEV))
    s.synchronize()
    for k, v in ref.items():
        _same(out[k], v, k)


# ------------------------------------------------------------------------------------------------ the learner under MI355PPO_RND=fused
def _init_1thread(seed, build):
    n = torch.get_num_threads()
    torch.set_num_threads(1)          # as when minted
    torch.manual_seed(seed)
    out = build()
    torch.set_num_threads(n)
    return out


def _delta_matches(got_now, init_sub, final_sub, what, frac=0.98, rtol=5e-2, atol=2e-5):
    delta, want = got_now - init_sub, final_sub - init_sub
    close = np.isclose(delta, want, rtol=rtol, atol=atol)
    assert close.mean() > frac, f"{what}: only {close.mean():.4f} of sampled parameters moved as the reference's did"


def test_fused_rnd_teacher_forced_against_reference_iteration(monkeypatch):
    """tests/test_zz_gpu_new_scripts.py::test_rnd_hip_path_teacher_forced_against_reference_iteration under the fused backend, at that
    test's bars; on the forced raw rewards ``scaled_curiosity`` is additionally the reference's bit for bit, and ``finish_rollout``
    copies nothing to the host."""
    from cleanrl_amd.agents import RNDAgent, RNDModel
    from cleanrl_amd.learner_rnd import DeviceRunningMeanStd, RNDPPOLearner

    monkeypatch.setenv("MI355PPO_RND", "fused")
    g = load_golden("rnd_iteration")["rnd_T8_N4"]
    T, N = g["rewards"].shape
    envs = SimpleNamespace(single_observation_space=E.Box(0, 255, (4, 84, 84), np.uint8),
                           single_action_space=E.Discrete(int(g["n_actions"])))
    agent, rnd_model = _init_1thread(int(g["init_seed"]), lambda: (RNDAgent(envs), RNDModel(4, envs.single_action_space.n)))
    agent, rnd_model = agent.to(DEV), rnd_model.to(DEV)
    args = default_args(num_steps=T, num_minibatches=2, update_epochs=1, gamma=0.999, int_gamma=0.99, clip_coef=0.1,
                        ent_coef=0.001, update_proportion=0.25, int_coef=1.0, ext_coef=2.0, learning_rate=1e-4)
    L = RNDPPOLearner(agent, rnd_model, args, envs.single_observation_space, envs.single_action_space, N, DEV, sample_seed=1)
    assert L.hip and L.obs.dtype == torch.uint8 and L.rnd_fused and isinstance(L.reward_rms, DeviceRunningMeanStd)
    stride = int(g["stride"])
    np.testing.assert_allclose(L.flat.params[::stride].cpu().numpy(), g["init_params_sub"], rtol=1e-4, atol=1e-5)
    L.obs_rms.mean, L.obs_rms.var, L.obs_rms.count = g["obs_mean0"].copy(), g["obs_var0"].copy(), float(g["obs_count0"])
    L.refresh_obs_stats()
    frames, step_done = g["frames_u8"], g["step_done"]
    F = lambda k: torch.from_numpy(g[k]).to(DEV)      # noqa: E731
    L.observe(0, frames[0], step_done[0])
    for step in range(T):
        L.act(step)
        np.testing.assert_allclose(L.values[step].cpu().numpy(), g["ext_values"][step], rtol=1e-3, atol=2e-4)
        np.testing.assert_allclose(L.int_values[step].cpu().numpy(), g["int_values"][step], rtol=1e-3, atol=2e-4)
        L.actions[step].copy_(F("actions")[step]); L.logprobs[step].copy_(F("logprobs")[step])
        L.values[step].copy_(F("ext_values")[step]); L.int_values[step].copy_(F("int_values")[step])
        L.store_reward(step, g["rewards"][step])
        L.observe(step + 1, frames[step + 1], step_done[step + 1])
        L.curiosity(step)
        np.testing.assert_allclose(L.curiosity_rewards[step].cpu().numpy(), g["raw_curiosity"][step], rtol=2e-3, atol=1e-5)
        L.curiosity_rewards[step].copy_(F("raw_curiosity")[step])
    torch.cuda.synchronize()
    # no device-to-host copy in finish_rollout unless reward_rms is read
    copies = []
    real = {n: getattr(torch.Tensor, n) for n in ("cpu", "item", "tolist", "numpy")}
    for n, fn in real.items():
        monkeypatch.setattr(torch.Tensor, n, lambda self, *a, _n=n, _fn=fn, **kw: (copies.append(_n), _fn(self, *a, **kw))[1])
    L.finish_rollout()
    for n, fn in real.items():
        monkeypatch.setattr(torch.Tensor, n, fn)
    assert copies == [], f"finish_rollout copied to the host: {copies}"
    assert np.array_equal(L.curiosity_rewards.cpu().numpy(), g["scaled_curiosity"])
    assert abs(L.reward_rms.var - float(g["reward_var"])) <= 1e-6 * float(g["reward_var"])
    for mine, gold in ((L.curiosity_rewards, "scaled_curiosity"), (L.advantages, "ext_advantages"), (L.returns, "ext_returns"),
                       (L.int_advantages, "int_advantages"), (L.int_returns, "int_returns")):
        np.testing.assert_allclose(mine.cpu().numpy(), g[gold], rtol=1e-3, atol=3e-4, err_msg=gold)
        mine.copy_(F(gold))
    np.random.seed(int(g["shuffle_seed"]))
    torch.manual_seed(int(g["mask_seed"]))
    # the distillation mask (:473 torch.rand(..., device=device)) is forced too: drawn from the CPU generator as when minted
    real_rand = torch.rand
    monkeypatch.setattr(torch, "rand", lambda *a, device=None, **kw: real_rand(*a, **kw).to(device) if device is not None
                        else real_rand(*a, **kw))
    m = L.update(float(g["lr"]))
    monkeypatch.setattr(torch, "rand", real_rand)
    assert m["num_updates"] == 2
    np.testing.assert_allclose(L.obs_rms.mean, g["obs_mean1"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(L.obs_rms.var, g["obs_var1"], rtol=1e-6, atol=0)
    for key, gold in (("policy_loss", "last_pg_loss"), ("value_loss", "last_v_loss"), ("entropy", "last_entropy")):
        ref = float(np.asarray(g[gold]).reshape(-1)[0])
        assert abs(m[key] - ref) <= 2e-3 * max(1.0, abs(ref)), (key, m[key], ref)
    ref = float(g["last_fwd_loss"][0])
    assert abs(m["fwd_loss"] - ref) <= 2e-3 * max(1.0, abs(ref)), ("fwd_loss", m["fwd_loss"], ref)
    _delta_matches(L.flat.params[::stride].cpu().numpy(), g["init_params_sub"], g["final_params_sub"], "RND update", frac=0.9)
    L.flat.check_views()


def test_ppo_rnd_envpool_script_runs_fused_on_gpu(monkeypatch):
    from cleanrl_amd import ppo_rnd_envpool

    monkeypatch.setenv("MI355PPO_RND", "fused")
    L = ppo_rnd_envpool.main(["--num-envs", "8", "--num-steps", "16", "--total-timesteps", "256", "--num-minibatches", "4",
                              "--num-iterations-obs-norm-init", "1"])
    assert L.hip and L.rnd_fused and L.obs.dtype == torch.uint8 and L.flat.numel == sum(p.numel() for p in L.combined_parameters)
    assert np.isfinite(L.last_metrics["loss"]) and np.isfinite(L.last_metrics["fwd_loss"])
    assert L.int_returns.abs().sum().item() > 0 and L.curiosity_rewards.min().item() >= 0.0
    assert L.reward_rms.count > 1.0 and np.isfinite(L.reward_rms.var) and L._rnd_rewems.abs().sum().item() > 0
    L.flat.check_views()
