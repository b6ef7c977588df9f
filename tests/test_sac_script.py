"""sac_continuous_action.py against whole runs of the reference's own lines (tests/golden/sac_iteration.npz, minted by
tools/mint_sac_goldens.py): the CLI surface, the ``torch`` backend bit for bit, the ``fused`` backend through the host twins within
the recorded sensitivity, the random streams, the launch budget, and short runs of the script."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sac_replay as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def test_cli_surface_equals_the_reference():
    from cleanrl_amd import sac_continuous_action as mod

    want = R.surface()["sac_continuous_action"]
    fields = dataclasses.fields(mod.Args)
    assert [f.name for f in fields] == want["order"]
    assert {f.name: f.default for f in fields if f.name != "exp_name"} == want["defaults"]
    assert mod.Args().exp_name == "sac_continuous_action"


@pytest.mark.parametrize("name", R.CASES)
def test_torch_backend_reproduces_the_reference_bit_for_bit(name, one_thread):
    g = R.golden_case(name)
    rec = R.replay(name, "torch")
    assert rec["init_checksum"] == float(g["init_checksum"])
    assert np.array_equal(rec["actions"], g["actions"])
    for k in R.SCALARS:
        assert np.array_equal(rec[k], g[k], equal_nan=True), k
    s = int(g["stride"])
    for k in R.FINAL:
        assert torch.equal(rec["final_" + k][::s], torch.from_numpy(g[f"final_{k}_sub"])), k
        assert rec["final_" + k].double().sum().item() == float(g[f"final_{k}_checksum"]), k
    assert rec["final_log_alpha"] == float(g["final_log_alpha"])
    L = rec["learner"]
    assert (L.pos, L.full) == (100 % L.slots, True)


@pytest.mark.parametrize("name", R.CASES)
def test_fused_backend_on_the_twins_stays_within_the_sensitivity_bar(name, one_thread):
    R.assert_within_sensitivity(name, R.replay(name, "fused"))


def test_fused_free_running_draws_the_reference_streams(one_thread, monkeypatch):
    """Not teacher-forced: the fused backend's own draws (sample(), randint x 2, one randn per get_action) follow the reference's
    order, so its sampled indices and its noises are the golden ones and its actions before the first update are the golden ones up
    to rounding."""
    from cleanrl_amd.learner_sac import SACLearner

    g = R.golden_case("sac_n2")
    idx, noises = [], []
    orig_idx, orig_upd = SACLearner.sample_indices, SACLearner.update_kernels
    monkeypatch.setattr(SACLearner, "sample_indices", lambda self, n: (idx.append(orig_idx(self, n)), idx[-1])[1])
    monkeypatch.setattr(SACLearner, "update_kernels", lambda self, bi, ei, nz, *a, **k: (noises.extend(nz), orig_upd(self, bi, ei, nz, *a, **k))[1])
    rec = R.replay("sac_n2", "fused", forced=False)
    trained = g["batch_inds"][:, 0] >= 0
    assert len(idx) == int(trained.sum())
    for (bi, ei), gb, ge in zip(idx, g["batch_inds"][trained], g["env_inds"][trained]):
        assert np.array_equal(bi, gb) and np.array_equal(ei, ge)
    want = [d for ds in R.golden_noise("sac_n2") for d in ds]
    assert len(noises) == len(want) and all(torch.equal(a, b) for a, b in zip(noises, want))
    first = int(np.flatnonzero(trained)[0])
    assert np.array_equal(rec["actions"][:first - 1], g["actions"][:first - 1])
    assert np.abs(rec["actions"][:first + 1] - g["actions"][:first + 1]).max() < 1e-5


CRITIC_STEP = ["mi355ppo_replay_add_f32", "mi355ppo_sac_target_f32", "mi355ppo_td3_critic_fwd_bwd_f32", "mi355ppo_clip_adam_f32",
               "mi355ppo_polyak_f32", "mi355ppo_sac_policy_f32"]
POLICY_ITER = ["mi355ppo_sac_actor_fwd_bwd_f32", "mi355ppo_clip_adam_f32", "mi355ppo_sac_policy_f32", "mi355ppo_sac_alpha_f32"]
POLICY_STEP = CRITIC_STEP[:4] + POLICY_ITER * 2 + CRITIC_STEP[4:]
LAUNCHES = {"mi355ppo_replay_add_f32": 1, "mi355ppo_sac_target_f32": 1, "mi355ppo_td3_critic_fwd_bwd_f32": 2, "mi355ppo_clip_adam_f32": 2,
            "mi355ppo_polyak_f32": 1, "mi355ppo_sac_policy_f32": 1, "mi355ppo_sac_actor_fwd_bwd_f32": 2, "mi355ppo_sac_alpha_f32": 1}


def test_launch_budget_of_a_sac_step(monkeypatch):
    """With the reference defaults (policy_frequency 2, target_network_frequency 1) a critic-only step is 8 launches and a step with
    the policy update 20, by name and in order.  What is counted is the library calls a step makes on the twins' ``_lib.call``; the
    launches per call in ``LAUNCHES`` are read off the entry points' source (csrc/sac.hip, csrc/offpolicy.hip, csrc/optim.hip), not
    measured.  tests/test_gpu_sac.py counts the same calls on the device path's ``ops._launch``."""
    from cleanrl_amd import host_ops
    from cleanrl_amd.learner_sac import SACLearner

    real_call = host_ops._lib.call
    calls = []
    monkeypatch.setattr(host_ops._lib, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    steps = []
    orig_store = SACLearner.store
    monkeypatch.setattr(SACLearner, "store", lambda self, *a: (steps.append(len(calls)), orig_store(self, *a))[1])
    R.replay("sac", "fused", forced=False)
    assert set(calls) <= {n + "_cpu" for n in LAUNCHES}
    per_step = [[n[: -len("_cpu")] for n in calls[a:b]] for a, b in zip(steps[:-1], steps[1:])]
    tail = per_step[20:]
    assert all(s in (CRITIC_STEP, POLICY_STEP) for s in tail) and CRITIC_STEP in tail and POLICY_STEP in tail
    assert sum(LAUNCHES[n] for n in CRITIC_STEP) == 8 and sum(LAUNCHES[n] for n in POLICY_STEP) == 20


def test_no_autotune_keeps_alpha_and_skips_the_alpha_launch(monkeypatch):
    from cleanrl_amd import host_ops

    calls = []
    real_call = host_ops._lib.call
    monkeypatch.setattr(host_ops._lib, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    rec = R.replay("sac_fixed", "fused")
    assert "mi355ppo_sac_alpha_f32_cpu" not in calls and "mi355ppo_sac_actor_fwd_bwd_f32_cpu" in calls
    assert rec["learner"].metrics()["alpha"] == float(np.float32(0.2)) and "alpha_loss" not in rec["learner"].metrics()


@pytest.mark.parametrize("backend", ["torch", "fused"])
def test_script_runs_end_to_end_on_the_cpu(backend, tmp_path):
    env = dict(os.environ, MI355PPO_OFFPOLICY=backend, MI355PPO_STANDIN_HORIZON="50")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "cleanrl_amd", "sac_continuous_action.py"), "--no-cuda", "--total-timesteps", "302",
                        "--learning-starts", "100", "--buffer-size", "128", "--batch-size", "64"], env=env, capture_output=True, text=True,
                       timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "SPS:" in r.stdout and "episodic_return" in r.stdout


def test_unknown_backend_is_refused(monkeypatch):
    monkeypatch.setenv("MI355PPO_OFFPOLICY", "eager")
    with pytest.raises(ValueError, match="MI355PPO_OFFPOLICY"):
        R.build("sac", None)
