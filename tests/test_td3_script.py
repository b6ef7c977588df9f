"""ddpg_continuous_action.py / td3_continuous_action.py drop-ins against whole runs of the reference's own lines
(tests/golden/td3_iteration.npz, minted by tools/mint_td3_goldens.py): the CLI surface, the ``torch`` backend bit for bit, the
``fused`` backend through the host twins within the recorded sensitivity, the launch budget, and short runs of both scripts."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import td3_replay as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("td3", "td3_n2", "ddpg")


@pytest.fixture
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("script", ["ddpg_continuous_action", "td3_continuous_action"])
def test_cli_surface_equals_the_reference(script):
    mod = __import__("cleanrl_amd." + script, fromlist=["Args"])
    want = R.surface()[script]
    fields = dataclasses.fields(mod.Args)
    assert [f.name for f in fields] == want["order"]
    assert {f.name: f.default for f in fields if f.name != "exp_name"} == want["defaults"]
    assert mod.Args().exp_name == script


@pytest.mark.parametrize("name", CASES)
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
    L = rec["learner"]
    assert (L.pos, L.full) == (100 % L.slots, True)


@pytest.mark.parametrize("name", CASES)
def test_fused_backend_on_the_twins_stays_within_the_sensitivity_bar(name, one_thread):
    R.assert_within_sensitivity(name, R.replay(name, "fused"))


def test_fused_free_running_draws_the_reference_streams(one_thread):
    """Not teacher-forced: the fused backend's own draws (sample(), torch.normal, randint x 2, randn) follow the reference's order, so
    its sampled indices are the golden ones and its actions before the first update are the golden ones up to rounding."""
    g = R.golden_case("td3_n2")
    idx = []
    from cleanrl_amd.learner_offpolicy import OffPolicyLearner

    orig = OffPolicyLearner.sample_indices

    def spy(self, n):
        out = orig(self, n)
        idx.append(out)
        return out

    OffPolicyLearner.sample_indices = spy
    try:
        acts = _free_fused("td3_n2")
    finally:
        OffPolicyLearner.sample_indices = orig
    trained = g["batch_inds"][:, 0] >= 0
    assert len(idx) == int(trained.sum())
    for (bi, ei), gb, ge in zip(idx, g["batch_inds"][trained], g["env_inds"][trained]):
        assert np.array_equal(bi, gb) and np.array_equal(ei, ge)
    # up to and including the first step after learning_starts no update has run: sample() is exact, the first actor output differs
    # by rounding only (op_tanh is within 3e-7 of tanh; the sums are f32 in another order)
    first = int(np.flatnonzero(trained)[0])
    assert np.array_equal(acts[:first - 1], g["actions"][:first - 1])
    assert np.abs(acts[:first + 1] - g["actions"][:first + 1]).max() < 1e-5


def _free_fused(name):
    import json
    import random

    from cleanrl_amd import envs as E
    from cleanrl_amd.agents import ActionValueNetwork, Actor
    from cleanrl_amd.learner_offpolicy import OffPolicyLearner
    from cleanrl_amd.td3_continuous_action import Args

    g = R.golden_case(name)
    cfg = json.loads(bytes(g["config"]).decode())
    args = Args(**cfg["args"])
    random.seed(args.seed), np.random.seed(args.seed), torch.manual_seed(args.seed)
    envs = E.SyntheticReplayVecEnv(args.num_envs, seed=args.seed, horizon=cfg["horizon"])
    actor, qfs = Actor(envs), [ActionValueNetwork(envs) for _ in range(2)]
    qts, ta = [ActionValueNetwork(envs) for _ in range(2)], Actor(envs)
    ta.load_state_dict(actor.state_dict())
    for q, t in zip(qfs, qts):
        t.load_state_dict(q.state_dict())
    L = OffPolicyLearner(actor, qfs, ta, qts, args, envs, torch.device("cpu"), td3=True, backend="fused")
    obs, _ = envs.reset(seed=args.seed)
    acts = []
    for global_step in range(cfg["steps"]):
        actions = L.act(obs, global_step)
        acts.append(np.asarray(actions, np.float32))
        next_obs, rewards, terminations, truncations, infos = envs.step(actions)
        real_next_obs = next_obs.copy()
        for i, tr in enumerate(truncations):
            if tr:
                real_next_obs[i] = infos["final_observation"][i]
        L.store(obs, real_next_obs, actions, rewards, terminations)
        obs = next_obs
        if global_step > args.learning_starts:
            L.train_step(global_step % args.policy_frequency == 0)
    return np.stack(acts)


def test_launch_budget_of_a_td3_step(monkeypatch):
    """add 1 + target 1 + critic 1 call (2 launches) + Adam 1 call (2) + actor 1 call (2) + Adam (2) + Polyak 1 + act 1: 8 library
    calls, 12 launches.  What is counted is the library calls a step makes (on the twins' ``_lib.call``); the launches per call in
    ``LAUNCHES`` are read off the entry points' source (csrc/offpolicy.hip, csrc/optim.hip), not measured: an entry point that grew
    a launch would have to be entered here by hand.  tests/test_gpu_offpolicy.py counts the same calls on the device path."""
    from cleanrl_amd import _lib

    LAUNCHES = {"mi355ppo_replay_add_f32_cpu": 1, "mi355ppo_ddpg_act_f32_cpu": 1, "mi355ppo_td3_target_f32_cpu": 1,
                "mi355ppo_td3_critic_fwd_bwd_f32_cpu": 2, "mi355ppo_td3_actor_fwd_bwd_f32_cpu": 2, "mi355ppo_clip_adam_f32_cpu": 2,
                "mi355ppo_polyak_f32_cpu": 1}
    seen = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (seen.append(name), real(name, *a))[1])
    steps = []

    import td3_replay

    orig_store = td3_replay.OffPolicyLearner.store

    def store(self, *a):
        steps.append(len(seen))
        return orig_store(self, *a)

    monkeypatch.setattr(td3_replay.OffPolicyLearner, "store", store)
    _free_fused("td3")
    assert set(seen) <= set(LAUNCHES)
    # a step = everything from one store() to the next (store, train, the next act)
    per_step = [sum(LAUNCHES[n] for n in seen[a:b]) for a, b in zip(steps[:-1], steps[1:])]
    assert max(per_step) == 12 and sorted(set(per_step[20:])) == [7, 12]


@pytest.mark.parametrize("script", ["ddpg_continuous_action.py", "td3_continuous_action.py"])
@pytest.mark.parametrize("backend", ["torch", "fused"])
def test_scripts_run_end_to_end_on_the_cpu(script, backend, tmp_path):
    env = dict(os.environ, MI355PPO_OFFPOLICY=backend, MI355PPO_STANDIN_HORIZON="25")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "cleanrl_amd", script), "--no-cuda", "--total-timesteps", "102", "--learning-starts",
                        "30", "--buffer-size", "64", "--batch-size", "16", "--save-model"], env=env, capture_output=True, text=True, timeout=600,
                       cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "SPS:" in r.stdout and "episodic_return" in r.stdout and "model saved to" in r.stdout
    r = subprocess.run([sys.executable, os.path.join(ROOT, "cleanrl_amd", script), "--no-cuda", "--total-timesteps", "3", "--save-model",
                        "--upload-model"], env=env, capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert r.returncode != 0 and "upload-model" in r.stderr


def test_unknown_backend_is_refused(monkeypatch):
    from cleanrl_amd.learner_offpolicy import offpolicy_backend

    monkeypatch.setenv("MI355PPO_OFFPOLICY", "eager")
    with pytest.raises(ValueError, match="MI355PPO_OFFPOLICY"):
        offpolicy_backend("cpu")
