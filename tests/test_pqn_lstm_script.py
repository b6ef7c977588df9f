"""pqn_atari_envpool_lstm.py drop-in: AtariLSTMQNetwork + LSTMPQNLearner against two iterations of the reference's own lines
(tests/golden/pqn_lstm_iteration.npz, minted by tools/mint_pqn_lstm_goldens.py), the fused backend through the host twins, the CLI
surface and short runs of the script."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pqn_lstm_cases as C
from test_pqn_script import ITER_BAR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROLLOUT = ("actions", "values", "rewards", "dones", "returns", "next_done", "initial_h", "initial_c")


@pytest.fixture
def one_thread():
    """The golden was minted on one CPU thread (orthogonal_'s QR and the GEMM reductions round differently with more)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def test_golden_conditions():
    """What makes the case a test of the recurrence: the state is reset in mid-rollout in both iterations, iteration 2 starts from
    a non-zero state, the bootstrap sees a finished env, and greedy as well as random actions occur."""
    g = C.golden_case()
    assert g["dones"].shape[0] == 2
    assert all(g["dones"][it][1:].sum() >= 1 for it in range(2))
    assert np.abs(g["initial_h"][0]).max() == 0 and np.abs(g["initial_h"][1]).max() > 0 and np.abs(g["initial_c"][1]).max() > 0
    assert len(np.unique(g["actions"])) >= 3
    assert g["next_done"].sum() >= 1


def test_seeded_construction_equals_the_reference_weights(one_thread):
    from cleanrl_amd.agents import AtariLSTMQNetwork

    g = C.golden_case()
    args, cfg = C.golden_args(g)
    torch.manual_seed(args.seed)
    init = C.flat(AtariLSTMQNetwork(C.golden_envs(args, cfg)))
    assert torch.equal(init[::int(g["stride"])], torch.from_numpy(g["init_params_sub"]))
    assert init.double().sum().item() == float(g["init_checksum"])


def test_torch_backend_reproduces_the_reference_bit_for_bit(one_thread):
    g = C.golden_case()
    recs, metrics, net, learner = C.replay(g, backend="torch")
    for it, r in enumerate(recs):
        for k in ROLLOUT:
            assert torch.equal(r[k], torch.from_numpy(g[k][it])), (it, k)
    for it, m in enumerate(metrics):
        assert m["td_loss"] == float(g["s_td_loss"][it]) and m["q_values"] == float(g["s_q_values"][it]), (it, m)
    assert learner.global_step == int(g["s_global_step"][-1])
    assert torch.equal(learner.next_lstm_state[0], torch.from_numpy(g["final_h"]))
    assert torch.equal(learner.next_lstm_state[1], torch.from_numpy(g["final_c"]))
    final = C.flat(net)
    assert torch.equal(final[::int(g["stride"])], torch.from_numpy(g["final_params_sub"]))
    assert final.double().sum().item() == float(g["final_checksum"])


def test_fused_backend_on_the_twins_within_the_bar(one_thread):
    g = C.golden_case()
    recs, metrics, net, learner = C.replay(g, backend="fused")
    assert learner.fused
    for it, r in enumerate(recs):
        for k in ("actions", "rewards", "dones", "next_done"):
            assert torch.equal(r[k], torch.from_numpy(g[k][it])), (it, k)
        for k in ("values", "returns", "initial_h", "initial_c"):
            ref = torch.from_numpy(g[k][it])
            err = (r[k].double() - ref.double()).abs().max().item()
            print(it, k, err)
            assert err <= ITER_BAR["values"] * max(1.0, ref.abs().max().item()), (it, k, err)
    for it, m in enumerate(metrics):
        for k in ("td_loss", "q_values"):
            a, b = float(g["s_" + k][it]), float(m[k])
            print(it, k, abs(a - b))
            assert abs(a - b) <= ITER_BAR["scalar"] * max(1.0, abs(a)), (it, k, a, b)
    err = (C.flat(net)[::int(g["stride"])] - torch.from_numpy(g["final_params_sub"])).abs().max().item()
    print("params", err)
    assert err <= ITER_BAR["params"]


def test_backend_switch_is_mi355ppo_pqn_alone(monkeypatch):
    from cleanrl_amd.agents import AtariLSTMQNetwork
    from cleanrl_amd.learner_pqn_lstm import LSTMPQNLearner

    g = C.golden_case()
    args, cfg = C.golden_args(g)
    envs = C.golden_envs(args, cfg)
    make = lambda: LSTMPQNLearner(AtariLSTMQNetwork(envs), args, envs.single_observation_space.shape, 4, args.num_envs, "cpu")  # noqa: E731
    monkeypatch.delenv("MI355PPO_PQN", raising=False)
    monkeypatch.setenv("MI355PPO_LSTM", "fused")                      # not read by this script
    assert make().backend == "torch"
    monkeypatch.setenv("MI355PPO_PQN", "fused")
    monkeypatch.setenv("MI355PPO_LSTM", "torch")
    assert make().backend == "fused"
    monkeypatch.setenv("MI355PPO_PQN", "triton")
    with pytest.raises(ValueError, match="MI355PPO_PQN"):
        make()


def test_cli_surface_matches_the_reference():
    from cleanrl_amd import pqn_atari_envpool_lstm as mod

    with open(os.path.join(ROOT, "tests", "golden", "pqn_lstm_cli_surface.json")) as fh:
        ref = json.load(fh)["lstm"]
    mine = {f.name: f.default for f in dataclasses.fields(mod.Args)}
    assert mine.pop("exp_name") == "pqn_atari_envpool_lstm"
    assert mine == ref and mine["max_grad_norm"] == 0.5


@pytest.mark.parametrize("backend", ["torch", "fused"])
def test_script_runs_on_the_stand_in(backend, tmp_path):
    env = dict(os.environ, MI355PPO_PQN=backend)
    cmd = [sys.executable, os.path.join(ROOT, "cleanrl_amd", "pqn_atari_envpool_lstm.py"), "--no-cuda", "--num-minibatches", "2",
           "--update-epochs", "1", "--num-envs", "4", "--num-steps", "8", "--total-timesteps", "64"]
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp_path, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert len([ln for ln in out.stdout.splitlines() if ln.startswith("SPS: ")]) == 2
