"""dqn_atari.py / c51_atari.py drop-ins against whole runs of the reference's own lines (tests/golden/dqn_atari_iteration.npz, minted by
tools/mint_dqn_atari_goldens.py): the CLI surface, the ``torch`` backend bit for bit, the ``fused`` backend through the host twins within
the recorded sensitivity, the random streams of a free-running fused run, and short runs of both scripts."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dqn_atari_replay as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("script", ["dqn_atari", "c51_atari"])
def test_cli_surface_equals_the_reference(script):
    mod = __import__("cleanrl_amd." + script, fromlist=["Args"])
    want = R.surface()[script]
    fields = dataclasses.fields(mod.Args)
    assert [f.name for f in fields] == want["order"]
    assert {f.name: f.default for f in fields if f.name != "exp_name"} == want["defaults"]
    assert mod.Args().exp_name == script


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
    L = rec["learner"]
    assert (L.pos, L.full) == (40 % L.slots, True)


@pytest.mark.parametrize("name", R.CASES)
def test_fused_backend_on_the_twins_stays_within_the_sensitivity_bar(name, one_thread):
    rec = R.replay(name, "fused")
    R.assert_within_sensitivity(name, rec)
    L = rec["learner"]
    assert (L.pos, L.full) == (40 % L.slots, True)


@pytest.mark.parametrize("name", ["dqn_atari", "c51_small"])
def test_fused_free_running_draws_the_reference_streams(name, one_thread, monkeypatch):
    """Not teacher-forced: the fused backend's own draws (random.random, sample(), randint x 2) follow the reference's order, so its
    sampled indices are the golden ones and every action of the random branch is the golden one."""
    from cleanrl_amd.learner_dqn_atari import AtariDQNLearner as DQNLearner

    g = R.golden_case(name)
    idx = []
    orig = DQNLearner.sample_indices
    monkeypatch.setattr(DQNLearner, "sample_indices", lambda self, n: (idx.append(orig(self, n)), idx[-1])[1])
    rec = R.replay(name, "fused", forced=False)
    trained = g["batch_inds"][:, 0] >= 0
    assert len(idx) == int(trained.sum())
    for (bi, ei), gb, ge in zip(idx, g["batch_inds"][trained], g["env_inds"][trained]):
        assert np.array_equal(bi, gb) and np.array_equal(ei, ge)
    rb = g["random_branch"].astype(bool)
    assert 0 < rb.sum() < len(rb)
    assert np.array_equal(rec["actions"][rb], g["actions"][rb])
    first = int(np.flatnonzero(trained)[0])
    assert np.array_equal(rec["actions"][:first + 1], g["actions"][:first + 1])       # no update has run yet: the greedy actions too


@pytest.mark.parametrize("script", ["dqn_atari.py", "c51_atari.py"])
@pytest.mark.parametrize("backend", ["torch", "fused"])
def test_scripts_run_end_to_end_on_the_cpu(script, backend, tmp_path):
    env = dict(os.environ, MI355PPO_OFFPOLICY=backend, MI355PPO_STANDIN_HORIZON="10")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "cleanrl_amd", script), "--no-cuda", "--total-timesteps", "202", "--learning-starts",
                        "30", "--buffer-size", "16", "--batch-size", "8", "--train-frequency", "2", "--target-network-frequency", "6",
                        "--save-model"], env=env, capture_output=True, text=True, timeout=600, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "SPS:" in r.stdout and "episodic_return" in r.stdout and "model saved to" in r.stdout


def test_c51_target_update_is_a_copy_not_a_polyak_step():
    """``load_state_dict`` keeps ``-0.0`` and never reads the old target; ``1 * p + 0 * t`` would do neither."""
    g, mod, args, envs, L, _ = R.build("c51_small", "fused")
    with torch.no_grad():
        L.online[0] = -0.0
        L.target[1] = float("inf")
    L.sync_target()
    assert torch.equal(L.target, L.online) and torch.signbit(L.target[0]) and torch.isfinite(L.target).all()


def test_out_of_limit_sizes_raise_the_named_error_from_the_script(monkeypatch):
    from cleanrl_amd import c51_atari

    monkeypatch.setenv("MI355PPO_OFFPOLICY", "fused")
    with pytest.raises(ValueError, match="MI355PPO_OFFPOLICY=torch"):
        c51_atari.main(["--no-cuda", "--n-atoms", "102", "--buffer-size", "16", "--total-timesteps", "4"])
