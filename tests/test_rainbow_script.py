"""The rainbow_atari.py drop-in against the reference: its CLI surface (tests/golden/rainbow_cli_surface.json), whole runs of the reference's
own lines (tests/golden/rainbow_iteration.npz, both minted by tools/mint_rainbow_goldens.py) through ``RainbowLearner`` on both backends, and
runs as a script on the stand-in environment."""
import dataclasses
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import rainbow_cases as R
import rainbow_replay as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def test_cli_surface_equals_the_reference():
    """Every field in the reference's order, with its default and its help string (the string literal under the field)."""
    from cleanrl_amd import rainbow_atari

    want = P.surface()
    fields = dataclasses.fields(rainbow_atari.Args)
    assert [f.name for f in fields] == want["order"] and len(fields) == 32
    assert {f.name: f.default for f in fields if f.name != "exp_name"} == want["defaults"]
    assert rainbow_atari.Args().exp_name == "rainbow_atari"
    src = inspect.getsource(rainbow_atari.Args)
    helps = dict(re.findall(r'^    (\w+): [^\n]+\n    """(.*?)"""$', src, flags=re.M | re.S))
    assert helps == want["help"] and all(helps.values())
    with pytest.raises(AssertionError, match="vectorized envs"):
        rainbow_atari.main(["--no-cuda", "--num-envs", "2", "--total-timesteps", "2"])


@pytest.mark.parametrize("name", P.RUNS)
def test_torch_backend_follows_the_minted_run_free_running(name, one_thread):
    """Not teacher-forced: the backend's own noise, actions and draws.  The construction, every action, every sampled index and the
    final tree are the reference's; the scalars hold the family's bar."""
    rec = P.replay_run(name, "torch")
    g = rec["golden"]
    assert rec["init_checksum"] == float(g["init_checksum"])
    assert np.array_equal(rec["actions"], g["actions"]) and np.array_equal(rec["beta"], g["beta"])
    assert P.assert_run_within_bar(rec) == 15
    assert np.array_equal(rec["tree"].view(np.int32), g["tree"].view(np.int32))
    L = rec["learner"]
    assert (L.rb.pos, L.rb.size) == tuple(g["pos_size"]) and np.float32(L.rb.max_priority) == g["max_priority"]
    s = int(g["stride"])
    assert torch.allclose(rec["final_online"][::s], torch.from_numpy(g["final_online_sub"]), rtol=1e-3, atol=1e-6)
    assert torch.allclose(rec["final_target"][::s], torch.from_numpy(g["final_target_sub"]), rtol=1e-3, atol=1e-6)


@pytest.mark.parametrize("name", P.RUNS)
def test_fused_backend_on_the_twins_follows_the_minted_run_teacher_forced(name, one_thread):
    rec = P.replay_run(name, "fused")
    g = rec["golden"]
    assert P.assert_run_within_bar(rec) == 15
    # a leaf is (|loss_per_sample| + eps) ** alpha with alpha <= 1: it inherits at most the loss's own bar; the inner nodes are exact sums
    assert np.allclose(rec["tree"], g["tree"], rtol=P.RTOL, atol=P.ATOL) and R.same_bits(rec["tree"], R.rebuild(rec["tree"], 16))
    L = rec["learner"]
    assert (L.rb.pos, L.rb.size) == tuple(g["pos_size"]) and abs(L.rb.max_priority - float(g["max_priority"])) <= P.ATOL + P.RTOL * float(g["max_priority"])
    first = int(np.flatnonzero(g["trained"])[0])
    assert np.array_equal(rec["actions"][:first + 1], g["actions"][:first + 1])        # no update has run yet: the fused act is the reference's


class _Tags:
    def __init__(self):
        self.tags = set()

    def add_scalar(self, tag, value, step):
        assert np.isfinite(value), tag
        self.tags.add(tag)

    def add_text(self, *a, **k):
        pass

    def close(self):
        pass


def test_the_logging_branch_writes_the_references_tags_and_lines(monkeypatch, capsys, tmp_path):
    """Step 100 trains here, so the ``global_step % 100 == 0`` branch runs: the four tags of that branch, the episodic ones and 'SPS:'."""
    from cleanrl_amd import rainbow_atari, runner

    w = _Tags()
    monkeypatch.setattr(runner, "open_writer", lambda args, run_name: w)
    monkeypatch.setenv("MI355PPO_STANDIN_HORIZON", "10")
    monkeypatch.setenv("MI355PPO_OFFPOLICY", "torch")
    monkeypatch.chdir(tmp_path)
    rainbow_atari.main(["--no-cuda", "--total-timesteps", "101", "--learning-starts", "97", "--buffer-size", "16", "--batch-size", "4",
                        "--train-frequency", "2", "--target-network-frequency", "100", "--n-atoms", "5"])
    assert w.tags == {"losses/td_loss", "losses/q_values", "charts/SPS", "charts/beta", "charts/episodic_return", "charts/episodic_length"}
    out = capsys.readouterr().out
    assert "SPS:" in out and "global_step=9, episodic_return=" in out


@pytest.mark.parametrize("backend", ["torch", "fused"])
def test_script_runs_end_to_end_on_the_cpu(backend, tmp_path):
    env = dict(os.environ, MI355PPO_OFFPOLICY=backend, MI355PPO_STANDIN_HORIZON="10")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "cleanrl_amd", "rainbow_atari.py"), "--no-cuda", "--total-timesteps", "42",
                        "--learning-starts", "12", "--buffer-size", "16", "--batch-size", "8", "--train-frequency", "2",
                        "--target-network-frequency", "6", "--n-atoms", "5", "--save-model"], env=env, capture_output=True, text=True, timeout=600,
                       cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "episodic_return" in r.stdout and "model saved to" in r.stdout


def test_out_of_limit_sizes_raise_the_named_error_from_the_script(monkeypatch):
    from cleanrl_amd import rainbow_atari

    monkeypatch.setenv("MI355PPO_OFFPOLICY", "fused")
    with pytest.raises(ValueError, match="MI355PPO_OFFPOLICY=torch"):
        rainbow_atari.main(["--no-cuda", "--n-atoms", "102", "--buffer-size", "16", "--total-timesteps", "4"])
