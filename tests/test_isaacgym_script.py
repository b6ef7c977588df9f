"""ppo_continuous_action_isaacgym.py without a GPU: the flag surface and the logged tags against the fixture minted from the reference
(tools/mint_isaacgym_goldens.py), a two-iteration run on the torch modules, and the agent's state dict."""
import dataclasses
import json
import math
import os
from types import SimpleNamespace

import pytest

from cleanrl_amd import envs as E, ppo_continuous_action_isaacgym as script, runner
from cleanrl_amd.agents import IsaacGymAgent, mlp256_backend

SURFACE = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "isaacgym_cli_surface.json")))


def test_args_fields_and_defaults_are_the_references():
    ours = {f.name: f.default for f in dataclasses.fields(script.Args)}
    assert list(ours) == list(SURFACE["fields"]) and ours == SURFACE["fields"]


def test_two_iterations_on_the_torch_modules_write_the_references_tags(monkeypatch, tmp_path):
    written = []
    writer = SimpleNamespace(add_scalar=lambda tag, value, step: written.append((tag, float(value))), add_text=lambda *a: None, close=lambda: None)
    monkeypatch.setattr(runner, "open_writer", lambda args, run_name: writer)
    monkeypatch.chdir(tmp_path)
    learner = script.main(["--no-cuda", "--num-envs", "8", "--num-steps", "16", "--total-timesteps", "256"])
    assert learner.mlp256 is None and learner.device_randperm
    tags = [t for t, _ in written]
    per_iteration = [t for t in tags if t not in SURFACE["episode_tags"]]
    assert per_iteration == SURFACE["iteration_tags"] * 2 and set(tags) <= set(SURFACE["iteration_tags"] + SURFACE["episode_tags"])
    assert all(math.isfinite(v) for _, v in written)


def test_agent_state_dict_is_the_references_for_ant(monkeypatch):
    envs = SimpleNamespace(single_observation_space=E.Box(-1.0, 1.0, (60,)), single_action_space=E.Box(-1.0, 1.0, (8,)))
    shapes = {k: tuple(v.shape) for k, v in IsaacGymAgent(envs).state_dict().items()}
    want = {"actor_logstd": (1, 8)}                  # a module's own parameters come before its children's
    for net, n_out in (("critic", 1), ("actor_mean", 8)):
        for i, (o, k) in zip((0, 2, 4), ((256, 60), (256, 256), (n_out, 256))):
            want[f"{net}.{i}.weight"], want[f"{net}.{i}.bias"] = (o, k), (o,)
    assert shapes == want and list(shapes) == list(want)
    monkeypatch.setenv("MI355PPO_MLP256", "hipblas")
    with pytest.raises(ValueError):
        mlp256_backend()
