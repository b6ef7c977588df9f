"""ppo_trxl.py drop-in: TrXLAgent + TrXLLearner against whole iterations of the reference's own lines
(tests/golden/trxl_iteration.npz, minted by tools/mint_trxl_goldens.py from cleanrl/ppo_trxl/ppo_trxl.py on the synthetic
memory task), the fused backend through the host twins, the CLI surface and a short run of the script."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import trxl_cases as C
from cleanrl_amd import envs as E
from cleanrl_amd.agents import TrXLAgent
from cleanrl_amd.ppo_trxl import Args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("vec_discrete", "vec_multidiscrete", "image")
ROLLOUT = ("actions", "log_probs", "values", "rewards", "dones", "stored_memory_masks", "stored_memory_indices", "stored_memory_index",
           "advantages", "returns", "next_done")


@pytest.fixture
def one_thread():
    """The goldens were minted on one CPU thread (orthogonal_'s QR and the GEMM reductions round differently with more)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _flat(agent):
    return torch.cat([p.detach().reshape(-1) for p in agent.parameters()])


@pytest.mark.parametrize("name", CASES)
def test_torch_backend_reproduces_the_reference_bit_for_bit(name, one_thread, monkeypatch):
    monkeypatch.delenv("MI355PPO_TRXL", raising=False)
    g = C.golden_case(name)
    recs, metrics, agent, learner = C.replay(g, backend="torch")
    for it, r in enumerate(recs):
        for k in ROLLOUT:
            assert torch.equal(r[k].to(torch.from_numpy(g[k][it]).dtype), torch.from_numpy(g[k][it])), (it, k)
    for it, m in enumerate(metrics):
        for gk, mk in C.SCALAR_KEYS:
            a, b = float(g["s_" + gk][it]), float(m[mk])
            assert a == b or (np.isnan(a) and np.isnan(b)), (it, gk, a, b)
    final = _flat(agent)
    assert torch.equal(final[::int(g["stride"])], torch.from_numpy(g["final_params_sub"]))
    assert final.double().sum().item() == float(g["final_checksum"])


def test_goldens_cover_episode_ends_and_the_trim():
    """The fixtures exercise what the bookkeeping must get right: episodes ending mid-rollout and at the last step, and the
    ``actual_max_episode_steps`` trim both taken and not taken."""
    gs = {n: C.golden_case(n) for n in CASES}
    assert all(g["dones"][:, 1:].sum() > 0 for g in gs.values())
    assert any(g["next_done"].sum() > 0 for g in gs.values())
    trims = [bool(a < g["memory_length"]) for g in gs.values() for a in g["s_actual_max_episode_steps"]]
    assert any(trims) and not all(trims)


def test_seeded_construction_equals_the_reference_weights(one_thread, monkeypatch):
    monkeypatch.delenv("MI355PPO_TRXL", raising=False)
    for name in CASES:
        g = C.golden_case(name)
        cfg = json.loads(bytes(g["config"]).decode())
        args = Args(**cfg["args"])
        envs = E.SyntheticMemoryVecEnv(cfg["env_id"], args.num_envs, **cfg["env"])
        args.trxl_memory_length = min(args.trxl_memory_length, int(g["max_episode_steps"]))
        shape = (envs.single_action_space.n,) if hasattr(envs.single_action_space, "n") else tuple(envs.single_action_space.nvec)
        torch.manual_seed(args.seed)
        agent = TrXLAgent(args, envs.single_observation_space, shape, int(g["max_episode_steps"]))
        init = _flat(agent)
        assert torch.equal(init[::int(g["stride"])], torch.from_numpy(g["init_params_sub"])), name
        assert init.double().sum().item() == float(g["init_checksum"]), name


# bars for a whole teacher-forced iteration through the fused attention, set on the host twins (observed: 8e-7 on values,
# 2.4e-7 on log-probs, 6e-8 on the loss scalars, 3e-8 on the parameters)
ITER_BAR = dict(rollout=1e-5, scalar=1e-5, params=1e-5)


def check_fused_iteration(g, recs, metrics, agent):
    for it, r in enumerate(recs):
        for k in ("actions", "stored_memory_index", "stored_memory_indices", "stored_memory_masks", "dones"):
            assert torch.equal(r[k].to(torch.from_numpy(g[k][it]).dtype), torch.from_numpy(g[k][it])), (it, k)
        for k in ("log_probs", "values", "advantages", "returns"):
            err = (r[k].double() - torch.from_numpy(g[k][it]).double()).abs().max().item()
            assert err <= ITER_BAR["rollout"], (it, k, err)
    for it, m in enumerate(metrics):
        for gk, mk in C.SCALAR_KEYS[:8]:
            a, b = float(g["s_" + gk][it]), float(m[mk])
            assert abs(a - b) <= ITER_BAR["scalar"] * max(1.0, abs(a)), (it, gk, a, b)
    final = _flat(agent).cpu()
    err = (final[::int(g["stride"])] - torch.from_numpy(g["final_params_sub"])).abs().max().item()
    assert err <= ITER_BAR["params"], err


@pytest.mark.parametrize("name", ["vec_discrete", "vec_multidiscrete"])
def test_fused_backend_on_the_twins_within_the_bar(name, one_thread):
    g = C.golden_case(name)
    recs, metrics, agent, _ = C.replay(g, backend="fused", force_actions=True)
    check_fused_iteration(g, recs, metrics, agent)


def test_backend_switch(monkeypatch):
    args = Args(trxl_dim=64, trxl_num_layers=1, trxl_positional_encoding="learned")
    space = E.Box(0, 1, (8,))
    monkeypatch.setenv("MI355PPO_TRXL", "fused")
    with pytest.raises(ValueError, match="learned"):
        TrXLAgent(args, space, (4,), 16)
    args.trxl_positional_encoding = "absolute"
    assert TrXLAgent(args, space, (4,), 16).trxl_backend == "fused"
    monkeypatch.setenv("MI355PPO_TRXL", "triton")
    with pytest.raises(ValueError, match="MI355PPO_TRXL"):
        TrXLAgent(args, space, (4,), 16)
    monkeypatch.delenv("MI355PPO_TRXL")
    assert TrXLAgent(args, space, (4,), 16).trxl_backend == "torch"


def test_single_sample_keeps_the_batch_dimension(monkeypatch):
    """The reference's ``x.squeeze()`` + ``unsqueeze(0)``: one sample still gives (1, ...) outputs, on both backends."""
    args = Args(trxl_dim=64, trxl_num_layers=2, trxl_memory_length=4)
    torch.manual_seed(0)
    agent = TrXLAgent(args, E.Box(0, 1, (8,)), (3, 2), 16)
    obs, win, mask, idx = torch.randn(1, 8), torch.randn(1, 4, 2, 64), torch.tensor([[1, 1, 0, 0]]), torch.arange(4).reshape(1, 4)
    outs = {}
    for backend in ("torch", "fused"):
        agent.trxl_backend = backend
        a, lp, ent, v, mem = agent.get_action_and_value(obs, win, mask, idx, torch.tensor([[1, 0]]))
        assert lp.shape == (1, 2) and ent.shape == (1,) and v.shape == (1,) and mem.shape == (1, 2, 64)
        outs[backend] = v
    assert (outs["torch"] - outs["fused"]).abs().item() < 1e-5


def test_cli_surface_matches_the_reference():
    with open(os.path.join(ROOT, "tests", "golden", "trxl_cli_surface.json")) as fh:
        ref = json.load(fh)["args"]
    mine = {f.name: f.default for f in dataclasses.fields(Args)}
    assert mine.pop("exp_name") == "ppo_trxl"
    assert mine == ref


def test_script_runs_on_the_stand_in(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "cleanrl_amd", "ppo_trxl.py"), "--no-cuda", "--num-envs", "2", "--num-steps", "16",
           "--total-timesteps", "64", "--num-minibatches", "2", "--update-epochs", "1", "--trxl-dim", "64", "--trxl-num-layers", "1",
           "--trxl-memory-length", "8", "--env-id", "MemoryVector-MultiDiscrete-v0"]
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp_path, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if "SPS=" in ln]
    assert len(lines) == 2 and lines[0].split()[0] == "1" and lines[1].split()[0] == "2"
