"""pqn.py / pqn_atari_envpool.py drop-ins: QNetwork / AtariQNetwork + PQNLearner against whole iterations of the reference's own
lines (tests/golden/pqn_iteration.npz, minted by tools/mint_pqn_goldens.py), the fused backend through the host twins, the CLI
surface and short runs of both scripts."""
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pqn_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("pqn", "atari")
ROLLOUT = ("actions", "values", "rewards", "dones", "returns", "next_done")


@pytest.fixture
def one_thread():
    """The goldens were minted on one CPU thread (orthogonal_'s QR and the GEMM reductions round differently with more)."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def _params_match(g, final, exact, bar=0.0):
    if "final_params" in g:
        ref = torch.from_numpy(g["final_params"])
        got = final
    else:
        ref = torch.from_numpy(g["final_params_sub"])
        got = final[::int(g["stride"])]
    if exact:
        return torch.equal(got, ref) and final.double().sum().item() == float(g["final_checksum"])
    return (got - ref).abs().max().item() <= bar


@pytest.mark.parametrize("name", CASES)
def test_seeded_construction_equals_the_reference_weights(name, one_thread):
    from cleanrl_amd import envs as E
    from cleanrl_amd.agents import AtariQNetwork, QNetwork

    g = C.golden_case(name)
    cfg = json.loads(bytes(g["config"]).decode())
    seed = cfg["args"]["seed"]
    torch.manual_seed(seed)
    if name == "pqn":
        init = C.flat(QNetwork(E.CartPoleVecEnv(4, seed=seed)))
        assert torch.equal(init, torch.from_numpy(g["init_params"]))
    else:
        init = C.flat(AtariQNetwork(E.SyntheticAtariVecEnv(4, seed=seed, api="gym")))
        assert torch.equal(init[::int(g["stride"])], torch.from_numpy(g["init_params_sub"]))
    assert init.double().sum().item() == float(g["init_checksum"])


@pytest.mark.parametrize("name", CASES)
def test_torch_backend_reproduces_the_reference_bit_for_bit(name, one_thread):
    g = C.golden_case(name)
    recs, metrics, net, learner = C.replay(g, backend="torch")
    for it, r in enumerate(recs):
        for k in ROLLOUT:
            assert torch.equal(r[k], torch.from_numpy(g[k][it])), (it, k)
    for it, m in enumerate(metrics):
        assert m["td_loss"] == float(g["s_td_loss"][it]) and m["q_values"] == float(g["s_q_values"][it]), (it, m)
    assert learner.global_step == int(g["s_global_step"][-1])
    assert _params_match(g, C.flat(net), exact=True)


def test_goldens_cover_greedy_and_random_actions_and_episode_ends():
    g = C.golden_case("pqn")
    assert g["dones"].sum() > 0 and len(np.unique(g["actions"])) == 2
    a = C.golden_case("atari")
    assert len(np.unique(a["actions"])) >= 3


# bars for whole iterations through the fused twins (observed on the host: 0 on actions / returns, ~1e-7 on scalars and parameters)
ITER_BAR = dict(scalar=1e-5, params=1e-5, values=1e-5)


def check_fused_iteration(g, recs, metrics, net, exact_returns=True):
    for it, r in enumerate(recs):
        for k in ("actions", "rewards", "dones", "next_done"):
            assert torch.equal(r[k], torch.from_numpy(g[k][it])), (it, k)
        for k in ("values", "returns"):
            ref = torch.from_numpy(g[k][it])
            err = (r[k].double() - ref.double()).abs().max().item()
            assert err <= ITER_BAR["values"] * max(1.0, ref.abs().max().item()), (it, k, err)
    for it, m in enumerate(metrics):
        for k in ("td_loss", "q_values"):
            a, b = float(g["s_" + k][it]), float(m[k])
            assert abs(a - b) <= ITER_BAR["scalar"] * max(1.0, abs(a)), (it, k, a, b)
    assert _params_match(g, C.flat(net), exact=False, bar=ITER_BAR["params"])


@pytest.mark.parametrize("name", CASES)
def test_fused_backend_on_the_twins_within_the_bar(name, one_thread):
    g = C.golden_case(name)
    recs, metrics, net, learner = C.replay(g, backend="fused")
    assert learner.fused
    check_fused_iteration(g, recs, metrics, net)


def test_backend_switch(monkeypatch):
    from cleanrl_amd.learner_pqn import pqn_backend

    monkeypatch.delenv("MI355PPO_PQN", raising=False)
    assert pqn_backend("cpu") == "torch"
    monkeypatch.setenv("MI355PPO_PQN", "fused")
    assert pqn_backend("cpu") == "fused"
    monkeypatch.setenv("MI355PPO_PQN", "triton")
    with pytest.raises(ValueError, match="MI355PPO_PQN"):
        pqn_backend("cpu")


def test_cli_surface_matches_the_reference():
    from cleanrl_amd import pqn, pqn_atari_envpool

    with open(os.path.join(ROOT, "tests", "golden", "pqn_cli_surface.json")) as fh:
        ref = json.load(fh)
    for key, mod, exp in (("pqn", pqn, "pqn"), ("atari", pqn_atari_envpool, "pqn_atari_envpool")):
        mine = {f.name: f.default for f in dataclasses.fields(mod.Args)}
        assert mine.pop("exp_name") == exp
        assert mine == ref[key], key


@pytest.mark.parametrize("script,extra", [("pqn.py", ["--num-envs", "4", "--num-steps", "16", "--total-timesteps", "128"]),
                                          ("pqn_atari_envpool.py", ["--num-envs", "4", "--num-steps", "8", "--total-timesteps", "64"])])
@pytest.mark.parametrize("backend", ["torch", "fused"])
def test_script_runs_on_the_stand_in(script, extra, backend, tmp_path):
    env = dict(os.environ, MI355PPO_PQN=backend)
    cmd = [sys.executable, os.path.join(ROOT, "cleanrl_amd", script), "--no-cuda", "--num-minibatches", "2", "--update-epochs", "1"] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp_path, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert len([ln for ln in out.stdout.splitlines() if ln.startswith("SPS: ")]) == 2
