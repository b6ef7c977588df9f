"""The sac_atari.py drop-in against whole runs of the reference's own lines (tests/golden/sac_atari_iteration.npz, minted by
tools/mint_sac_atari_goldens.py): the CLI surface and the logged tags, the ``torch`` backend bit for bit (free-running: it meets the
reference's random streams, ``Categorical.sample`` included), the ``fused`` backend through the host twins within the recorded
sensitivity, a short run of the script and the refusal of sizes the fused heads do not take."""
import dataclasses
import os
import re

import numpy as np
import pytest
import torch

import sac_atari_replay as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


def test_cli_surface_and_logged_tags_equal_the_reference():
    from cleanrl_amd import sac_atari

    want = R.surface()["sac_atari"]
    fields = dataclasses.fields(sac_atari.Args)
    assert [f.name for f in fields] == want["order"]
    assert {f.name: f.default for f in fields if f.name != "exp_name"} == want["defaults"]
    assert sac_atari.Args().exp_name == "sac_atari"
    src = open(os.path.join(ROOT, "cleanrl_amd", "sac_atari.py")).read()
    assert re.findall(r'writer\.add_scalar\("([^"]+)"', src) == want["tags"]


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
    assert (L.pos, L.full) == (40 % L.slots, True)
    assert int(g["target_update"].sum()) >= 2 and int((g["batch_inds"][:, 0] >= 0).sum()) >= 5


@pytest.mark.parametrize("name", R.CASES)
def test_fused_backend_on_the_twins_stays_within_the_sensitivity_bar(name, one_thread):
    rec = R.replay(name, "fused")
    R.assert_within_sensitivity(name, rec)
    L = rec["learner"]
    assert (L.pos, L.full) == (40 % L.slots, True)


def test_fused_free_running_draws_the_reference_streams_up_to_the_policys(one_thread, monkeypatch):
    """Not teacher-forced: ``space.sample()`` and the two ``np.random`` draws follow the reference's order, so the actions before
    ``learning_starts`` and every sampled batch index are the golden ones (``fused`` consumes no ``np.random`` elsewhere)."""
    from cleanrl_amd.learner_sac_atari import SACAtariLearner

    g = R.golden_case("sac_atari")
    idx = []
    orig = SACAtariLearner.sample_indices
    monkeypatch.setattr(SACAtariLearner, "sample_indices", lambda self, n: (idx.append(orig(self, n)), idx[-1])[1])
    rec = R.replay("sac_atari", "fused", forced=False)
    trained = g["batch_inds"][:, 0] >= 0
    assert len(idx) == int(trained.sum())
    for (bi, ei), gb, ge in zip(idx, g["batch_inds"][trained], g["env_inds"][trained]):
        assert np.array_equal(bi, gb) and np.array_equal(ei, ge)
    assert np.array_equal(rec["actions"][:8], g["actions"][:8])
    assert ((rec["actions"] >= 0) & (rec["actions"] < 6)).all()


@pytest.mark.parametrize("backend", ["torch", "fused"])
def test_main_runs_end_to_end_on_the_cpu(backend, tmp_path, monkeypatch, capsys):
    from cleanrl_amd import sac_atari

    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("MI355PPO_OFFPOLICY", backend)
    monkeypatch.setenv("MI355PPO_STANDIN_HORIZON", "10")
    L = sac_atari.main(["--no-cuda", "--total-timesteps", "202", "--learning-starts", "30", "--buffer-size", "16", "--batch-size", "4",
                        "--update-frequency", "4", "--target-network-frequency", "8"])
    out = capsys.readouterr().out
    assert "SPS:" in out and "episodic_return" in out
    assert L.backend == backend and L.q_step == L.actor_step == L.alpha_step == len(range(32, 202, 4))
    m = L.metrics()
    assert set(m) == {"qf1_values", "qf2_values", "qf1_loss", "qf2_loss", "qf_loss", "actor_loss", "alpha", "alpha_loss"}
    assert all(np.isfinite(v) for v in m.values())


def test_tau_one_target_update_is_a_copy():
    """``tau == 1``: a flat copy keeps ``-0.0`` and never reads the old target; ``1 * p + 0 * t`` would do neither."""
    g, args, envs, L, _ = R.build("sac_atari", "fused")
    with torch.no_grad():
        L.online[L.stride] = -0.0
        L.target[1] = float("inf")
    L.sync_target()
    assert torch.equal(L.target[:L.stride + L.P], L.online[L.stride:2 * L.stride + L.P])
    assert torch.signbit(L.target[0]) and torch.isfinite(L.target).all()
    assert torch.equal(R.H.flat(*L.qf_targets), R.H.flat(*L.qfs))


def test_out_of_limit_sizes_raise_the_named_error(monkeypatch):
    import sac_atari_cases as S
    from cleanrl_amd import sac_atari

    with pytest.raises(ValueError, match="MI355PPO_OFFPOLICY=torch"):
        S.make_learner(torch.device("cpu"), "fused", n=19)
    with pytest.raises(ValueError, match="MI355PPO_OFFPOLICY=torch"):
        S.make_learner(torch.device("cpu"), "fused", M=1025, slots=4)
    assert S.make_learner(torch.device("cpu"), "torch", n=19, slots=4).backend == "torch"
    monkeypatch.setenv("MI355PPO_OFFPOLICY", "fused")
    with pytest.raises(ValueError, match="MI355PPO_OFFPOLICY=torch"):
        sac_atari.main(["--no-cuda", "--batch-size", "2000", "--buffer-size", "16", "--total-timesteps", "4"])
