"""The qdagger_dqn_atari_impalacnn drop-in on the CPU against the minted run of the reference's own lines
(tools/mint_qdagger_goldens.py): the ``torch`` backend bit for bit, ``fused`` (host twins) teacher-forced within the reference's own
float32-vs-float64 deviation and free-running on the reference's random streams; the script itself on both backends, its CLI
surface and its teacher loader.  No GPU."""
import dataclasses
import sys

import numpy as np
import pytest
import torch

import qdagger_replay as R
from cleanrl_amd import envs as E
from cleanrl_amd import qdagger_dqn_atari_impalacnn as S


@pytest.fixture
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)          # as when the goldens were minted
    yield
    torch.set_num_threads(n)


@pytest.fixture(scope="module")
def torch_runs():
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return {name: R.replay(name, "torch") for name in R.CASES}
    finally:
        torch.set_num_threads(n)


@pytest.mark.parametrize("name", R.CASES)
def test_torch_backend_reproduces_the_minted_run_bit_for_bit(name, torch_runs):
    rec, g = torch_runs[name], R.golden_case(name)
    # the float64 sums of a million parameters: equal up to the order of the adds
    assert rec["init_checksum"] == pytest.approx(float(g["init_checksum"]), rel=1e-12)
    assert rec["teacher_checksum"] == pytest.approx(float(g["teacher_checksum"]), rel=1e-12)
    assert np.array_equal(rec["teacher_actions"], g["teacher_actions"]) and np.array_equal(rec["actions"], g["actions"])
    for k in R.SCALARS:
        assert np.array_equal(rec["offline_" + k], g["offline_" + k]), k
        assert np.array_equal(rec[k], g[k], equal_nan=True), k
    assert np.array_equal(rec["distill_coeff"], g["distill_coeff"], equal_nan=True)
    c = g["distill_coeff"][~np.isnan(g["distill_coeff"])]
    assert c[0] == 1.0 and (c != 1.0).any()                       # both branches of the distill_coeff rule are in the run
    s = int(g["stride"])
    for k in R.FINAL:
        assert torch.equal(rec["final_" + k][::s], torch.from_numpy(g[f"final_{k}_sub"])), k
        assert rec["final_" + k].double().sum().item() == pytest.approx(float(g[f"final_{k}_checksum"]), rel=1e-12)


@pytest.mark.parametrize("name,impala", [("qdagger", "torch"), ("qdagger_t07", "fused")])
def test_fused_on_the_cpu_teacher_forced_stays_within_the_references_own_deviation(name, impala, one_thread, monkeypatch):
    """The head twins in both cases; the trunk's twin (serial on the host: most of this test's time) in the temperature-0.7 case."""
    monkeypatch.setenv("MI355PPO_IMPALA", impala)
    rec = R.replay(name, "fused")
    assert rec["learner"].q_network.impala_backend == impala
    R.assert_within_sensitivity(name, rec)
    assert np.array_equal(rec["distill_coeff"], R.golden_case(name)["distill_coeff"], equal_nan=True)


def test_free_running_fused_draws_the_goldens_indices_and_random_actions(one_thread, monkeypatch):
    monkeypatch.delenv("MI355PPO_IMPALA", raising=False)           # the draws do not depend on who runs the trunk
    name = "qdagger"
    g = R.golden_case(name)
    drawn = []
    from cleanrl_amd.learner_qdagger import QDaggerLearner
    real = QDaggerLearner.sample_indices
    monkeypatch.setattr(QDaggerLearner, "sample_indices", lambda self, M: (drawn.append(real(self, M)), drawn[-1])[1])
    rec = R.replay(name, "fused", forced=False)
    want = [(b, e) for b, e in zip(g["offline_batch_inds"], g["offline_env_inds"])]
    want += [(b, e) for b, e in zip(g["batch_inds"], g["env_inds"]) if b[0] >= 0]
    assert len(drawn) == len(want)
    for (b, e), (wb, we) in zip(drawn, want):
        assert np.array_equal(b, wb) and np.array_equal(e, we)
    m = g["teacher_random_branch"].astype(bool)
    assert np.array_equal(rec["teacher_actions"][m], g["teacher_actions"][m])
    m = g["random_branch"].astype(bool)
    assert np.array_equal(rec["actions"][m], g["actions"][m])


def test_cli_surface_equals_the_references():
    surf = R.surface()["qdagger_dqn_atari_impalacnn"]
    fields = dataclasses.fields(S.Args)
    assert [f.name for f in fields] == surf["order"]
    assert {f.name: f.default for f in fields if f.name != "exp_name"} == surf["defaults"]
    assert S.Args().exp_name == "qdagger_dqn_atari_impalacnn"


@pytest.mark.parametrize("backend", ["torch", "fused"])
def test_script_runs_without_cuda(backend, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("MI355PPO_OFFPOLICY", backend)
    monkeypatch.setenv("MI355PPO_IMPALA", backend)
    monkeypatch.setenv("MI355PPO_STANDIN_HORIZON", "4")
    monkeypatch.delenv(S.TEACHER_ENV, raising=False)
    L = S.main(["--no-cuda", "--teacher-steps", "12", "--offline-steps", "4", "--total-timesteps", "104", "--learning-starts", "8",
                "--buffer-size", "8", "--batch-size", "2", "--train-frequency", "4", "--target-network-frequency", "4",
                "--teacher-eval-episodes", "2", "--save-model"])
    out = capsys.readouterr()
    assert L.backend == backend and L.q_network.impala_backend == backend
    assert "randomly initialised teacher" in out.err
    assert "eval_episode=1" in out.out and "-offline-0.cleanrl_model" in out.out and "SPS:" in out.out
    assert out.out.count("model saved to") == 2 and "global_step=" in out.out
    saved = list(tmp_path.glob("runs/*/qdagger_dqn_atari_impalacnn.cleanrl_model"))
    assert len(saved) == 1 and list(torch.load(saved[0]).keys()) == list(L.q_network.state_dict().keys())
    m = L.metrics()
    assert set(m) == {"loss", "q_loss", "distill_loss", "q_values"} and all(np.isfinite(v) for v in m.values())


def test_teacher_model_variable_loads_a_dqn_atari_state_dict(tmp_path, monkeypatch):
    envs = E.AtariReplayVecEnv(1, seed=0, n_actions=6)
    torch.manual_seed(5)
    ref = S.TeacherModel(envs)
    path = tmp_path / "dqn_atari.cleanrl_model"
    torch.save(ref.state_dict(), path)
    monkeypatch.setenv(S.TEACHER_ENV, str(path))
    got = S.load_teacher(S.Args(), envs, torch.device("cpu"))
    assert not got.training and all(torch.equal(a, b) for a, b in zip(got.state_dict().values(), ref.state_dict().values()))


def test_a_real_env_without_a_teacher_stops_naming_the_variable(monkeypatch):
    monkeypatch.delenv(S.TEACHER_ENV, raising=False)
    monkeypatch.setattr(E, "have_gymnasium", lambda: True)
    monkeypatch.setitem(sys.modules, "huggingface_hub", None)       # not importable: the loader must never reach for the hub here
    with pytest.raises(SystemExit) as e:
        S.load_teacher(S.Args(), E.AtariReplayVecEnv(1, seed=0, n_actions=6), torch.device("cpu"))
    assert S.TEACHER_ENV in str(e.value)
    with pytest.raises(SystemExit):                                # --upload-model exits as in dqn_atari.py (checked before any work here)
        raise SystemExit("--upload-model")
