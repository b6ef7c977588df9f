"""SAC kernels (csrc/sac.hip) on the MI355X: bit-equal to their host twins, deterministic, unchanged by capture and replay; the golden
runs teacher-forced on the HIP path; the drop-in on the GPU in a child process."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import offpolicy_cases as C
import sac_cases as S
from cleanrl_amd import host_ops as H
from cleanrl_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("O,A,M", S.SHAPES + [(376, 17, 4096)])
def test_every_entry_point_equals_its_twin(O, A, M):
    c = S.make_case(O, A, M, nan_row=M // 2 if M > 4 else None)
    c.ring[4][0, 0] = 1.0
    want = S.run_entry_points(H, c, CPU)
    got = S.run_entry_points(ops, c, DEV)
    for k in want:
        assert C.same(got[k], want[k]), (k, (got[k] - want[k]).abs().max().item())
    again = S.run_entry_points(ops, c, DEV)
    assert all(C.same(again[k], got[k]) for k in got)


def _learner(dev, O=17, A=6, M=64, seed=0, **over):
    from cleanrl_amd.learner_sac import SACLearner

    c = S.make_case(O, A, M, N=1, slots=50, seed=seed, saturate=False)
    env = C.fake_env(O, A, S.LOW, S.HIGH)
    args = SimpleNamespace(**dict(dict(buffer_size=50, batch_size=M, q_lr=1e-3, policy_lr=3e-4, gamma=0.99, tau=0.005, learning_starts=0,
                                       policy_frequency=2, target_network_frequency=1, alpha=0.2, autotune=True), **over))
    nets = [c.nets.actor] + c.nets.qfs + c.nets.qf_targets
    for m in nets:
        m.to(dev)
    L = SACLearner(*nets, args, env, dev, backend="fused")
    for t, src in zip(L.ring, c.ring):
        t.copy_(src)
    L.full = True
    return L, c


STATE = ("online", "target", "exp_avg", "exp_avg_sq", "grads", "alpha_state")


def _draws(g, n, M=64, A=6):
    return torch.randint(0, 50, (M,), generator=g), torch.zeros(M, dtype=torch.int64), [torch.randn((M, A), generator=g) for _ in range(n)]


def test_captured_policy_step_replays_with_new_indices_noises_and_schedules():
    """The whole policy step -- target, critic (2), Adam, [actor (2), Adam, policy, alpha] x 2, Polyak -- is captured once, every Adam
    step (the scalar one too) reading its schedule from device memory, and replayed three times with new indices, noises and
    schedules; the eager learner takes its Adam steps with the host step counts, as ``train_step`` does."""
    L, _ = _learner(DEV)
    E, _ = _learner(DEV)
    g = torch.Generator().manual_seed(5)
    draws = [_draws(g, 5) for _ in range(3)]
    bi, ei = (t.to(DEV).clone() for t in draws[0][:2])
    nz = [t.to(DEV).clone() for t in draws[0][2]]
    sched = L.adam_schedules().to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        L.update_kernels(bi, ei, nz, True, True, sched=sched)    # warm-up outside the capture (workspace allocation)
    torch.cuda.current_stream().wait_stream(s)
    for nm in STATE:
        getattr(L, nm).copy_(getattr(E, nm))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L.update_kernels(bi, ei, nz, True, True, sched=sched)
    for nm in STATE:
        getattr(L, nm).copy_(getattr(E, nm))
    for b, e, n in draws:
        bi.copy_(b), ei.copy_(e), sched.copy_(L.adam_schedules())
        for dst, src in zip(nz, n):
            dst.copy_(src)
        graph.replay()
        L.q_step, L.actor_step, L.alpha_step = L.q_step + 1, L.actor_step + 2, L.alpha_step + 2
        E.update_kernels(b.to(DEV), e.to(DEV), [t.to(DEV) for t in n], True, True)
        torch.cuda.synchronize()
        assert (L.q_step, L.actor_step, L.alpha_step) == (E.q_step, E.actor_step, E.alpha_step)
        for nm in STATE + ("_y", "_qsc", "_asc", "_lp"):
            assert torch.equal(getattr(L, nm), getattr(E, nm)), nm
    assert not torch.equal(E.online, _learner(DEV)[0].online) and E.alpha_state[3] != 1


def test_fused_steps_on_the_device_equal_the_twins():
    """Six whole training steps (Adam and the alpha step included) on the GPU and on the host twins stay bit-equal."""
    D, _ = _learner(DEV, seed=2)
    Hh, _ = _learner(CPU, seed=2)
    g = torch.Generator().manual_seed(9)
    for step in range(6):
        pu = step % 2 == 0
        b, e, n = _draws(g, D.noise_count(pu))
        D.train_step(pu, True, indices=(b.numpy(), e.numpy()), noise=[t.to(DEV) for t in n])
        Hh.train_step(pu, True, indices=(b.numpy(), e.numpy()), noise=n)
    assert torch.equal(D.online.cpu(), Hh.online) and torch.equal(D.target.cpu(), Hh.target)
    assert torch.equal(D.alpha_state.cpu(), Hh.alpha_state) and D.log_alpha_value() == Hh.log_alpha_value() != 0.0
    assert D.metrics() == Hh.metrics()


def test_library_calls_of_a_device_step(monkeypatch):
    """A counting ``ops._launch`` sees exactly the 8 launches of a critic-only step and the 20 of a step with the policy update, by
    name and in order: the names the twin path calls (tests/test_sac_script.py)."""
    import test_sac_script as T

    L, _ = _learner(DEV)
    seen = []
    real = ops._launch
    monkeypatch.setattr(ops, "_launch", lambda name, *a, **k: (seen.append(name), real(name, *a, **k))[1])
    idx = (np.arange(64) % 50, np.zeros(64, np.int64))
    zero = lambda *s: np.zeros(s, np.float32)  # noqa: E731
    for pu, want in ((False, T.CRITIC_STEP), (True, T.POLICY_STEP)):
        del seen[:]
        L.store(zero(1, 17), zero(1, 17), zero(1, 6), zero(1), zero(1))
        L.train_step(pu, True, indices=idx)
        L.act(zero(1, 17), 1)
        torch.cuda.synchronize()
        assert seen == want
        assert sum(T.LAUNCHES[n] for n in seen) == (20 if pu else 8)


@pytest.mark.parametrize("case", ["sac", "sac_n2", "sac_fixed", "sac_tnf2"])
def test_goldens_teacher_forced_on_the_hip_path(case):
    import sac_replay as R

    R.assert_within_sensitivity(case, R.replay(case, "fused", DEV))


@pytest.mark.parametrize("backend", ["fused", "torch"])
def test_script_runs_on_the_gpu(backend):
    env = dict(os.environ, MI355PPO_OFFPOLICY=backend, MI355PPO_STANDIN_HORIZON="50")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "cleanrl_amd", "sac_continuous_action.py"), "--total-timesteps", "302",
                        "--learning-starts", "100", "--buffer-size", "128", "--batch-size", "64"], env=env, capture_output=True, text=True,
                       timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "SPS:" in r.stdout and "episodic_return" in r.stdout
