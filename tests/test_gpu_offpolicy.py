"""DDPG / TD3 kernels (csrc/offpolicy.hip) on the MI355X: bit-equal to their host twins, deterministic, unchanged by capture and
replay; the golden run teacher-forced on the HIP path; both drop-ins on the GPU in a child process."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import offpolicy_cases as C
from cleanrl_amd import host_ops as H
from cleanrl_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("O,A,M,n_critics,use_noise", [(17, 6, 256, 2, True), (376, 17, 256, 2, True), (17, 6, 1, 1, False),
                                                       (376, 17, 4096, 2, True), (5, 1, 70, 2, True), (512, 20, 9, 1, False)])
def test_every_entry_point_equals_its_twin(O, A, M, n_critics, use_noise):
    c = C.make_case(O, A, M, n_critics=n_critics, low=-2.0, high=2.0)
    c.ring[4][0, 0] = 1.0
    c.noise[0, 0] = float("nan")
    want = C.run_entry_points(H, c, torch.device("cpu"), use_noise)
    got = C.run_entry_points(ops, c, DEV, use_noise)
    for k in want:
        assert C.same(got[k], want[k]), (k, (got[k] - want[k]).abs().max().item())
    again = C.run_entry_points(ops, c, DEV, use_noise)
    assert all(C.same(again[k], got[k]) for k in got)


def test_ring_add_on_the_device_follows_the_twin():
    N, O, A, slots = 3, 17, 6, 5
    rings = [tuple(torch.zeros(s, device=d) for s in ((slots, N, O), (slots, N, O), (slots, N, A), (slots, N), (slots, N)))
             for d in ("cpu", DEV)]
    g = torch.Generator().manual_seed(0)
    for step in range(12):
        data = [torch.randn((N, O), generator=g), torch.randn((N, O), generator=g), torch.randn((N, A), generator=g),
                torch.randn(N, generator=g), (torch.rand(N, generator=g) < 0.5).float()]
        H.replay_add(rings[0], step % slots, *data)
        ops.replay_add(rings[1], step % slots, *[t.to(DEV) for t in data])
    assert all(torch.equal(a, b.cpu()) for a, b in zip(*rings))


def test_adam_equals_twin_and_torch():
    g = torch.Generator().manual_seed(3)
    n = 200003
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * 0.1 for _ in range(C.ADAM_STEPS)]
    want = C.adam_reference(p0, grads)
    hp, hm, hv = p0.clone(), torch.zeros(n), torch.zeros(n)
    dp, dm, dv = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    for i, gr in enumerate(grads):
        H.clip_adam_(hp, gr.clone(), hm, hv, i + 1, 3e-4, math.inf, 1.0, eps=1e-8)
        ops.clip_adam_(dp, gr.to(DEV), dm, dv, i + 1, 3e-4, math.inf, 1.0, eps=1e-8)
    assert torch.equal(dp.cpu(), hp)
    torch.testing.assert_close(dp.cpu(), want, rtol=1e-5, atol=1e-7)


def _learner(dev, backend="fused", O=17, A=6, M=64, seed=0):
    from types import SimpleNamespace

    from cleanrl_amd.learner_offpolicy import OffPolicyLearner

    c = C.make_case(O, A, M, N=1, slots=50, seed=seed)
    env = C.fake_env(O, A)
    args = SimpleNamespace(buffer_size=50, batch_size=M, learning_rate=3e-4, gamma=0.99, tau=0.005, policy_noise=0.2, noise_clip=0.5,
                           exploration_noise=0.1, learning_starts=0)
    nets = c.nets
    for m in [nets.actor, nets.target_actor] + nets.qfs + nets.qf_targets:
        m.to(dev)
    L = OffPolicyLearner(nets.actor, nets.qfs, nets.target_actor, nets.qf_targets, args, env, dev, td3=True, backend=backend)
    for t, src in zip(L.ring, c.ring):
        t.copy_(src)
    L.full = True
    return L, c


STATE = ("online", "target", "exp_avg", "exp_avg_sq", "grads")


def test_captured_update_step_replays_with_new_indices_and_noise():
    """The whole step -- target, critic (2), Adam, actor (2), Adam, Polyak -- is captured once, with both Adam steps reading their
    schedule from device memory, and replayed with new indices, noise and schedule; the eager learner takes its Adam steps through
    ``clip_adam_`` with the host step count, as ``train_step`` does."""
    L, c = _learner(DEV)
    E, _ = _learner(DEV)
    g = torch.Generator().manual_seed(5)
    draws = [(torch.randint(0, 50, (64,), generator=g), torch.zeros(64, dtype=torch.int64), torch.randn((64, 6), generator=g))
             for _ in range(3)]
    bi, ei, nz = (t.to(DEV).clone() for t in draws[0])
    sched = L.adam_schedules().to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        L.update_kernels(bi, ei, nz, True, sched=sched)         # warm-up outside the capture (workspace allocation)
    torch.cuda.current_stream().wait_stream(s)
    for nm in STATE:
        getattr(L, nm).copy_(getattr(E, nm))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        L.update_kernels(bi, ei, nz, True, sched=sched)
    for nm in STATE:
        getattr(L, nm).copy_(getattr(E, nm))
    for b, e, n in draws:
        bi.copy_(b), ei.copy_(e), nz.copy_(n), sched.copy_(L.adam_schedules())
        graph.replay()
        L.q_step += 1
        L.actor_step += 1
        E.update_kernels(b.to(DEV), e.to(DEV), n.to(DEV), True)
        torch.cuda.synchronize()
        assert (L.q_step, L.actor_step) == (E.q_step, E.actor_step)
        for nm in STATE + ("_y", "_qsc", "_asc"):
            assert torch.equal(getattr(L, nm), getattr(E, nm)), nm
    assert not torch.equal(E.online, _learner(DEV)[0].online)


def test_fused_steps_on_the_device_equal_the_twins():
    """Whole training steps (12 launches each, Adam included) on the GPU and on the host twins stay bit-equal."""
    D, c = _learner(DEV, seed=2)
    Hh, _ = _learner(torch.device("cpu"), seed=2)
    g = torch.Generator().manual_seed(9)
    for step in range(6):
        idx = (torch.randint(0, 50, (64,), generator=g).numpy(), np.zeros(64, np.int64))
        nz = torch.randn((64, 6), generator=g)
        D.train_step(step % 2 == 0, indices=idx, noise=nz.to(DEV))
        Hh.train_step(step % 2 == 0, indices=idx, noise=nz)
    assert torch.equal(D.online.cpu(), Hh.online) and torch.equal(D.target.cpu(), Hh.target)
    assert D.metrics() == Hh.metrics()


def test_library_calls_of_a_device_step(monkeypatch):
    """The device path makes the same eight library calls a step as the twins (target, critic, Adam, actor, Adam, Polyak; add and
    act), each through ``ops._launch``, and no other."""
    L, c = _learner(DEV)
    seen = []
    real = ops._launch
    monkeypatch.setattr(ops, "_launch", lambda name, *a, **k: (seen.append(name), real(name, *a, **k))[1])
    idx = (np.arange(64) % 50, np.zeros(64, np.int64))
    L.store(np.zeros((1, 17), np.float32), np.zeros((1, 17), np.float32), np.zeros((1, 6), np.float32), np.zeros(1), np.zeros(1))
    L.train_step(True, indices=idx)
    L.act(np.zeros((1, 17), np.float32), 1)
    torch.cuda.synchronize()
    assert seen == ["mi355ppo_replay_add_f32", "mi355ppo_td3_target_f32", "mi355ppo_td3_critic_fwd_bwd_f32", "mi355ppo_clip_adam_f32",
                    "mi355ppo_td3_actor_fwd_bwd_f32", "mi355ppo_clip_adam_f32", "mi355ppo_polyak_f32", "mi355ppo_ddpg_act_f32"]


@pytest.mark.parametrize("case", ["td3", "td3_n2", "ddpg"])
def test_goldens_teacher_forced_on_the_hip_path(case):
    import td3_replay as R

    dev = R.replay(case, "fused", DEV)
    R.assert_within_sensitivity(case, dev)


@pytest.mark.parametrize("script", ["ddpg_continuous_action.py", "td3_continuous_action.py"])
@pytest.mark.parametrize("backend", ["fused", "torch"])
def test_scripts_run_on_the_gpu(script, backend):
    env = dict(os.environ, MI355PPO_OFFPOLICY=backend, MI355PPO_STANDIN_HORIZON="50")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "cleanrl_amd", script), "--total-timesteps", "302", "--learning-starts", "100",
                        "--buffer-size", "128", "--batch-size", "64"], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "SPS:" in r.stdout and "episodic_return" in r.stdout
