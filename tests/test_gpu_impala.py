"""The IMPALA-CNN trunk kernels (csrc/impala.hip) on the GPU: against float64 autograd of the reference's modules, against
their host twins, determinism, batch invariance, graph capture, the procgen / PPG goldens and script runs with
MI355PPO_IMPALA=fused."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import impala_cases as C
import test_zz_gpu_new_scripts as zz
from cleanrl_amd import agents, host_ops, ops
from cleanrl_amd import envs as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev_params(agent):
    agent.to(DEV)
    return C.trunk_params(agent)


@pytest.mark.parametrize("B", [1, 3, 64, 2048])
@pytest.mark.parametrize("init", C.INITS)
def test_kernels_against_float64(B, init):
    agent = C.make_agent(init, seed=B)
    x, dy = C.make_frames("flat", B, seed=B).to(DEV), C.upstream(B, seed=B + 7).to(DEV)
    params = _dev_params(agent)
    y, saved, arg = ops.impala_forward(x, params)
    grads = ops.impala_backward(x, params, saved, arg, dy)
    agent.cpu()
    args = C.argmax_planes(arg.cpu(), B)
    if B <= 64:
        C.check_argmax(agent, x.cpu(), args)
    C.check_against_f64(agent, x.cpu(), dy.cpu(), y.cpu(), [g.cpu() for g in grads], args)


@pytest.mark.parametrize("frames", C.FRAMES)
def test_device_equals_twin_bit_for_bit(frames):
    B = 2
    agent = C.make_agent("procgen", seed=5)
    x, dy = C.make_frames(frames, B, seed=5), C.upstream(B, seed=6)
    hy, hs, ha = host_ops.impala_forward(x, C.trunk_params(agent))
    hg = host_ops.impala_backward(x, C.trunk_params(agent), hs, ha, dy)
    params = _dev_params(agent)
    y, saved, arg = ops.impala_forward(x.to(DEV), params)
    grads = ops.impala_backward(x.to(DEV), params, saved, arg, dy.to(DEV))
    assert torch.equal(y.cpu(), hy) and torch.equal(saved.cpu(), hs) and torch.equal(arg.cpu(), ha)
    for g, h in zip(grads, hg):
        assert torch.equal(g.cpu(), h)


def test_maxpool_kernels_equal_torch():
    for B, H, Cc in ((2, 64, 16), (3, 32, 32), (5, 16, 32)):
        g = torch.Generator().manual_seed(H)
        x = torch.randint(0, 3, (B, H, H, Cc), generator=g).float()
        y, arg = ops.impala_maxpool_forward(x.to(DEV))
        hy, ha = host_ops.impala_maxpool_forward(x)
        assert torch.equal(y.cpu(), hy) and torch.equal(arg.cpu(), ha)
        dy = torch.randn((B, H // 2, H // 2, Cc), generator=g)
        assert torch.equal(ops.impala_maxpool_backward(dy.to(DEV), arg).cpu(), host_ops.impala_maxpool_backward(dy, ha))


def test_determinism_and_batch_invariance():
    B = 2048
    agent = C.make_agent("ppg", seed=11)
    params = _dev_params(agent)
    x = C.make_frames("flat", B, seed=11).to(DEV)
    dy = C.upstream(B, seed=12).to(DEV)
    y1, s1, a1 = ops.impala_forward(x, params)
    y2, s2, a2 = ops.impala_forward(x, params)
    assert torch.equal(y1, y2) and torch.equal(s1, s2) and torch.equal(a1, a2)
    g1 = ops.impala_backward(x, params, s1, a1, dy)
    g2 = ops.impala_backward(x, params, s2, a2, dy)
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    for i in (0, 1, 1023, 2047):
        yi, si, ai = ops.impala_forward(x[i:i + 1].contiguous(), params)
        assert torch.equal(yi[0], y1[i])
        for s in range(3):                                          # every saved activation plane and the argmax of image i
            for which in range(5 if s < 2 else 4):
                n = C.argmax_planes(a1, B)[s][0].numel()
                off = sum((5 if t < 2 else 4) * C.argmax_planes(a1, B)[t][0].numel() for t in range(s)) + which * n
                assert torch.equal(si[off:off + n], s1[off * B + i * n:off * B + (i + 1) * n])
            assert torch.equal(C.argmax_planes(ai, 1)[s][0], C.argmax_planes(a1, B)[s][i])


def test_graph_capture_of_the_b64_forward():
    agent = C.make_agent("procgen", seed=2)
    params = _dev_params(agent)
    x = C.make_frames("noise", 64, seed=2).to(DEV)
    with torch.no_grad():
        eager = ops.impala_trunk(x, params)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ops.impala_trunk(x, params)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = ops.impala_trunk(x, params)
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_procgen_golden_on_the_fused_path(monkeypatch):
    monkeypatch.setenv("MI355PPO_IMPALA", "fused")
    envs = SimpleNamespace(single_observation_space=E.Box(0, 255, (64, 64, 3), np.uint8), single_action_space=E.Discrete(15))
    assert agents.ProcgenAgent(envs).impala_backend == "fused"
    zz.test_procgen_and_ma_atari_hip_minibatch_steps_against_reference_lines("procgen")


def test_ppg_golden_on_the_fused_path(monkeypatch, capsys):
    monkeypatch.setenv("MI355PPO_IMPALA", "fused")
    envs = SimpleNamespace(single_observation_space=E.Box(0, 255, (64, 64, 3), np.uint8), single_action_space=E.Discrete(15))
    assert agents.PPGAgent(envs).impala_backend == "fused"
    zz.test_ppg_hip_path_teacher_forced_against_reference_phase(capsys)


@pytest.mark.parametrize("script,extra", [("ppo_procgen.py", ["--total-timesteps", "512", "--num-minibatches", "2",
                                                               "--update-epochs", "1"]),
                                          ("ppg_procgen.py", ["--total-timesteps", "1024", "--num-minibatches", "2", "--n-iteration", "2",
                                                              "--e-auxiliary", "1", "--num-aux-rollouts", "4"])])
def test_scripts_run_fused(tmp_path, script, extra):
    env = dict(os.environ, MI355PPO_IMPALA="fused")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "cleanrl_amd", script), "--num-envs", "8", "--num_steps", "32"] + extra,
                         capture_output=True, text=True, cwd=tmp_path, timeout=900, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "SPS:" in out.stdout and "nan" not in out.stdout.lower()
