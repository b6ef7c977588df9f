"""MI355PPO_IMPALA=pooled (kernel ICP and the un-pooling gradient launches of csrc/impala.hip).  The pooled path runs the fused path's
own fmaf chains, tie rule and folds, so the GPU tests hold it to the host twins with ``torch.equal``; the float64 bars are impala_cases.py's."""
import ctypes

import pytest
import torch

import impala_cases as C
import test_zz_gpu_new_scripts as zz
from cleanrl_amd import _lib, agents, host_ops, ops

DEV = torch.device("cuda:0")


def _run(agent, x, dy):
    agent.to(DEV)
    params = C.trunk_params(agent)
    y, saved, arg = ops.impala_forward(x.to(DEV), params, pooled=True)
    grads = ops.impala_backward(x.to(DEV), params, saved, arg, dy.to(DEV), pooled=True)
    agent.cpu()
    return y.cpu(), saved.cpu(), arg.cpu(), [g.cpu() for g in grads]


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 5])
@pytest.mark.parametrize("frames", C.FRAMES)
def test_pooled_kernels_equal_the_twins_bit_for_bit(frames, B):
    agent = C.make_agent("procgen", seed=B)
    x, dy = C.make_frames(frames, B, seed=B), C.upstream(B, seed=B + 3)
    hy, hs, ha = host_ops.impala_forward(x, C.trunk_params(agent))
    hg = host_ops.impala_backward(x, C.trunk_params(agent), hs, ha, dy)
    y, saved, arg, grads = _run(agent, x, dy)
    assert torch.equal(y, hy) and torch.equal(saved, hs) and torch.equal(arg, ha)
    assert [i for i, (g, h) in enumerate(zip(grads, hg)) if not torch.equal(g, h)] == []


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("init", C.INITS)
def test_pooled_kernels_against_float64(init, B):
    agent = C.make_agent(init, seed=B)
    x, dy = C.make_frames("flat", B, seed=B), C.upstream(B, seed=B + 7)
    y, _, arg, grads = _run(agent, x, dy)
    args = C.argmax_planes(arg, B)
    C.check_argmax(agent, x, args)
    C.check_against_f64(agent, x, dy, y, grads, args)


@pytest.mark.gpu
def test_pooled_autograd_and_graph_capture():
    B = 3
    agent = C.make_agent("ppg", seed=4)
    x, dy = C.make_frames("noise", B, seed=4), C.upstream(B, seed=5)
    _, _, _, direct = _run(agent, x, dy)
    agent.to(DEV)
    params, xd = C.trunk_params(agent), x.to(DEV)
    ops.impala_trunk(xd, params, pooled=True).backward(dy.to(DEV))
    assert all(torch.equal(p.grad.cpu(), g) for p, g in zip(params, direct))
    with torch.no_grad():
        eager = ops.impala_trunk(xd, params, pooled=True)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ops.impala_trunk(xd, params, pooled=True)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = ops.impala_trunk(xd, params, pooled=True)
        for _ in range(3):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager)


@pytest.mark.gpu
def test_procgen_golden_on_the_pooled_path(monkeypatch):
    monkeypatch.setenv("MI355PPO_IMPALA", "pooled")
    assert C.make_agent("procgen").impala_backend == "pooled"
    zz.test_procgen_and_ma_atari_hip_minibatch_steps_against_reference_lines("procgen")


def test_switch_twins_and_refusals(monkeypatch):
    monkeypatch.setenv("MI355PPO_IMPALA", "fused")
    fused = {init: C.make_agent(init) for init in C.INITS}
    monkeypatch.setenv("MI355PPO_IMPALA", "pooled")
    x = C.make_frames("flat", 2, seed=9)
    for init, ref in fused.items():
        a = C.make_agent(init, seed=1)
        assert a.impala_backend == "pooled" and list(a.state_dict().keys()) == list(ref.state_dict().keys())
        a.load_state_dict(ref.state_dict())
        with torch.no_grad():                                         # CPU frames: the plain pair's host twins, whatever the flag
            assert torch.equal(agents._impala_features(a, x.permute(0, 3, 1, 2)), agents._impala_features(ref, x.permute(0, 3, 1, 2)))
    with pytest.raises(NotImplementedError, match="MI355PPO_IMPALA=fused"):
        agents.AtariImpalaQNetwork(6)
    monkeypatch.setenv("MI355PPO_IMPALA", "pool")
    with pytest.raises(ValueError):
        agents.AtariImpalaQNetwork(6)

    lib, B, ch, big = _lib.load(), 1, (16, 32, 32), 1 << 40
    P = (ctypes.c_void_p * 30)(*[p.data_ptr() for p in C.trunk_params(fused["procgen"])])
    y, dy = torch.full((B, 8, 8, 32), 7.0), torch.zeros((B, 8, 8, 32))
    saved = torch.full((int(lib.mi355ppo_impala_saved_floats(B)),), 7.0)
    arg = torch.full((int(lib.mi355ppo_impala_argmax_bytes(B)),), 9, dtype=torch.uint8)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    fwd = lambda xs, a, shape, ws: lib.mi355ppo_impala_fwd_pooled_f32(xs, P, ptr(y), ptr(saved), a, B, *shape, *ch, ptr(saved), ws, None)
    bwd = lambda xs, a, shape, ws: lib.mi355ppo_impala_bwd_pooled_f32(xs, P, ptr(saved), a, ptr(dy), P, B, *shape, *ch, ptr(saved), ws, None)
    for call, short in ((fwd, 16), (bwd, lib.mi355ppo_impala_workspace_bytes(B, 0))):       # refused before any launch
        assert call(None, ptr(arg), (64, 64, 3), big) == -1 and call(ptr(x), None, (64, 64, 3), big) == -1
        assert call(ptr(x), ptr(arg), (64, 64, 3), short) == -4 and call(ptr(x), ptr(arg), (84, 84, 4), big) == -1
    assert (y == 7.0).all() and (saved == 7.0).all() and (arg == 9).all()
