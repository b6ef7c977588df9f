"""The TrXL memory attention (csrc/trxl_attn.hip) on the MI355X: against float64 autograd of the reference's window path at the bar
set on the host twins (tests/trxl_cases.py), against the twins, deterministic, batch-invariant, a B = 32 forward under graph
capture, the index guard, a teacher-forced golden iteration with ``MI355PPO_TRXL=fused`` and a short script run."""
import os
import subprocess
import sys

import pytest
import torch

import trxl_cases as C
from cleanrl_amd import host_ops, ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ("memory", "layer", "ep", "rows", "pos", "mask", "pe", "gamma", "beta")


def _kernel_args(case):
    a = [case[k] for k in ARGS]
    a[5] = (a[5] != 0).to(torch.uint8)
    return a


@pytest.mark.parametrize("B,L,D,H", [(32, 119, 384, 4), (2048, 119, 384, 4), (1, 119, 384, 4), (257, 119, 384, 4),
                                     (5, 1, 64, 1), (5, 7, 512, 8), (33, 256, 512, 8), (9, 119, 64, 4), (3, 256, 384, 1)])
@pytest.mark.parametrize("mask", C.MASKS)
def test_device_against_float64(B, L, D, H, mask):
    for pe in ("absolute", ""):
        case = C.make_case(D, H, L, B, mask, pe, device=DEV)
        e_got, e_ref, scale = C.errors(C.fused_window_attention, case)
        assert C.within_bar(e_got, e_ref, scale), (pe, e_got, e_ref, scale)


@pytest.mark.parametrize("B,L,D,H", [(32, 119, 384, 4), (7, 256, 512, 8), (5, 7, 64, 1)])
def test_device_matches_the_twins(B, L, D, H):
    case = C.make_case(D, H, L, B, "tril", "absolute")
    cpu = _kernel_args(case)
    dev = [t.to(DEV) if isinstance(t, torch.Tensor) else t for t in cpu]
    q, du = case["q"], case["dout"]
    u_h, s_h = host_ops.trxl_attn_forward(*cpu, q)
    u_d, s_d = ops.trxl_attn_forward(*dev, q.to(DEV))
    g_h = host_ops.trxl_attn_backward(*cpu, q, u_h, s_h, du)
    g_d = ops.trxl_attn_backward(*dev, q.to(DEV), u_d, s_d, du.to(DEV))
    for h, d in zip((u_h, s_h) + tuple(g_h), (u_d, s_d) + tuple(g_d)):
        scale = max(1.0, h.abs().max().item())
        assert (h - d.cpu()).abs().max().item() <= 1e-5 * scale       # the same folds; only expf / sqrtf differ


def test_two_calls_give_equal_bits():
    case = C.make_case(384, 4, 119, 2048, "random", "absolute", device=DEV)
    a = _kernel_args(case)
    r1 = ops.trxl_attn_forward(*a, case["q"])
    r2 = ops.trxl_attn_forward(*a, case["q"])
    g1 = ops.trxl_attn_backward(*a, case["q"], *r1, case["dout"])
    g2 = ops.trxl_attn_backward(*a, case["q"], *r2, case["dout"])
    for x, y in zip(r1 + g1, r2 + g2):
        assert torch.equal(x, y)


def test_batch_invariance():
    case = C.make_case(384, 4, 119, 257, "tril", "absolute", device=DEV)
    a = _kernel_args(case)
    q, du = case["q"], case["dout"]
    u, st = ops.trxl_attn_forward(*a, q)
    dq, _, _ = ops.trxl_attn_backward(*a, q, u, st, du)
    for b in range(257):
        sl = slice(b, b + 1)
        ab = a[:2] + [a[2][sl], a[3][sl], a[4][sl], a[5][sl]] + a[6:]
        ub, sb = ops.trxl_attn_forward(*ab, q[sl])
        dqb, _, _ = ops.trxl_attn_backward(*ab, q[sl], ub, sb, du[sl])
        assert torch.equal(ub[0], u[b]) and torch.equal(sb[0], st[b]) and torch.equal(dqb[0], dq[b]), b


def test_graph_capture_replays_eager_bits():
    case = C.make_case(384, 4, 119, 32, "tril", "absolute", device=DEV)
    a = _kernel_args(case)
    q = case["q"].clone()
    u_eager, s_eager = ops.trxl_attn_forward(*a, q)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.trxl_attn_forward(*a, q, err=err)                       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        u_g, s_g = ops.trxl_attn_forward(*a, q, err=err)
    q.copy_(case["q"] * 0.5)
    g.replay()
    torch.cuda.synchronize()
    u_half, s_half = ops.trxl_attn_forward(*a, q)
    assert torch.equal(u_g, u_half) and torch.equal(s_g, s_half)
    q.copy_(case["q"])
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(u_g, u_eager) and torch.equal(s_g, s_eager) and err.item() == 0


def test_out_of_range_indices_are_clamped_and_reported():
    case = C.make_case(64, 4, 7, 3, "random", "absolute", device=DEV)
    a = _kernel_args(case)
    E, T = case["memory"].shape[:2]
    bad_rows = a[3].clone()
    bad_rows[1, 2] = T + 5
    with pytest.raises(IndexError):
        ops.trxl_attn_forward(*a[:3], bad_rows, *a[4:], case["q"])
    bad_ep = a[2].clone()
    bad_ep[0] = -3
    with pytest.raises(IndexError):
        ops.trxl_attn_forward(*a[:2], bad_ep, *a[3:], case["q"])
    ops.trxl_attn_forward(*a, case["q"])                             # and the library is still fine


def test_fused_iteration_against_the_golden():
    from test_trxl_script import check_fused_iteration

    n = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        g = C.golden_case("vec_discrete")
        recs, metrics, agent, _ = C.replay(g, device=DEV, backend="fused", force_actions=True)
    finally:
        torch.set_num_threads(n)
    check_fused_iteration(g, recs, metrics, agent)


def test_script_runs_fused_on_the_gpu(tmp_path):
    env = dict(os.environ, MI355PPO_TRXL="fused")
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "cleanrl_amd", "ppo_trxl.py"), "--num-envs", "8",
           "--num-steps", "64", "--total-timesteps", "1536", "--num-minibatches", "4", "--update-epochs", "1"]
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp_path, env=env, timeout=330)
    assert out.returncode == 0, out.stderr[-3000:]
    assert len([ln for ln in out.stdout.splitlines() if "SPS=" in ln]) == 3
