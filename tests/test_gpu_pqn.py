"""PQN kernels (csrc/pqn.hip) on the MI355X: bit-equal to their host twins, the MLP at the float64 bar, deterministic,
batch-invariant, capturable; the golden iterations teacher-forced on the fused path; both drop-ins on the GPU."""
import os
import subprocess
import sys

import pytest
import torch

import pqn_cases as C
from cleanrl_amd import host_ops as H
from cleanrl_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    a, b = a.cpu(), b.cpu()
    return torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def _d(*ts):
    return [t.to(DEV) for t in ts]


@pytest.mark.parametrize("T,N,A", [(16, 1, 2), (128, 65, 6), (32, 4096, 18), (1, 3, 4)])
def test_qlambda_equals_twin(T, N, A):
    g = torch.Generator().manual_seed(N)
    r, v = torch.randn((T, N), generator=g), torch.randn((T, N), generator=g)
    d, nd = (torch.rand((T, N), generator=g) < 0.2).float(), (torch.rand((N,), generator=g) < 0.5).float()
    nq = torch.randn((N, A), generator=g)
    nq[0, 0] = float("nan")
    want = H.pqn_qlambda(r, d, v, nd, nq, 0.99, 0.65)
    assert _same(ops.pqn_qlambda(*_d(r, d, v, nd, nq), 0.99, 0.65), want)
    assert _same(want, C.reference_qlambda(r, d, v, nd, nq, 0.99, 0.65))


@pytest.mark.parametrize("N,A", [(1, 2), (65, 18), (4096, 4), (300, 1)])
def test_egreedy_equals_twin(N, A):
    g = torch.Generator().manual_seed(N + A)
    q = torch.randint(-2, 3, (N, A), generator=g).float()
    q[0, -1] = float("nan")
    rnd, u = torch.randint(0, A, (N,), generator=g), torch.rand((N,), generator=g)
    for eps in (0.0, 0.5, 1.0, float(u[0])):
        ha, hv, h64 = torch.empty(N), torch.empty(N), torch.empty(N, dtype=torch.int64)
        H.pqn_egreedy(q, rnd, u, eps, ha, hv, h64)
        da, dv, d64 = torch.empty(N, device=DEV), torch.empty(N, device=DEV), torch.empty(N, dtype=torch.int64, device=DEV)
        ops.pqn_egreedy(*_d(q, rnd, u), eps, da, dv, d64)
        assert torch.equal(da.cpu(), ha) and _same(dv, hv) and torch.equal(d64.cpu(), h64)


@pytest.mark.parametrize("M,A,B", [(1, 2, 4), (65, 18, 300), (32768, 6, 65536)])
def test_td_loss_equals_twin(M, A, B):
    g = torch.Generator().manual_seed(M)
    q = torch.randn((M, A), generator=g)
    mb = torch.randperm(B, generator=g)[:M]
    ba, br = torch.randint(0, A, (B,), generator=g).float(), torch.randn((B,), generator=g)
    hdq, hsc = H.pqn_td_loss(q, mb, ba, br)
    ddq, dsc = ops.pqn_td_loss(*_d(q, mb, ba, br))
    assert torch.equal(ddq.cpu(), hdq) and torch.equal(dsc.cpu(), hsc)


def _mlp_case(O, A, M, seed=0):
    params = C.random_mlp_params(O, A, seed=O * 7 + A + seed)
    B = M + 17
    g = torch.Generator().manual_seed(M + seed)
    b_obs = torch.randn((B, O), generator=g) * 2
    mb = torch.randperm(B, generator=g)[:M]
    return params, b_obs, mb, torch.randint(0, A, (B,), generator=g).float(), torch.randn((B,), generator=g) * 3


@pytest.mark.parametrize("O,A,M", [(4, 2, 1), (6, 3, 65), (8, 18, 512), (64, 2, 4096), (4, 2, 32768)])
def test_mlp_equals_twin(O, A, M):
    params, b_obs, mb, ba, br = _mlp_case(O, A, M)
    x = b_obs[mb].contiguous()
    assert torch.equal(ops.pqn_mlp_forward(x.to(DEV), params.to(DEV), A).cpu(), H.pqn_mlp_forward(x, params, A))
    hg, dg = torch.empty_like(params), torch.zeros(params.numel(), device=DEV)
    hs = H.pqn_mlp_td_fwd_bwd(b_obs, mb, params, ba, br, hg, A)
    ds = ops.pqn_mlp_td_fwd_bwd(*_d(b_obs, mb, params, ba, br, dg), A)
    assert torch.equal(dg.cpu(), hg) and torch.equal(ds.cpu(), hs)
    g = torch.Generator().manual_seed(1)
    rnd, u, din = torch.randint(0, A, (M,), generator=g), torch.rand((M,), generator=g), torch.rand((M,), generator=g)
    outs = []
    for mod, dev in ((H, "cpu"), (ops, DEV)):
        act, val, a64 = torch.empty(M, device=dev), torch.empty(M, device=dev), torch.empty(M, dtype=torch.int64, device=dev)
        ost, dst = torch.empty((M, O), device=dev), torch.empty(M, device=dev)
        mod.pqn_mlp_act(x.to(dev), params.to(dev), A, rnd.to(dev), u.to(dev), 0.3, act, val, a64, obs_row_out=ost, done_in=din.to(dev),
                        done_row_out=dst)
        outs.append([t.cpu() for t in (act, val, a64, ost, dst)])
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_mlp_within_the_float64_bar_at_32768_rows():
    O, A, M = 8, 4, 32768
    params, b_obs, mb, ba, br = _mlp_case(O, A, M, seed=3)
    q64, l64, m64, g64 = C.reference_mlp_td(params, O, A, b_obs, mb, ba, br, torch.float64)
    q32, l32, m32, g32 = C.reference_mlp_td(params, O, A, b_obs, mb, ba, br, torch.float32)
    grads = torch.zeros(params.numel(), device=DEV)
    sc = ops.pqn_mlp_td_fwd_bwd(*_d(b_obs, mb, params, ba, br, grads), A)
    for got, r64, r32 in ((grads, g64, g32), (sc[0:1], l64.reshape(1), l32.reshape(1)), (sc[1:2], m64.reshape(1), m32.reshape(1)),
                          (ops.pqn_mlp_forward(b_obs[mb].contiguous().to(DEV), params.to(DEV), A), q64, q32)):
        ok, err, own = C.within_bar(got, r64, r32)
        assert ok, (err, own)


def test_deterministic_and_batch_invariant():
    O, A = 6, 5
    params, b_obs, mb, ba, br = _mlp_case(O, A, 2048)
    p, x = params.to(DEV), b_obs.to(DEV)
    g1, g2 = torch.zeros(params.numel(), device=DEV), torch.zeros(params.numel(), device=DEV)
    s1 = ops.pqn_mlp_td_fwd_bwd(x, mb.to(DEV), p, ba.to(DEV), br.to(DEV), g1, A).clone()
    s2 = ops.pqn_mlp_td_fwd_bwd(x, mb.to(DEV), p, ba.to(DEV), br.to(DEV), g2, A)
    assert torch.equal(g1, g2) and torch.equal(s1, s2)
    full = ops.pqn_mlp_forward(x, p, A)
    rnd = torch.randint(0, A, (x.shape[0],), device=DEV)
    u = torch.rand(x.shape[0], device=DEV)
    a_full = torch.empty(x.shape[0], dtype=torch.int64, device=DEV)
    ops.pqn_mlp_act(x, p, A, rnd, u, 0.1, torch.empty(x.shape[0], device=DEV), torch.empty(x.shape[0], device=DEV), a_full)
    for n in (1, 63, 65, 1000):
        assert torch.equal(ops.pqn_mlp_forward(x[:n].contiguous(), p, A), full[:n])
        a = torch.empty(n, dtype=torch.int64, device=DEV)
        ops.pqn_mlp_act(x[:n].contiguous(), p, A, rnd[:n].contiguous(), u[:n].contiguous(), 0.1, torch.empty(n, device=DEV),
                        torch.empty(n, device=DEV), a)
        assert torch.equal(a, a_full[:n])


@pytest.mark.parametrize("n", [11_000, 1_700_000])
def test_clip_radam_equals_twin(n):
    torch.manual_seed(n)
    p0 = torch.randn(n) * 0.1
    hp, hm, hv = p0.clone(), torch.zeros(n), torch.zeros(n)
    dp, dm, dv = hp.to(DEV), hm.to(DEV), hv.to(DEV)
    for step in range(1, 9):
        gr = torch.randn(n) * (30.0 if step == 3 else 0.01)
        hg, dg = gr.clone(), gr.to(DEV)
        ht = H.clip_radam_(hp, hg, hm, hv, step, 1e-3, 10.0)
        dt = ops.clip_radam_(dp, dg, dm, dv, step, 1e-3, 10.0)
        assert torch.equal(dp.cpu(), hp) and torch.equal(dm.cpu(), hm) and torch.equal(dv.cpu(), hv), step
        assert torch.equal(dt.cpu(), ht) and int(torch.count_nonzero(dg)) == 0


def test_every_entry_point_replays_from_a_graph():
    O, A, N, T = 4, 2, 64, 16
    params, b_obs, mb, ba, br = _mlp_case(O, A, 256)
    p, x, mbd, bad, brd = _d(params, b_obs, mb, ba, br)
    rnd, u = torch.randint(0, A, (N,), device=DEV), torch.rand(N, device=DEV)
    obs = x[:N].contiguous()
    r, d, v = torch.randn((T, N), device=DEV), torch.zeros((T, N), device=DEV), torch.randn((T, N), device=DEV)
    nd = torch.zeros(N, device=DEV)
    act, val, a64 = torch.empty(N, device=DEV), torch.empty(N, device=DEV), torch.empty(N, dtype=torch.int64, device=DEV)
    q = torch.empty((N, A), device=DEV)
    ret = torch.empty((T, N), device=DEV)
    grads, sc = torch.zeros(params.numel(), device=DEV), torch.empty(2, device=DEV)
    dq, sc2 = torch.empty((256, A), device=DEV), torch.empty(2, device=DEV)
    qtd = torch.randn((256, A), device=DEV)
    fp, fm, fv = p.clone(), torch.zeros_like(p), torch.zeros_like(p)
    sched = torch.tensor(ops.radam_schedule(1e-3, 1), device=DEV)
    e_act, e_val = torch.empty(N, device=DEV), torch.empty(N, device=DEV)

    def body():
        ops.pqn_mlp_act(obs, p, A, rnd, u, 0.2, act, val, a64)
        ops.pqn_mlp_forward(obs, p, A, q)
        ops.pqn_egreedy(q, rnd, u, 0.2, e_act, e_val)
        ops.pqn_qlambda(r, d, v, nd, q, 0.99, 0.65, ret)
        ops.pqn_td_loss(qtd, mbd, bad, brd, dq, sc2)
        ops.pqn_mlp_td_fwd_bwd(x, mbd, p, bad, brd, grads, A, sc)
        ops.clip_radam_sched_(fp, grads, fm, fv, sched, 10.0)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body()                                      # warm-up (workspaces)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager = [t.clone() for t in (act, val, a64, q, e_act, e_val, ret, dq, sc2, grads, sc)]
    fp.copy_(p), fm.zero_(), fv.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    fp.copy_(p), fm.zero_(), fv.zero_()
    for t in (act, val, q, ret, dq, grads):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    got = [act, val, a64, q, e_act, e_val, ret, dq, sc2, grads, sc]
    assert all(torch.equal(a, b) for a, b in zip(got[:-2], eager[:-2])) and torch.equal(sc, eager[-1])
    # the optimizer's slot is read at replay: rewriting the table gives step 7's update (the rectified branch)
    hp, hm, hv = params.clone(), torch.zeros_like(params), torch.zeros_like(params)
    hg = torch.empty_like(params)                   # the minibatch gradient the graph feeds to the optimizer (the twin's bits)
    H.pqn_mlp_td_fwd_bwd(b_obs, mb, params, ba, br, hg, A)
    H.clip_radam_(hp, hg.clone(), hm, hv, 1, 1e-3, 10.0)
    assert torch.equal(fp.cpu(), hp)
    sched.copy_(torch.tensor(ops.radam_schedule(5e-4, 7), device=DEV))
    graph.replay()
    torch.cuda.synchronize()
    H.clip_radam_(hp, hg.clone(), hm, hv, 7, 5e-4, 10.0)
    assert torch.equal(fp.cpu(), hp) and torch.equal(fm.cpu(), hm)


@pytest.mark.parametrize("name", ["pqn", "atari"])
def test_golden_iterations_teacher_forced_on_the_fused_path(name):
    from test_pqn_script import ITER_BAR

    g = C.golden_case(name)
    recs, metrics, net, learner = C.replay(g, backend="fused", device="cuda", force_actions=True)
    assert learner.fused and learner.device.type == "cuda"
    for it, r in enumerate(recs):
        for k in ("actions", "rewards", "dones"):
            assert torch.equal(r[k], torch.from_numpy(g[k][it])), (it, k)
        for k in ("values", "returns"):
            ref = torch.from_numpy(g[k][it]).double()
            err = (r[k].double() - ref).abs().max().item()
            assert err <= 1e-4 * max(1.0, ref.abs().max().item()), (it, k, err)
    for it, m in enumerate(metrics):
        for k in ("td_loss", "q_values"):
            a, b = float(g["s_" + k][it]), float(m[k])
            assert abs(a - b) <= 1e-4 * max(1.0, abs(a)), (it, k, a, b)
    final = C.flat(net)
    ref = torch.from_numpy(g["final_params"]) if "final_params" in g else torch.from_numpy(g["final_params_sub"])
    got = final if "final_params" in g else final[::int(g["stride"])]
    assert (got - ref).abs().max().item() <= 1e-4, ITER_BAR


@pytest.mark.parametrize("script,extra", [("pqn.py", ["--num-envs", "4", "--total-timesteps", "1024"]),
                                          ("pqn_atari_envpool.py", ["--num-envs", "8", "--num-steps", "32", "--total-timesteps", "512"])])
def test_script_runs_on_the_gpu(script, extra, tmp_path):
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "cleanrl_amd", script)] + extra
    env = dict(os.environ)
    env.pop("MI355PPO_PQN", None)
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp_path, timeout=330, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert len([ln for ln in out.stdout.splitlines() if ln.startswith("SPS: ")]) == 2
