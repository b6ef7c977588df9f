"""The recurrent PQN tail (csrc/pqn_lstm.hip) on the MI355X: the TD kernel bit-equal to its twin, the act kernel's state bit-equal
to the device scan at T = 1 and its e-greedy equal to the reference's on its own q, device against twin at the bar rule,
deterministic, batch-invariant, capturable; the golden iterations teacher-forced on the fused path; the drop-in on the GPU."""
import os
import subprocess
import sys

import pytest
import torch

import lstm_cases as L
import pqn_lstm_cases as C
from cleanrl_amd import host_ops as H
from cleanrl_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD_CASES = [(1, None), (256, None), (256, (32, 16, [3, 0, 9, 5, 1, 15, 2, 8])), (4096 + 3, None)]


@pytest.mark.parametrize("M,envwise", TD_CASES)
def test_td_kernel_equals_twin(M, envwise):
    c = C.make_td_case(M, 6, seed=2, envwise=envwise, actions=(0, 2, 3))
    dev, host = C.run_td(ops, c, DEV), C.run_td(H, c)
    for k in ("dh", "dwq", "dbq", "scalars"):
        assert torch.equal(dev[k], host[k]), k
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(M))
    assert torch.equal(C.run_td(ops, c, DEV, perm=perm)["dh"], dev["dh"][perm])
    c18 = C.make_td_case(M, 18, seed=3, envwise=envwise)
    dev, host = C.run_td(ops, c18, DEV), C.run_td(H, c18)
    assert all(torch.equal(dev[k], host[k]) for k in ("dh", "dwq", "dbq", "scalars"))


@pytest.mark.parametrize("A", C.ACT_A)
@pytest.mark.parametrize("N", C.ACT_N + (257, 600))
@pytest.mark.parametrize("pattern", ("random20", "nonbinary", "all"))
def test_act_kernel(pattern, N, A):
    c = C.make_act_case(N, A, pattern, seed=1)
    out = C.run_act(ops, c, DEV)
    # the state: the device scan's bits at T = 1
    _, hT, cT, _ = ops.lstm_seq_forward(c["gx"][None].contiguous().to(DEV), c["w_hh"].to(DEV), c["h0"].to(DEV), c["c0"].to(DEV),
                                        c["done"].to(DEV))
    assert torch.equal(out["h"], hT.cpu()) and torch.equal(out["c"], cT.cpu())
    # e-greedy on the kernel's own q, also with NaN / inf planted through the bias
    C.check_egreedy(out, c, 0.3)
    planted = C.run_act(ops, c, DEV, bq=C.planted_bias(c))
    assert planted["q"].isnan().any()
    C.check_egreedy(planted, c, 0.3)
    # device against twin and against float64, at the bar of the f32 reference (the twin's expf / tanhf are libm's)
    host = C.run_act(H, c)
    r64, r32 = C.reference_act(c, torch.float64), C.reference_act(c, torch.float32)
    for name, a64, a32 in zip(("h", "c", "q"), r64, r32):
        own = L.max_err(a32, a64)
        L.assert_bar(name + " vs float64", L.max_err(out[name], a64), own, L.FWD_FLOOR)
        L.assert_bar(name + " vs twin", L.max_err(out[name], host[name].double()), own, L.FWD_FLOOR)
    # bootstrap form and aliased state
    boot = C.run_act(ops, c, DEV, bootstrap=True)
    assert torch.equal(boot["q"], out["q"]) and torch.equal(boot["h_in"], c["h0"]) and torch.equal(boot["c_in"], c["c0"])
    al = C.run_act(ops, c, DEV, alias=True)
    assert all(torch.equal(al[k], out[k]) for k in out)


def test_deterministic_and_batch_invariant():
    N, A = 257, 6
    c = C.make_act_case(N, A, "random20", seed=4)
    full, again = C.run_act(ops, c, DEV), C.run_act(ops, c, DEV)
    assert all(torch.equal(full[k], again[k]) for k in full)
    for n in (0, 1, 128, 255, 256):                                   # env n alone: another E, another workgroup, the same chain
        one = dict(c, N=1, gx=c["gx"][n:n + 1].contiguous(), h0=c["h0"][n:n + 1].contiguous(), c0=c["c0"][n:n + 1].contiguous(),
                   done=c["done"][:, n:n + 1].contiguous(), rnd=c["rnd"][n:n + 1].contiguous(), u=c["u"][n:n + 1].contiguous())
        alone = C.run_act(ops, one, DEV)
        assert all(torch.equal(alone[k][0], full[k][n]) for k in full), n
    t = C.make_td_case(2048, A, seed=5)
    a, b = C.run_td(ops, t, DEV), C.run_td(ops, t, DEV)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_both_entry_points_replay_from_a_graph():
    N, A, M = 64, 6, 512
    c, t = C.make_act_case(N, A, "random20", seed=6), C.make_td_case(M, A, seed=6)
    d = lambda x: x.to(DEV)  # noqa: E731
    gx, w, h0, c0, wq, bq, rnd, u = (d(c[k]) for k in ("gx", "w_hh", "h0", "c0", "wq", "bq", "rnd", "u"))
    done = d(c["done"][0].contiguous())
    h, cc = h0.clone(), c0.clone()
    q, qb = torch.empty((N, A), device=DEV), torch.empty((N, A), device=DEV)
    act, val, a64, drow = (torch.empty(N, device=DEV), torch.empty(N, device=DEV), torch.empty(N, dtype=torch.int64, device=DEV),
                           torch.empty(N, device=DEV))
    th, tmb, tba, tbr, twq, tbq = (d(t[k]) for k in ("h", "mb", "b_actions", "b_returns", "wq", "bq"))
    dh, dwq, dbq, sc = torch.empty((M, C.H), device=DEV), torch.empty((A, C.H), device=DEV), torch.empty(A, device=DEV), torch.empty(2, device=DEV)

    def body(eps):
        ops.pqn_lstm_act(gx, w, h, cc, done, wq, bq, rnd, u, eps, h_out=h, c_out=cc, q_out=q, actions_out=act, values_out=val,
                         action_i64_out=a64, done_row_out=drow)                       # the state advances in place
        ops.pqn_lstm_act(gx, w, h, cc, done, wq, bq, q_out=qb)                        # the bootstrap form on the new state
        ops.pqn_lstm_td_fwd_bwd(th, tmb, tba, tbr, twq, tbq, dwq, dbq, dh=dh, scalars=sc)

    outs = (h, cc, q, qb, act, val, a64, drow, dh, dwq, dbq, sc)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        body(0.5)                                                                     # warm-up (workspaces)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    eager = {}
    for eps in (0.0, 1.0):                                                            # epsilon is baked into a capture
        h.copy_(h0), cc.copy_(c0)
        body(eps)
        torch.cuda.synchronize()
        eager[eps] = [x.clone() for x in outs]
    assert not torch.equal(eager[0.0][6], eager[1.0][6])
    graphs = []                                                                       # kept alive: the workspace may sit in the first one's pool
    for eps in (0.0, 1.0):
        h.copy_(h0), cc.copy_(c0)
        graph = torch.cuda.CUDAGraph()
        graphs.append(graph)
        with torch.cuda.graph(graph):
            body(eps)
        h.copy_(h0), cc.copy_(c0)
        for x in (q, qb, act, val, drow, dh, dwq, dbq, sc):
            x.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outs, eager[eps])), eps


def test_golden_iterations_teacher_forced_on_the_fused_path():
    g = C.golden_case()
    recs, metrics, net, learner = C.replay(g, backend="fused", device="cuda", force_actions=True)
    assert learner.fused and learner.device.type == "cuda"
    for it, r in enumerate(recs):
        for k in ("actions", "rewards", "dones"):
            assert torch.equal(r[k], torch.from_numpy(g[k][it])), (it, k)
        for k in ("values", "returns"):
            ref = torch.from_numpy(g[k][it]).double()
            err = (r[k].double() - ref).abs().max().item()
            print(it, k, err)
            assert err <= 1e-4 * max(1.0, ref.abs().max().item()), (it, k, err)
    for it, m in enumerate(metrics):
        for k in ("td_loss", "q_values"):
            a, b = float(g["s_" + k][it]), float(m[k])
            print(it, k, abs(a - b))
            assert abs(a - b) <= 1e-4 * max(1.0, abs(a)), (it, k, a, b)
    err = (C.flat(net)[::int(g["stride"])] - torch.from_numpy(g["final_params_sub"])).abs().max().item()
    print("params", err)
    assert err <= 1e-4


def test_script_runs_on_the_gpu(tmp_path):
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "cleanrl_amd", "pqn_atari_envpool_lstm.py"), "--num-envs", "8",
           "--num-steps", "32", "--total-timesteps", "512"]
    env = dict(os.environ)
    env.pop("MI355PPO_PQN", None)
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp_path, timeout=330, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert len([ln for ln in out.stdout.splitlines() if ln.startswith("SPS: ")]) == 2
