"""The LayerNorm NatureCNN of pqn_atari_envpool.py on the device: the LayerNorm + ReLU kernels against their host twins (bits), the
pre-activation forwards against the ReLU forwards (bits), the whole network against float64, PQNLearner with MI355PPO_PQN_TRUNK=fused on
the golden iterations, a captured forward + backward chain, and the script."""
import os
import subprocess
import sys
import types

import pytest
import torch
import torch.nn.functional as F

import guard_arena as GA
import pqn_cases as C
import pqn_trunk_cases as PC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")


@pytest.mark.parametrize("rows,C_,HW", PC.BWD_SHAPES)
def test_device_layernorm_returns_the_twins_bits(rows, C_, HW):
    from cleanrl_amd import cnn, host_ops, ops

    act_mask = (rows, C_, HW) == (257, 512, 1)
    z, gamma, beta, dy = PC.inputs(rows, C_, HW, seed=4)
    D = C_ * HW
    hb, hr = torch.zeros(rows * D // 32, dtype=torch.int32), torch.zeros(PC.AMAX_WORDS, dtype=torch.int32)
    ha, hm, hs = host_ops.layernorm_relu_fwd(z, gamma, beta, C_, HW, PC.EPS, bits=hb, amax=hr)
    if not act_mask:
        dy = dy * (ha > 0)
    hr2 = torch.zeros(PC.AMAX_WORDS, dtype=torch.int32)
    hdz, hdg, hdb = host_ops.layernorm_relu_bwd(dy, z, hm, hs, gamma, C_, HW, act=ha if act_mask else None, amax=hr2)
    zd, gd, bd, dd = (t.to(DEV) for t in (z, gamma, beta, dy))
    runs = []
    for _ in range(2):
        rec = cnn.new_amax(2, DEV)
        bits = torch.full((rows * D // 32,), -1, dtype=torch.int32, device=DEV)
        a, m, s = ops.layernorm_relu_fwd(zd, gd, bd, C_, HW, PC.EPS, bits=bits, amax=rec[0])
        dz, dg, db = ops.layernorm_relu_bwd(dd, zd, m, s, gd, C_, HW, act=a if act_mask else None, amax=rec[1])
        runs.append([t.cpu() for t in (a, m, s, bits, dz, dg, db)] + [cnn.amax_value(rec[0]), cnn.amax_value(rec[1])])
    for name, got, again, ref in zip(("a", "mean", "rstd", "bits", "dz", "dgamma", "dbeta"), runs[0], runs[1], (ha, hm, hs, hb, hdz, hdg, hdb)):
        assert torch.equal(got, ref), (name, (got.double() - ref.double()).abs().max().item())
        assert torch.equal(got, again), name
    assert runs[0][7] == runs[1][7] == PC.amax_value(hr) == ha.max().item()
    assert runs[0][8] == runs[1][8] == PC.amax_value(hr2) == hdz.abs().max().item()


@pytest.mark.parametrize("rows,C_,HW,act_mask", [(1, 512, 1, True), (3, 64, 49, False), (5, 32, 400, False), (70, 64, 81, False), (257, 512, 1, True)])
def test_device_layernorm_stays_inside_its_tensors(rows, C_, HW, act_mask, monkeypatch):
    from cleanrl_amd import ops

    got = [PC.run_guarded_layernorm(ops, DEV, s, rows, C_, HW, act_mask, monkeypatch) for s in GA.SENTINELS]
    for x, y in zip(got[0][:7], got[1][:7]):
        assert GA.same_bits(x, y)
    assert got[0][7:] == got[1][7:]


def _weights(seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=g)      # noqa: E731
    return {"W1": 0.05 * r(32, 4, 8, 8), "b1": 0.5 * r(32), "W2": 0.05 * r(64, 32, 4, 4), "b2": 0.5 * r(64), "W3": 0.05 * r(64, 64, 3, 3),
            "b3": 0.5 * r(64), "Wf": 0.02 * r(512, 3136), "bf": 0.5 * r(512)}, g


@pytest.mark.parametrize("rows", [3, 70, 256])
def test_relu_of_every_pre_activation_forward_is_the_relu_forward(rows):
    from cleanrl_amd import cnn, ln_cnn, ops

    w, g = _weights(rows)
    w = {k: v.to(DEV) for k, v in w.items()}
    frames = torch.randint(0, 256, (rows + 3, 84, 84, 4), generator=g, dtype=torch.uint8).to(DEV)
    inds = torch.randperm(rows + 3, generator=g)[:rows].to(DEV)
    rec = cnn.new_amax(4, DEV)
    # layer 1: kernel Q
    bt1 = cnn.repack_weights(w["W1"], 1, cnn.MODE_FWD_Q)
    a1 = cnn.conv1q_fwd_amax(frames, bt1, w["b1"], inds, torch.empty((rows, 20, 20, 32), device=DEV), None, rec[0])
    z1 = ops.conv1q_pre_fwd(frames, bt1, w["b1"], inds)
    assert (z1 < 0).any() and torch.equal(torch.relu(z1), a1)
    # layers 2 / 3: kernel Z's Z_BIAS against the default route (kernel R / RS: kernel Z's bits)
    p2, p3 = cnn.conv_zpack_f16x2(w["W2"], 2, cnn.MODE_FWD), cnn.conv_zpack_f16x2(w["W3"], 3, cnn.MODE_FWD)
    a2 = cnn.conv_fwd_packed(a1, p2, w["b2"], 2, amax=(rec[0], rec[1]))
    z2 = ln_cnn.conv_pre_packed(a1, p2, w["b2"], 2, rec[0])
    assert (z2 < 0).any() and torch.equal(torch.relu(z2), a2)
    a3 = cnn.conv_fwd_packed(a2, p3, w["b3"], 3, amax=(rec[1], rec[2]))
    z3 = ln_cnn.conv_pre_packed(a2, p3, w["b3"], 3, rec[1])
    assert (z3 < 0).any() and torch.equal(torch.relu(z3), a3)
    # FC: the K split of the ReLU forward, folded without the ReLU
    pf = cnn.fc_pack_f16x2(w["Wf"])
    h = cnn.fc_fwd_relu_packed(a3.view(rows, 3136), pf, w["bf"], 512, amax=(rec[2], None))
    zf = ln_cnn.fc_pre_packed(a3.view(rows, 3136), pf, w["bf"], 512, rec[2])
    assert (zf < 0).any() and torch.equal(torch.relu(zf), h)


def _network(seed, n_actions=6):
    from cleanrl_amd import envs as E
    from cleanrl_amd.agents import AtariQNetwork

    torch.manual_seed(seed)
    env = types.SimpleNamespace(single_action_space=E.Discrete(n_actions))
    net = AtariQNetwork(env)
    with torch.no_grad():                       # non-trivial LayerNorm affines
        for i in (1, 4, 7, 11):
            net.network[i].weight.add_(0.2 * torch.randn_like(net.network[i].weight))
            net.network[i].bias.add_(0.2 * torch.randn_like(net.network[i].bias))
    return net


def _td_grads(net, x, actions, returns):
    for p in net.parameters():
        p.grad = None
    q = net(x)
    F.mse_loss(returns.to(q.dtype), q.gather(1, actions.unsqueeze(-1)).squeeze(-1)).backward()
    return q.detach(), [p.grad.detach().clone() for p in net.parameters()]


def test_whole_network_at_70_rows_is_within_the_bar_of_float64():
    import copy

    from cleanrl_amd import ln_cnn

    rows, A = 70, 6
    net = _network(11, A)
    g = torch.Generator().manual_seed(12)
    frames = torch.randint(0, 256, (rows + 10, 84, 84, 4), generator=g, dtype=torch.uint8)
    inds = torch.randperm(rows + 10, generator=g)[:rows]
    actions, returns = torch.randint(0, A, (rows,), generator=g), torch.randn(rows, generator=g)
    x = frames[inds].permute(0, 3, 1, 2).contiguous()
    q64, g64 = _td_grads(copy.deepcopy(net).double(), x.double(), actions, returns.double())
    net32 = copy.deepcopy(net).to(DEV)
    q32, g32 = _td_grads(net32, x.float().to(DEV), actions.to(DEV), returns.to(DEV))
    fused = copy.deepcopy(net).to(DEV)
    trunk = ln_cnn.LnNatureTrunk()
    for p in fused.parameters():
        p.grad = None
    q = fused.network[13](trunk(frames.to(DEV), inds.to(DEV), fused.network))
    F.mse_loss(returns.to(DEV), q.gather(1, actions.to(DEV).unsqueeze(-1)).squeeze(-1)).backward()
    names = ["q"] + [n for n, _ in fused.named_parameters()]
    assert len(names) == 19
    failures = []
    for name, got, r64, r32 in zip(names, [q] + [p.grad for p in fused.parameters()], [q64] + g64, [q32] + g32):
        try:
            PC.bar(name, got, r64, r32)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


def test_golden_iterations_teacher_forced_on_the_fused_trunk(monkeypatch):
    from test_pqn_script import ITER_BAR

    monkeypatch.setenv("MI355PPO_PQN_TRUNK", "fused")
    g = C.golden_case("atari")
    recs, metrics, net, learner = C.replay(g, backend="fused", device="cuda", force_actions=True)
    assert learner.fused and learner.fused_trunk and learner.device.type == "cuda"
    assert learner.obs.dtype == torch.uint8 and tuple(learner.obs.shape[2:]) == (84, 84, 4)
    for it, r in enumerate(recs):
        for k in ("actions", "rewards", "dones"):
            assert torch.equal(r[k], torch.from_numpy(g[k][it])), (it, k)
        for k in ("values", "returns"):
            ref = torch.from_numpy(g[k][it]).double()
            err = (r[k].double() - ref).abs().max().item()
            print(f"iteration {it} {k}: error {err:.3e}, max |ref| {ref.abs().max().item():.3e}")
            assert err <= 1e-4 * max(1.0, ref.abs().max().item()), (it, k, err)
    for it, m in enumerate(metrics):
        for k in ("td_loss", "q_values"):
            a, b = float(g["s_" + k][it]), float(m[k])
            print(f"iteration {it} {k}: golden {a:.7g}, got {b:.7g}")
            assert abs(a - b) <= 1e-4 * max(1.0, abs(a)), (it, k, a, b)
    final = C.flat(net)
    ref = torch.from_numpy(g["final_params"]) if "final_params" in g else torch.from_numpy(g["final_params_sub"])
    got = final if "final_params" in g else final[::int(g["stride"])]
    print(f"final parameters: error {(got - ref).abs().max().item():.3e}")
    assert (got - ref).abs().max().item() <= 1e-4, ITER_BAR


def test_a_captured_forward_and_backward_chain_replays_the_eager_bits():
    from cleanrl_amd import ln_cnn

    rows = 70
    net = _network(21).to(DEV)
    g = torch.Generator().manual_seed(22)
    frames = torch.randint(0, 256, (rows + 4, 84, 84, 4), generator=g, dtype=torch.uint8).to(DEV)
    inds = torch.randperm(rows + 4, generator=g)[:rows].to(DEV)
    dh = torch.randn((rows, 512), generator=g).to(DEV)
    trunk = ln_cnn.LnNatureTrunk(net.network)
    params = []
    for i in trunk.LAYERS:
        params += [net.network[i].weight.detach(), net.network[i].bias.detach()]

    def chain():                                 # the node's forward and backward called directly: one linear sequence of launches
        ctx = types.SimpleNamespace()
        h = ln_cnn.LnNatureFn.forward(ctx, frames, inds, trunk, True, *params)
        return [h] + [t for t in ln_cnn.LnNatureFn.backward(ctx, dh) if t is not None]

    eager = [t.clone() for t in chain()]
    again = [t.clone() for t in chain()]
    assert len(eager) == 17 and all(torch.equal(a, b) for a, b in zip(eager, again))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = chain()
    for _ in range(2):
        for t in outs:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(eager, outs)):
            assert torch.equal(a, b), i


def test_the_node_refuses_the_bf16_split(monkeypatch):
    from cleanrl_amd import ln_cnn

    net = _network(31).to(DEV)
    trunk = ln_cnn.LnNatureTrunk()
    trunk.bufs.split = "bf16x3"
    frames = torch.zeros((2, 84, 84, 4), dtype=torch.uint8, device=DEV)
    with pytest.raises(NotImplementedError, match="MI355PPO_SPLIT"):
        trunk(frames, None, net.network)


def test_script_runs_on_the_gpu_with_the_fused_trunk(tmp_path):
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "cleanrl_amd", "pqn_atari_envpool.py"), "--num-envs", "8",
           "--num-steps", "32", "--total-timesteps", "512"]
    env = dict(os.environ)
    env.pop("MI355PPO_PQN", None)
    env["MI355PPO_PQN_TRUNK"] = "fused"
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp_path, timeout=330, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert len([ln for ln in out.stdout.splitlines() if ln.startswith("SPS: ")]) == 2
