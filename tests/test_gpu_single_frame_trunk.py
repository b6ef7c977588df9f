"""The one-frame LayerNorm NatureCNN of pqn_atari_envpool_lstm.py on the device: kernel Q1 (conv1 forward on (R, 84, 84) uint8 frames)
against its host twin (bits), kernel P1 (conv1 weight + bias gradient) against float64, their guard bands, the whole network against
float64, LSTMPQNLearner with MI355PPO_PQN_TRUNK=fused on the golden iterations, a captured forward + backward chain, and the script."""
import copy
import os
import subprocess
import sys
import types

import pytest
import torch
import torch.nn.functional as F

import guard_arena as GA
import pqn_lstm_cases as PL
import pqn_trunk_cases as PC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")


def _case(stored, seed):
    g = torch.Generator().manual_seed(9000 + seed)
    frames = torch.randint(0, 256, (stored, 84, 84), generator=g, dtype=torch.uint8)      # exactly stored x 7,056 bytes, its own allocation
    return frames, 0.05 * torch.randn((32, 1, 8, 8), generator=g), 0.5 * torch.randn(32, generator=g), g


def _second_tile_count():
    """The smallest image count at which some wave of kernel Q1's persistent grid walks a second tile (the prefetch of the next tile and the
    loop's back edge run): the launch is 3 workgroups of 4 waves per CU (csrc/conv1q1.hip, kernel Q's grid at rollout sizes), an image is 12.5
    tiles of 32 pixels -- so more than 12 * CUs tiles.  On a 256-CU part: 3,072 wave slots, 246 images = 3,075 tiles; the case runs 256 images
    (3,200 tiles, kernel Q's own case) or the derived count where that is larger."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return max(256, 12 * cus * 32 // 400 + 1)


@pytest.mark.parametrize("images,inds", [(1, None), (3, [3, 0, 3]), (70, None), ("second tile", None)])
def test_forward_equals_the_twin_bit_for_bit(images, inds):
    from cleanrl_amd import host_ops, ops

    if images == "second tile":
        images = _second_tile_count()
    stored = images if inds is None else 4
    frames, W, b, _ = _case(stored, seed=images)
    ii = None if inds is None else torch.tensor(inds, dtype=torch.int64)
    ref = host_ops.conv1q1_pre_fwd(frames, host_ops.conv1q1_pack(W), b, ii)
    fd, Wd, bd, iid = frames.to(DEV), W.to(DEV), b.to(DEV), None if ii is None else ii.to(DEV)
    pack = ops.conv1q1_pack(Wd)
    assert torch.equal(pack.view(torch.int32).cpu(), host_ops.conv1q1_pack(W).view(torch.int32))
    runs = [ops.conv1q1_pre_fwd(fd, pack, bd, iid).cpu() for _ in range(2)]
    assert runs[0].shape == (images, 20, 20, 32) and (runs[0] < 0).any()
    assert torch.equal(runs[0], ref), (runs[0].double() - ref.double()).abs().max().item()
    assert torch.equal(runs[0], runs[1])
    if inds is not None:
        assert torch.equal(runs[0][0], runs[0][2])


# Kernel P1's partition (csrc/conv1p1.hip, csrc/conv.hip): min(images, 512) workgroups, one partial per wave = 4 per workgroup; stage 1 of
# the fold adds chunks of 32 partials, stage 2 the chunk sums.  1 image: 4 partials, one chunk.  9 images: 36 partials -- the smallest count
# at which stage 2 adds more than one chunk sum (both stages in one launch up to 8 chunks).  70 images: 280 partials = 9 chunks, the
# two-launch fold.  513 images: the smallest count at which a workgroup walks a second image (both LDS stages, the loop's back edge).
WGRAD_CASES = [(1, None), (3, [3, 0, 3]), (9, None), (70, None), (513, None)]


def _wgrad_case(images, inds, scale=1.0):
    from cleanrl_amd import cnn

    stored = images if inds is None else 4
    frames, _, _, g = _case(stored, seed=100 + images)
    dz = (torch.randn((images, 20, 20, 32), generator=g) * scale).to(DEV)
    rec = cnn.absmax(dz, cnn.new_amax(1, DEV)[0])            # the record as a producer's epilogue fills it: atomic max of the bit patterns over the slots
    ii = None if inds is None else torch.tensor(inds, dtype=torch.int64, device=DEV)
    return frames.to(DEV), dz, rec, ii


def _wgrad_reference(frames, dz, ii, dtype):
    x = (frames if ii is None else frames[ii]).unsqueeze(1).to(dtype) / 255.0
    W = torch.zeros((32, 1, 8, 8), dtype=dtype, device=DEV, requires_grad=True)
    b = torch.zeros(32, dtype=dtype, device=DEV, requires_grad=True)
    return torch.autograd.grad(F.conv2d(x, W, b, stride=4), (W, b), dz.permute(0, 3, 1, 2).to(dtype))


@pytest.mark.parametrize("images,inds,scale", [(m, i, 1.0) for m, i in WGRAD_CASES] + [(70, None, 1e-15), (70, None, 1e10)])
def test_weight_and_bias_gradient_are_within_the_bar_of_float64(images, inds, scale):
    from cleanrl_amd import ops

    frames, dz, rec, ii = _wgrad_case(images, inds, scale)
    runs = [ops.conv1p1_wgrad(frames, dz, rec, ii) for _ in range(2)]
    (W64, b64), (W32, b32) = _wgrad_reference(frames, dz, ii, torch.float64), _wgrad_reference(frames, dz, ii, torch.float32)
    failures = []
    for name, got, r64, r32 in (("dW1", runs[0][0], W64, W32), ("db1", runs[0][1], b64, b32)):
        try:
            PC.bar(f"{name} ({images} images, scale {scale:g})", got, r64, r32)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)
    assert runs[0][0].shape == (32, 1, 8, 8) and runs[0][1].shape == (32,)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("images,inds", [(3, [3, 0, 3]), (70, None)])
def test_device_kernels_stay_inside_their_tensors(images, inds, monkeypatch):
    from cleanrl_amd import _lib, cnn, ops

    got = []
    for sentinel in GA.SENTINELS:
        arena = GA.Arena(DEV, sentinel, words=1 << 23)
        stored = images if inds is None else 4
        frames_, W_, b_, g = _case(stored, seed=200 + images)
        frames, W, bias = arena.input(frames_.to(DEV), "frames"), arena.input(W_.to(DEV), "W"), arena.input(b_.to(DEV), "bias")
        ii = None if inds is None else arena.input(torch.tensor(inds, dtype=torch.int64, device=DEV), "inds")
        dz_ = torch.randn((images, 20, 20, 32), generator=g).to(DEV)
        dz = arena.input(dz_, "dz")
        rec = arena.carve((PC.AMAX_WORDS,), torch.int32, "dz_amax").zero_()
        cnn.absmax(dz, rec)
        pack = arena.carve((_lib.load().mi355ppo_cnn_conv1q1_pack_bytes() // 4,), name="pack")
        z1, dW, db = arena.carve((images, 20, 20, 32), name="z1"), arena.carve((32, 1, 8, 8), name="dW1"), arena.carve((32,), name="db1")
        with GA.exact_workspaces(monkeypatch, arena) as requested:
            arena.stage = "conv1q1 pack: "
            ops.conv1q1_pack(W, pack)
            arena.stage = "conv1q1 pre fwd: "
            ops.conv1q1_pre_fwd(frames, pack, bias, ii, z1)
            arena.stage = "conv1p1 wgrad: "
            ops.conv1p1_wgrad(frames, dz, rec, ii, out=(dW, db))
        arena.assert_guards_intact()
        assert len(requested) == 1 and requested[0] > 0
        got.append([t.detach().cpu().clone() for t in (pack.view(torch.int32), z1, dW, db)])
    for x, y in zip(*got):
        assert GA.same_bits(x, y)                                      # nothing read that was not written
    assert all(torch.isfinite(t).all() for t in got[0][1:])


def _network(seed, n_actions=6):
    from cleanrl_amd import envs as E
    from cleanrl_amd.agents import AtariLSTMQNetwork

    torch.manual_seed(seed)
    env = types.SimpleNamespace(single_action_space=E.Discrete(n_actions))
    net = AtariLSTMQNetwork(env)
    with torch.no_grad():                       # non-trivial LayerNorm affines
        for i in (1, 4, 7, 11):
            net.network[i].weight.add_(0.2 * torch.randn_like(net.network[i].weight))
            net.network[i].bias.add_(0.2 * torch.randn_like(net.network[i].bias))
    return net


def test_whole_network_at_70_rows_is_within_the_bar_of_float64():
    from cleanrl_amd import ln_cnn

    rows = 70
    net = _network(11)
    g = torch.Generator().manual_seed(12)
    frames = torch.randint(0, 256, (rows + 10, 84, 84), generator=g, dtype=torch.uint8)
    inds = torch.randperm(rows + 10, generator=g)[:rows]
    dh = torch.randn((rows, 512), generator=g)
    x = frames[inds].unsqueeze(1)

    def torch_run(n, xx, d):
        for p in n.parameters():
            p.grad = None
        h = n.network(xx / 255.0)
        gx = n.gates(xx)
        h.backward(d)
        return h.detach(), gx.detach(), [p.grad.detach().clone() for p in n.network.parameters()]

    h64, gx64, g64 = torch_run(copy.deepcopy(net).double(), x.double(), dh.double())
    h32, gx32, g32 = torch_run(copy.deepcopy(net).to(DEV), x.float().to(DEV), dh.to(DEV))
    fused = copy.deepcopy(net).to(DEV)
    trunk = ln_cnn.LnNatureTrunk()
    for p in fused.parameters():
        p.grad = None
    with torch.no_grad():
        gx = fused.gates_fused(trunk, frames.to(DEV), inds.to(DEV)).clone()
    h = trunk(frames.to(DEV), inds.to(DEV), fused.network)
    h.backward(dh.to(DEV))
    names = ["h", "gx"] + [n for n, _ in fused.network.named_parameters()]
    assert len(names) == 18
    failures = []
    for name, got, r64, r32 in zip(names, [h, gx] + [p.grad for p in fused.network.parameters()], [h64, gx64] + g64, [h32, gx32] + g32):
        try:
            PC.bar(name, got, r64, r32)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


def test_golden_iterations_teacher_forced_on_the_fused_trunk(monkeypatch):
    monkeypatch.setenv("MI355PPO_PQN_TRUNK", "fused")
    g = PL.golden_case()
    recs, metrics, net, learner = PL.replay(g, backend="fused", device="cuda", force_actions=True)
    assert learner.fused and learner.fused_trunk and learner.device.type == "cuda"
    assert learner.obs.dtype == torch.uint8 and tuple(learner.obs.shape[2:]) == (84, 84)
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
    err = (PL.flat(net)[::int(g["stride"])] - torch.from_numpy(g["final_params_sub"])).abs().max().item()
    print(f"final parameters: error {err:.3e}")
    assert err <= 1e-4


def test_a_captured_forward_and_backward_chain_replays_the_eager_bits():
    from cleanrl_amd import ln_cnn

    rows = 70
    net = _network(21).to(DEV)
    g = torch.Generator().manual_seed(22)
    frames = torch.randint(0, 256, (rows + 4, 84, 84), generator=g, dtype=torch.uint8).to(DEV)
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
    assert len(eager) == 17 and eager[1].shape == (32, 1, 8, 8) and all(torch.equal(a, b) for a, b in zip(eager, again))
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


def test_script_runs_on_the_gpu_with_the_fused_trunk(tmp_path):
    cmd = ["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "cleanrl_amd", "pqn_atari_envpool_lstm.py"), "--num-envs", "8",
           "--num-steps", "32", "--total-timesteps", "512"]
    env = dict(os.environ)
    env.pop("MI355PPO_PQN", None)
    env["MI355PPO_PQN_TRUNK"] = "fused"
    out = subprocess.run(cmd, capture_output=True, text=True, cwd=tmp_path, timeout=330, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert len([ln for ln in out.stdout.splitlines() if ln.startswith("SPS: ")]) == 2
