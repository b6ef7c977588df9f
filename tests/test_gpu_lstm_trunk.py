"""The one-frame plain NatureCNN of ppo_atari_lstm.py on the device (MI355PPO_LSTM_TRUNK=fused): kernel Q1's ReLU instances against their host
twin (bits: output, mask words, amax value), their guard bands, the one-frame branch of cnn.NatureTrunkFn + the FC layer against float64,
LSTMPPOLearner on the golden iteration with both LSTM backends, and the script."""
import copy
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import guard_arena as GA
import pqn_trunk_cases as PC
from conftest import load_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda")


def _case(stored, seed):
    g = torch.Generator().manual_seed(9500 + seed)
    frames = torch.randint(0, 256, (stored, 84, 84), generator=g, dtype=torch.uint8)      # exactly stored x 7,056 bytes, its own allocation
    return frames, 0.05 * torch.randn((32, 1, 8, 8), generator=g), 0.5 * torch.randn(32, generator=g), g


def _second_tile_count():
    """The smallest image count at which some wave of kernel Q1's persistent grid walks a second tile (the prefetch of the next tile and the
    loop's back edge run): 3 workgroups of 4 waves per CU, an image is 12.5 tiles of 32 pixels -- so more than 12 * CUs tiles; 256 images where
    that is larger (as tests/test_gpu_single_frame_trunk.py derives it)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return max(256, 12 * cus * 32 // 400 + 1)


# 1 image: 12.5 tiles, the last one half past P.  3 images through inds: a tile straddles two images, and the gather.  70: several workgroups.
# The second-tile count: the prefetch and the loop's back edge.
@pytest.mark.parametrize("images,inds", [(1, None), (3, [3, 0, 3]), (70, None), ("second tile", None)])
def test_forward_equals_the_twin_bit_for_bit(images, inds):
    from cleanrl_amd import cnn, host_ops, ops

    if images == "second tile":
        images = _second_tile_count()
    stored = images if inds is None else 4
    frames, W, b, _ = _case(stored, seed=images)
    ii = None if inds is None else torch.tensor(inds, dtype=torch.int64)
    ref_bits, ref_rec = torch.empty(images * 400, dtype=torch.int32), torch.zeros(PC.AMAX_WORDS, dtype=torch.int32)
    ref = host_ops.conv1q1_fwd(frames, host_ops.conv1q1_pack(W), b, ii, bits=ref_bits, amax=ref_rec)
    assert (ref == 0).any() and (ref > 0).any()
    fd, Wd, bd, iid = frames.to(DEV), W.to(DEV), b.to(DEV), None if ii is None else ii.to(DEV)
    pack = ops.conv1q1_pack(Wd)

    def device_run(entry, with_bits):
        out = torch.full((images, 20, 20, 32), float("nan"), device=DEV)
        bits = torch.full((images * 400,), 0x5A5A5A5A, dtype=torch.int32, device=DEV) if with_bits else None
        rec = cnn.new_amax(1, DEV)[0]
        if entry == "amax":
            ops.conv1q1_fwd_amax(fd, pack, bd, iid, out, bits, rec)
        else:
            ops.conv1q1_fwd_bits(fd, pack, bd, iid, out, bits)
        return out.cpu(), None if bits is None else bits.cpu(), rec.cpu()

    for entry, with_bits in (("amax", True), ("amax", False), ("bits", True)):
        runs = [device_run(entry, with_bits) for _ in range(2)]
        out, bits, rec = runs[0]
        assert torch.equal(out, ref), (entry, with_bits, (out.double() - ref.double()).abs().max().item())
        if with_bits:
            assert torch.equal(bits, ref_bits), (entry, int((bits != ref_bits).sum()))
            assert torch.equal(bits, PC.packed_bits(out))
        if entry == "amax":
            assert PC.amax_value(rec) == PC.amax_value(ref_rec) == ref.max().item(), entry
        else:
            assert int((rec != 0).sum()) == 0
        assert torch.equal(out, runs[1][0]) and (bits is None or torch.equal(bits, runs[1][1])) and PC.amax_value(rec) == PC.amax_value(runs[1][2])
    if inds is not None:
        assert torch.equal(ref[0], ref[2])


@pytest.mark.parametrize("images,inds", [(3, [3, 0, 3]), (70, None)])
def test_device_kernels_stay_inside_their_tensors(images, inds, monkeypatch):
    from cleanrl_amd import _lib, ops

    got = []
    for sentinel in GA.SENTINELS:
        arena = GA.Arena(DEV, sentinel, words=1 << 23)
        stored = images if inds is None else 4
        frames_, W_, b_, _ = _case(stored, seed=300 + images)
        frames, W, bias = arena.input(frames_.to(DEV), "frames"), arena.input(W_.to(DEV), "W"), arena.input(b_.to(DEV), "bias")
        ii = None if inds is None else arena.input(torch.tensor(inds, dtype=torch.int64, device=DEV), "inds")
        pack = arena.carve((_lib.load().mi355ppo_cnn_conv1q1_pack_bytes() // 4,), name="pack")
        a1, a1b = arena.carve((images, 20, 20, 32), name="a1"), arena.carve((images, 20, 20, 32), name="a1 (bits entry)")
        bits, bits_b = arena.carve((images * 400,), torch.int32, "mask bits"), arena.carve((images * 400,), torch.int32, "mask bits (bits entry)")
        rec = arena.carve((PC.AMAX_WORDS,), torch.int32, "a1_amax").zero_()
        with GA.exact_workspaces(monkeypatch, arena):
            arena.stage = "conv1q1 pack: "
            ops.conv1q1_pack(W, pack)
            arena.stage = "conv1q1 fwd amax: "
            ops.conv1q1_fwd_amax(frames, pack, bias, ii, a1, bits, rec)
            arena.stage = "conv1q1 fwd bits: "
            ops.conv1q1_fwd_bits(frames, pack, bias, ii, a1b, bits_b)
        arena.assert_guards_intact()
        assert GA.same_bits(a1, a1b) and GA.same_bits(bits, bits_b)
        got.append([t.detach().cpu().clone() for t in (a1, bits)] + [PC.amax_value(rec.cpu())])
    (x1, m1, r1), (x2, m2, r2) = got
    assert GA.same_bits(x1, x2) and GA.same_bits(m1, m2) and r1 == r2 == x1.max().item()      # nothing read that was not written
    assert torch.isfinite(x1).all() and torch.equal(m1, PC.packed_bits(x1))


# ------------------------------------------------------------------------------------------------------------ trunk + FC against float64
def _agent(seed, n_actions=4):
    from cleanrl_amd import envs as E
    from cleanrl_amd.agents import AtariLSTMAgent

    torch.manual_seed(seed)
    return AtariLSTMAgent(SimpleNamespace(single_observation_space=E.Box(0, 255, (1, 84, 84), np.uint8), single_action_space=E.Discrete(n_actions)))


@pytest.mark.parametrize("rows", [5, 70])
def test_one_frame_trunk_and_fc_are_within_the_bar_of_float64(rows):
    from cleanrl_amd import cnn

    net = _agent(31).network
    with torch.no_grad():                        # layer_init's zero biases would leave the bias paths untested
        for i in (0, 2, 4, 7):
            net[i].bias.add_(0.1 * torch.randn_like(net[i].bias))
    g = torch.Generator().manual_seed(32 + rows)
    frames = torch.randint(0, 256, (rows + 3, 84, 84, 1), generator=g, dtype=torch.uint8)      # the learner's storage layout
    inds = torch.randperm(rows + 3, generator=g)[:rows]
    inds[rows - 1] = inds[0]                     # a repeat
    dh = torch.randn((rows, 512), generator=g)
    x = frames[inds].permute(0, 3, 1, 2)

    def torch_run(n, xx, d):
        h = n(xx / 255.0)
        grads = torch.autograd.grad(h, list(n.parameters()), d)
        return h.detach(), [t.detach() for t in grads]

    h64, g64 = torch_run(copy.deepcopy(net).double(), x.double(), dh.double())
    h32, g32 = torch_run(copy.deepcopy(net).to(DEV), x.float().to(DEV), dh.to(DEV))
    fused = copy.deepcopy(net).to(DEV)
    fd, idd, dhd = frames.to(DEV), inds.to(DEV), dh.to(DEV)

    def fused_run():
        trunk = cnn.NatureTrunk()
        feats = trunk(fd, idd, fused[0], fused[2], fused[4])
        h = cnn.LinearReLUHwcFn.apply(feats, fused[7].weight, fused[7].bias, trunk.bufs)
        grads = torch.autograd.grad(h, list(fused.parameters()), dhd)
        return [h.detach().clone()] + [t.detach().clone() for t in grads]

    runs = [fused_run() for _ in range(2)]
    names = ["h"] + ["d " + n for n, _ in fused.named_parameters()]
    assert len(names) == 9 and runs[0][1].shape == (32, 1, 8, 8)
    failures = []
    for name, got, r64, r32 in zip(names, runs[0], [h64] + g64, [h32] + g32):
        try:
            PC.bar(f"{name} ({rows} rows)", got, r64, r32)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)
    for name, a, b in zip(names, *runs):
        assert torch.equal(a, b), name


def test_the_one_frame_branch_refuses_what_it_does_not_cover():
    from cleanrl_amd import cnn

    net = _agent(33).network.to(DEV)
    frames = torch.zeros((2, 84, 84, 1), dtype=torch.uint8, device=DEV)
    trunk = cnn.NatureTrunk()
    trunk.bufs.split = "bf16x3"
    with torch.no_grad(), pytest.raises(NotImplementedError, match="MI355PPO_LSTM_TRUNK=torch"):
        trunk(frames, None, net[0], net[2], net[4])


# ------------------------------------------------------------------------------------------------------------ the learner
def _learner(g, T, N):
    from cleanrl_amd import envs as E
    from cleanrl_amd.agents import AtariLSTMAgent
    from cleanrl_amd.learner_lstm import LSTMPPOLearner
    from cleanrl_amd.learner_smoke import default_args

    envs = SimpleNamespace(single_observation_space=E.Box(0, 255, (1, 84, 84), np.uint8), single_action_space=E.Discrete(4))
    n = torch.get_num_threads()
    torch.set_num_threads(1)          # as when minted: orthogonal_'s QR of the LSTM weights rounds per thread count
    torch.manual_seed(int(g["init_seed"]))
    agent = AtariLSTMAgent(envs).to(torch.device("cuda:0"))
    torch.set_num_threads(n)
    args = default_args(num_steps=T, num_minibatches=2, update_epochs=2)
    return agent, LSTMPPOLearner(agent, args, envs.single_observation_space, envs.single_action_space, N, torch.device("cuda:0"), sample_seed=1)


@pytest.mark.parametrize("lstm_backend", ["torch", "fused"])
def test_lstm_learner_on_the_fused_trunk_teacher_forced_against_reference_iteration(lstm_backend, monkeypatch):
    """The steps and tolerances of tests/test_zz_gpu_new_scripts.py::test_lstm_hip_path_teacher_forced_against_reference_iteration."""
    monkeypatch.setenv("MI355PPO_LSTM_TRUNK", "fused")
    monkeypatch.setenv("MI355PPO_LSTM", lstm_backend)
    g = load_golden("lstm_iteration")["lstm_T8_N4"]
    T, N = g["rewards"].shape
    agent, L = _learner(g, T, N)
    assert L.hip and L.fused_trunk and not L.fused_cnn and agent.lstm_backend == lstm_backend
    assert L.obs.dtype == torch.uint8 and tuple(L.obs.shape) == (T, N, 84, 84, 1) and L._x_roll is None
    stride = int(g["stride"])
    np.testing.assert_allclose(L.flat.params[::stride].cpu().numpy(), g["init_params_sub"], rtol=1e-4, atol=1e-5)
    frames, step_done = g["frames_u8"], g["step_done"]
    L.observe(0, frames[0], step_done[0])
    for step in range(T):
        L.act(step)
        np.testing.assert_allclose(L.values[step].cpu().numpy(), g["values"][step], rtol=1e-3, atol=2e-4)
        L.actions[step].copy_(torch.from_numpy(g["actions"][step]))
        L.logprobs[step].copy_(torch.from_numpy(g["logprobs"][step]))
        L.values[step].copy_(torch.from_numpy(g["values"][step]))
        L.store_reward(step, g["rewards"][step])
        L.observe(step + 1, frames[step + 1], step_done[step + 1])
    np.testing.assert_allclose(L.next_lstm_state[0].cpu().numpy(), g["next_h"], rtol=1e-3, atol=2e-4)
    np.testing.assert_allclose(L.next_lstm_state[1].cpu().numpy(), g["next_c"], rtol=1e-3, atol=2e-4)
    L.finish_rollout()
    np.testing.assert_allclose(L.advantages.cpu().numpy(), g["advantages"], rtol=1e-3, atol=3e-4)
    np.testing.assert_allclose(L.returns.cpu().numpy(), g["returns"], rtol=1e-3, atol=3e-4)
    L.advantages.copy_(torch.from_numpy(g["advantages"]))
    L.returns.copy_(torch.from_numpy(g["returns"]))
    bufs = agent._trunk.bufs
    assert bufs.cache_weights and not bufs.direct_grads and bufs.weights_version == 0
    np.random.seed(int(g["shuffle_seed"]))
    m = L.update(float(g["lr"]))
    assert m["num_updates"] == 4 and bufs.weights_version == 4           # one bump per optimizer step: the packs follow the flat Adam kernel
    np.testing.assert_allclose(m["loss"], float(g["last_loss"]), rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(m["value_loss"], float(g["last_v_loss"]), rtol=2e-3, atol=2e-4)
    np.testing.assert_allclose(m["entropy"], float(g["last_entropy"]), rtol=1e-3)
    delta = L.flat.params[::stride].cpu().numpy() - g["init_params_sub"]
    want = g["final_params_sub"] - g["init_params_sub"]
    close = np.isclose(delta, want, rtol=5e-2, atol=2e-5)
    assert close.mean() > 0.98, f"only {close.mean():.4f} of sampled parameters match the reference update"
    assert L._x_mb is None and L._x_roll is None                          # no f32 copy of the gathered minibatch or of a rollout slot
    L.flat.check_views()

    # a second update() from this state, twice: as it is, and with the version bump withheld after every optimizer step -- from the second
    # minibatch on the trunk then reads the packs of the weights before the step (stale), and the parameters come out different
    snap = [t.clone() for t in (L.flat.params, L.flat.exp_avg, L.flat.exp_avg_sq)], L.flat.step

    def second_update(stale):
        for t, s in zip((L.flat.params, L.flat.exp_avg, L.flat.exp_avg_sq), snap[0]):
            t.copy_(s)                           # (a torch write: the tensors' version counters move, the first minibatch repacks either way)
        L.flat.step = snap[1]
        step = type(L).optimizer_step_hip

        def held_back(lr):
            step(L, lr)
            bufs.weights_version -= 1

        if stale:
            L.optimizer_step_hip = held_back     # (an instance attribute in front of the method)
        np.random.seed(int(g["shuffle_seed"]) + 1)
        v0 = bufs.weights_version
        try:
            L.update(float(g["lr"]))
        finally:
            if stale:
                del L.optimizer_step_hip
        return L.flat.params.clone(), bufs.weights_version - v0

    p_fresh, moved = second_update(False)
    p_again, _ = second_update(False)
    assert moved == 4 and torch.equal(p_fresh, p_again)
    p_stale, moved = second_update(True)
    assert moved == 0 and not torch.equal(p_fresh, p_stale)


def test_script_runs_on_the_gpu_with_the_fused_trunk(tmp_path):
    code = ("import numpy as np, torch\n"
            "from cleanrl_amd import ppo_atari_lstm\n"
            "L = ppo_atari_lstm.main(['--num-envs', '8', '--num-steps', '16', '--total-timesteps', '256', '--num-minibatches', '4'])\n"
            "assert L.hip and L.fused_trunk and not L.fused_cnn and L.agent._trunk is not None\n"
            "assert L.obs.dtype == torch.uint8 and tuple(L.obs.shape[2:]) == (84, 84, 1) and L._x_mb is None and L._x_roll is None\n"
            "assert np.isfinite(L.last_metrics['loss']) and L.last_metrics['num_updates'] == 16\n"
            "print('fused trunk: ok')\n")
    env = dict(os.environ)
    env["MI355PPO_LSTM_TRUNK"] = "fused"
    env.pop("MI355PPO_LSTM", None)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", code], capture_output=True, text=True, cwd=tmp_path, timeout=330,
                         env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "fused trunk: ok" in out.stdout
