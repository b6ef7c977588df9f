"""MI355PPO_MA_ATARI=fused on the MI355X: the new entry points against their host twins inside the guard arena, the row-bias instance of
kernel Q against the plain one and against the full six-channel convolution in float64, and the learner -- the reference's lines, the
default backend, the script, the store-time flag, captured against eager updates.

Shapes: a tile of 32 output pixels against 400 per image straddles images from M = 2 on; M = 33 has more than one workgroup's worth of
tiles and a last tile that ends inside an image pair; the fold has 9 partials there (four images each, four interleaved chains)."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from guard_arena import SENTINELS, Arena, exact_workspaces
from cleanrl_amd import _lib
from cleanrl_amd import envs as E
from cleanrl_amd.learner_smoke import default_args

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from cleanrl_amd import cnn

DEV = torch.device("cuda:0")
MIX = [(1, 0), (0, 1), (0, 0), (3, 250)]
PACK_BYTES = 33408


def P(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _frames6(n, seed, mix=MIX):
    rs = np.random.RandomState(seed)
    f = rs.randint(0, 256, size=(n, 84, 84, 6)).astype(np.uint8)
    for i in range(n):
        f[i, :, :, 4], f[i, :, :, 5] = mix[i % len(mix)]
    return f


def _weights6(seed):
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(32, 6, 8, 8, generator=g) * (1.0 / np.sqrt(6 * 64))
    b = torch.randn(32, generator=g) * 0.1
    return W.contiguous(), b


def _close(got, ref, what, tol=2e-5):
    """tests/test_gpu_cnn.py's bar for kernel Q's forward and kernel P's weight gradient: 2e-5 of the float64 result's scale."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    scale, err = ref.abs().max().item(), (got - ref).abs().max().item()
    print(f"{what}: max err {err:.3e}, scale {scale:.3e}, rel {err / max(scale, 1e-30):.2e}")
    assert err <= tol * scale + 1e-30, f"{what}: max err {err:.3e} vs scale {scale:.3e} (rel {err / max(scale, 1e-30):.2e})"


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("with_inds", [False, True])
@pytest.mark.parametrize("M", [1, 3, 33])
def test_entry_points_return_their_twins_bits_inside_the_guard_arena(monkeypatch, M, with_inds):
    lib = _lib.load()
    R = M + 2 if with_inds else M
    f = _frames6(R, 20 + M)
    inds_np = np.random.RandomState(M).permutation(R)[:M].astype(np.int64) if with_inds else None
    W6, b = _weights6(3)
    dz_np = np.random.RandomState(7).standard_normal((M, 20, 20, 32)).astype(np.float32)
    dW4_np = np.random.RandomState(8).standard_normal((32, 4, 8, 8)).astype(np.float32)
    # ---- the twins
    rows_t, ind_t, flag_t = np.zeros((R, 84, 84, 4), np.uint8), np.zeros((R, 2), np.uint8), np.zeros(1, np.uint32)
    _lib.call("mi355ppo_ma_atari_split_u8_cpu", P(f), P(rows_t), P(ind_t), P(flag_t), R)
    pack_t, tap_t, W6n, bn = np.zeros(PACK_BYTES, np.uint8), np.zeros(64, np.float32), W6.numpy(), b.numpy()
    _lib.call("mi355ppo_ma_atari_conv1_pack_f32_cpu", P(W6n), P(pack_t), P(tap_t))
    out_t, mask_t = np.zeros((M, 20, 20, 32), np.float32), np.zeros(M * 400, np.uint32)
    _lib.call("mi355ppo_ma_atari_conv1_fwd_cpu", P(rows_t), P(inds_np), P(ind_t), P(pack_t), P(tap_t), P(bn), P(out_t), P(mask_t), M)
    dW6_t = np.zeros((32, 6, 8, 8), np.float32)
    _lib.call("mi355ppo_ma_atari_conv1_wgrad_fold_f32_cpu", P(dz_np), P(inds_np), P(ind_t), P(dW4_np), P(dW6_t), M)
    assert flag_t[0] == 0 and len({tuple(r) for r in ind_t[:4]}) == min(R, 4)
    results = []
    for sentinel in SENTINELS:
        A = Arena(DEV, sentinel)
        frames = A.input(torch.from_numpy(f), "frames6")
        rows, ind = A.carve((R, 84, 84, 4), torch.uint8, "rows4"), A.carve((R, 2), torch.uint8, "ind")
        flag = A.input(torch.zeros(1, dtype=torch.int32), "flag")
        cnn.ma_split(frames, rows, ind, flag)
        pack, tapsum = A.carve((cnn.QPACK_NUMEL,), torch.float32, "pack"), A.carve((64,), torch.float32, "tapsum")
        cnn.ma_conv1_pack(A.input(W6, "W6"), pack, tapsum)
        inds = None if inds_np is None else A.input(torch.from_numpy(inds_np), "inds")
        bias = A.input(b, "bias")
        out_b, mask_b = A.carve((M, 20, 20, 32), torch.float32, "a1 (bits)"), A.carve((M * 400,), torch.int32, "mask (bits)")
        cnn.ma_conv1_fwd_bits(rows, ind, pack, tapsum, bias, inds, out_b, mask_b)
        out_a, mask_a = A.carve((M, 20, 20, 32), torch.float32, "a1 (amax)"), A.carve((M * 400,), torch.int32, "mask (amax)")
        rec = A.input(torch.zeros(cnn.AMAX_WORDS, dtype=torch.int32), "amax record")
        cnn.ma_conv1_fwd_amax(rows, ind, pack, tapsum, bias, inds, out_a, mask_a, rec)
        out_n = A.carve((M, 20, 20, 32), torch.float32, "a1 (amax, no bits)")
        cnn.ma_conv1_fwd_amax(rows, ind, pack, tapsum, bias, inds, out_n, None, A.input(torch.zeros(cnn.AMAX_WORDS, dtype=torch.int32), "rec2"))
        dz, dW4 = A.input(torch.from_numpy(dz_np), "dz1"), A.input(torch.from_numpy(dW4_np), "dW4")
        dW6, dW6b = A.carve((32, 6, 8, 8), torch.float32, "dW6"), A.carve((32, 6, 8, 8), torch.float32, "dW6 again")
        with exact_workspaces(monkeypatch, A) as asked:
            A.stage = "fold: "
            cnn.ma_conv1_wgrad_fold(dz, ind, inds, dW4, dW6)
            cnn.ma_conv1_wgrad_fold(dz, ind, inds, dW4, dW6b)
        assert asked == [lib.mi355ppo_ma_atari_conv1_wgrad_fold_workspace_bytes(M)] * 2
        A.assert_guards_intact()
        assert torch.equal(rows.cpu(), torch.from_numpy(rows_t)) and torch.equal(ind.cpu(), torch.from_numpy(ind_t)) and flag.item() == 0
        assert np.array_equal(pack.cpu().numpy().view(np.uint8), pack_t) and np.array_equal(tapsum.cpu().numpy().view(np.uint32), tap_t.view(np.uint32))
        for got in (out_b, out_a, out_n):
            assert np.array_equal(got.cpu().numpy().view(np.uint32), out_t.view(np.uint32))
        for got in (mask_b, mask_a):
            assert np.array_equal(got.cpu().numpy().view(np.uint32), mask_t)
        assert cnn.amax_value(rec) == float(out_t.max())
        assert np.array_equal(dW6.cpu().numpy().view(np.uint32), dW6_t.view(np.uint32))
        assert torch.equal(_bits(dW6), _bits(dW6b)), "the fold must give the same bits twice"
        results.append((_bits(out_b), _bits(dW6)))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1])


def test_split_flag_is_set_by_a_deviating_pixel_and_never_cleared():
    f = _frames6(3, 5)
    rows, ind = torch.empty((3, 84, 84, 4), dtype=torch.uint8, device=DEV), torch.empty((3, 2), dtype=torch.uint8, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    cnn.ma_split(torch.from_numpy(f).to(DEV), rows, ind, flag)
    assert flag.item() == 0
    for where in ((2, 83, 83, 5), (1, 0, 1, 4)):
        bad = f.copy()
        bad[where] ^= 1
        fl = torch.zeros(1, dtype=torch.int32, device=DEV)
        cnn.ma_split(torch.from_numpy(bad).to(DEV), rows, ind, fl)
        assert fl.item() != 0, where
        cnn.ma_split(torch.from_numpy(f).to(DEV), rows, ind, fl)        # a clean store leaves it set
        assert fl.item() != 0


def test_all_zero_indicators_are_kernel_q_bit_for_bit():
    M, R = 33, 40
    f = _frames6(R, 9, [(0, 0)])
    rows = torch.from_numpy(np.ascontiguousarray(f[..., :4])).to(DEV)
    ind = torch.zeros((R, 2), dtype=torch.uint8, device=DEV)
    inds = torch.from_numpy(np.random.RandomState(2).permutation(R)[:M]).to(DEV)
    W6, b = _weights6(5)
    pack, tapsum = cnn.ma_conv1_pack(W6.to(DEV))
    pack4 = cnn.repack_weights(W6[:, :4].contiguous().to(DEV), 1, cnn.MODE_FWD_Q)
    assert torch.equal(_bits(pack), _bits(pack4))
    bias = b.to(DEV)
    new = lambda: (torch.empty((M, 20, 20, 32), device=DEV), torch.empty(M * 400, dtype=torch.int32, device=DEV), cnn.new_amax(1, DEV)[0])
    (o1, m1, r1), (o2, m2, r2), (o3, m3, _), (o4, m4, _) = new(), new(), new(), new()
    cnn.ma_conv1_fwd_amax(rows, ind, pack, tapsum, bias, inds, o1, m1, r1)
    cnn.conv1q_fwd_amax(rows, pack4, bias, inds, o2, m2, r2)
    cnn.ma_conv1_fwd_bits(rows, ind, pack, tapsum, bias, inds, o3, m3)
    cnn.conv1q_fwd_bits(rows, pack4, bias, inds, o4, m4)
    assert torch.equal(_bits(o1), _bits(o2)) and torch.equal(m1, m2) and torch.equal(r1, r2)
    assert torch.equal(_bits(o3), _bits(o4)) and torch.equal(m3, m4) and torch.equal(_bits(o1), _bits(o3))


def test_against_the_full_six_channel_convolution_in_float64():
    """conv1's output and the six-channel dW1 against float64 on constant-plane observations built from the same rows, at the bar
    tests/test_gpu_cnn.py holds kernel Q's forward and kernel P's dW1 to (2e-5 of the float64 result's scale) -- the frame channels and
    the indicator channels of dW1 each on their OWN scale (the indicator channels' is ~400 M times larger), which is stricter than the one
    scale over the tensor.  The fold adds in double: measured on the MI355X, 3e-8 of the indicator channels' scale."""
    M, R = 33, 37
    f = _frames6(R, 11)
    inds_np = np.random.RandomState(3).permutation(R)[:M]
    W6, b = _weights6(6)
    g = torch.Generator().manual_seed(12)
    dz = torch.randn(M, 32, 20, 20, generator=g)
    Wd, bd = W6.double().requires_grad_(True), b.double().requires_grad_(True)
    x = torch.from_numpy(f[inds_np]).permute(0, 3, 1, 2).double()
    x = torch.cat([x[:, :4] / 255.0, x[:, 4:]], 1)                          # only the frame channels are divided by 255 (:104)
    pre = F.conv2d(x, Wd, bd, stride=4)
    refW, refb = torch.autograd.grad(pre, (Wd, bd), dz.double())
    rows, ind = torch.empty((R, 84, 84, 4), dtype=torch.uint8, device=DEV), torch.empty((R, 2), dtype=torch.uint8, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    cnn.ma_split(torch.from_numpy(f).to(DEV), rows, ind, flag)
    inds = torch.from_numpy(inds_np).to(DEV)
    pack, tapsum = cnn.ma_conv1_pack(W6.to(DEV))
    out, mask = torch.empty((M, 20, 20, 32), device=DEV), torch.empty(M * 400, dtype=torch.int32, device=DEV)
    cnn.ma_conv1_fwd_bits(rows, ind, pack, tapsum, b.to(DEV), inds, out, mask)
    _close(out, torch.relu(pre).detach().permute(0, 2, 3, 1), "row-bias conv1 forward")
    dzd = dz.permute(0, 2, 3, 1).contiguous().to(DEV)
    for name, amax in (("f32 pipe", None), ("f16x2", "rec")):
        if amax is not None:
            rec = cnn.new_amax(1, DEV)[0]
            cnn.absmax(dzd, rec)
            amax = (None, rec)
        dW4, db = cnn.conv_wgrad(rows, dzd, 1, inds, amax=amax)
        dW6 = cnn.ma_conv1_wgrad_fold(dzd, ind, inds, dW4)
        _close(dW6[:, :4], refW[:, :4], f"dW1 frame channels ({name})")
        _close(dW6[:, 4:], refW[:, 4:], f"dW1 indicator channels ({name})")
        _close(db, refb, f"db1 ({name})")


def _delta_matches(got_now, init_sub, final_sub, what, frac=0.98, rtol=5e-2, atol=2e-5):
    delta, want = got_now - init_sub, final_sub - init_sub
    close = np.isclose(delta, want, rtol=rtol, atol=atol)
    assert close.mean() > frac, f"{what}: only {close.mean():.4f} of sampled parameters moved as the reference's did"


def _init_1thread(seed, build):
    n = torch.get_num_threads()
    torch.set_num_threads(1)          # as when minted
    torch.manual_seed(seed)
    out = build()
    torch.set_num_threads(n)
    return out


def _ma_learner(monkeypatch, backend, N, T, nmb, seed=0, epochs=1, clip=0.1, agent=None):
    from cleanrl_amd.agents import MAAtariAgent
    from cleanrl_amd.learner import PPOLearner

    envs = SimpleNamespace(single_observation_space=E.Box(0, 255, (84, 84, 6), np.uint8), single_action_space=E.Discrete(6))
    if agent is None:
        torch.manual_seed(seed)
        agent = MAAtariAgent(envs).to(DEV)
    if backend == "fused":
        monkeypatch.setenv("MI355PPO_MA_ATARI", "fused")
    else:
        monkeypatch.delenv("MI355PPO_MA_ATARI", raising=False)
    L = PPOLearner(agent, default_args(num_steps=T, num_minibatches=nmb, update_epochs=epochs, clip_coef=clip), envs.single_observation_space,
                   envs.single_action_space, N, DEV, sample_seed=1)
    monkeypatch.delenv("MI355PPO_MA_ATARI", raising=False)
    assert L.ma_fused == (backend == "fused") and L.fused_cnn == L.ma_fused
    return L


def test_fused_minibatch_steps_against_the_reference_lines(monkeypatch):
    """tests/golden/ma_atari_update.npz through the fused backend, held to what the default path is held to
    (test_procgen_and_ma_atari_hip_minibatch_steps_against_reference_lines): rtol 1e-3 / atol 2e-4 on log-probs and values, the loss
    within 2e-3, 90 % of the sampled parameters moving as the reference's did."""
    from cleanrl_amd.agents import MAAtariAgent

    g = load_golden("ma_atari_update")["ma_2steps"]
    envs = SimpleNamespace(single_observation_space=E.Box(0, 255, (84, 84, 6), np.uint8), single_action_space=E.Discrete(6))
    agent = _init_1thread(int(g["init_seed"]), lambda: MAAtariAgent(envs)).to(DEV)
    stride, B = int(g["stride"]), g["b_actions"].shape[0]
    L = _ma_learner(monkeypatch, "fused", 4, B // 4, 2, agent=agent)
    assert tuple(L.obs.shape[2:]) == (84, 84, 4) and not L.partial_scale and L.hwc_frames and not L.relayout
    np.testing.assert_allclose(L.flat.params[::stride].cpu().numpy(), g["init_params_sub"], rtol=1e-4, atol=1e-5)
    Fg = lambda k: torch.from_numpy(g[k]).to(DEV)
    cnn.ma_split(Fg("b_obs_u8").view(B, 84, 84, 6).contiguous(), L.obs.view(B, 84, 84, 4), L.ind.view(B, 2), L._ma_flag)
    assert L._ma_flag.item() == 0 and torch.equal(L.obs.view(B, 84, 84, 4), Fg("b_obs_u8").view(B, 84, 84, 6)[..., :4])
    b_obs, b_ind = L.obs.reshape((-1,) + L.obs_shape), L.ind.reshape(-1, 2)
    with torch.no_grad():
        logits, v = agent.heads_u8(b_obs, None, b_ind)
        lp = torch.log_softmax(logits, 1).gather(1, Fg("b_actions").long().view(-1, 1)).view(-1)
    np.testing.assert_allclose(lp.cpu().numpy(), g["logprob_all"], rtol=1e-3, atol=2e-4)
    np.testing.assert_allclose(v.view(-1).cpu().numpy(), g["value_all"], rtol=1e-3, atol=2e-4)
    M = 16
    sc = torch.zeros(2, 7, device=DEV)
    prev = g["init_params_sub"]
    for k in range(2):
        idx = torch.from_numpy(np.ascontiguousarray(g["perm"][k * M:(k + 1) * M])).to(DEV)
        L._minibatch_hip(idx, b_obs, Fg("b_actions"), Fg("b_logprobs"), Fg("b_advantages"), Fg("b_returns"), Fg("b_values"), float(g["lr"]), sc[k])
        ref = float(g["losses"][k])
        assert abs(sc[k, 0].item() - ref) <= 2e-3 * max(1.0, abs(ref)), (k, sc[k, 0].item(), ref)
        now = L.flat.params[::stride].cpu().numpy()
        _delta_matches(now, prev, g[f"params_sub_after_{k + 1}"], f"fused ma_atari minibatch step {k + 1}", frac=0.9)
        prev = g[f"params_sub_after_{k + 1}"]
        L.flat.params[::stride].copy_(torch.from_numpy(prev).to(DEV))
        L._bump_weights_version()
    L.flat.check_views()


def _rollout(L, env):
    for step in range(L.T):
        action = L.act(step)
        obs, reward, done, _ = env.step(action.cpu().numpy())
        L.store_reward(step, reward)
        L.observe(step + 1, obs, done.astype(np.float32))
    L.finish_rollout()


def _started(monkeypatch, backend, N=8, T=16, nmb=4, graphs=False, env_seed=3):
    L = _ma_learner(monkeypatch, backend, N, T, nmb, seed=4)
    env = E.SyntheticMAAtariVecEnv(N, seed=env_seed)
    L.observe(0, env.reset(), np.zeros(N, np.float32))
    if graphs:
        L.capture_update()
    return L, env


def test_fused_backend_agrees_with_the_default_backend(monkeypatch):
    (Lt, envt), (Lf, envf) = _started(monkeypatch, "torch"), _started(monkeypatch, "fused")
    _rollout(Lt, envt)
    _rollout(Lf, envf)
    assert torch.equal(Lf.obs, Lt.obs[..., :4]) and torch.equal(Lf.boot_obs, Lt.boot_obs[..., :4])
    assert torch.equal(Lf.ind, Lt.obs[:, :, 0, 0, 4:]) and torch.equal(Lf.actions, Lt.actions)
    np.testing.assert_allclose(Lf.logprobs.cpu().numpy(), Lt.logprobs.cpu().numpy(), rtol=1e-3, atol=2e-4)
    np.testing.assert_allclose(Lf.values.cpu().numpy(), Lt.values.cpu().numpy(), rtol=1e-3, atol=2e-4)
    np.random.seed(5)
    mt = Lt.update(2.5e-4)
    np.random.seed(5)
    mf = Lf.update(2.5e-4)
    assert mt["num_updates"] == mf["num_updates"] == 4
    assert abs(mf["loss"] - mt["loss"]) <= 2e-3 * max(1.0, abs(mt["loss"])), (mf, mt)


def test_script_takes_the_fused_trunk_when_the_switch_is_set(monkeypatch):
    from cleanrl_amd import ppo_pettingzoo_ma_atari

    monkeypatch.setenv("MI355PPO_MA_ATARI", "fused")
    L = ppo_pettingzoo_ma_atari.main(["--num-envs", "8", "--num-steps", "16", "--total-timesteps", "256", "--num-minibatches", "4"])
    assert L.hip and L.obs.dtype == torch.uint8 and tuple(L.obs.shape[2:]) == (84, 84, 4) and tuple(L.ind.shape) == (16, 8, 2)
    assert L.ma_fused and L.fused_cnn and not L.partial_scale
    bufs = L.agent._trunk.bufs
    assert "ma_tapsum" in bufs._bt and ("ma_dw4", DEV) in bufs.by_m          # conv1's row-bias pack and the fold's temporary were used
    assert L._update_graphs is not None                                      # the same graph policy as ppo_atari.py
    assert np.isfinite(L.last_metrics["loss"]) and L.last_metrics["num_updates"] == 16


def test_a_deviating_indicator_pixel_raises_with_the_updates_diagnostics(monkeypatch):
    L, env = _started(monkeypatch, "fused", N=4, T=2, nmb=2)
    for step in range(L.T):
        action = L.act(step)
        obs, reward, done, _ = env.step(action.cpu().numpy())
        if step == 0:
            obs = obs.copy()
            obs[1, 40, 41, 4] ^= 1
        L.store_reward(step, reward)
        L.observe(step + 1, obs, done.astype(np.float32))
    L.finish_rollout()
    with pytest.raises(RuntimeError, match="not constant") as exc:
        L.update(2.5e-4)
    assert "MI355PPO_MA_ATARI" in str(exc.value)


def test_captured_update_is_bit_identical_to_the_eager_update(monkeypatch):
    (Le, enve), (Lg, envg) = _started(monkeypatch, "fused"), _started(monkeypatch, "fused", graphs=True)
    assert Lg._update_graphs is not None and Le._update_graphs is None
    assert torch.equal(Le.flat.params, Lg.flat.params) and not Lg.flat.grads.any()
    for it in range(2):
        _rollout(Le, enve)
        _rollout(Lg, envg)
        np.random.seed(100 + it)
        me = Le.update(2.5e-4)
        np.random.seed(100 + it)
        mg = Lg.update(2.5e-4)
        Le.start_iteration(); Lg.start_iteration()
        assert torch.equal(Le.flat.params, Lg.flat.params), it
        assert torch.equal(Le.flat.exp_avg, Lg.flat.exp_avg) and torch.equal(Le.flat.exp_avg_sq, Lg.flat.exp_avg_sq), it
        assert me == mg or all(me[k] == mg[k] or (np.isnan(me[k]) and np.isnan(mg[k])) for k in me), (it, me, mg)
