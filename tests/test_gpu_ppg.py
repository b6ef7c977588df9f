"""The PPG auxiliary-phase kernels (csrc/ppg.hip, the split step of csrc/optim.hip) on the MI355X: every entry point bit-equal to its
host twin at the tile edges, the minted cases of the reference's lines at the project's numeric rule, the gather against
``obs_u8_to_f32`` and past 4 GiB, the guard-band cases on device tensors with exact workspaces, a non-default stream, the split
step against ``clip_adam_``, and ``MI355PPO_PPG=fused`` in the learner -- teacher-forced against the reference's phase, against the
``torch`` backend from the same state, without a device-to-host copy during the epochs, and in the script."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import guard_arena as GA
import ppg_cases as P
from conftest import load_golden
from cleanrl_amd import envs as E
from cleanrl_amd import host_ops as H
from cleanrl_amd import ops
from cleanrl_amd.learner_smoke import default_args
from test_ppg_bounds import run_guarded

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CPU = torch.device("cpu")


def _same(a, b, what):
    assert GA.same_bits(a, b), f"{what}: the device differs from its twin"


# ---------------------------------------------------------------------------------------------- the entry points against their twins
@pytest.mark.parametrize("T,n", P.EDGE_SHAPES)
@pytest.mark.parametrize("A", P.EDGE_ACTIONS)
def test_every_entry_point_equals_its_twin_at_the_tile_edges(T, n, A):
    c = P.case(T, n, A)
    _same(P.run_gather(ops, c, *P.plain(DEV)), P.run_gather(H, c, *P.plain(CPU)), "gather")
    _same(P.run_old(ops, c, *P.plain(DEV)), P.run_old(H, c, *P.plain(CPU)), "old logits")
    for prefill in (None, c["prefill"]):
        dev, host = P.run_aux(ops, c, *P.plain(DEV), prefill=prefill), P.run_aux(H, c, *P.plain(CPU), prefill=prefill)
        for k in host:
            _same(dev[k], host[k], f"aux accumulate={prefill is not None} {k}")
        assert all(torch.isfinite(v).all() for v in dev.values())


@pytest.mark.parametrize("name", list(P.GOLDEN_CASES))
def test_minted_cases_within_the_rule(name):
    c = P.golden_as_case(name)
    got = P.run_aux(ops, c, *P.plain(DEV))
    got["aux_pi_rows"] = P.run_old(ops, dict(c, aux_pi=torch.zeros_like(c["aux_pi"])), *P.plain(DEV))
    assert set(got) == set(P.COMPARED)
    P.assert_within_rule(name, got)


@pytest.mark.parametrize("frame", [(4, 5, 3), (36, 38, 3), (64, 64, 3)], ids=str)
def test_gather_has_the_bits_of_obs_u8_to_f32_on_the_selected_rows(frame):
    c = P.case(9, 4, 2, frame=frame)
    obs, cols = c["aux_obs"].to(DEV), c["cols"].to(DEV)
    got = ops.ppg_aux_gather(obs, cols)
    rows = obs.index_select(1, cols).reshape((-1,) + frame).contiguous()
    assert got.shape == rows.shape and torch.equal(got, ops.obs_u8_to_f32(rows))
    assert torch.equal(got.cpu(), rows.cpu().float() / 255.0)


def test_gather_addresses_past_4_gib():
    """(2, 175,000, 12,288) u8 is 4.3 GB: the last stored rollout of the second step starts 4.3e9 bytes in.  Only the two rows that are
    compared are written; the other two gathered rows are whatever the allocation held."""
    T, R, row = 2, 175_000, 12_288
    obs = torch.empty((T, R, 64, 64, 3), dtype=torch.uint8, device=DEV)
    assert obs.numel() > 1 << 32
    gen = torch.Generator().manual_seed(5)
    first, last = (torch.randint(0, 256, (64, 64, 3), generator=gen, dtype=torch.uint8) for _ in range(2))
    obs[0, 0].copy_(first)
    obs[1, R - 1].copy_(last)
    got = ops.ppg_aux_gather(obs, torch.tensor([0, R - 1], device=DEV))        # flat rows: (0, 0), (0, R-1), (1, 0), (1, R-1)
    assert got.shape == (4, 64, 64, 3)
    assert torch.equal(got[0], ops.obs_u8_to_f32(first.to(DEV)[None])[0]) and torch.equal(got[3], ops.obs_u8_to_f32(last.to(DEV)[None])[0])
    assert torch.equal(got[3].cpu(), last.float() / 255.0)
    del obs, got
    torch.cuda.empty_cache()


@pytest.mark.parametrize("sentinel", GA.SENTINELS, ids=[f"0x{s:08X}" for s in GA.SENTINELS])
def test_kernels_stay_inside_their_tensors_and_exact_workspaces(sentinel, monkeypatch):
    ref = P.every_entry_point(H, *P.plain(CPU))
    out, arena, requested = run_guarded(ops, DEV, monkeypatch, sentinel)
    arena.assert_guards_intact()
    assert requested and max(requested) > 0
    for k, v in ref.items():
        _same(out[k], v, f"sentinel 0x{sentinel:08X}, {k}")


def test_a_non_default_stream_gives_the_same_bits():
    ref = P.every_entry_point(ops, *P.plain(DEV))
    torch.cuda.synchronize()
    s = torch.cuda.Stream(DEV)
    with torch.cuda.stream(s):
        out = P.every_entry_point(ops, *P.plain(DEV))
    s.synchronize()
    for k, v in ref.items():
        _same(out[k], v, k)


@pytest.mark.parametrize("n", [5, 1001, 4100, 626513])
def test_clip_adam_split_is_clip_adam_on_each_range_on_the_device(n):
    c = P.adam_case(n)
    put, out_of = P.plain(DEV)
    head, tail = P.run_plain_adam(ops, c, put, 7), P.run_plain_adam(ops, c, put, 3)
    for n_split in (n, n // 3, n - 1):                            # n_split = n: the bits of clip_adam_
        out = P.run_split(ops, c, put, out_of, n_split, 7, 3)
        for k, (o, h, t) in enumerate(zip(out[:4], head, tail)):
            assert torch.equal(o[:n_split], h[:n_split]) and torch.equal(o[n_split:], t[n_split:]), (n_split, k)
        assert torch.count_nonzero(out[1]).item() == 0
    same = P.run_split(ops, c, put, out_of, n // 2, 7, 7)         # equal steps: clip_adam_ on the whole buffer
    assert all(torch.equal(o, h) for o, h in zip(same[:4], head))
    if n <= 4100:
        for o, t in zip(same, P.run_split(H, c, *P.plain(CPU), n // 2, 7, 7)):
            _same(o, t, "clip_adam_split_")


# ---------------------------------------------------------------------------------------------- the learner under MI355PPO_PPG=fused
def _init_1thread(seed, build):
    n = torch.get_num_threads()
    torch.set_num_threads(1)          # as when minted
    torch.manual_seed(seed)
    out = build()
    torch.set_num_threads(n)
    return out


def _delta_matches(got_now, init_sub, final_sub, what, frac=0.98, rtol=5e-2, atol=2e-5):
    delta, want = got_now - init_sub, final_sub - init_sub
    close = np.isclose(delta, want, rtol=rtol, atol=atol)
    assert close.mean() > frac, f"{what}: only {close.mean():.4f} of sampled parameters moved as the reference's did"


def _fused_learner_after_the_policy_phase(g):
    """tests/test_zz_gpu_new_scripts.py::test_ppg_hip_path_teacher_forced_against_reference_phase up to the auxiliary phase, with its
    checks, on a learner built under MI355PPO_PPG=fused."""
    from cleanrl_amd.agents import PPGAgent
    from cleanrl_amd.learner_ppg import PPGLearner

    T, N = g["rewards"].shape
    envs = SimpleNamespace(single_observation_space=E.Box(0, 255, (64, 64, 3), np.uint8), single_action_space=E.Discrete(15))
    agent = _init_1thread(int(g["init_seed"]), lambda: PPGAgent(envs)).to(DEV)
    args = default_args(num_steps=T, num_minibatches=2, gamma=0.999, clip_coef=0.2, adv_norm_fullbatch=True, e_policy=1,
                        e_auxiliary=2, beta_clone=1.0, num_aux_rollouts=2, n_aux_grad_accum=1, aux_batch_rollouts=N, n_iteration=1,
                        learning_rate=5e-4)
    L = PPGLearner(agent, args, envs.single_observation_space, envs.single_action_space, N, DEV, sample_seed=1)
    assert L.hip and L.ppg_fused and L.adam_eps == 1e-8 and L.obs.dtype == torch.uint8
    stride = int(g["stride"])
    np.testing.assert_allclose(L.flat.params[::stride].cpu().numpy(), g["init_params_sub"], rtol=1e-6, atol=1e-7)
    frames, step_done = g["frames_u8"], g["step_done"]
    F = lambda k: torch.from_numpy(g[k]).to(DEV)      # noqa: E731
    L.observe(0, frames[0], step_done[0])
    for step in range(T):
        L.act(step)
        np.testing.assert_allclose(L.values[step].cpu().numpy(), g["values"][step], rtol=1e-3, atol=2e-4)
        L.actions[step].copy_(F("actions")[step]); L.logprobs[step].copy_(F("logprobs")[step]); L.values[step].copy_(F("values")[step])
        L.store_reward(step, g["rewards"][step])
        L.observe(step + 1, frames[step + 1], step_done[step + 1])
    L.finish_rollout()
    np.testing.assert_allclose(L.returns.cpu().numpy(), g["returns"], rtol=1e-3, atol=3e-4)
    L.returns.copy_(F("returns"))
    L.advantages.copy_(L.returns - L.values)
    np.random.seed(int(g["shuffle_seed"]))
    m = L.update(float(g["lr"]))
    assert abs(m["loss"] - float(g["policy_loss"])) <= 2e-3 * max(1.0, abs(float(g["policy_loss"])))
    _delta_matches(L.flat.params[::stride].cpu().numpy(), g["init_params_sub"], g["policy_params_sub"], "PPG policy phase", frac=0.9)
    assert torch.equal(L.aux_obs[:, :N].cpu(), torch.from_numpy(g["frames_u8"][:T]))
    return L


def test_fused_ppg_teacher_forced_against_reference_phase_and_the_torch_backend_from_the_same_state(monkeypatch, capsys):
    """The fused auxiliary phase at the bars of test_ppg_hip_path_teacher_forced_against_reference_phase; then, from the same state
    (parameters, Adam moments and step counts, the stale gradient, the shuffle stream), the ``torch`` backend: the fused backend's
    deviation of the sampled final parameters from the golden is at most twice the ``torch`` backend's, plus 2e-6 -- a bar against
    the parent's code path.  No device-to-host copy lands between the first auxiliary minibatch and the end of the last."""
    monkeypatch.setenv("MI355PPO_PPG", "fused")
    monkeypatch.delenv("MI355PPO_IMPALA", raising=False)
    g = load_golden("ppg_phase")["ppg_T8_N4"]
    L = _fused_learner_after_the_policy_phase(g)
    stride, f = int(g["stride"]), L.flat
    state = dict(bufs=[t.clone() for t in (f.params, f.grads, f.exp_avg, f.exp_avg_sq)], step=f.step, tail=L._aux_tail_step, upd=L._aux_update,
                 stale=L._stale_grads.clone())
    torch.cuda.synchronize()
    events = []
    real = {n: getattr(torch.Tensor, n) for n in ("cpu", "item", "tolist", "numpy")}
    real_loss, real_step = ops.ppg_aux_fwd_bwd, ops.clip_adam_split_
    for n, fn in real.items():
        monkeypatch.setattr(torch.Tensor, n, lambda self, *a, _n=n, _fn=fn, **kw: (events.append(_n), _fn(self, *a, **kw))[1])
    monkeypatch.setattr(ops, "ppg_aux_fwd_bwd", lambda *a, **kw: (events.append("minibatch"), real_loss(*a, **kw))[1])
    monkeypatch.setattr(ops, "clip_adam_split_", lambda *a, **kw: (real_step(*a, **kw), events.append("stepped"))[0])
    np.random.seed(4)
    aux = L.aux_phase()
    for n, fn in real.items():
        monkeypatch.setattr(torch.Tensor, n, fn)
    monkeypatch.setattr(ops, "ppg_aux_fwd_bwd", real_loss)
    monkeypatch.setattr(ops, "clip_adam_split_", real_step)
    assert "aux epoch 2" in capsys.readouterr().out
    assert events.count("minibatch") == events.count("stepped") == 4
    window = events[events.index("minibatch"):len(events) - events[::-1].index("stepped")]
    assert set(window) == {"minibatch", "stepped"}, f"the auxiliary epochs copied to the host: {window}"
    for key in ("kl_loss", "aux_value_loss", "real_value_loss"):
        ref = float(g[key])
        assert abs(aux[key] - ref) <= 5e-2 * max(abs(ref), 1e-3), (key, aux[key], ref)
    fused_sub = f.params[::stride].cpu().numpy()
    _delta_matches(fused_sub, g["init_params_sub"], g["final_params_sub"], "PPG auxiliary phase (fused)", frac=0.85)
    assert L._aux_update == 0 and L._stale_grads is None and L._aux_tail_step == state["tail"] + 4 and f.step == state["step"] + 4
    L.flat.check_views()
    # the torch backend from the same state
    for t, saved in zip((f.params, f.grads, f.exp_avg, f.exp_avg_sq), state["bufs"]):
        t.copy_(saved)
    f.step, L._aux_tail_step, L._aux_update, L._stale_grads, L.ppg_fused = state["step"], state["tail"], state["upd"], state["stale"], False
    np.random.seed(4)
    aux_torch = L.aux_phase()
    capsys.readouterr()
    torch_sub = f.params[::stride].cpu().numpy()
    dev_fused, dev_torch = np.abs(fused_sub - g["final_params_sub"]).max(), np.abs(torch_sub - g["final_params_sub"]).max()
    print(f"final_params_sub: fused {dev_fused:.3e}, torch {dev_torch:.3e} (bar {2 * dev_torch + 2e-6:.3e}); "
          f"fused vs torch {np.abs(fused_sub - torch_sub).max():.3e}; losses fused {aux} torch {aux_torch}")
    assert dev_fused <= 2 * dev_torch + 2e-6, (dev_fused, dev_torch)


@pytest.mark.parametrize("impala", ["torch", "fused"])
def test_ppg_procgen_script_runs_fused_on_gpu(impala, monkeypatch):
    from cleanrl_amd import ppg_procgen

    monkeypatch.setenv("MI355PPO_PPG", "fused")
    monkeypatch.setenv("MI355PPO_IMPALA", impala)
    L = ppg_procgen.main(["--num-envs", "8", "--num-steps", "16", "--total-timesteps", "512", "--num-minibatches", "4",
                          "--n-iteration", "2", "--e-auxiliary", "1", "--num-aux-rollouts", "4"])
    assert L.hip and L.ppg_fused and L.agent.impala_backend == impala and L.aux_obs.is_cuda and L.aux_obs.dtype == torch.uint8
    assert np.isfinite(L.last_metrics["loss"]) and all(np.isfinite(v) for v in L.last_aux.values()) and len(L.last_aux) == 3
    L.flat.check_views()
