"""Discrete-SAC kernels (csrc/sac_atari.hip) on the MI355X: the two frame rings against the plain buffer's rules, the heads bit-equal
to their host twins, deterministic, row by row, inside their outputs and workspaces, unchanged by capture and replay; the learner's
update against float64 autograd, whole steps on both backends, the minted runs teacher-forced and the script itself."""
import numpy as np
import pytest
import torch

import bounds_cases as B
import sac_atari_cases as S
from cleanrl_amd import host_ops as H
from cleanrl_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CPU = torch.device("cpu")


def _cpu(d):
    return {k: v.cpu() for k, v in d.items()}


# ================================================================================================== rings
@pytest.mark.parametrize("slots", [1, 2, 7])
@pytest.mark.parametrize("N", [1, 3])
def test_rings_follow_the_plain_buffers_rules_and_the_twin(slots, N):
    steps = S.ring_steps(slots, N, max(slots + 3, 8))
    ring, ref, idx, out = S.run_ring(ops, DEV, slots, N, steps)
    twin_ring, _, _, twin_out = S.run_ring(H, CPU, slots, N, steps)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(ring + out, twin_ring + twin_out))
    S.check_ring_against_model(ring, ref, idx, out)


# ================================================================================================== heads
@pytest.mark.parametrize("M,n", S.GPU_HEADS)
def test_heads_equal_their_twins_and_repeat(M, n):
    c = S.make_head_case(M, n)
    want = S.run_heads(H, c, CPU)
    got = _cpu(S.run_heads(ops, c, DEV))
    for k in want:
        assert S.same(got[k], want[k]), (k, (got[k].double() - want[k].double()).abs().max().item())
    again = _cpu(S.run_heads(ops, c, DEV))
    assert all(S.same(again[k], got[k]) for k in got)


def test_heads_within_the_reference_bar_at_the_scripts_shape():
    """M = 64, 18 actions on the device against float64 autograd: twice the f32 reference's own error plus 2e-6."""
    c = S.make_head_case(64, 18)
    got = S.run_heads(ops, c, DEV)
    for ref, keys in ((S.reference_critic, S.CRITIC_OUTS), (S.reference_actor, S.ACTOR_OUTS)):
        r64, r32 = ref(c, torch.float64), ref(c, torch.float32)
        for k in keys:
            ok, err, own = S.within_bar(got[k], r64[k], r32[k])
            print(f"{k}: err {err:.3e} reference's own {own:.3e}")
            assert ok, (k, err, own)
    assert not got["dw1"][17].any() and not got["dw2"][17].any() and got["db1"][17] == 0 and got["db2"][17] == 0
    assert got["probs"][63, 1] == 0 and all(torch.isfinite(got[k]).all() for k in S.HEAD_OUTS if k != "act")


def test_non_finite_inputs_follow_the_twin():
    for key in ("h_q1", "h_pi_next", "h_pi"):
        c = S.make_head_case(5, 6)
        getattr(c, key)[2, 7] = float("nan")
        c.rewards[1] = float("inf")
        want = S.run_heads(H, c, CPU)
        got = _cpu(S.run_heads(ops, c, DEV))
        assert all(S.same(got[k], want[k]) for k in want), key
        assert got["y"][1] == float("inf") and any(got[k].isnan().any() for k in ("dh1", "V", "dh"))


def test_each_row_of_a_batch_is_the_row_alone():
    """Row r of a 64-row batch through both updates equals the row alone with its gradients scaled by 1 / 64 (a power of two: exact)."""
    c = S.make_head_case(64, 6)
    full = S.run_heads(ops, c, DEV)
    for r in (0, 63):
        one = S.make_head_case(1, 6)
        for k in S.H_KEYS + ("actions", "rewards", "dones", "noise"):
            setattr(one, k, getattr(c, k)[r:r + 1].clone())
        for k in S.NETS:
            setattr(one, "w_" + k, getattr(c, "w_" + k))
            setattr(one, "b_" + k, getattr(c, "b_" + k))
        alone = S.run_heads(ops, one, DEV)
        for k in ("dh1", "dh2", "dh"):
            assert torch.equal(full[k][r], alone[k][0] / 64), (k, r)
        for k in ("V", "y", "e_rows", "act"):
            assert torch.equal(full[k][r], alone[k][0]), (k, r)


def test_captured_gather_and_head_updates_replay_with_new_indices():
    """gather (1 launch) + critic update (4) + actor update (3) captured once; replays with new indices are bit-identical to eager calls."""
    slots, N, M, n = 7, 3, 64, 6
    ring, _, _, _ = S.run_ring(ops, DEV, slots, N, S.ring_steps(slots, N, 9))
    ring[2].remainder_(n)
    c = S.make_head_case(M, n)
    T = {k: getattr(c, k).to(DEV) for k in S.H_KEYS + ("alpha",)}
    hd = {k: (getattr(c, "w_" + k).to(DEV), getattr(c, "b_" + k).to(DEV)) for k in S.NETS}

    def buffers():
        z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=DEV)  # noqa: E731
        return dict(frames=z(2 * M, 84, 84, 4, dtype=torch.uint8), actions=z(M, dtype=torch.int64), rewards=z(M), dones=z(M), dh1=z(M, 512),
                    dh2=z(M, 512), dw1=z(n, 512), db1=z(n), dw2=z(n, 512), db2=z(n), sc=z(4), V=z(M), y=z(M), dh=z(M, 512), dw=z(n, 512), db=z(n),
                    er=z(M), al=z(1))

    def step(o, bi, ei):
        ops.replay_gather2_u8(ring, bi, ei, o["frames"], o["actions"], o["rewards"], o["dones"])
        ops.sacd_critic_fwd_bwd(tuple(T[k] for k in S.H_KEYS[:5]), tuple(hd[k] for k in S.NETS), o["actions"], o["rewards"], o["dones"], T["alpha"],
                                c.gamma, (o["dh1"], o["dh2"]), ((o["dw1"], o["db1"]), (o["dw2"], o["db2"])), o["sc"], o["V"], o["y"])
        ops.sacd_actor_fwd_bwd((T["h_pi"], T["h_q1"], T["h_q2"]), (hd["pi"], hd["q1"], hd["q2"]), T["alpha"], c.target_entropy, o["dh"], o["dw"],
                               o["db"], o["er"], o["al"])

    g = torch.Generator().manual_seed(11)
    draws = [(torch.randint(0, slots, (M,), generator=g), torch.randint(0, N, (M,), generator=g)) for _ in range(3)]
    bi, ei = (t.to(DEV).clone() for t in draws[0])
    G, E = buffers(), buffers()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(G, bi, ei)                                                      # warm-up outside the capture (workspace allocation)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(G, bi, ei)
    seen = []
    for b_, e_ in draws:
        bi.copy_(b_), ei.copy_(e_)
        graph.replay()
        step(E, b_.to(DEV), e_.to(DEV))
        torch.cuda.synchronize()
        for k in G:
            assert torch.equal(G[k], E[k]), k
        seen.append(E["sc"].clone())
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])


# ================================================================================================== guard bands
@pytest.mark.parametrize("shape", S.GUARD_HEADS, ids=lambda s: "-".join(map(str, s)))
def test_head_kernels_stay_inside_their_outputs_and_workspaces(shape, monkeypatch):
    B.check(S.bounds_head_case(*shape), ops, DEV, monkeypatch)


@pytest.mark.parametrize("shape", S.GUARD_RINGS, ids=lambda s: "-".join(map(str, s)))
def test_ring_kernels_stay_inside_the_rings_and_the_batch(shape, monkeypatch):
    B.check(S.bounds_ring_case(*shape), ops, DEV, monkeypatch)


# ================================================================================================== the learner
def test_trunks_fc_and_heads_together_at_the_scripts_batch():
    """One update at M = 64 through gather, this library's trunks and FCs, the head kernels and ``h.backward(dh)``, against float64
    autograd at DESIGN.md section 4's "trunk + FC" row: forward 5e-5, every gradient max(5e-5 x its scale, 4 x the error of torch's
    f32 backward against float64); the critic segment and the actor segment each on their own."""
    L = S.make_learner(DEV, "fused", M=64, slots=72, n=6, fill=True)
    g = torch.Generator().manual_seed(1)
    bi, ei = torch.randint(0, 72, (64,), generator=g).numpy(), torch.zeros(64, dtype=torch.int64).numpy()
    idx = L._stage_indices(bi, ei)
    L.update_kernels(idx[0], idx[1], adam=False)
    torch.cuda.synchronize()
    r64, r32 = S.reference_update(L, bi, ei, torch.float64), S.reference_update(L, bi, ei, torch.float32)
    sc = torch.cat([L._qsc, L._asc]).cpu().double()
    ferr = (sc - r64["scalars"]).abs().max().item()
    print(f"forward: err {ferr:.3e} scalars {sc.tolist()}")
    assert ferr <= 5e-5 * max(1.0, r64["scalars"].abs().max().item())
    got = S.learner_grads(L)
    for seg in ("critic_grads", "actor_grads"):
        for name, ref in r64[seg].items():
            err, own = (got[name].double() - ref).abs().max().item(), (r32[seg][name].double() - ref).abs().max().item()
            bar = max(5e-5 * ref.abs().max().item(), 4 * own)
            print(f"{name}: err {err:.3e} torch f32 {own:.3e} bar {bar:.3e}")
            assert err <= bar, (name, err, bar)


@pytest.mark.parametrize("backend", ["torch", "fused"])
def test_whole_steps_through_the_learner(backend):
    """store / act (both branches) / train_step / sync_target on the device; ``fused`` through the new entry points and no eager head."""
    import random

    random.seed(3), np.random.seed(3), torch.manual_seed(3)
    L = S.make_learner(DEV, backend, M=4, slots=6)
    L.args.learning_starts = 3
    before = [f.clone() for f in L.flat_params()]
    seen = []
    real = ops._launch
    ops._launch = lambda name, *a, **k: (seen.append(name), real(name, *a, **k))[1]
    try:
        for t, s in enumerate(S.ring_steps(6, 1, 9)):
            obs, nxt, _, rew, done = (x.numpy() for x in s)
            a = L.act(obs, t)
            assert a.shape == (1,) and 0 <= int(a[0]) < 6
            L.store(obs, nxt, a, rew, done)
            if t >= 3:
                L.train_step()
                if t % 4 == 0:
                    L.sync_target()
    finally:
        ops._launch = real
    m = L.metrics()
    assert set(m) == {"qf1_values", "qf2_values", "qf1_loss", "qf2_loss", "qf_loss", "actor_loss", "alpha", "alpha_loss"}
    assert all(np.isfinite(v) for v in m.values())
    after = L.flat_params()
    assert all(torch.isfinite(f).all() and not torch.equal(f, b) for f, b in zip(after, before))
    if backend == "fused":
        assert {"mi355ppo_replay_add2_u8", "mi355ppo_replay_gather2_u8", "mi355ppo_sacd_head_act_f32", "mi355ppo_sacd_critic_fwd_bwd_f32",
                "mi355ppo_sacd_actor_fwd_bwd_f32", "mi355ppo_sac_alpha_f32", "mi355ppo_clip_adam_f32"} <= set(seen)
        assert not any("heads_" in s or "dqn_head" in s for s in seen)
    else:
        assert not any("sacd" in s or "replay" in s for s in seen)


# ================================================================================================== whole iterations
@pytest.mark.parametrize("name", ["sac_atari", "sac_atari_fixed", "sac_atari_polyak"])
def test_goldens_teacher_forced_on_the_hip_path(name, monkeypatch):
    """The minted runs teacher-forced through the fused learner on the device, at the bars DESIGN.md section 4 holds this trunk to
    across Adam steps: logged scalars and ``alpha`` rtol 1e-3 with an absolute floor of 1e-4, and at the first update the pre-Adam flat
    gradient of each segment within 1e-3 of its largest element with 1 - cosine <= 1e-5 against the reference's lines in f32."""
    import sac_atari_replay as R
    from cleanrl_amd.learner_sac_atari import SACAtariLearner

    first = {}
    orig = SACAtariLearner.update_kernels

    def spy(self, bi, ei, adam=True, aux=None):
        if not first:
            want = S.reference_update(self, bi.cpu().numpy(), ei.cpu().numpy(), torch.float32)
            orig(self, bi, ei, adam=False)
            got = S.learner_grads(self)
            for seg in ("critic_grads", "actor_grads"):
                first[seg] = (torch.cat([got[k].reshape(-1) for k in want[seg]]).double(), torch.cat([v.reshape(-1) for v in want[seg].values()]).double())
        return orig(self, bi, ei, adam=adam, aux=aux)

    monkeypatch.setattr(SACAtariLearner, "update_kernels", spy)
    rec = R.replay(name, "fused", DEV)
    g = R.golden_case(name)
    bad = []
    for seg, (got, want) in first.items():
        worst = ((got - want).abs().max() / want.abs().max()).item()
        cos = torch.nn.functional.cosine_similarity(got, want, dim=0).item()
        print(f"{name}: first update {seg} max|dg|/absmax {worst:.2e}, 1-cosine {1 - cos:.2e}")
        if not (worst <= 1e-3 and 1 - cos <= 1e-5):
            bad.append((seg, worst, 1 - cos))
    for k in R.SCALARS:
        m = ~np.isnan(g[k])
        assert np.array_equal(np.isnan(rec[k]), np.isnan(g[k]))
        if not m.any():
            continue
        dev = np.abs(rec[k][m] - g[k][m]).max()
        print(f"{name}: {k} max deviation {dev:.3e} (reference's own f32-vs-f64 {R.sensitivity(name)[k]:.3e})")
        if not np.allclose(rec[k][m], g[k][m], rtol=1e-3, atol=1e-4):
            bad.append((k, dev))
    assert not bad, bad


@pytest.mark.parametrize("backend", ["torch", "fused"])
def test_the_script_runs_on_the_device(backend, tmp_path, monkeypatch, capsys):
    from cleanrl_amd import sac_atari

    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("MI355PPO_OFFPOLICY", backend)
    monkeypatch.setenv("MI355PPO_STANDIN_HORIZON", "10")
    L = sac_atari.main(["--total-timesteps", "102", "--learning-starts", "30", "--buffer-size", "16", "--batch-size", "4", "--update-frequency", "4",
                        "--target-network-frequency", "8"])
    out = capsys.readouterr().out
    assert "SPS:" in out and "episodic_return" in out
    assert L.device.type == "cuda" and L.backend == backend and L.q_step == L.actor_step == L.alpha_step == len(range(32, 102, 4))
    assert all(np.isfinite(v) for v in L.metrics().values())
    assert all(torch.isfinite(f).all() for f in L.flat_params())
