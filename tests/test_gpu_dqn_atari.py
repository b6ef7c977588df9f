"""Atari DQN / C51 kernels (csrc/dqn_atari.hip) on the MI355X: the frame ring against the reference buffer's rules and past 4 GiB,
the wide heads bit-equal to their host twins, deterministic, row by row, inside their outputs and workspaces, unchanged by capture
and replay."""
import pytest
import torch

import bounds_cases as B
import dqn_atari_cases as A
from cleanrl_amd import host_ops as H
from cleanrl_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CPU = torch.device("cpu")


# ================================================================================================== ring
@pytest.mark.parametrize("slots", [1, 2, 7])
@pytest.mark.parametrize("N", [1, 3])
def test_ring_follows_the_reference_buffers_rules_and_the_twin(slots, N):
    steps = A.ring_steps(slots, N, max(slots + 3, 8))
    ring, ref, (bi, ei), out = A.run_ring(ops, DEV, slots, N, steps)
    twin_ring, _, _, twin_out = A.run_ring(H, CPU, slots, N, steps)
    assert torch.equal(ring[0].cpu(), ref.frames_hwc())
    assert all(torch.equal(a.cpu(), b) for a, b in zip(ring + out, twin_ring + twin_out))
    obs, nxt, act, rew, done = ref.get(bi, ei)
    M = len(bi)
    hwc = lambda a: torch.from_numpy(a).permute(0, 2, 3, 1).contiguous()  # noqa: E731
    assert torch.equal(out[0][:M].cpu(), hwc(obs)) and torch.equal(out[0][M:].cpu(), hwc(nxt))
    assert torch.equal(out[1].cpu(), torch.from_numpy(act)) and torch.equal(out[2].cpu(), torch.from_numpy(rew))
    assert torch.equal(out[3].cpu(), torch.from_numpy(done))


def test_a_ring_past_4_gib_is_addressed_with_64_bit_offsets():
    """160,000 slots x 1 env = 4.5 GB: slot 159,999 starts past 2^32 bytes, the smallest size at which a 32-bit byte offset wraps.
    The add lands in slot 159,999 and (next_obs) slot 0, the gather reads both back, the guard in front of the ring and every other
    slot stay untouched.  The kernels index 4-byte pixel words, and word 1.13e9 is still below 2^31: what this size proves is that no BYTE
    offset is formed in 32 bits.  A word offset past 2^31 is checked on the host, where no ring that large is needed
    (test_dqn_atari_twins.py::test_frame_offsets_past_2_31_words_are_64_bit: the same ``da_frame`` both sides compile)."""
    slots, guard = 160_000, 1 << 20
    fb = 84 * 84 * 4
    buf = torch.zeros(guard + slots * fb, dtype=torch.uint8, device=DEV)
    buf[:guard] = 0xA5
    ring = (buf[guard:].view(slots, 1, 84, 84, 4), torch.zeros((slots, 1), dtype=torch.int64, device=DEV),
            torch.zeros((slots, 1), device=DEV), torch.zeros((slots, 1), device=DEV))
    assert (slots - 1) * fb > 1 << 32
    obs, nxt, act, rew, done = (t.to(DEV) for t in A.ring_steps(2, 1, 1, seed=7)[0])
    obs, nxt = obs.clamp(min=1), nxt.clamp(min=1)                            # every byte written is non-zero
    ops.replay_add_u8(ring, slots - 1, obs, nxt, act, rew, done)
    M = 1
    out = (torch.zeros((2 * M, 84, 84, 4), dtype=torch.uint8, device=DEV), torch.zeros(M, dtype=torch.int64, device=DEV),
           torch.zeros(M, device=DEV), torch.zeros(M, device=DEV))
    ops.replay_gather_u8(ring, torch.tensor([slots - 1], device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV), *out)
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], obs[0].permute(1, 2, 0)) and torch.equal(out[0][1], nxt[0].permute(1, 2, 0))
    assert torch.equal(ring[0][slots - 1, 0], obs[0].permute(1, 2, 0)) and torch.equal(ring[0][0, 0], nxt[0].permute(1, 2, 0))
    assert out[1].item() == act.item() and out[2].item() == rew.item() and out[3].item() == done.item()
    assert bool((buf[:guard] == 0xA5).all()) and not bool(ring[0][1:slots - 1].any())


# ================================================================================================== heads
@pytest.mark.parametrize("M,n,na", A.GPU_HEADS)
def test_heads_equal_their_twins_and_repeat(M, n, na):
    c = A.make_head_case(M, n, na)
    want = A.run_heads(H, c, CPU)
    got = {k: v.cpu() for k, v in A.run_heads(ops, c, DEV).items()}
    for k in want:
        assert A.same(got[k], want[k]), (k, (got[k].double() - want[k].double()).abs().max().item())
    again = {k: v.cpu() for k, v in A.run_heads(ops, c, DEV).items()}
    assert all(A.same(again[k], got[k]) for k in got)


def test_heads_within_the_reference_bar_at_the_scripts_shape():
    """M = 32, 18 actions, 51 atoms on the device against float64 autograd: twice the f32 reference's own error plus 2e-6."""
    for na in (1, 51):
        c = A.make_head_case(32, 18, na)
        got = A.run_heads(ops, c, DEV)
        r64, r32 = A.reference_head(c, torch.float64), A.reference_head(c, torch.float32)
        for k in ("q", "aux_a", "aux_b", "scalars", "dh", "dw", "db"):
            ok, err, own = A.within_bar(got[k], r64[k], r32[k])
            print(f"atoms={na} {k}: err {err:.3e} reference's own {own:.3e}")
            assert ok, (k, err, own)
        assert not got["dw"].view(18, na, -1)[17].any() and not got["db"].view(18, na)[17].any()


def test_ties_and_non_finite_inputs_follow_the_twin():
    for na in (1, 5):
        c = A.make_head_case(5, 6, na, tie=True)
        c.h[2, 7] = float("nan")
        c.rewards[1] = float("inf")
        want = A.run_heads(H, c, CPU)
        got = {k: v.cpu() for k, v in A.run_heads(ops, c, DEV).items()}
        assert all(A.same(got[k], want[k]) for k in want)
        assert not (got["act"] == 1).any() and got["act"][2] == 0


@pytest.mark.parametrize("na", [1, 51])
def test_each_row_of_a_batch_is_the_row_alone(na):
    c = A.make_head_case(32, 6, na)
    full = A.run_heads(ops, c, DEV)
    for r in (0, 31):
        one = A.make_head_case(1, 6, na)
        for k in ("h", "h_next", "actions", "rewards", "dones"):
            setattr(one, k, getattr(c, k)[r:r + 1].clone())
        for k in ("w", "b", "wt", "bt"):
            setattr(one, k, getattr(c, k))
        assert torch.equal(full["dh"][r], A.run_heads(ops, one, DEV)["dh"][0] / 32)


@pytest.mark.parametrize("na", [1, 51])
def test_captured_gather_and_head_replay_with_new_indices(na):
    """gather (1 launch) + head update (3 launches) captured once; replays with new indices are bit-identical to eager calls."""
    slots, N, M, n = 7, 3, 32, 6
    ring, _, _, _ = A.run_ring(ops, DEV, slots, N, A.ring_steps(slots, N, 9))
    ring[1].remainder_(n)
    c = A.make_head_case(M, n, na)
    h, hn, w, b, wt, bt = (t.to(DEV) for t in (c.h, c.h_next, c.w, c.b, c.wt, c.bt))
    atoms = None if na == 1 else c.atoms.to(DEV)

    def buffers():
        return dict(frames=torch.zeros((2 * M, 84, 84, 4), dtype=torch.uint8, device=DEV), actions=torch.zeros(M, dtype=torch.int64, device=DEV),
                    rewards=torch.zeros(M, device=DEV), dones=torch.zeros(M, device=DEV), dh=torch.zeros((M, 512), device=DEV),
                    dw=torch.zeros((n * na, 512), device=DEV), db=torch.zeros(n * na, device=DEV), sc=torch.zeros(2, device=DEV))

    def step(o, bi, ei):
        ops.replay_gather_u8(ring, bi, ei, o["frames"], o["actions"], o["rewards"], o["dones"])
        if na == 1:
            ops.dqn_head_td_fwd_bwd(h, hn, w, b, wt, bt, o["actions"], o["rewards"], o["dones"], n, 0.99, o["dh"], o["dw"], o["db"], o["sc"])
        else:
            ops.c51_head_fwd_bwd(h, hn, w, b, wt, bt, atoms, o["actions"], o["rewards"], o["dones"], n, 0.99, -10.0, 10.0, o["dh"], o["dw"],
                                 o["db"], o["sc"])

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
    assert not torch.equal(seen[0], seen[1])


# ================================================================================================== guard bands
@pytest.mark.parametrize("shape", A.GUARD_HEADS, ids=lambda s: "-".join(map(str, s)))
def test_head_kernels_stay_inside_their_outputs_and_workspaces(shape, monkeypatch):
    B.check(A.bounds_head_case(*shape), ops, DEV, monkeypatch)


@pytest.mark.parametrize("shape", A.GUARD_RINGS, ids=lambda s: "-".join(map(str, s)))
def test_ring_kernels_stay_inside_the_ring_and_the_batch(shape, monkeypatch):
    B.check(A.bounds_ring_case(*shape), ops, DEV, monkeypatch)


# ================================================================================================== the learner
@pytest.mark.parametrize("c51", [False, True])
def test_trunk_fc_and_head_together_at_the_scripts_batch(c51):
    """One update at M = 32 through gather, this library's trunk and FC, the head kernels and ``h.backward(dh)``, against float64
    autograd at DESIGN.md section 4's "trunk + FC" row: forward 5e-5, every gradient max(5e-5 x scale, 4 x the error of torch's f32
    backward against float64)."""
    L = A.make_learner(DEV, c51, "fused", M=32, slots=40, n=6, n_atoms=51, fill=True)
    g = torch.Generator().manual_seed(1)
    bi, ei = torch.randint(0, 40, (32,), generator=g).numpy(), torch.zeros(32, dtype=torch.int64).numpy()
    idx = L._stage_indices(bi, ei)
    L.update_kernels(idx[0], idx[1], adam=False)
    torch.cuda.synchronize()
    r64, r32 = A.reference_update(L, bi, ei, torch.float64), A.reference_update(L, bi, ei, torch.float32)
    sc = L._sc.cpu().double()
    ferr = (sc - r64["scalars"]).abs().max().item()
    print(f"c51={c51} forward: err {ferr:.3e}")
    assert ferr <= 5e-5 * max(1.0, r64["scalars"].abs().max().item())
    got, off = L.grads.cpu().double(), 0
    for name, p in L.q_network.named_parameters():
        sl = slice(off, off + p.numel())
        off += p.numel()
        ref = r64["grads"][sl]
        err, own = (got[sl] - ref).abs().max().item(), (r32["grads"][sl].double() - ref).abs().max().item()
        bar = max(5e-5 * ref.abs().max().item(), 4 * own)
        print(f"c51={c51} {name}: err {err:.3e} torch f32 {own:.3e} bar {bar:.3e}")
        assert err <= bar, (name, err, bar)


def test_adam_with_c51s_eps_follows_torch_optim_adam():
    """``clip_adam_`` at ``eps = 0.01 / 32`` over 12 steps against ``torch.optim.Adam``: rtol 1e-5, atol 1e-7 (section 3.15's bar)."""
    L = A.make_learner(DEV, True, "fused", M=32, slots=4, n=6, n_atoms=51)
    assert L.eps == 0.01 / 32
    p = torch.nn.Parameter(L.online.detach().clone())
    opt = torch.optim.Adam([p], lr=L.args.learning_rate, eps=L.eps)
    g = torch.Generator().manual_seed(2)
    for step in range(1, 13):
        grad = (torch.randn(L.online.numel(), generator=g) * 10.0 ** float(torch.randint(-6, 1, (1,), generator=g))).to(DEV)
        L.grads.copy_(grad)
        p.grad = grad.clone()
        L._adam(L._flats, step, L.args.learning_rate, L.eps)
        opt.step()
    torch.cuda.synchronize()
    assert torch.allclose(L.online, p.detach(), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("c51", [False, True])
@pytest.mark.parametrize("backend", ["torch", "fused"])
def test_whole_steps_through_the_learner(c51, backend):
    """store / act (both branches) / train_step / sync_target on the device; ``fused`` through the new entry points and no eager head."""
    import random

    import numpy as np

    random.seed(3), np.random.seed(3)
    L = A.make_learner(DEV, c51, backend, M=4, slots=6)
    seen = []
    real = ops._launch
    ops._launch = lambda name, *a, **k: (seen.append(name), real(name, *a, **k))[1]
    try:
        for t, s in enumerate(A.ring_steps(6, 1, 9)):
            obs, nxt, _, rew, done = (x.numpy() for x in s)
            a = L.act(obs, t, 1.0 if t % 2 == 0 else 0.0)
            assert a.shape == (1,) and 0 <= int(a[0]) < 6
            L.store(obs, nxt, a, rew, done)
            if t >= 3:
                L.train_step()
                if t % 4 == 0:
                    L.sync_target()
    finally:
        ops._launch = real
    m = L.metrics()
    assert np.isfinite(m["loss"]) and np.isfinite(m["q_values"])
    if backend == "fused":
        update = "mi355ppo_c51_head_fwd_bwd_f32" if c51 else "mi355ppo_dqn_head_td_fwd_bwd_f32"
        assert {"mi355ppo_replay_add_u8", "mi355ppo_replay_gather_u8", "mi355ppo_dqn_head_act_f32", update, "mi355ppo_clip_adam_f32"} <= set(seen)
        on, tg = L.flat_params()
        assert torch.isfinite(on).all() and not torch.equal(on, A.make_learner(DEV, c51, backend, M=4, slots=6).flat_params()[0])


# ================================================================================================== whole iterations
@pytest.mark.parametrize("name", ["dqn_atari", "c51_atari", "c51_small"])
def test_goldens_teacher_forced_on_the_hip_path(name, monkeypatch):
    """The minted runs teacher-forced through the fused learner on the device, at the bars DESIGN.md section 4 holds this trunk to
    across Adam steps (the config-B row): loss scalars rtol 1e-3 with an absolute floor of 1e-4 (the q values cross zero, where a
    relative bar means nothing; 1e-4 is 1e-3 of their 0.1 scale at initialisation), and at the first update the pre-Adam flat gradient
    within 1e-3 of its largest element with 1 - cosine <= 1e-5 against the reference's lines in f32."""
    import numpy as np

    import dqn_atari_replay as R
    from cleanrl_amd.learner_dqn_atari import AtariDQNLearner

    first = {}
    orig = AtariDQNLearner.update_kernels

    def spy(self, bi, ei, adam=True, aux=None):
        if not first:
            want = A.reference_update(self, bi.cpu().numpy(), ei.cpu().numpy(), torch.float32)["grads"]
            orig(self, bi, ei, adam=False)
            first["got"], first["want"] = self.grads.detach().cpu().clone(), want
        return orig(self, bi, ei, adam=adam, aux=aux)

    monkeypatch.setattr(AtariDQNLearner, "update_kernels", spy)
    rec = R.replay(name, "fused", DEV)
    g = R.golden_case(name)
    got, want = first["got"].double(), first["want"].double()
    worst = ((got - want).abs().max() / want.abs().max()).item()
    cos = torch.nn.functional.cosine_similarity(got, want, dim=0).item()
    print(f"{name}: first update max|dg|/absmax {worst:.2e}, 1-cosine {1 - cos:.2e}")
    assert worst <= 1e-3 and 1 - cos <= 1e-5
    for k in R.SCALARS:
        m = ~np.isnan(g[k])
        dev = np.abs(rec[k][m] - g[k][m]).max()
        print(f"{name}: {k} max deviation {dev:.3e} (reference's own f32-vs-f64 {R.sensitivity(name)[k]:.3e})")
        assert np.allclose(rec[k][m], g[k][m], rtol=1e-3, atol=1e-4), k
        assert np.array_equal(np.isnan(rec[k]), np.isnan(g[k]))
