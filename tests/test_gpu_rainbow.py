"""Rainbow kernels (csrc/rainbow.hip) on the MI355X: the prioritized buffer against the reference's recorded buffer and against its
host twin, two frame rings past 4 GiB, the noise composition as torch's bits, everything inside its buffers, unchanged by capture and
replay."""
import numpy as np
import pytest
import torch

import bounds_cases as B
import rainbow_cases as R
import rainbow_replay as P
from cleanrl_amd import host_ops as H
from cleanrl_amd import ops

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CPU = torch.device("cpu")


def _device_fixture_ids():
    d = R.per_fixture()
    return [k for k in range(int(d["n_cases"])) if int(d[f"c{k}_meta"][0]) in (1, 2, 3, 5, 37)]


# ================================================================================================== the buffer
@pytest.mark.parametrize("k", _device_fixture_ids())
def test_buffer_follows_the_references_recorded_buffer(k):
    """Capacities 1, 2, 3, 5, 37 x batches 1, 5, 32 with duplicates: from the reference's own uploaded tree the sampled indices are the
    reference's exactly and the weights within 4 ulp; after an add or an update the leaves are within 1 ulp, the inner nodes what the
    leaves determine, max_priority and size equal."""
    c = R.fixture_case(R.per_fixture(), k)
    adds, samples, updates = R.replay_fixture_case(ops, DEV, c)
    assert adds >= c.slots + 3 and samples == 5 and updates == 5


# leaves at one depth and at two, no level at all, a batch wider than the workgroup on a tree of 11 levels
@pytest.mark.parametrize("slots,batch", [(1, 1), (2, 5), (3, 32), (5, 5), (37, 32), (37, 1), (600, 1024)])
def test_buffer_equals_its_twin_and_repeats(slots, batch):
    T = R.per_script(slots, batch)
    Td = {k: v.to(DEV) for k, v in T.items()}
    got = R.run_per(ops, DEV, slots, batch, Td)
    want = R.run_per(H, CPU, slots, batch, T)
    R.check_ring_contents(got, T, slots)
    R.check_per_against(got, want, slots, f"slots={slots} B={batch}")
    again = R.run_per(ops, DEV, slots, batch, Td)
    assert all(R.same_bits(again[k], got[k]) for k in got)


def test_duplicate_indices_keep_the_highest_batch_position():
    slots = 5
    buf = ops.rainbow_new_buffer(slots, DEV)
    ops.rainbow_per_update(buf, torch.tensor([3, 1, 3, 3, 1], device=DEV), torch.tensor([0.5, 0.25, 2.0, 0.125, 4.0], device=DEV), 0.5, 0.0)
    assert torch.equal(buf[5][slots - 1:].cpu(), torch.tensor([0.0, 2.0, 0.0, 0.125 ** 0.5, 0.0])) and buf[6][0].item() == 4.0
    assert R.same_bits(buf[5], R.rebuild(buf[5], slots))


def test_two_rings_past_4_gib_are_addressed_with_64_bit_offsets():
    """160,000 slots = 4.5 GB per ring: slot 159,999 starts past 2^32 bytes, the smallest size at which a 32-bit byte offset wraps.
    One add lands in slot 159,999 of both rings, the gather reads both back, the guard in front of each ring and every other slot
    stay untouched.  A WORD offset past 2^31 is checked on the host (test_rainbow_twins.py: the same ``da_frame`` both sides compile)."""
    slots, guard = 160_000, 1 << 20
    fb = 84 * 84 * 4
    assert (slots - 1) * fb > 1 << 32
    bufs = [torch.zeros(guard + slots * fb, dtype=torch.uint8, device=DEV) for _ in range(2)]
    for b in bufs:
        b[:guard] = 0xA5
    small = ops.rainbow_new_buffer(1, DEV)
    buf = (bufs[0][guard:].view(slots, 84, 84, 4), bufs[1][guard:].view(slots, 84, 84, 4), torch.zeros(slots, dtype=torch.int64, device=DEV),
           torch.zeros(slots, device=DEV), torch.zeros(slots, device=DEV), torch.zeros(2 * slots - 1, device=DEV), small[6], small[7])
    T = {k: v.to(DEV) for k, v in R.per_script(1, 1, seed=7).items()}
    obs, nxt = T["obs"][0], T["next_obs"][0]
    ops.rainbow_per_add_u8(buf, slots - 1, obs, nxt, T["action"][0], T["reward"][0], T["done"][0], 0.5)
    out = (torch.zeros((2, 84, 84, 4), dtype=torch.uint8, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, device=DEV),
           torch.zeros(1, device=DEV))
    ops.rainbow_per_gather_u8(buf, torch.tensor([slots - 1], device=DEV), *out)
    torch.cuda.synchronize()
    assert torch.equal(out[0][0], R.hwc(obs)) and torch.equal(out[0][1], R.hwc(nxt)) and not torch.equal(out[0][0], out[0][1])
    assert torch.equal(buf[0][slots - 1], R.hwc(obs)) and torch.equal(buf[1][slots - 1], R.hwc(nxt))
    assert out[1].item() == T["action"][0].item() and out[2].item() == T["reward"][0].item() and out[3].item() == T["done"][0].item()
    for b, ring in zip(bufs, buf[:2]):
        assert bool((b[:guard] == 0xA5).all()) and not bool(ring[:slots - 1].any())
    tree = buf[5].cpu()
    assert tree[2 * slots - 2].item() == 1.0 and tree.sum().item() == (2 * slots - 1).bit_length() and buf[7].item() == 1
    assert R.same_bits(tree, R.rebuild(tree, slots))


@pytest.mark.parametrize("slots,batch,alpha", P.LOCKSTEP)
def test_device_buffer_keeps_step_with_the_host_buffer(slots, batch, alpha):
    """``DevicePrioritizedReplay`` on the device beside ``HostPrioritizedReplay``: n-step adds, samples from one ``np.random`` seed,
    updates, a settable beta."""
    P.lockstep(DEV, slots, batch, alpha)


# ================================================================================================== the noisy layers
@pytest.mark.parametrize("n,na", R.NOISY_SHAPES)
def test_compose_and_grad_are_torchs_bits_and_the_twins(n, na):
    net = R.make_network(n, na)
    params, eps = R.noisy_flat(net)
    g = torch.randn(eps.numel(), generator=torch.Generator().manual_seed(3))
    want_eff, want_grads = R.reference_noisy(net, g)
    T = dict(params=params, eps=eps, g=g)
    twin = R.run_noisy(H, CPU, n, na, T)
    got = R.run_noisy(ops, DEV, n, na, {k: v.to(DEV) for k, v in T.items()})
    for k, want in (("effective", want_eff), ("grads", want_grads)):
        assert R.same_bits(got[k], want) and R.same_bits(got[k], twin[k]), k


# ================================================================================================== guard bands
@pytest.mark.parametrize("shape", R.GUARD_PER, ids=lambda s: "-".join(map(str, s)))
def test_buffer_kernels_stay_inside_their_buffers(shape, monkeypatch):
    B.check(R.bounds_per_case(*shape), ops, DEV, monkeypatch)


@pytest.mark.parametrize("shape", R.GUARD_NOISY, ids=lambda s: "-".join(map(str, s)))
def test_noisy_kernels_stay_inside_their_buffers(shape, monkeypatch):
    B.check(R.bounds_noisy_case(*shape), ops, DEV, monkeypatch)


# ================================================================================================== capture
def test_captured_sample_gather_update_replays_with_new_draws_and_beta():
    """sample + gather + update (three launches on one stream: a single chain) captured once, the warm-up outside the capture.  Replays
    read new uniforms and a new beta from device memory and walk the tree the previous replay's update left; each is bit-identical to
    the same calls made eagerly on a second buffer."""
    slots, M = 37, 32
    T = {k: v.to(DEV) for k, v in R.per_script(slots, M).items()}

    def filled():
        buf = ops.rainbow_new_buffer(slots, DEV)
        for s in range(slots):
            ops.rainbow_per_add_u8(buf, s, T["obs"][s], T["next_obs"][s], T["action"][s], T["reward"][s], T["done"][s], 0.6)
        return buf

    def outputs():
        return dict(idx=torch.zeros(M, dtype=torch.int64, device=DEV), w=torch.zeros(M, device=DEV),
                    frames=torch.zeros((2 * M, 84, 84, 4), dtype=torch.uint8, device=DEV), actions=torch.zeros(M, dtype=torch.int64, device=DEV),
                    rewards=torch.zeros(M, device=DEV), dones=torch.zeros(M, device=DEV))

    def step(buf, o, u, loss):
        ops.rainbow_per_sample(buf, u, o["idx"], o["w"])
        ops.rainbow_per_gather_u8(buf, o["idx"], o["frames"], o["actions"], o["rewards"], o["dones"])
        ops.rainbow_per_update(buf, o["idx"], loss, 0.6, R.EPS)

    gbuf, ebuf, G, E = filled(), filled(), outputs(), outputs()
    u, loss = T["u"][0].clone(), T["loss"][0].clone()
    warm = filled()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(warm, outputs(), u, loss)                                        # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(gbuf, G, u, loss)
    seen = []
    for k, beta in enumerate((0.4, 0.55, 1.0)):
        u.copy_(T["u"][k]), loss.copy_(T["loss"][k])
        gbuf[6][1:2].fill_(beta), ebuf[6][1:2].fill_(beta)
        graph.replay()
        step(ebuf, E, T["u"][k], T["loss"][k])
        torch.cuda.synchronize()
        for name in G:
            assert R.same_bits(G[name], E[name]), (k, name)
        assert all(R.same_bits(a, b) for a, b in zip(gbuf, ebuf)), k
        seen.append((E["idx"].clone(), E["w"].clone()))
    assert not torch.equal(seen[0][0], seen[1][0]) and not torch.equal(seen[1][1], seen[2][1])


# ================================================================================================== the dueling distributional head
@pytest.mark.parametrize("M,n,na", R.GPU_HEADS)
def test_heads_equal_their_twins_and_repeat(M, n, na):
    c = R.make_head_case(M, n, na)
    want = R.run_heads(H, c, CPU)
    got = {k: v.cpu() for k, v in R.run_heads(ops, c, DEV).items()}
    for k in want:
        assert R.same(got[k], want[k]) if want[k].is_floating_point() else torch.equal(got[k], want[k]), (
            k, (got[k].double() - want[k].double()).abs().max().item())
    again = {k: v.cpu() for k, v in R.run_heads(ops, c, DEV).items()}
    assert all(R.same_bits(again[k], got[k]) for k in got)


def test_heads_within_the_reference_bar_at_the_scripts_shape():
    """M = 32, 18 actions, 51 atoms on the device against float64 autograd: twice the f32 reference's own error plus 2e-6."""
    c = R.make_head_case(32, 18, 51)
    got = {k: v.cpu() for k, v in R.run_heads(ops, c, DEV).items()}
    r64, r32 = R.reference_head(c, torch.float64), R.reference_head(c, torch.float32)
    assert torch.equal(got["best"], r64["best"])
    for k in ("q", "next_pmfs", "target_pmfs", "loss_per_sample", "scalars", "dh", "dw", "db"):
        ok, err, own = R.within_bar(got[k], r64[k], r32[k])
        print(f"{k}: err {err:.3e} reference's own {own:.3e}")
        assert ok, (k, err, own)


def test_head_ties_and_non_finite_inputs_follow_the_twin():
    c = R.make_head_case(5, 6, 5, tie=True)
    c.h[2, 7] = float("nan")
    c.rewards[1] = float("inf")
    want = R.run_heads(H, c, CPU)
    got = {k: v.cpu() for k, v in R.run_heads(ops, c, DEV).items()}
    assert all(R.same(got[k], want[k]) if want[k].is_floating_point() else torch.equal(got[k], want[k]) for k in want)
    assert not (got["act"] == 1).any() and got["act"][2] == 0


def test_each_row_of_a_batch_is_the_row_alone_times_its_weight_over_m():
    c = R.make_head_case(32, 6, 51)
    full = {k: v.cpu() for k, v in R.run_heads(ops, c, DEV).items()}
    for r in (0, 31):
        one = R.make_head_case(1, 6, 51)
        for k in ("h", "h_next", "h_next_target", "actions", "rewards", "dones"):
            setattr(one, k, getattr(c, k)[r:r + 1].clone())
        for k in ("w", "b", "wt", "bt"):
            setattr(one, k, getattr(c, k))
        one.weights = torch.ones(1)
        alone = {k: v.cpu() for k, v in R.run_heads(ops, one, DEV).items()}
        assert R.same_bits(full["loss_per_sample"][r], alone["loss_per_sample"][0])
        scale = (c.weights[r] * torch.tensor(1 / 32, dtype=torch.float32)).item()
        assert torch.allclose(full["dh"][r], alone["dh"][0] * scale, rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("shape", R.GUARD_HEADS, ids=lambda s: "-".join(map(str, s)))
def test_head_kernels_stay_inside_their_outputs_and_workspaces(shape, monkeypatch):
    B.check(R.bounds_head_case(*shape), ops, DEV, monkeypatch)


def test_captured_update_chain_with_the_head_replays_bit_identically():
    """sample + gather + head + priority update (1 + 1 + 3 + 1 launches on one stream: a single chain, nothing read back) captured
    once; replays with new uniforms and a new beta, both read from device memory, are bit-identical to eager calls on a second buffer."""
    slots, M, n, na = 37, 32, 6, 51
    T = {k: v.to(DEV) for k, v in R.per_script(slots, M).items()}
    T["action"] = T["action"] % n
    c = R.make_head_case(M, n, na)
    h, hn, hnt, w, b, wt, bt, support = (t.to(DEV) for t in (c.h, c.h_next, c.h_next_target, c.w, c.b, c.wt, c.bt, c.support))

    def filled():
        buf = ops.rainbow_new_buffer(slots, DEV)
        for s in range(slots):
            ops.rainbow_per_add_u8(buf, s, T["obs"][s], T["next_obs"][s], T["action"][s], T["reward"][s], T["done"][s], 0.5)
        return buf

    def outputs():
        z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=DEV)  # noqa: E731
        return dict(idx=z(M, torch.int64), w=z(M), frames=z((2 * M, 84, 84, 4), torch.uint8), actions=z(M, torch.int64), rewards=z(M), dones=z(M),
                    dh=z((M, 1024)), dw=z(((n + 1) * na, 512)), db=z((n + 1) * na), sc=z(2), lps=z(M))

    def step(buf, o, u):
        ops.rainbow_per_sample(buf, u, o["idx"], o["w"])
        ops.rainbow_per_gather_u8(buf, o["idx"], o["frames"], o["actions"], o["rewards"], o["dones"])
        ops.rainbow_head_fwd_bwd(h, hn, hnt, w, b, wt, bt, support, o["actions"], o["rewards"], o["dones"], o["w"], n, 0.99 ** 3, -10.0, 10.0,
                                 o["dh"], o["dw"], o["db"], o["sc"], o["lps"])
        ops.rainbow_per_update(buf, o["idx"], o["lps"], 0.5, R.EPS)

    gbuf, ebuf, G, E = filled(), filled(), outputs(), outputs()
    u = T["u"][0].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(filled(), outputs(), u)                                         # warm-up outside the capture (workspace allocation)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(gbuf, G, u)
    seen = []
    for k, beta in enumerate((0.4, 0.55, 1.0)):
        u.copy_(T["u"][k])
        gbuf[6][1:2].fill_(beta), ebuf[6][1:2].fill_(beta)
        graph.replay()
        step(ebuf, E, T["u"][k])
        torch.cuda.synchronize()
        for name in G:
            assert R.same_bits(G[name], E[name]), (k, name)
        assert all(R.same_bits(a_, b_) for a_, b_ in zip(gbuf, ebuf)), k
        seen.append(E["sc"].clone())
    assert not torch.equal(seen[0], seen[1])


# ================================================================================================== trunk + Linear(3136, 1024) + head
def _reference_update(net, tgt, batch, weights, n_step, gamma, dtype):
    """rainbow_atari.py's training lines on copies of the two networks in ``dtype`` -> (scalars, gradient per parameter name)."""
    import copy

    q, t = copy.deepcopy(net).to("cpu", dtype), copy.deepcopy(tgt).to("cpu", dtype)
    obs, nxt, actions, rewards, dones = batch
    obs, nxt, rewards, dones, weights = (x.to(dtype) for x in (obs, nxt, rewards, dones, weights))
    M, na = len(obs), q.n_atoms
    with torch.no_grad():
        next_dist, support = t(nxt), t.support
        best_actions = torch.argmax(torch.sum(q(nxt) * support, dim=2), dim=1)
        next_pmfs = next_dist[torch.arange(M), best_actions]
        next_atoms = rewards.reshape(-1, 1) + gamma**n_step * support * (1 - dones.reshape(-1, 1))
        tz = next_atoms.clamp(q.v_min, q.v_max)
        b = (tz - q.v_min) / q.delta_z
        l, u = b.floor().clamp(0, na - 1), b.ceil().clamp(0, na - 1)
        d_m_l, d_m_u = (u + (l == b).to(dtype) - b) * next_pmfs, (b - l) * next_pmfs
        target_pmfs = torch.zeros_like(next_pmfs)
        for i in range(M):
            target_pmfs[i].index_add_(0, l[i].long(), d_m_l[i])
            target_pmfs[i].index_add_(0, u[i].long(), d_m_u[i])
    pred_dist = q(obs)[torch.arange(M), actions]
    loss_per_sample = -(target_pmfs * torch.log(pred_dist.clamp(min=1e-5, max=1 - 1e-5))).sum(dim=1)
    loss = (loss_per_sample * weights).mean()
    loss.backward()
    scalars = torch.stack([loss.detach(), (pred_dist * q.support).sum(dim=1).mean().detach()])
    return scalars, {name: p.grad for name, p in q.named_parameters()}, best_actions


def test_one_update_through_gather_trunk_fc_1024_head_and_backward_against_float64():
    """M = 32 through the device buffer's sample and gather, this library's trunk, BOTH streams' hidden layers as ONE
    ``Linear(3136, 1024)`` on the composed effective weights (``cnn.LinearReLUHwcFn``), the head kernels, ``h.backward(dh)`` and the
    noise gradient kernel, against float64 autograd of the reference's lines at DESIGN.md section 4's "trunk + FC" row: forward 5e-5,
    every parameter gradient max(5e-5 x scale, 4 x the error of torch's f32 backward against float64)."""
    from cleanrl_amd import cnn
    from cleanrl_amd.rainbow_replay import DevicePrioritizedReplay

    M, n, na, slots, n_step, gamma = 32, 6, 51, 40, 3, 0.99
    net, tgt = R.make_network(n, na).to(DEV), R.make_network(n, na, seed=1).to(DEV)
    rb = DevicePrioritizedReplay(slots, DEV, 1, gamma, 0.5)
    g = torch.Generator().manual_seed(5)
    for t in range(slots):
        f = torch.randint(0, 256, (2, 1, 4, 84, 84), dtype=torch.uint8, generator=g).numpy()
        rb.add(f[0], np.array([t % n]), np.array([float(torch.randn((), generator=g))]), f[1], np.array([t % 5 == 4]))
    np.random.seed(3)
    o = rb.sample(M)
    frames, actions, rewards, dones, weights = o["frames"], o["actions"], o["rewards"], o["dones"], o["weights"]

    def effective(network):
        params, eps = (t.to(DEV) for t in R.noisy_flat(network))
        E, _ = ops.rainbow_noisy_counts(n, na)
        eff = ops.rainbow_noisy_compose(params, eps, torch.zeros(E, device=DEV), n, na)
        a, b_ = 1024 * 3136, 1024 * 3136 + 1024
        J = (n + 1) * na
        return eps, eff[:a].view(1024, 3136), eff[a:b_], eff[b_:b_ + J * 512].view(J, 512), eff[b_ + J * 512:]

    def hidden(network, trunk, W_fc, b_fc, rows):
        seq = network.network
        return cnn.LinearReLUHwcFn.apply(trunk(rows, None, seq[0], seq[2], seq[4]), W_fc, b_fc, trunk.bufs)

    eps, W_fc, b_fc, W_out, b_out = effective(net)
    _, W_fc_t, b_fc_t, W_out_t, b_out_t = effective(tgt)
    W_fc, b_fc = W_fc.detach().requires_grad_(), b_fc.detach().requires_grad_()
    trunk, trunk_t = cnn.NatureTrunk(), cnn.NatureTrunk()
    with torch.no_grad():
        h_next_target = hidden(tgt, trunk_t, W_fc_t, b_fc_t, frames[M:]).contiguous()
        h_next = hidden(net, trunk, W_fc, b_fc, frames[M:]).contiguous().clone()
    h = hidden(net, trunk, W_fc, b_fc, frames[:M])
    J = (n + 1) * na
    dh, dW_out, db_out = torch.zeros((M, 1024), device=DEV), torch.zeros((J, 512), device=DEV), torch.zeros(J, device=DEV)
    sc, lps, best = torch.zeros(2, device=DEV), torch.zeros(M, device=DEV), torch.zeros(M, dtype=torch.int64, device=DEV)
    ops.rainbow_head_fwd_bwd(h.detach().contiguous(), h_next, h_next_target, W_out, b_out, W_out_t, b_out_t, net.support, actions, rewards, dones,
                             weights, n, gamma**n_step, net.v_min, net.v_max, dh, dW_out, db_out, sc, lps, best)
    h.backward(dh)
    E, P = ops.rainbow_noisy_counts(n, na)
    g_eff = torch.cat([W_fc.grad.reshape(-1), b_fc.grad.reshape(-1), dW_out.reshape(-1), db_out])
    head_grads = ops.rainbow_noisy_grad(g_eff, eps, torch.zeros(P, device=DEV), n, na).cpu()
    torch.cuda.synchronize()

    hwc = lambda x: x.cpu().permute(0, 3, 1, 2).contiguous()  # noqa: E731
    batch = (hwc(frames[:M]), hwc(frames[M:]), actions.cpu(), rewards.cpu(), dones.cpu())
    s64, g64, best64 = _reference_update(net, tgt, batch, weights.cpu(), n_step, gamma, torch.float64)
    s32, g32, _ = _reference_update(net, tgt, batch, weights.cpu(), n_step, gamma, torch.float32)
    assert torch.equal(best.cpu(), best64)
    ferr = (sc.cpu().double() - s64).abs().max().item()
    print(f"forward: err {ferr:.3e}")
    assert ferr <= 5e-5 * max(1.0, s64.abs().max().item())
    got, off = {name: p.grad.cpu() for name, p in net.named_parameters() if name.startswith("network.")}, 0
    for name, p in net.named_parameters():
        if not name.startswith("network."):
            got[name] = head_grads[off:off + p.numel()].view(p.shape)
            off += p.numel()
    assert off == P
    for name, ref in g64.items():
        err, own = (got[name].double() - ref).abs().max().item(), (g32[name].double() - ref).abs().max().item()
        bar = max(5e-5 * ref.abs().max().item(), 4 * own)
        print(f"{name}: err {err:.3e} torch f32 {own:.3e} bar {bar:.3e}")
        assert err <= bar, (name, err, bar)


# ================================================================================================== the learner
def test_whole_steps_through_the_learner_on_both_backends(monkeypatch):
    """store / act / train_step / sync_target: ``fused`` on the device beside ``torch`` on the CPU, the same transitions, noise and draws,
    at the family's bar (rtol 1e-3, atol 1e-4 on loss, q_values and loss_per_sample; the same sampled indices); the fused steps launch
    every new entry point and, with the same observation, pick the torch backend's action."""
    launched = set()
    orig = ops._launch
    monkeypatch.setattr(ops, "_launch", lambda name, *a: (launched.add(name), orig(name, *a))[1])
    T, F, out = P.lockstep_updates(DEV, 51)
    P.assert_lockstep(out)
    obs = P.fill(P.make_learner(CPU, "torch"), 1)
    assert np.array_equal(F.act(obs), T.act(obs))
    want = {"mi355ppo_rainbow_" + n for n in ("per_add_u8", "per_sample", "per_gather_u8", "per_update", "noisy_compose_f32", "noisy_grad_f32",
                                              "head_act_f32", "head_fwd_bwd_f32")}
    assert want <= launched, want - launched
    (to, tt), (fo, ft) = T.flat_params(), F.flat_params()
    assert torch.allclose(fo.cpu(), to, rtol=1e-3, atol=1e-5) and torch.allclose(ft.cpu(), tt, rtol=1e-3, atol=1e-5)


def test_torch_backend_runs_whole_steps_on_the_device():
    L = P.make_learner(DEV, "torch", n_atoms=51)
    obs = P.fill(L, 22)
    np.random.seed(1)
    for k in range(3):
        L.beta = 0.5
        L.train_step()
        L.sync_target()
    m = L.metrics()
    assert np.isfinite(m["loss"]) and np.isfinite(m["q_values"]) and L.act(obs).shape == (1,)


@pytest.mark.parametrize("name", P.RUNS)
def test_goldens_teacher_forced_on_the_hip_path(name):
    """The minted runs of the reference's own lines, teacher-forced (the golden actions and draws, the noise regenerated from the seed)
    through the fused learner on the device: every update's loss, q_values and loss_per_sample at rtol 1e-3, atol 1e-4, the sampled
    indices equal; the first update's pre-Adam flat gradient against the torch backend's on the CPU (itself held to the minted run
    here): within 1e-3 of its largest element, 1 - cosine <= 1e-5."""
    grads = {}
    rec = P.replay_run(name, "fused", DEV)
    grads["fused"] = rec["first_grad"]
    assert P.assert_run_within_bar(rec) == 15
    ref = P.replay_run(name, "torch", CPU, forced=True, on_first_update=lambda L: grads.setdefault(
        "torch", torch.cat([p.grad.reshape(-1) for p in L.q_network.parameters()]).double().clone()))
    assert P.assert_run_within_bar(ref) == 15
    g, r = grads["fused"], grads["torch"]
    err, cos = (g - r).abs().max().item(), 1.0 - (torch.dot(g, r) / (g.norm() * r.norm())).item()
    print(f"{name}: first-update gradient max abs dg / absmax {err / r.abs().max().item():.2e}, 1 - cosine {cos:.2e}")
    assert err <= 1e-3 * r.abs().max().item() and cos <= 1e-5
    tree = rec["golden"]["tree"]
    assert np.allclose(rec["tree"], tree, rtol=P.RTOL, atol=P.ATOL) and R.same_bits(rec["tree"], R.rebuild(rec["tree"], 16))
