"""GPU tests of K8, the 256-wide tanh MLP family (csrc/mlp256.hip): the forward chain and one minibatch's gradients against float64 on
the CPU under the per-row bars of tests/row_bars.py, guard bands, refusals, and ppo_continuous_action_isaacgym.py on the kernels."""
import ctypes
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn

from cleanrl_amd import _lib, ops
from cleanrl_amd.agents import layer_init
from guard_arena import SENTINELS, Arena, same_bits
from row_bars import C_BIAS_GRAD, C_MAX, C_WGRAD, row_bar

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
C_FORWARD = 4.0            # row_bars' rule: starts at 4 (a chain of at most 16 k-steps per layer)
CASES = [(60, 8, 1, False), (60, 8, 65, True), (17, 6, 63, True), (5, 1, 64, False), (108, 21, 200, True), (211, 20, 129, False),
         (256, 32, 4097, True)]


def _nets(O, nout, seed):
    """tests/test_gpu_mlp.py::_nets at 256-256: orthogonal weights, output layers std 1.0 / 0.5, biases N(0, 0.1)."""
    torch.manual_seed(seed)
    mk = lambda n, s: nn.Sequential(layer_init(nn.Linear(O, 256)), nn.Tanh(), layer_init(nn.Linear(256, 256)), nn.Tanh(),      # noqa: E731
                                    layer_init(nn.Linear(256, n), std=s))
    critic, actor = mk(1, 1.0), mk(nout, 0.5)
    with torch.no_grad():
        for m in list(critic) + list(actor):
            if isinstance(m, nn.Linear):
                m.bias.normal_(0, 0.1)
    return actor, critic


def _copy(seq, dtype, device="cpu"):
    d = nn.Sequential(*[nn.Linear(m.in_features, m.out_features) if isinstance(m, nn.Linear) else nn.Tanh() for m in seq])
    d.load_state_dict(seq.state_dict())
    return d.to(device=device, dtype=dtype)


def _chain(seq, x):
    h1 = torch.tanh(seq[0](x))
    h2 = torch.tanh(seq[2](h1))
    return h1, h2, seq[4](h2)


def _loss(actor, critic, logstd, x, act, lp_old, adv, ret):
    """The reference's minibatch loss at its defaults (norm_adv, clip 0.2, clip_vloss off, vf_coef 2, ent_coef 0), :336-371."""
    mean, value = actor(x), critic(x).view(-1)
    std = torch.exp(logstd.expand_as(mean))
    lp = (-((act - mean) ** 2) / (2 * std ** 2) - logstd - 0.5 * torch.log(torch.tensor(2 * torch.pi, dtype=x.dtype))).sum(1)
    ratio = (lp - lp_old).exp()
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    pg = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 0.8, 1.2)).mean()
    return pg + 2.0 * 0.5 * ((value - ret) ** 2).mean()


def _grads(actor, critic, logstd, c, n, dtype):
    a, cr, ls = _copy(actor, dtype), _copy(critic, dtype), logstd.detach().to(dtype).requires_grad_(True)
    t = lambda v: v[:n].to(dtype)      # noqa: E731
    _loss(a, cr, ls, t(c.x), t(c.act), t(c.lp_old), t(c.adv), t(c.ret)).backward()
    return [p.grad for p in list(a.parameters()) + list(cr.parameters())] + [ls.grad]


@functools.lru_cache(maxsize=None)
def _case(O, nout, M, gather):
    """Everything a case needs, on the CPU, once: ``max(M, 64)`` rows of one recipe (the kernel gets the first ``M``), observations ~N(0, 1)
    times a per-row factor over 2^-8, the float64 references of the first ``M`` rows and torch's f32 / f64 pair on all rows (the yardstick)."""
    rows = max(M, 64)
    actor, critic = _nets(O, nout, 100 + O)
    g = torch.Generator().manual_seed(7 * M + O)
    x = torch.randn(rows, O, generator=g) * torch.exp2(-8 * torch.rand(rows, 1, generator=g))
    if gather:
        inds = torch.randperm(rows + 9, generator=g)[:rows]
        store = torch.randn(rows + 9, O, generator=g)
        store[inds] = x
    else:
        inds, store = None, x
    with torch.no_grad():
        f32 = [_chain(n, x) for n in (actor, critic)]
        f64 = [_chain(_copy(n, torch.float64), x.double()) for n in (actor, critic)]
    # behaviour rows: a tenth of the ratios outside the clip range, so that both branches of the surrogate carry gradient
    logstd = torch.randn(1, nout, generator=g) * 0.2
    act = f64[0][2].float() + torch.exp(logstd) * torch.randn(rows, nout, generator=g)
    lp_new = (-((act.double() - f64[0][2]) ** 2) / (2 * torch.exp(logstd.double()) ** 2) - logstd.double()
              - 0.5 * torch.log(torch.tensor(2 * torch.pi, dtype=torch.float64))).sum(1)
    ratio = 1 + 0.15 * (2 * torch.rand(rows, generator=g) - 1)
    far = torch.rand(rows, generator=g) < 0.1
    ratio[far] = torch.where(torch.rand(rows, generator=g) < 0.5, 0.6, 1.4)[far]
    c = SimpleNamespace(O=O, nout=nout, M=M, rows=rows, actor=actor, critic=critic, x=x, inds=inds, store=store, f32=f32, f64=f64, logstd=logstd,
                        act=act, lp_old=(lp_new - torch.log(ratio.double())).float(), adv=torch.randn(rows, generator=g),
                        ret=torch.randn(rows, generator=g), val=torch.randn(rows, generator=g))
    if M >= 2:
        c.g64 = _grads(actor, critic, logstd, c, M, torch.float64)
        c.g32_yard, c.g64_yard = _grads(actor, critic, logstd, c, rows, torch.float32), _grads(actor, critic, logstd, c, rows, torch.float64)
    return c


def _device(c):
    actor, critic = _copy(c.actor, torch.float32, DEV), _copy(c.critic, torch.float32, DEV)
    for p in list(actor.parameters()) + list(critic.parameters()):
        p.grad = torch.zeros_like(p)
    M = c.M
    if c.inds is not None:
        store, inds = c.store.to(DEV), c.inds[:M].to(DEV)
    else:
        store, inds = c.x[:M].contiguous().to(DEV), None
    return ops.Mlp256Nets(actor, critic), store, inds


@pytest.mark.parametrize("O,nout,M,gather", CASES)
def test_forward_chain_against_float64(O, nout, M, gather):
    c = _case(O, nout, M, gather)
    nets, store, inds = _device(c)
    mean, value = ops.mlp256_forward(store, nets, inds=inds, save=True)
    h1, h2 = (t.clone() for t in nets.saved(M)[:2])
    got = {"mean": mean, "value": value.view(M, 1), "actor h1": h1[0], "critic h1": h1[1], "actor h2": h2[0], "critic h2": h2[1]}
    pick = {"mean": (0, 2), "value": (1, 2), "actor h1": (0, 0), "critic h1": (1, 0), "actor h2": (0, 1), "critic h2": (1, 1)}
    ratios = {}
    for name, (net, k) in pick.items():
        ratios[name] = row_bar(f"K8 forward {name} ({O}, {nout}, {M})", got[name], c.f64[net][k][:M], c.f32[net][k], c.f64[net][k], c=C_FORWARD)
    print("K8 forward ratios", (O, nout, M), {k: round(v, 2) for k, v in ratios.items()})
    mean2, value2 = ops.mlp256_forward(store, nets, inds=inds, save=True)
    assert same_bits(mean, mean2) and same_bits(value, value2) and same_bits(h1, nets.saved(M)[0]) and same_bits(h2, nets.saved(M)[1])


def _minibatch(c, nets, store, inds, slabs=0):
    """forward (save) -> K3's Normal loss -> data-gradient chain -> weight gradients + fold; -> the 13 gradients, the reference's order."""
    M = c.M
    for t in nets.tensors[0] + nets.tensors[1]:
        t.grad.zero_()
    d = lambda v: v.to(DEV)      # noqa: E731
    if c.inds is not None:       # the behaviour arrays live at the gathered rows, as a rollout's do
        full = lambda v: torch.zeros((c.store.shape[0],) + v.shape[1:]).index_copy_(0, c.inds, v).to(DEV)      # noqa: E731
    else:
        full = lambda v: v[:M].contiguous().to(DEV)      # noqa: E731
    mean, value = ops.mlp256_forward(store, nets, inds=inds, save=True)
    _, dmean, dlogstd, dvalue = ops.ppo_loss_normal(mean, d(c.logstd), value, inds, full(c.act), full(c.lp_old), full(c.adv), full(c.ret),
                                                    full(c.val), 0.2, 0.0, 2.0, True, False)
    ops.mlp256_backward(store, nets, dmean, dvalue, inds=inds, slabs=slabs)
    return [t.grad.clone() for t in nets.tensors[0] + nets.tensors[1]] + [dlogstd.view(1, -1), dmean, dvalue]


@pytest.mark.parametrize("O,nout,M,gather", CASES[1:])
def test_minibatch_gradients_against_float64_autograd(O, nout, M, gather):
    c = _case(O, nout, M, gather)
    nets, store, inds = _device(c)
    got = _minibatch(c, nets, store, inds)
    names = [f"{n} {p}" for n in ("actor", "critic") for p in ("W1", "b1", "W2", "b2", "W3", "b3")] + ["actor_logstd"]
    ratios = {}
    for name, g, r64, y32, y64 in zip(names, got, c.g64, c.g32_yard, c.g64_yard):
        if g.dim() == 2 and name != "actor_logstd":
            ratios[name] = row_bar(f"K8 {name} ({O}, {nout}, {M})", g, r64, y32, y64, row_axis=0, c=C_WGRAD)
        else:                    # a bias / logstd gradient is one row
            ratios[name] = row_bar(f"K8 {name} ({O}, {nout}, {M})", g.view(1, -1), r64.view(1, -1), y32.view(1, -1), y64.view(1, -1), c=C_BIAS_GRAD)
    print("K8 gradient ratios", (O, nout, M), {k: round(v, 2) for k, v in ratios.items()})
    again = _minibatch(c, nets, store, inds)
    assert all(same_bits(a, b) for a, b in zip(got, again)), "the default grid twice: not the same bits"


def test_one_slab_and_default_slabs_agree_to_the_folds_rounding():
    """200 rows = 4 tiles: one slab against four.  A weight gradient adds the same four slot products (scales are per 64-row slot) in the same
    order either way, in the accumulator or in the fold: at most 4 roundings of 2^-24 of the running sum each way, held as 4 * 2^-23 of the
    row's largest element.  A bias gradient is an f32 sum of the column of dz whose terms are grouped differently (a thread's rows of its
    slab, the 16 row groups, the slabs: chains of at most 16 + 16 + 4 additions), each addition rounding 2^-24 of a partial sum that is at
    most the column's sum of magnitudes: held as 2 * 36 * 2^-24 of that sum."""
    c = _case(108, 21, 200, True)
    nets, store, inds = _device(c)
    one, dflt = _minibatch(c, nets, store, inds, slabs=1), _minibatch(c, nets, store, inds)
    _, _, dz2, dz1 = nets.saved(c.M)
    for t in range(2):
        colsum = [dz1[t].abs().sum(0), dz2[t].abs().sum(0), one[-2 + t].abs().view(c.M, -1).sum(0)]      # |dz1|, |dz2|, |dmean| or |dvalue|
        for l in range(3):
            w1, wd, r = (g[6 * t + 2 * l].double().cpu() for g in (one, dflt, c.g64))
            assert bool(((w1 - wd).abs().amax(1) <= 4 * 2.0 ** -23 * r.abs().amax(1)).all())
            b1, bd = one[6 * t + 2 * l + 1].double(), dflt[6 * t + 2 * l + 1].double()
            assert bool(((b1 - bd).abs() <= 2 * 36 * 2.0 ** -24 * colsum[l].double()).all())


@pytest.mark.parametrize("O,nout,M", [(17, 6, 65), (256, 32, 129)])
def test_guard_bands_stay_intact(O, nout, M):
    c = _case(O, nout, max(M, 64), True)
    lib = _lib.load()
    results = []
    for sentinel in SENTINELS:
        arena = Arena(DEV, sentinel, words=1 << 24)
        actor, critic = _copy(c.actor, torch.float32, DEV), _copy(c.critic, torch.float32, DEV)
        for p in list(actor.parameters()) + list(critic.parameters()):
            p.grad = arena.carve(p.shape, name=f"grad{tuple(p.shape)}").zero_()
        nets = ops.Mlp256Nets(actor, critic)
        nets._pack = (None, arena.carve(lib.mi355ppo_mlp256_pack_bytes(O, nout), torch.uint8, "pack"))
        nets._ws = arena.carve(lib.mi355ppo_mlp256_workspace_bytes(M, O, nout), torch.uint8, "workspace", align=16)
        store, inds = arena.input(c.store.to(DEV), "obs"), arena.input(c.inds[:M].to(DEV), "inds")
        mean, value = arena.carve((M, nout), name="mean"), arena.carve((M,), name="value")
        ops.mlp256_forward(store, nets, inds=inds, save=True, mean_out=mean, value_out=value)
        dmean, dvalue = arena.input(torch.tanh(mean) * 1e-3, "dmean"), arena.input(torch.tanh(value) * 1e-3, "dvalue")
        ops.mlp256_backward(store, nets, dmean, dvalue, inds=inds)
        arena.assert_guards_intact()
        results.append([mean.clone(), value.clone()] + [t.clone() for t in nets.saved(M)] + [t.grad.clone() for t in nets.tensors[0] + nets.tensors[1]])
    assert all(same_bits(a, b) for a, b in zip(*results)), "the results depend on what lies outside the tensors"


def test_refusals_leave_the_outputs_untouched():
    lib = _lib.load()
    c = _case(60, 8, 65, True)
    nets, store, _ = _device(c)
    M, pack = 65, nets.pack()
    ws = nets.workspace(M)
    mean, value = torch.full((M, 33), 7.0, device=DEV), torch.full((M,), 7.0, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    fwd = lambda M_, O, n, pk, w, wb: lib.mi355ppo_mlp256_fwd_f32(p(store), None, M_, O, n, pk, p(mean), p(value), w, wb, None)      # noqa: E731
    assert fwd(M, 257, 8, p(pack), None, 0) == -1
    assert fwd(M, 60, 33, p(pack), None, 0) == -1
    assert fwd(0, 60, 8, p(pack), None, 0) == -1
    assert fwd(M, 60, 8, None, None, 0) == -1
    assert fwd(M, 60, 8, p(pack), p(ws), ws.numel() - 1) == -4
    assert lib.mi355ppo_mlp256_dgrad_f32(p(mean), p(value), M, 60, 8, p(pack), p(ws), ws.numel() - 1, None) == -4
    ga, gc = nets.grads()
    assert lib.mi355ppo_mlp256_wgrad_f32(p(store), None, p(mean), p(value), M, 60, 8, ga, gc, 0, None, 0, None) == -4
    assert lib.mi355ppo_mlp256_pack_f32(nets._ptrs(nets.tensors[0]), nets._ptrs(nets.tensors[1]), 257, 8, p(pack), pack.numel(), None) == -1
    assert b"mlp256" in lib.mi355ppo_last_error()
    assert lib.mi355ppo_mlp256_workspace_bytes(M, 257, 8) == 0 and not ops.mlp256_supported(257, 8) and not ops.mlp256_supported(60, 33)
    torch.cuda.synchronize()
    assert bool((mean == 7.0).all()) and bool((value == 7.0).all())
    assert all(bool((t.grad == 0).all()) for t in nets.tensors[0] + nets.tensors[1])


def test_script_trains_on_the_k8_kernels(monkeypatch, capsys):
    import math

    from cleanrl_amd import ppo_continuous_action_isaacgym as script

    monkeypatch.setenv("MI355PPO_MLP256", "fused")
    served, backward = [], ops.mlp256_backward
    monkeypatch.setattr(ops, "mlp256_backward", lambda *a, **k: (served.append(a[1]), backward(*a, **k))[1])
    learner = script.main(["--num-envs", "256", "--num-steps", "16", "--total-timesteps", "8192"])
    assert learner.mlp256 is not None and served == [learner.mlp256] * (2 * 4 * 2), "two iterations of 4 epochs x 2 minibatches on the K8 handle"
    assert "K8 kernels" in capsys.readouterr().err
    m = learner.last_metrics
    assert all(math.isfinite(float(m[k])) for k in ("value_loss", "policy_loss", "entropy", "old_approx_kl", "approx_kl", "clipfrac"))
    assert bool(torch.isfinite(learner.flat.params).all())


def _learner(monkeypatch, backend, seed=3, num_envs=128):
    from cleanrl_amd import envs as E, ppo_continuous_action_isaacgym as script
    from cleanrl_amd.learner import PPOLearner

    monkeypatch.setenv("MI355PPO_MLP256", backend)
    args = script.Args(num_envs=num_envs, num_steps=16)
    args.batch_size, args.minibatch_size = num_envs * 16, num_envs * 8
    env = E.DeviceLinearContinuousVecEnv(num_envs, DEV, seed=seed)
    torch.manual_seed(seed)
    agent = script.Agent(env).to(DEV)
    L = PPOLearner(agent, args, env.single_observation_space, env.single_action_space, num_envs, DEV, sample_seed=seed)
    L.device_randperm = True
    return L, env


_STORAGE = ("obs", "actions", "logprobs", "rewards", "dones", "values", "advantages", "returns", "boot_obs", "boot_done")


def _flat_batch(L):
    return (L.obs.reshape(-1, 60), L.actions.reshape(-1, 8), L.logprobs.reshape(-1), L.advantages.reshape(-1), L.returns.reshape(-1),
            L.values.reshape(-1))


def _learner_grads(L, idx):
    L.flat.grads.zero_()
    L._mb_adv_md = None
    L.forward_backward_hip(idx, *_flat_batch(L), torch.zeros(7, device=DEV))
    return {n: p.grad.clone() for n, p in L.agent.named_parameters()}


def _reference_grads(L, idx, dtype):
    """The reference's minibatch loss on a CPU copy of the learner's current parameters, through autograd."""
    a, c = _copy(L.agent.actor_mean, dtype), _copy(L.agent.critic, dtype)
    ls = L.agent.actor_logstd.detach().cpu().to(dtype).requires_grad_(True)
    obs, act, lp, adv, ret, _ = (t[idx].cpu().to(dtype) for t in _flat_batch(L))
    _loss(a, c, ls, obs, act, lp, adv, ret).backward()
    out = {"actor_logstd": ls.grad}
    for prefix, net in (("critic", c), ("actor_mean", a)):
        out.update({f"{prefix}.{n}": p.grad for n, p in net.named_parameters()})
    return out


def _hold_to_float64(L, idx, what, c_w=C_WGRAD, c_b=C_BIAS_GRAD):
    """-> the worst ratio.  (``c_w = c_b = C_MAX`` with the result only printed: a measurement of code that is not under test.)"""
    got, r64, r32 = _learner_grads(L, idx), _reference_grads(L, idx, torch.float64), _reference_grads(L, idx, torch.float32)
    assert set(got) == set(r64)
    worst = 0.0
    for n, g in got.items():
        if n.endswith("weight"):
            worst = max(worst, row_bar(f"{what}: {n}", g, r64[n], r32[n], r64[n], row_axis=0, c=c_w))
        else:
            worst = max(worst, row_bar(f"{what}: {n}", g.view(1, -1), r64[n].view(1, -1), r32[n].view(1, -1), r64[n].view(1, -1), c=c_b))
    return worst


def test_learner_on_k8_against_float64_and_the_torch_backend(monkeypatch):
    """The learner's wiring, not the kernels: two learners from one seed, one rollout copied into both.  On the K8 backend the flat gradient of
    the first minibatch, and -- after one clip + Adam step, so that a pack that was not refreshed would show -- of the second one at the
    stepped parameters, is held to float64 autograd of the reference's loss under the gradient test's bars (C_WGRAD per output unit,
    C_BIAS_GRAD for biases and actor_logstd).  Parameters: an Adam step moves an element by at most lr at step 1 and by at most
    lr (1 - beta1) / sqrt(1 - beta2) = 3.17 lr later, whatever its gradient, and a near-zero gradient element may take opposite signs on the
    two backends, so the two parameter vectors are held to twice that per step: 2 lr after one step, 2 lr (1 + 8 * 3.17) after the update's
    eight more.  (A bound inside the gradient bars is not reachable for parameters: Adam's first steps are lr * g / (|g| + eps).)"""
    F, env = _learner(monkeypatch, "fused")
    T, _ = _learner(monkeypatch, "torch")
    assert F.mlp256 is not None and T.mlp256 is None and torch.equal(F.flat.params, T.flat.params)
    F.observe(0, env.obs(), torch.zeros(F.N, device=DEV))
    for step in range(F.T):
        obs, r, d = env.step(F.act(step))
        F.store_reward(step, r)
        F.observe(step + 1, obs, d)
    F.finish_rollout()
    for name in _STORAGE:
        getattr(T, name).copy_(getattr(F, name))
    lr = F.args.learning_rate
    perm = torch.randperm(F.batch_size, generator=torch.Generator().manual_seed(5)).to(DEV)
    first, second = perm[:F.minibatch_size].contiguous(), perm[F.minibatch_size:].contiguous()
    ratios = [_hold_to_float64(F, first, "fused learner, first minibatch")]
    _learner_grads(T, first)
    for L in (F, T):
        L.optimizer_step_hip(lr)
    d1 = float((F.flat.params - T.flat.params).abs().max())
    assert d1 <= 2 * lr, d1
    ratios.append(_hold_to_float64(F, second, "fused learner, second minibatch after one step"))
    # (the torch backend's own gradient is measured, not held: hipBLASLt's GEMMs are not under test; they read 4.72 at critic.2.weight)
    ratios.append(_hold_to_float64(T, second, "torch learner, second minibatch after one step", C_MAX, C_MAX))
    for L in (F, T):
        L.flat.grads.zero_()
    for L in (F, T):
        torch.manual_seed(11)                      # the same epoch permutations on both
        m = L.update(lr)
        assert all(bool(torch.isfinite(torch.as_tensor(float(v)))) for v in m.values())
    d9 = float((F.flat.params - T.flat.params).abs().max())
    print("K8 learner: worst gradient ratios (fused 1st, fused 2nd, torch 2nd)", ratios, "max |fused - torch| parameter after 1 step", d1, "after 9", d9, "lr", lr)
    assert d9 <= 2 * lr * (1 + 8 * 3.17), d9
