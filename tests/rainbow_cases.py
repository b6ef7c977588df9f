"""Shared case builders and references for the Rainbow kernels (csrc/rainbow.hip) and their host twins: the prioritized replay
buffer of rainbow_atari.py (two u8 frame rings and the f32 sum tree) and the noise composition of its four NoisyLinear layers.

What is compared how (include/mi355ppo.h, the Rainbow section):
* a leaf, and ``max_priority ** alpha``, is ``pow`` in double rounded once to f32: at most 1 ulp from the reference's ``powf`` and
  from the other side's ``pow``;
* an inner node is the f32 sum of its two children: GIVEN the leaves the whole tree is determined bit for bit (``rebuild``);
* the indices of a sample are determined by the tree and the draws; the weights pass through two powers and two divisions: 4 ulp;
* ring contents, ``max_priority`` and ``size`` pass through no power: equal.
"""
import os
from types import SimpleNamespace

import numpy as np
import torch

from offpolicy_cases import same, within_bar  # noqa: F401

FRAME = (84, 84, 4)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 1e-6


def per_fixture():
    return np.load(os.path.join(GOLDEN, "rainbow_per_cases.npz"))


def network_fixture():
    return np.load(os.path.join(GOLDEN, "rainbow_network_init.npz"))


# ================================================================================================== comparisons
def ulps(a, b):
    """Elementwise distance in f32 units in the last place (same-sign finite values; equal bits, NaN against NaN included, give 0)."""
    a = torch.as_tensor(a, dtype=torch.float32).cpu().contiguous()
    b = torch.as_tensor(b, dtype=torch.float32).cpu().contiguous()
    return (a.view(torch.int32).to(torch.int64) - b.view(torch.int32).to(torch.int64)).abs()


def rebuild(tree, slots):
    """The tree that the leaves of ``tree`` determine: every inner node the f32 sum of its children, deepest first."""
    t = np.array(torch.as_tensor(tree).cpu().numpy(), dtype=np.float32, copy=True)
    for p in range(slots - 2, -1, -1):
        t[p] = t[2 * p + 1] + t[2 * p + 2]
    return torch.from_numpy(t)


def same_bits(a, b):
    a, b = torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)


def tree_matches(tree, want, slots, what=""):
    """``tree`` against a tree from another side: leaves within 1 ulp, inner nodes exactly what ``tree``'s own leaves determine."""
    tree, want = torch.as_tensor(tree).cpu(), torch.as_tensor(want).cpu()
    worst = int(ulps(tree[slots - 1:], want[slots - 1:]).max())
    assert worst <= 1, f"{what}: a leaf is {worst} ulp away"
    assert same_bits(tree, rebuild(tree, slots)), f"{what}: an inner node is not the f32 sum of its children"


# ================================================================================================== the buffer
def new_buffer(mod, slots, dev, beta=0.4, K=None):
    if K is None:
        return mod.rainbow_new_buffer(slots, dev, beta)
    shapes = ((("ring obs"), (slots,) + FRAME, torch.uint8), ("ring next_obs", (slots,) + FRAME, torch.uint8), ("ring actions", (slots,), torch.int64),
              ("ring rewards", (slots,), torch.float32), ("ring dones", (slots,), torch.float32), ("tree", (2 * slots - 1,), torch.float32),
              ("state", (2,), torch.float32), ("size", (1,), torch.int64))
    buf = tuple(K.new(nm, shape, dt).zero_() for nm, shape, dt in shapes)
    buf[6].copy_(torch.tensor([1.0, beta]))
    return buf


BUF_NAMES = ("ring_obs", "ring_next_obs", "ring_actions", "ring_rewards", "ring_dones", "tree", "state", "size")


def per_script(slots, B, seed=0):
    """Inputs of ``run_per``: slots + 2 transitions (the ring wraps), three batches of draws and losses, and an index batch with
    duplicates and two entries outside the ring."""
    g = torch.Generator().manual_seed(7000 + 100 * slots + B + seed)
    S = slots + 2
    frames = lambda: torch.randint(1, 256, (S, 1, 4, 84, 84), dtype=torch.uint8, generator=g)  # noqa: E731
    dup = torch.randint(0, slots, (B,), generator=g)
    if B >= 5:
        dup[-1], dup[0], dup[1], dup[2] = dup[0].item(), slots + 3, -2, dup[3].item()
    loss = torch.randn((3, B), generator=g) * torch.tensor([[0.3], [4.0], [1e-3]])
    return dict(obs=frames(), next_obs=frames(), action=torch.randint(0, 18, (S, 1), generator=g), reward=torch.randn((S, 1), generator=g),
                done=(torch.rand((S, 1), generator=g) < 0.3).float(), u=torch.rand((3, B), dtype=torch.float64, generator=g), loss=loss, dup=dup)


def run_per(mod, dev, slots, B, T, K=None, alpha=0.6, betas=(0.4, 0.7)):
    """The buffer's four entry points through ``mod`` on the script ``T`` (tensors already on ``dev``) -> dict of tensors."""
    new = (lambda nm, shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)) if K is None else K.new
    buf = new_buffer(mod, slots, dev, betas[0], K)
    for s in range(slots + 2):
        mod.rainbow_per_add_u8(buf, s % slots, T["obs"][s], T["next_obs"][s], T["action"][s], T["reward"][s], T["done"][s], alpha)
    out = {}
    for k in range(3):
        idx, w = new(f"indices{k}", (B,), torch.int64), new(f"weights{k}", (B,))
        if k == 2:
            buf[6][1:2].fill_(betas[1])
        mod.rainbow_per_sample(buf, T["u"][k], idx, w)
        mod.rainbow_per_update(buf, T["dup"] if k == 1 else idx, T["loss"][k], alpha, EPS)
        out[f"indices{k}"], out[f"weights{k}"] = idx, w
        out[f"tree{k}"] = buf[5].clone()
    gathered = (new("frames", (2 * B,) + FRAME, torch.uint8), new("actions", (B,), torch.int64), new("rewards", (B,)), new("dones", (B,)))
    mod.rainbow_per_gather_u8(buf, T["dup"], *gathered)
    out.update(zip(("frames", "actions", "rewards", "dones"), gathered))
    out.update(zip(BUF_NAMES, buf))
    return out


PER_OUTS = BUF_NAMES + ("frames", "actions", "rewards", "dones") + tuple(f"{n}{k}" for k in range(3) for n in ("indices", "weights"))


def hwc(stack):
    """(1, 4, 84, 84) as the env gives it -> the ring's (84, 84, 4)."""
    return stack[0].permute(1, 2, 0).contiguous()


def check_ring_contents(out, T, slots):
    """Every slot holds the last transition written to it, obs and next_obs apart; the gather returns the clamped slots' contents."""
    o = {k: v.cpu() for k, v in out.items()}
    for slot in range(slots):
        s = max(x for x in range(slots + 2) if x % slots == slot)
        assert torch.equal(o["ring_obs"][slot], hwc(T["obs"][s].cpu())) and torch.equal(o["ring_next_obs"][slot], hwc(T["next_obs"][s].cpu()))
        assert o["ring_actions"][slot] == T["action"][s, 0].cpu() and same_bits(o["ring_rewards"][slot], T["reward"][s, 0])
        assert same_bits(o["ring_dones"][slot], T["done"][s, 0])
    idx = T["dup"].cpu().clamp(0, slots - 1)
    B = len(idx)
    assert torch.equal(o["frames"][:B], o["ring_obs"][idx]) and torch.equal(o["frames"][B:], o["ring_next_obs"][idx])
    assert torch.equal(o["actions"], o["ring_actions"][idx]) and same_bits(o["rewards"], o["ring_rewards"][idx])
    assert same_bits(o["dones"], o["ring_dones"][idx]) and o["size"].item() == slots


def check_per_against(got, want, slots, what):
    """One side's ``run_per`` against another's (device against twin): the bars of this module's docstring."""
    g, w = ({k: v.cpu() for k, v in d.items()} for d in (got, want))
    for k in ("ring_obs", "ring_next_obs", "ring_actions", "ring_rewards", "ring_dones", "size", "frames", "actions", "rewards", "dones"):
        assert same_bits(g[k], w[k]), (what, k)
    assert same_bits(g["state"], w["state"]), (what, "max_priority / beta")
    for k in range(3):
        tree_matches(g[f"tree{k}"], w[f"tree{k}"], slots, f"{what} tree{k}")
        # sample k walks the tree that update k - 1 left; the first walks leaves of max_priority ** alpha = 1.0 ** alpha, exactly 1.0 on
        # both sides.  Where the two sides' powers rounded a leaf apart, the walks may part too: the indices are held to each other on
        # equal trees (and to the reference's on the reference's own trees: replay_fixture_case).
        if k == 0 or same_bits(g[f"tree{k - 1}"], w[f"tree{k - 1}"]):
            assert torch.equal(g[f"indices{k}"], w[f"indices{k}"]), (what, k)
            assert int(ulps(g[f"weights{k}"], w[f"weights{k}"]).max()) <= 4, (what, k)


# ================================================================================================== the fixtures
def fixture_case(d, k):
    capacity, alpha, eps, B = d[f"c{k}_meta"]
    return SimpleNamespace(slots=int(capacity), alpha=float(alpha), eps=float(eps), B=int(B), **{n: d[f"c{k}_{n}"] for n in (
        "kind", "tree", "maxp", "size", "beta", "u", "idx", "val")})


def replay_fixture_case(mod, dev, c):
    """Every recorded operation through ``mod`` from the reference's own state before it (tree, max_priority and size uploaded), held
    against the reference's state after it.  -> the number of operations checked, per kind."""
    slots, B = c.slots, c.B
    buf = new_buffer(mod, slots, dev)
    zero = torch.zeros((1, 4, 84, 84), dtype=torch.uint8, device=dev)
    one = lambda v, dt: torch.tensor([v], dtype=dt, device=dev)  # noqa: E731
    idx_out, w_out = torch.zeros(B, dtype=torch.int64, device=dev), torch.zeros(B, device=dev)
    seen, pos = [0, 0, 0], 0
    for i, kind in enumerate(c.kind):
        buf[5].copy_(torch.from_numpy(c.tree[i]))
        buf[6].copy_(torch.tensor([float(c.maxp[i]), float(c.beta[i])]))
        buf[7].fill_(int(c.size[i]))
        what = f"slots={slots} B={B} alpha={c.alpha} operation {i} (kind {kind})"
        if kind == 0:
            mod.rainbow_per_add_u8(buf, pos, zero, zero, one(0, torch.int64), one(0.0, torch.float32), one(0.0, torch.float32), c.alpha)
            pos = (pos + 1) % slots
        elif kind == 1:
            mod.rainbow_per_sample(buf, torch.from_numpy(c.u[i]).to(dev), idx_out, w_out)
            assert torch.equal(idx_out.cpu(), torch.from_numpy(c.idx[i])), what
            worst = int(ulps(w_out, c.val[i]).max())
            assert worst <= 4, f"{what}: a weight is {worst} ulp from the reference's"
        else:
            mod.rainbow_per_update(buf, torch.from_numpy(c.idx[i]).to(dev), torch.from_numpy(c.val[i]).to(dev), c.alpha, c.eps)
        tree_matches(buf[5], c.tree[i + 1], slots, what)
        assert same_bits(buf[6][0], torch.tensor(c.maxp[i + 1])), f"{what}: max_priority"
        assert buf[7].item() == c.size[i + 1], f"{what}: size"
        seen[kind] += 1
    return seen


# ================================================================================================== the noisy layers
NOISY_SHAPES = [(2, 2), (6, 5), (18, 51), (9, 101)]             # (n_actions, n_atoms): the smallest, a ragged one, the script's, the widest atoms


def make_network(n, na, seed=0):
    from cleanrl_amd.agents import NoisyDuelingDistributionalNetwork

    torch.manual_seed(5000 + 31 * n + na + seed)
    env = SimpleNamespace(single_action_space=SimpleNamespace(n=n))
    return NoisyDuelingDistributionalNetwork(env, na, -10.0, 10.0)


def noisy_flat(net):
    """(the head's parameters, its noise) of ``net`` as the flat buffers the entry points take."""
    layers = net.noisy_layers()
    params = torch.cat([p.detach().reshape(-1) for l in layers for p in (l.weight_mu, l.weight_sigma, l.bias_mu, l.bias_sigma)])
    eps = torch.cat([b.reshape(-1) for l in layers for b in (l.weight_epsilon, l.bias_epsilon)])
    return params, eps


def effective_of(net, requires_grad=False):
    """The effective buffer by torch's own ops: W_fc | b_fc | W_out | b_out, the value stream's rows first."""
    v0, v2, a0, a2 = net.noisy_layers()
    W = lambda l: l.weight_mu + l.weight_sigma * l.weight_epsilon  # noqa: E731
    b = lambda l: l.bias_mu + l.bias_sigma * l.bias_epsilon  # noqa: E731
    parts = [W(v0), W(a0), b(v0), b(a0), W(v2), W(a2), b(v2), b(a2)]
    return torch.cat([p.reshape(-1) for p in parts])


def reference_noisy(net, g):
    """(effective, flat gradient of the head's parameters under the upstream gradient ``g``) by torch and autograd."""
    for p in net.parameters():
        p.grad = None
    eff = effective_of(net)
    eff.backward(g)
    grads = torch.cat([p.grad.reshape(-1) for l in net.noisy_layers() for p in (l.weight_mu, l.weight_sigma, l.bias_mu, l.bias_sigma)])
    return eff.detach(), grads


def run_noisy(mod, dev, n, na, T, K=None):
    new = (lambda nm, shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)) if K is None else K.new
    E, P = mod.rainbow_noisy_counts(n, na)
    eff, grads = new("effective", (E,)), new("grads", (P,))
    mod.rainbow_noisy_compose(T["params"], T["eps"], eff, n, na)
    mod.rainbow_noisy_grad(T["g"], T["eps"], grads, n, na)
    return dict(effective=eff, grads=grads)


# ================================================================================================== guard bands
GUARD_PER = [(1, 1), (3, 5), (37, 32), (5, 1024)]                # (slots, batch): the smallest, leaves at two depths, several levels, the widest batch
GUARD_NOISY = [(2, 2), (6, 5), (9, 101)]


def bounds_per_case(slots, B):
    """A ``bounds_cases.Case`` (not registered in ``bounds_cases.CASES``) over the buffer's four entry points: the rings, the tree, the
    state words, the staged transition and the batch are carved."""
    import bounds_cases as Bc

    def run(mod, dev, T, K):
        K.stage("rainbow buffer")
        out = run_per(mod, dev, slots, B, T, K)
        return {k: out[k] for k in PER_OUTS}

    return Bc.Case(f"rainbow buffer slots={slots} B={B}", lambda: per_script(slots, B), run, PER_OUTS, False, True, None, None)


def bounds_noisy_case(n, na):
    import bounds_cases as Bc

    def build():
        params, eps = noisy_flat(make_network(n, na))
        return dict(params=params, eps=eps, g=torch.randn(eps.numel(), generator=torch.Generator().manual_seed(n + na)))

    def run(mod, dev, T, K):
        K.stage("rainbow noisy layers")
        return run_noisy(mod, dev, n, na, T, K)

    return Bc.Case(f"rainbow noisy n={n} atoms={na}", build, run, ("effective", "grads"), False, True, None, None)


# ================================================================================================== the dueling distributional head
HID, H2 = 512, 1024
HEAD_OUTS = ("act", "q", "dh", "dw", "db", "scalars", "loss_per_sample", "best", "next_pmfs", "target_pmfs")
# (M, n, n_atoms): one row of the smallest head; a ragged row tile; the script's shape (19 x 51 = 969 outputs: 31 output tiles, the last
# ragged, the value / advantage boundary inside a tile); 19 x 53 = 1007 and 10 x 101 = 1010 of the 1024 outputs; 1024 rows
GPU_HEADS = [(1, 2, 2), (5, 6, 5), (32, 18, 51), (9, 18, 53), (3, 9, 101), (1024, 2, 2)]
GUARD_HEADS = [(1, 2, 2), (5, 6, 5), (9, 9, 101), (1024, 2, 2)]  # the last: the most rows


def make_head_case(M, n, na, seed=0, v_min=-10.0, v_max=10.0, gamma=0.99, n_step=3, tie=False):
    """Effective output layers of two seeded NoisyLinear pairs on post-ReLU rows of both streams.  The first rows' rewards and dones walk
    the projection's edges: b integral inside, b = 0, b at the top, both clamps.  ``tie``: actions 0 and 1 are exact copies in both heads."""
    from cleanrl_amd.agents import NoisyLinear

    torch.manual_seed(6000 + 97 * seed + 7 * M + 3 * n + na)
    J = (n + 1) * na

    def effective():
        v, a = NoisyLinear(HID, na), NoisyLinear(HID, n * na)
        W = lambda l: (l.weight_mu + l.weight_sigma * l.weight_epsilon).detach()  # noqa: E731
        b = lambda l: (l.bias_mu + l.bias_sigma * l.bias_epsilon).detach()  # noqa: E731
        return torch.cat([W(v), W(a)]).contiguous(), torch.cat([b(v), b(a)]).contiguous()

    (w, b), (wt, bt) = effective(), effective()
    if tie:
        for t in (w, b, wt, bt):
            t[na:].view(n, na, -1)[1] = t[na:].view(n, na, -1)[0]
    g = torch.Generator().manual_seed(seed + M)
    h, hn, hnt = (torch.relu(torch.randn((M, H2), generator=g)) for _ in range(3))
    actions = torch.randint(0, n, (M,), generator=g)
    rewards = torch.randn(M, generator=g) * 3
    dones = (torch.rand(M, generator=g) < 0.3).float()
    weights = torch.rand(M, generator=g) * 0.9 + 0.1
    weights[0] = 1.0
    mid = v_min + (v_max - v_min) * ((na - 1) // 2) / (na - 1)
    edge = [(mid, 1.0), (v_min, 1.0), (v_max, 1.0), (v_max + 15.0, 0.0), (v_min - 15.0, 0.0), (v_max + 15.0, 1.0), (v_min - 15.0, 1.0)]
    for r, (rew, dn) in enumerate(edge[:M - 1]):
        rewards[r], dones[r] = rew, dn
    return SimpleNamespace(M=M, n=n, na=na, J=J, h=h, h_next=hn, h_next_target=hnt, w=w, b=b, wt=wt, bt=bt, actions=actions, rewards=rewards,
                           dones=dones, weights=weights, support=torch.linspace(v_min, v_max, na), gamma=gamma, n_step=n_step, v_min=v_min,
                           v_max=v_max)


def reference_head(c, dtype):
    """rainbow_atari.py's training lines behind the trunks, on the effective output layers -> dict of the head's outputs."""
    import torch.nn.functional as F

    h, w, b = (t.to(dtype).clone().requires_grad_() for t in (c.h, c.w, c.b))
    hn, hnt, wt, bt, rew, done, wts = (t.to(dtype) for t in (c.h_next, c.h_next_target, c.wt, c.bt, c.rewards, c.dones, c.weights))
    support = torch.linspace(c.v_min, c.v_max, c.na).to(dtype)
    n, na, M = c.n, c.na, c.M

    def dist(x, W, B):
        value = F.linear(x[:, :HID], W[:na], B[:na]).view(-1, 1, na)
        advantage = F.linear(x[:, HID:], W[na:], B[na:]).view(-1, n, na)
        return F.softmax(value + advantage - advantage.mean(dim=1, keepdim=True), dim=2)

    rows = torch.arange(M)
    with torch.no_grad():
        next_dist = dist(hnt, wt, bt)
        next_dist_online = dist(hn, w, b)
        best_actions = torch.argmax(torch.sum(next_dist_online * support, dim=2), dim=1)
        next_pmfs = next_dist[rows, best_actions]
        gamma_n = c.gamma**c.n_step
        next_atoms = rew.reshape(-1, 1) + gamma_n * support * (1 - done.reshape(-1, 1))
        tz = next_atoms.clamp(c.v_min, c.v_max)
        delta_z = (c.v_max - c.v_min) / (na - 1)
        bb = (tz - c.v_min) / delta_z
        l = bb.floor().clamp(0, na - 1)
        u = bb.ceil().clamp(0, na - 1)
        d_m_l = (u + (l == bb).to(dtype) - bb) * next_pmfs
        d_m_u = (bb - l) * next_pmfs
        target_pmfs = torch.zeros_like(next_pmfs)
        for i in range(M):
            target_pmfs[i].index_add_(0, l[i].long(), d_m_l[i])
            target_pmfs[i].index_add_(0, u[i].long(), d_m_u[i])
    d = dist(h, w, b)
    q = torch.sum(d * support, dim=2)
    pred_dist = d[rows, c.actions]
    log_pred = torch.log(pred_dist.clamp(min=1e-5, max=1 - 1e-5))
    loss_per_sample = -(target_pmfs * log_pred).sum(dim=1)
    loss = (loss_per_sample * wts).mean()
    q_values = (pred_dist * support).sum(dim=1).mean()
    loss.backward()
    return dict(act=torch.argmax(q, 1), q=q.detach(), scalars=torch.stack([loss.detach(), q_values.detach()]), dh=h.grad, dw=w.grad, db=b.grad,
                loss_per_sample=loss_per_sample.detach(), best=best_actions, next_pmfs=next_pmfs, target_pmfs=target_pmfs)


def run_heads(mod, c, dev, K=None):
    """Both head entry points through ``mod`` on ``dev`` -> dict of tensors."""
    new = (lambda name, shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)) if K is None else K.new
    d = (lambda t: t.to(dev)) if K is None else (lambda t: t)
    M, n, na, J = c.M, c.n, c.na, c.J
    h, hn, hnt, w, b, wt, bt, support, actions, rewards, dones, weights = (d(t) for t in (
        c.h, c.h_next, c.h_next_target, c.w, c.b, c.wt, c.bt, c.support, c.actions, c.rewards, c.dones, c.weights))
    out = dict(act=new("actions", (M,), torch.int64), q=new("q", (M, n)), dh=new("dh", (M, H2)), dw=new("dw", (J, HID)), db=new("db", (J,)),
               scalars=new("scalars", (2,)), loss_per_sample=new("loss_per_sample", (M,)), best=new("best", (M,), torch.int64),
               next_pmfs=new("next_pmfs", (M, na)), target_pmfs=new("target_pmfs", (M, na)))
    mod.rainbow_head_act(h, w, b, support, n, out["act"], q_out=out["q"])
    mod.rainbow_head_fwd_bwd(h, hn, hnt, w, b, wt, bt, support, actions, rewards, dones, weights, n, c.gamma**c.n_step, c.v_min, c.v_max,
                             out["dh"], out["dw"], out["db"], out["scalars"], out["loss_per_sample"], out["best"], out["next_pmfs"],
                             out["target_pmfs"])
    return out


def bounds_head_case(M, n, na):
    import bounds_cases as Bc

    keys = ("h", "h_next", "h_next_target", "w", "b", "wt", "bt", "support", "actions", "rewards", "dones", "weights")

    def build():
        c = make_head_case(M, n, na)
        return {k: getattr(c, k) for k in keys}

    def run(mod, dev, T, K):
        c = SimpleNamespace(M=M, n=n, na=na, J=(n + 1) * na, gamma=0.99, n_step=3, v_min=-10.0, v_max=10.0, **{k: T[k] for k in keys})
        K.stage("rainbow heads")
        return run_heads(mod, c, dev, K)

    return Bc.Case(f"rainbow heads M={M} n={n} atoms={na}", build, run, HEAD_OUTS, True, True, None, None)
