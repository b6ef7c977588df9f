"""Shared case builders and references for the DQN / C51 kernels (csrc/dqn.hip) and their host twins."""
import copy
from types import SimpleNamespace

import torch

from cleanrl_amd.agents import C51Network, DQNNetwork
from cleanrl_amd.ops import dqn_counts
from offpolicy_cases import flat, same, within_bar  # noqa: F401


def fake_env(O, n):
    return SimpleNamespace(single_observation_space=SimpleNamespace(shape=(O,)), single_action_space=SimpleNamespace(n=n), num_envs=1)


def make_case(O, n, na, M, N=3, slots=7, seed=0, v_min=-10.0, v_max=10.0, gamma=0.99):
    """Networks from torch's own initialisation, a random ring (a ring of 7 slots that has wrapped: every slot is live) and a batch."""
    torch.manual_seed(2000 + seed + O + n + na)
    env = fake_env(O, n)
    mk = (lambda: C51Network(env, n_atoms=na, v_min=v_min, v_max=v_max)) if na > 1 else (lambda: DQNNetwork(env))
    nets = SimpleNamespace(online=mk(), target=mk())
    g = torch.Generator().manual_seed(seed + M)
    ring = (torch.randn((slots, N, O), generator=g), torch.randn((slots, N, O), generator=g),
            torch.randint(0, n, (slots, N, 1), generator=g).float(), torch.randn((slots, N), generator=g) * 3,
            (torch.rand((slots, N), generator=g) < 0.3).float())
    bi, ei = torch.randint(0, slots, (M,), generator=g), torch.randint(0, N, (M,), generator=g)
    c = SimpleNamespace(O=O, n=n, na=na, M=M, N=N, slots=slots, nets=nets, ring=ring, bi=bi, ei=ei, gamma=gamma, v_min=v_min, v_max=v_max,
                        online=flat(nets.online), target=flat(nets.target), atoms=nets.online.atoms.clone() if na > 1 else None)
    assert c.online.numel() == dqn_counts(O, n, na)
    return c


def batch(c, dtype):
    obs, nxt, act, rew, done = c.ring
    return (obs[c.bi, c.ei].to(dtype), act[c.bi, c.ei].long(), nxt[c.bi, c.ei].to(dtype), done[c.bi, c.ei].reshape(-1, 1).to(dtype),
            rew[c.bi, c.ei].reshape(-1, 1).to(dtype))


def copies(c, dtype):
    n = copy.deepcopy(c.nets)
    n.online.to(dtype), n.target.to(dtype)
    return n


def projection(next_pmfs, rewards, dones, atoms, gamma, v_min, v_max):
    """c51.py's projection lines on given ``next_pmfs`` -> target_pmfs."""
    n_atoms = atoms.numel()
    next_atoms = rewards + gamma * atoms * (1 - dones)
    delta_z = atoms[1] - atoms[0]
    tz = next_atoms.clamp(v_min, v_max)
    b = (tz - v_min) / delta_z
    l = b.floor().clamp(0, n_atoms - 1)  # noqa: E741
    u = b.ceil().clamp(0, n_atoms - 1)
    d_m_l = (u + (l == u).float() - b) * next_pmfs
    d_m_u = (b - l) * next_pmfs
    target_pmfs = torch.zeros_like(next_pmfs)
    for i in range(target_pmfs.size(0)):
        target_pmfs[i].index_add_(0, l[i].long(), d_m_l[i])
        target_pmfs[i].index_add_(0, u[i].long(), d_m_u[i])
    return target_pmfs


def reference_dqn(c, dtype):
    """dqn.py's training lines -> dict(grads, scalars, target_q, td_target)."""
    n = copies(c, dtype)
    obs, act, nxt, done, rew = batch(c, dtype)
    with torch.no_grad():
        tq = n.target(nxt)
        target_max, _ = tq.max(dim=1)
        td_target = rew.flatten() + c.gamma * target_max * (1 - done.flatten())
    old_val = n.online(obs).gather(1, act).squeeze(1)
    loss = torch.nn.functional.mse_loss(td_target, old_val)
    loss.backward()
    return dict(grads=flat_grad(n.online), scalars=torch.stack([loss.detach(), old_val.mean().detach()]), aux_a=tq, aux_b=td_target)


def reference_c51(c, dtype):
    """c51.py's training lines -> dict(grads, scalars, next_pmfs, target_pmfs)."""
    n = copies(c, dtype)
    obs, act, nxt, done, rew = batch(c, dtype)
    with torch.no_grad():
        _, next_pmfs = n.target.get_action(nxt)
        target_pmfs = projection(next_pmfs, rew, done, n.target.atoms, c.gamma, c.v_min, c.v_max)
    _, old_pmfs = n.online.get_action(obs, act.flatten())
    loss = (-(target_pmfs * old_pmfs.clamp(min=1e-5, max=1 - 1e-5).log()).sum(-1)).mean()
    loss.backward()
    old_val = (old_pmfs * n.online.atoms).sum(1)
    return dict(grads=flat_grad(n.online), scalars=torch.stack([loss.detach(), old_val.mean().detach()]), aux_a=next_pmfs, aux_b=target_pmfs)


def flat_grad(net):
    return torch.cat([p.grad.reshape(-1) for p in net.parameters()])


def reference_act(c, obs, dtype):
    n = copies(c, dtype)
    with torch.no_grad():
        if c.na > 1:
            pmfs = torch.softmax(n.online.network(obs.to(dtype)).view(len(obs), c.n, c.na), dim=2)
            q = (pmfs * n.online.atoms).sum(2)
        else:
            q = n.online(obs.to(dtype))
    return q


def act_rows(c):
    """The observations the act entry point is run on: the batch's first rows (at most 11: a tile and a ragged one)."""
    Nr = min(c.M, 11)
    return c.ring[0][c.bi[:Nr].clamp(0, c.slots - 1), c.ei[:Nr].clamp(0, c.N - 1)].contiguous()


def run_entry_points(mod, c, dev, K=None):
    """Every entry point through ``mod`` (ops or host_ops) on ``dev`` -> dict of tensors.  ``K``: the allocator of the outputs
    (bounds_cases.Plain / Carved); None: torch.zeros."""
    new = (lambda name, shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)) if K is None else K.new
    d = lambda t: t if K is not None else t.to(dev)  # noqa: E731
    ring = tuple(d(t) for t in c.ring)
    M, n, na = c.M, c.n, c.na
    P = c.online.numel()
    Nr = min(M, 11)
    obs = c.act_obs if K is not None else d(act_rows(c))
    acts, q = new("actions", (obs.shape[0],), torch.int64), new("q", (obs.shape[0], n))
    atoms = None if na == 1 else d(c.atoms)
    mod.dqn_act(obs, d(c.online), n, acts, atoms=atoms, q_out=q)
    grads, sc = new("grads", (P,)), new("scalars", (2,))
    if na == 1:
        aux_a, aux_b = new("target_q", (M, n)), new("td_target", (M,))
        mod.dqn_td_fwd_bwd(ring, d(c.bi), d(c.ei), d(c.online), d(c.target), n, c.gamma, grads, sc, aux_a, aux_b)
    else:
        aux_a, aux_b = new("next_pmfs", (M, na)), new("target_pmfs", (M, na))
        mod.c51_fwd_bwd(ring, d(c.bi), d(c.ei), d(c.online), d(c.target), atoms, n, c.gamma, c.v_min, c.v_max, grads, sc, aux_a, aux_b)
    return dict(act=acts, q=q, grads=grads, scalars=sc, aux_a=aux_a, aux_b=aux_b)


# the shapes of tests/test_gpu_dqn.py: O, n, n_atoms, M, N -- every O / n / n_atoms / M / N of the list at least once, n * n_atoms <= 512
# (18 x 28 = 504 is the edge), a partial row tile (5, 37), one row, the script's batch (128: 16 tiles)
GPU_SHAPES = [(4, 2, 1, 128, 1), (4, 2, 101, 128, 1), (8, 3, 51, 37, 3), (65, 18, 1, 5, 3), (65, 18, 28, 37, 1), (8, 2, 5, 1, 3),
              (4, 3, 101, 5, 1), (65, 3, 1, 37, 3), (8, 18, 5, 128, 3), (4, 5, 101, 1, 1)]


def bounds_case(O, n, na, M, N):
    """A ``bounds_cases.Case`` (not registered in ``bounds_cases.CASES``) over every entry point of the family."""
    import bounds_cases as B

    def build():
        c = make_case(O, n, na, M, N=N)
        d = dict(ring=c.ring, bi=c.bi, ei=c.ei, online=c.online, target=c.target, act_obs=act_rows(c), dims=(O, n, na, M, N, c.slots),
                 hp=(c.gamma, c.v_min, c.v_max))
        if na > 1:
            d["atoms"] = c.atoms
        return d

    def run(mod, dev, T, K):
        O_, n_, na_, M_, N_, slots = T["dims"]
        c = SimpleNamespace(O=O_, n=n_, na=na_, M=M_, N=N_, slots=slots, ring=T["ring"], bi=T["bi"], ei=T["ei"], online=T["online"],
                            target=T["target"], atoms=T.get("atoms"), act_obs=T["act_obs"], gamma=T["hp"][0], v_min=T["hp"][1], v_max=T["hp"][2])
        K.stage("dqn / c51")
        return run_entry_points(mod, c, dev, K)

    return B.Case(f"dqn O={O} n={n} atoms={na} M={M} N={N}", build, run, ("act", "q", "grads", "scalars", "aux_a", "aux_b"), True, True, None, None)
# the guard-band cases (tests/guard_arena.py): one row, a ragged tile, the script's batch; the smallest and the largest outputs
GUARD_SHAPES = [(4, 2, 1, 1, 1), (4, 2, 101, 37, 1), (65, 18, 28, 5, 3), (8, 18, 1, 128, 3), (8, 3, 51, 128, 3)]
