"""Shared case builders and references for the Atari DQN / C51 kernels (csrc/dqn_atari.hip) and their host twins: the u8 frame ring
of the reference's memory-optimised ``ReplayBuffer`` and the wide Q heads behind ``Linear(3136, 512)``."""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from dqn_cases import projection
from offpolicy_cases import same, within_bar  # noqa: F401

FRAME = (84, 84, 4)
HID = 512


# ================================================================================================== the frame ring
class RefRing:
    """The rules of ``ReplayBuffer(..., optimize_memory_usage=True, handle_timeout_termination=False)``: ONE observation array in the
    env's own layout (slots, N, 4, 84, 84); ``add`` writes obs to ``pos`` and then next_obs to ``(pos + 1) % slots``; ``sample`` skips
    ``pos`` when full; a sample's next_obs is the frame one slot on."""

    def __init__(self, buffer_size, N):
        self.slots, self.N = max(buffer_size // N, 1), N
        self.observations = np.zeros((self.slots, N, 4, 84, 84), np.uint8)
        self.actions = np.zeros((self.slots, N), np.int64)
        self.rewards = np.zeros((self.slots, N), np.float32)
        self.dones = np.zeros((self.slots, N), np.float32)
        self.pos, self.full = 0, False

    def add(self, obs, next_obs, action, reward, done):
        self.observations[self.pos] = np.array(obs)
        self.observations[(self.pos + 1) % self.slots] = np.array(next_obs)
        self.actions[self.pos] = np.array(action)
        self.rewards[self.pos] = np.array(reward)
        self.dones[self.pos] = np.array(done)
        self.pos += 1
        if self.pos == self.slots:
            self.full, self.pos = True, 0

    def sample_indices(self, batch_size):
        if self.full:
            batch_inds = (np.random.randint(1, self.slots, size=batch_size) + self.pos) % self.slots
        else:
            batch_inds = np.random.randint(0, self.pos, size=batch_size)
        return batch_inds, np.random.randint(0, high=self.N, size=(len(batch_inds),))

    def get(self, bi, ei):
        return (self.observations[bi, ei], self.observations[(bi + 1) % self.slots, ei], self.actions[bi, ei], self.rewards[bi, ei],
                self.dones[bi, ei])

    def frames_hwc(self):
        """The observation array in the device ring's layout (slots, N, 84, 84, 4)."""
        return torch.from_numpy(self.observations).permute(0, 1, 3, 4, 2).contiguous()


def new_ring(slots, N, dev, K=None):
    mk = (lambda nm, shape, dt: torch.zeros(shape, dtype=dt, device=dev)) if K is None else (lambda nm, shape, dt: K.new(nm, shape, dt).zero_())
    return (mk("ring frames", (slots, N) + FRAME, torch.uint8), mk("ring actions", (slots, N), torch.int64),
            mk("ring rewards", (slots, N), torch.float32), mk("ring dones", (slots, N), torch.float32))


def ring_steps(slots, N, steps, seed=0):
    """``steps`` transitions of N envs: an episode is truncated every 5th step, where next_obs is a ``final_observation`` the
    following obs does not continue (the reference then overwrites it in slot pos + 1 with that obs)."""
    g = torch.Generator().manual_seed(100 * slots + 10 * N + seed)
    out, obs = [], torch.randint(0, 256, (N, 4, 84, 84), dtype=torch.uint8, generator=g)
    for t in range(steps):
        nxt = torch.randint(0, 256, (N, 4, 84, 84), dtype=torch.uint8, generator=g)
        out.append((obs, nxt, torch.randint(0, 18, (N,), generator=g), torch.randn(N, generator=g), (torch.rand(N, generator=g) < 0.3).float()))
        obs = torch.randint(0, 256, (N, 4, 84, 84), dtype=torch.uint8, generator=g) if t % 5 == 4 else nxt
    return out


def run_ring(mod, dev, slots, N, steps, K=None):
    """The adds through ``mod`` and through ``RefRing`` side by side, then a gather of every slot -> (device ring, RefRing, gathered)."""
    ring, ref = new_ring(slots, N, dev, K), RefRing(slots * N, N)
    new = (lambda nm, shape, dt: torch.zeros(shape, dtype=dt, device=dev)) if K is None else K.new
    d = (lambda t, nm: t.to(dev)) if K is None else (lambda t, nm: K.input(t, nm))
    for s in steps:
        mod.replay_add_u8(ring, ref.pos, *[d(t.contiguous(), nm) for t, nm in zip(s, ("obs", "next_obs", "actions", "rewards", "dones"))])
        ref.add(*[t.numpy() for t in s])
    bi = torch.arange(slots).repeat_interleave(N)
    ei = torch.arange(N).repeat(slots)
    bi = torch.cat([bi, torch.tensor([slots + 3, -2])])                      # clamped into the ring
    ei = torch.cat([ei, torch.tensor([N + 1, -1])])
    M = bi.numel()
    out = (new("frames", (2 * M,) + FRAME, torch.uint8), new("actions", (M,), torch.int64), new("rewards", (M,), torch.float32),
           new("dones", (M,), torch.float32))
    mod.replay_gather_u8(ring, d(bi, "batch_inds"), d(ei, "env_inds"), *out)
    return ring, ref, (bi.clamp(0, slots - 1).numpy(), ei.clamp(0, N - 1).numpy()), out


# ================================================================================================== the heads
def make_head_case(M, n, na, seed=0, v_min=-10.0, v_max=10.0, gamma=0.99, tie=False, dead=False):
    """Two heads from torch's own ``nn.Linear(512, n * n_atoms)`` initialisation on post-ReLU rows.  The first rows' rewards and dones
    walk the projection's edges: b integral inside, b = 0, b at the top, both clamps.  ``tie``: actions 0 and 1 are exact copies in
    both heads.  ``dead``: atom 0 of every action is pushed below the pmf clamp in the online head."""
    torch.manual_seed(3000 + 97 * seed + 7 * M + 3 * n + na)
    J = n * na
    lin, lin_t = torch.nn.Linear(HID, J), torch.nn.Linear(HID, J)
    w, b, wt, bt = (t.detach().clone() for t in (lin.weight, lin.bias, lin_t.weight, lin_t.bias))
    if tie:
        for t in (w, b, wt, bt):
            t.view(n, na, -1)[1] = t.view(n, na, -1)[0]
    if dead:
        b.view(n, na)[:, 0] -= 30.0
    g = torch.Generator().manual_seed(seed + M)
    h, hn = torch.relu(torch.randn((M, HID), generator=g)), torch.relu(torch.randn((M, HID), generator=g))
    actions = torch.randint(0, n, (M,), generator=g)
    if n > 2:
        actions[actions == n - 1] = 0                                        # the last action is never taken: its dW rows are zeros
    rewards = torch.randn(M, generator=g) * 3
    dones = (torch.rand(M, generator=g) < 0.3).float()
    mid = v_min + (v_max - v_min) * ((na - 1) // 2) / max(na - 1, 1)        # an atom's own value: tz lands on it when done
    edge = [(mid, 1.0), (v_min, 1.0), (v_max, 1.0), (v_max + 15.0, 0.0), (v_min - 15.0, 0.0), (v_max + 15.0, 1.0), (v_min - 15.0, 1.0)]
    for r, (rew, dn) in enumerate(edge[:M - 1]):                             # the last row stays random
        rewards[r], dones[r] = rew, dn
    atoms = torch.linspace(v_min, v_max, steps=na) if na > 1 else None
    return SimpleNamespace(M=M, n=n, na=na, J=J, h=h, h_next=hn, w=w, b=b, wt=wt, bt=bt, actions=actions, rewards=rewards, dones=dones,
                           atoms=atoms, gamma=gamma, v_min=v_min, v_max=v_max)


def q_of(z, c, atoms):
    """Q values (M, n) of head outputs z (M, J), and the pmfs (None for DQN)."""
    if c.na == 1:
        return z, None
    pmfs = torch.softmax(z.view(len(z), c.n, c.na), dim=2)
    return (pmfs * atoms).sum(2), pmfs


def reference_head(c, dtype):
    """The training lines of dqn_atari.py / c51_atari.py behind the trunks -> dict(q, scalars, dh, dw, db, aux_a, aux_b)."""
    h, w, b = (t.to(dtype).clone().requires_grad_() for t in (c.h, c.w, c.b))
    hn, wt, bt, rew, done = (t.to(dtype) for t in (c.h_next, c.wt, c.bt, c.rewards, c.dones))
    atoms = None if c.atoms is None else c.atoms.to(dtype)
    rows = torch.arange(c.M)
    z = F.linear(h, w, b)
    with torch.no_grad():
        tq, tpm = q_of(F.linear(hn, wt, bt), c, atoms)
        if c.na == 1:
            target_max, _ = tq.max(dim=1)
            aux_a, aux_b = tq, rew + c.gamma * target_max * (1 - done)
        else:
            aux_a = tpm[rows, torch.argmax(tq, 1)]
            aux_b = projection(aux_a, rew.reshape(-1, 1), done.reshape(-1, 1), atoms, c.gamma, c.v_min, c.v_max)
    q, pm = q_of(z, c, atoms)
    if c.na == 1:
        old_val = q.gather(1, c.actions.reshape(-1, 1)).squeeze(1)
        loss = F.mse_loss(aux_b, old_val)
    else:
        old_pmfs = pm[rows, c.actions]
        loss = (-(aux_b * old_pmfs.clamp(min=1e-5, max=1 - 1e-5).log()).sum(-1)).mean()
        old_val = (old_pmfs * atoms).sum(1)
    loss.backward()
    return dict(q=q.detach(), scalars=torch.stack([loss.detach(), old_val.mean().detach()]), dh=h.grad, dw=w.grad, db=b.grad, aux_a=aux_a,
                aux_b=aux_b)


def run_heads(mod, c, dev, K=None):
    """The head entry points through ``mod`` (ops or host_ops) on ``dev`` -> dict of tensors.  ``K``: the allocator of the outputs
    (bounds_cases.Plain / Carved) when the case's tensors are already placed; None: torch.zeros and ``.to(dev)``."""
    new = (lambda name, shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)) if K is None else K.new
    d = (lambda t: t.to(dev)) if K is None else (lambda t: t)
    M, n, na, J = c.M, c.n, c.na, c.J
    h, hn, w, b, wt, bt, actions, rewards, dones = (d(t) for t in (c.h, c.h_next, c.w, c.b, c.wt, c.bt, c.actions, c.rewards, c.dones))
    atoms = None if na == 1 else d(c.atoms)
    act, q = new("actions", (M,), torch.int64), new("q", (M, n))
    mod.dqn_head_act(h, w, b, n, act, atoms=atoms, q_out=q)
    dh, dw, db, sc = new("dh", (M, HID)), new("dw", (J, HID)), new("db", (J,)), new("scalars", (2,))
    if na == 1:
        aux_a, aux_b = new("target_q", (M, n)), new("td_target", (M,))
        mod.dqn_head_td_fwd_bwd(h, hn, w, b, wt, bt, actions, rewards, dones, n, c.gamma, dh, dw, db, sc, aux_a, aux_b)
    else:
        aux_a, aux_b = new("next_pmfs", (M, na)), new("target_pmfs", (M, na))
        mod.c51_head_fwd_bwd(h, hn, w, b, wt, bt, atoms, actions, rewards, dones, n, c.gamma, c.v_min, c.v_max, dh, dw, db, sc, aux_a, aux_b)
    return dict(act=act, q=q, dh=dh, dw=dw, db=db, scalars=sc, aux_a=aux_a, aux_b=aux_b)


HEAD_OUTS = ("act", "q", "dh", "dw", "db", "scalars", "aux_a", "aux_b")
# M x n x n_atoms of the issue's grid: one row, a ragged row tile, the scripts' batch; the smallest game, Pong's, the full action set;
# DQN, the smallest C51, one below an output tile's 32 per action, the scripts' 51 (18 x 51 = 918 outputs: 29 output tiles, the last ragged)
HEAD_GRID = [(M, n, na) for M in (1, 5, 32) for n in (2, 6, 18) for na in (1, 2, 5, 51)]
# a smaller walk through every M / n / n_atoms for the device, plus the limits: 1024 outputs (18 x 56 = 1008, 10 x 101 = 1010), 1024 rows
GPU_HEADS = [(1, 2, 1), (5, 6, 2), (32, 18, 51), (32, 6, 1), (5, 18, 5), (1, 6, 51), (32, 2, 5), (9, 18, 56), (3, 10, 101), (1024, 2, 2)]
# guard bands: the smallest outputs, a ragged row and output tile, the scripts' two shapes, the widest head
GUARD_HEADS = [(1, 2, 1), (5, 6, 5), (32, 18, 1), (32, 18, 51), (9, 10, 101)]
GUARD_RINGS = [(1, 1), (2, 3), (7, 1)]


def bounds_head_case(M, n, na):
    """A ``bounds_cases.Case`` (not registered in ``bounds_cases.CASES``) over the three head entry points."""
    import bounds_cases as B

    def build():
        c = make_head_case(M, n, na)
        d = dict(h=c.h, h_next=c.h_next, w=c.w, b=c.b, wt=c.wt, bt=c.bt, actions=c.actions, rewards=c.rewards, dones=c.dones,
                 dims=(M, n, na), hp=(c.gamma, c.v_min, c.v_max))
        if na > 1:
            d["atoms"] = c.atoms
        return d

    def run(mod, dev, T, K):
        c = SimpleNamespace(M=M, n=n, na=na, J=n * na, atoms=T.get("atoms"), gamma=T["hp"][0], v_min=T["hp"][1], v_max=T["hp"][2],
                            **{k: T[k] for k in ("h", "h_next", "w", "b", "wt", "bt", "actions", "rewards", "dones")})
        K.stage("dqn_atari heads")
        return run_heads(mod, c, dev, K)

    return B.Case(f"dqn_atari heads M={M} n={n} atoms={na}", build, run, HEAD_OUTS, True, True, None, None)


def bounds_ring_case(slots, N):
    """A ``bounds_cases.Case`` over the ring's add and gather: the ring itself, the staged step and the batch are carved."""
    import bounds_cases as B

    def build():
        return dict(steps=ring_steps(slots, N, slots + 2))

    def run(mod, dev, T, K):
        K.stage("dqn_atari ring")
        ring, _, _, out = run_ring(mod, dev, slots, N, T["steps"], K)
        return dict(zip(("ring_frames", "ring_actions", "ring_rewards", "ring_dones", "frames", "actions", "rewards", "dones"), ring + out))

    outs = ("ring_frames", "ring_actions", "ring_rewards", "ring_dones", "frames", "actions", "rewards", "dones")
    return B.Case(f"dqn_atari ring slots={slots} N={N}", build, run, outs, False, True, None, None)


# ================================================================================================== the learner
def atari_env(n, N=1):
    from cleanrl_amd.envs import SamplingDiscrete

    return SimpleNamespace(single_observation_space=SimpleNamespace(shape=(4, 84, 84)), single_action_space=SamplingDiscrete(n), num_envs=N)


def make_learner(dev, c51, backend, M=8, slots=16, n=6, n_atoms=5, fill=False, seed=0):
    """An ``AtariDQNLearner`` on torch's own initialisation; ``fill``: a ring that has wrapped, through ``store``."""
    from cleanrl_amd.agents import AtariC51Network, AtariDQNNetwork
    from cleanrl_amd.learner_dqn_atari import AtariDQNLearner

    torch.manual_seed(4000 + seed)
    env = atari_env(n)
    mk = (lambda: AtariC51Network(env, n_atoms=n_atoms, v_min=-2.0, v_max=2.0)) if c51 else (lambda: AtariDQNNetwork(env))
    q, t = mk().to(dev), mk().to(dev)
    args = SimpleNamespace(buffer_size=slots, batch_size=M, learning_rate=1e-4, gamma=0.99, tau=1.0, n_atoms=n_atoms, v_min=-2.0, v_max=2.0)
    L = AtariDQNLearner(q, t, args, env, dev, c51=c51, backend=backend)
    if fill:
        for s in ring_steps(slots, 1, slots + 3, seed=seed):
            step = [x.numpy() for x in s]
            step[2] = step[2] % n
            L.store(*step)
    return L


def reference_update(L, bi, ei, dtype):
    """The reference's training lines on the fused learner's own ring and networks in ``dtype`` -> dict(scalars, grads)."""
    import copy

    a = L.args
    q, t = copy.deepcopy(L.q_network).to("cpu", dtype), copy.deepcopy(L.target_network).to("cpu", dtype)
    for p in q.parameters():
        p.grad = None
    frames, actions, rewards, dones = (x.cpu() for x in L.ring)
    bi, ei = torch.as_tensor(bi), torch.as_tensor(ei)
    obs = frames[bi, ei].permute(0, 3, 1, 2).to(dtype)
    nxt = frames[(bi + 1) % L.slots, ei].permute(0, 3, 1, 2).to(dtype)
    act, rew, done = actions[bi, ei], rewards[bi, ei].to(dtype), dones[bi, ei].to(dtype)
    if L.c51:
        with torch.no_grad():
            _, next_pmfs = t.get_action(nxt)
            target_pmfs = projection(next_pmfs, rew.reshape(-1, 1), done.reshape(-1, 1), t.atoms, a.gamma, a.v_min, a.v_max)
        _, old_pmfs = q.get_action(obs, act)
        loss = (-(target_pmfs * old_pmfs.clamp(min=1e-5, max=1 - 1e-5).log()).sum(-1)).mean()
        old_val = (old_pmfs * q.atoms).sum(1)
    else:
        with torch.no_grad():
            target_max, _ = t(nxt).max(dim=1)
            td_target = rew + a.gamma * target_max * (1 - done)
        old_val = q(obs).gather(1, act.reshape(-1, 1)).squeeze(1)
        loss = F.mse_loss(td_target, old_val)
    loss.backward()
    return dict(scalars=torch.stack([loss.detach(), old_val.mean().detach()]), grads=torch.cat([p.grad.reshape(-1) for p in q.parameters()]))
