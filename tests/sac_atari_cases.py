"""Shared case builders and references for the discrete-SAC kernels (csrc/sac_atari.hip) and their host twins: the two u8 frame rings
of the reference's plain ``ReplayBuffer`` and the five heads behind ``Linear(3136, 512)``."""
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from dqn_atari_cases import atari_env, ring_steps  # noqa: F401
from offpolicy_cases import same, within_bar  # noqa: F401

FRAME = (84, 84, 4)
HID = 512
GAP = 120.0


# ================================================================================================== the frame rings
class RefRing2:
    """The rules of ``ReplayBuffer(..., handle_timeout_termination=False)`` without ``optimize_memory_usage``: ``observations`` and
    ``next_observations`` are separate arrays in the env's own layout (slots, N, 4, 84, 84), both written at ``pos``."""

    def __init__(self, buffer_size, N):
        self.slots, self.N = max(buffer_size // N, 1), N
        self.observations = np.zeros((self.slots, N, 4, 84, 84), np.uint8)
        self.next_observations = np.zeros((self.slots, N, 4, 84, 84), np.uint8)
        self.actions = np.zeros((self.slots, N), np.int64)
        self.rewards = np.zeros((self.slots, N), np.float32)
        self.dones = np.zeros((self.slots, N), np.float32)
        self.pos, self.full = 0, False

    def add(self, obs, next_obs, action, reward, done):
        self.observations[self.pos] = np.array(obs)
        self.next_observations[self.pos] = np.array(next_obs)
        self.actions[self.pos] = np.array(action)
        self.rewards[self.pos] = np.array(reward)
        self.dones[self.pos] = np.array(done)
        self.pos += 1
        if self.pos == self.slots:
            self.full, self.pos = True, 0

    def get(self, bi, ei):
        return self.observations[bi, ei], self.next_observations[bi, ei], self.actions[bi, ei], self.rewards[bi, ei], self.dones[bi, ei]

    def frames_hwc(self):
        """Both arrays in the device rings' layout (slots, N, 84, 84, 4)."""
        return tuple(torch.from_numpy(a).permute(0, 1, 3, 4, 2).contiguous() for a in (self.observations, self.next_observations))


def new_ring(slots, N, dev, K=None):
    mk = (lambda nm, shape, dt: torch.zeros(shape, dtype=dt, device=dev)) if K is None else (lambda nm, shape, dt: K.new(nm, shape, dt).zero_())
    return (mk("ring obs", (slots, N) + FRAME, torch.uint8), mk("ring next_obs", (slots, N) + FRAME, torch.uint8),
            mk("ring actions", (slots, N), torch.int64), mk("ring rewards", (slots, N), torch.float32), mk("ring dones", (slots, N), torch.float32))


def run_ring(mod, dev, slots, N, steps, K=None):
    """The adds through ``mod`` and through ``RefRing2`` side by side, then a gather of every slot -> (rings, RefRing2, indices, gathered)."""
    ring, ref = new_ring(slots, N, dev, K), RefRing2(slots * N, N)
    new = (lambda nm, shape, dt: torch.zeros(shape, dtype=dt, device=dev)) if K is None else K.new
    d = (lambda t, nm: t.to(dev)) if K is None else (lambda t, nm: K.input(t, nm))
    for s in steps:
        mod.replay_add2_u8(ring, ref.pos, *[d(t.contiguous(), nm) for t, nm in zip(s, ("obs", "next_obs", "actions", "rewards", "dones"))])
        ref.add(*[t.numpy() for t in s])
    bi = torch.arange(slots).repeat_interleave(N)
    ei = torch.arange(N).repeat(slots)
    bi = torch.cat([bi, torch.tensor([slots + 3, -2])])                      # clamped into the ring
    ei = torch.cat([ei, torch.tensor([N + 1, -1])])
    M = bi.numel()
    out = (new("frames", (2 * M,) + FRAME, torch.uint8), new("actions", (M,), torch.int64), new("rewards", (M,), torch.float32),
           new("dones", (M,), torch.float32))
    mod.replay_gather2_u8(ring, d(bi, "batch_inds"), d(ei, "env_inds"), *out)
    return ring, ref, (bi.clamp(0, slots - 1).numpy(), ei.clamp(0, N - 1).numpy()), out


def check_ring_against_model(ring, ref, idx, out):
    """The rings equal the numpy model's arrays and the gathered batch equals ``ReplayBuffer._get_samples`` on it."""
    bi, ei = idx
    hwc = lambda a: torch.from_numpy(a).permute(0, 2, 3, 1).contiguous()  # noqa: E731
    fo, fn = ref.frames_hwc()
    assert torch.equal(ring[0].cpu(), fo) and torch.equal(ring[1].cpu(), fn)
    obs, nxt, act, rew, done = ref.get(bi, ei)
    M = len(bi)
    assert torch.equal(out[0][:M].cpu(), hwc(obs)) and torch.equal(out[0][M:].cpu(), hwc(nxt))
    assert torch.equal(out[1].cpu(), torch.from_numpy(act)) and torch.equal(out[2].cpu(), torch.from_numpy(rew))
    assert torch.equal(out[3].cpu(), torch.from_numpy(done))


# ================================================================================================== the heads
H_KEYS = ("h_q1", "h_q2", "h_pi_next", "h_q1t_next", "h_q2t_next", "h_pi")
NETS = ("q1", "q2", "pi", "q1t", "q2t")


def make_head_case(M, n, seed=0):
    """Five heads with sac_atari.py's ``kaiming_normal_`` weights (biases made non-zero) on post-ReLU rows.  Row 0 is done; rows 0 and 1
    took the same action; the last action is never taken (with two actions every row took action 0); the last row's actor logits
    span a gap of at least ``GAP`` on obs and on next_obs: hidden column 0 feeds actions 0 and 1 with +-(GAP / 2 + 4) and is zero on every other row,
    so there p_1 underflows to 0 in f32 while logp_1 stays finite."""
    g = torch.Generator().manual_seed(5000 + 97 * seed + 7 * M + 3 * n)
    c = SimpleNamespace(M=M, n=n, gamma=0.99, alpha=torch.tensor([0.37]), target_entropy=float(np.float32(0.89 * math.log(n))))
    for k in NETS:
        setattr(c, "w_" + k, torch.randn((n, HID), generator=g) * math.sqrt(2.0 / HID))
        setattr(c, "b_" + k, torch.randn(n, generator=g) * 0.1)
    for k in H_KEYS:
        setattr(c, k, torch.relu(torch.randn((M, HID), generator=g)))
    c.w_pi[:, 0] = 0.0
    c.w_pi[0, 0], c.w_pi[1, 0] = GAP / 2 + 4, -GAP / 2 - 4                # (the other 511 columns move a logit by about 1)
    for k in ("h_pi", "h_pi_next"):
        h = getattr(c, k)
        h[:, 0] = 0.0
        h[M - 1, 0] = 1.0
    c.actions = torch.randint(0, n, (M,), generator=g)
    c.actions[c.actions == n - 1] = 0
    if M > 1:
        c.actions[1] = c.actions[0]
    c.rewards = torch.randn(M, generator=g) * 3
    c.dones = (torch.rand(M, generator=g) < 0.3).float()
    c.dones[0] = 1.0
    c.noise = torch.empty((M, n)).exponential_(generator=g)
    return c


def _policy(h, w, b):
    logits = F.linear(h, w, b)
    return F.log_softmax(logits, dim=1), torch.softmax(logits - logits.logsumexp(dim=-1, keepdim=True), dim=-1)      # Categorical(logits=...).probs


def reference_critic(c, dtype):
    """``# CRITIC training`` of sac_atari.py behind the trunks -> dict(V, y, scalars, dh1, dh2, dw1, db1, dw2, db2)."""
    t = lambda x: x.to(dtype)  # noqa: E731
    h1, h2, w1, b1, w2, b2 = (t(x).clone().requires_grad_() for x in (c.h_q1, c.h_q2, c.w_q1, c.b_q1, c.w_q2, c.b_q2))
    alpha = t(c.alpha).item()
    with torch.no_grad():
        next_state_log_pi, next_state_action_probs = _policy(t(c.h_pi_next), t(c.w_pi), t(c.b_pi))
        qf1_next_target = F.linear(t(c.h_q1t_next), t(c.w_q1t), t(c.b_q1t))
        qf2_next_target = F.linear(t(c.h_q2t_next), t(c.w_q2t), t(c.b_q2t))
        min_qf_next_target = next_state_action_probs * (torch.min(qf1_next_target, qf2_next_target) - alpha * next_state_log_pi)
        min_qf_next_target = min_qf_next_target.sum(dim=1)
        next_q_value = t(c.rewards).flatten() + (1 - t(c.dones).flatten()) * c.gamma * (min_qf_next_target)
    qf1_a_values = F.linear(h1, w1, b1).gather(1, c.actions.reshape(-1, 1)).view(-1)
    qf2_a_values = F.linear(h2, w2, b2).gather(1, c.actions.reshape(-1, 1)).view(-1)
    qf1_loss = F.mse_loss(qf1_a_values, next_q_value)
    qf2_loss = F.mse_loss(qf2_a_values, next_q_value)
    (qf1_loss + qf2_loss).backward()
    sc = torch.stack([qf1_loss, qf2_loss, qf1_a_values.mean(), qf2_a_values.mean()]).detach()
    return dict(V=min_qf_next_target, y=next_q_value, scalars=sc, dh1=h1.grad, dh2=h2.grad, dw1=w1.grad, db1=b1.grad, dw2=w2.grad, db2=b2.grad)


def reference_actor(c, dtype):
    """``# ACTOR training`` and the temperature loss -> dict(actor_loss, e_rows, dh, dw, db, alpha_loss, alpha_grad)."""
    t = lambda x: x.to(dtype)  # noqa: E731
    h, w, b = (t(x).clone().requires_grad_() for x in (c.h_pi, c.w_pi, c.b_pi))
    log_alpha = t(c.alpha).log().clone().requires_grad_()
    alpha = t(c.alpha).item()
    log_pi, action_probs = _policy(h, w, b)
    with torch.no_grad():
        min_qf_values = torch.min(F.linear(t(c.h_q1), t(c.w_q1), t(c.b_q1)), F.linear(t(c.h_q2), t(c.w_q2), t(c.b_q2)))
    actor_loss = (action_probs * ((alpha * log_pi) - min_qf_values)).mean()
    actor_loss.backward()
    alpha_loss = (action_probs.detach() * (-log_alpha.exp() * (log_pi + c.target_entropy).detach())).mean()
    alpha_loss.backward()
    e_rows = (action_probs * (log_pi + c.target_entropy)).sum(1).detach() / c.n
    return dict(actor_loss=actor_loss.detach().reshape(1), e_rows=e_rows, dh=h.grad, dw=w.grad, db=b.grad, alpha_loss=alpha_loss.detach().reshape(1),
                alpha_grad=log_alpha.grad.reshape(1))


CRITIC_OUTS = ("V", "y", "scalars", "dh1", "dh2", "dw1", "db1", "dw2", "db2")
ACTOR_OUTS = ("actor_loss", "e_rows", "dh", "dw", "db")
HEAD_OUTS = ("act", "probs") + CRITIC_OUTS + ACTOR_OUTS


def run_heads(mod, c, dev, K=None):
    """The three head entry points through ``mod`` (ops or host_ops) on ``dev`` -> dict of tensors.  ``K``: the allocator of the
    outputs (bounds_cases.Plain / Carved) when the case's tensors are already placed; None: torch.zeros and ``.to(dev)``."""
    new = (lambda name, shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)) if K is None else K.new
    d = (lambda t: t.to(dev)) if K is None else (lambda t: t)
    M, n = c.M, c.n
    T = {k: d(getattr(c, k)) for k in H_KEYS + ("actions", "rewards", "dones", "alpha", "noise")}
    hd = {k: (d(getattr(c, "w_" + k)), d(getattr(c, "b_" + k))) for k in NETS}
    o = {}
    o["act"], o["probs"] = new("actions", (M,), torch.int64), new("probs", (M, n))
    mod.sacd_head_act(T["h_pi"], *hd["pi"], T["noise"], o["act"], o["probs"])
    for k, shape in (("V", (M,)), ("y", (M,)), ("scalars", (4,)), ("dh1", (M, HID)), ("dh2", (M, HID)), ("dw1", (n, HID)), ("db1", (n,)),
                     ("dw2", (n, HID)), ("db2", (n,)), ("actor_loss", (1,)), ("e_rows", (M,)), ("dh", (M, HID)), ("dw", (n, HID)), ("db", (n,))):
        o[k] = new(k, shape)
    mod.sacd_critic_fwd_bwd(tuple(T[k] for k in H_KEYS[:5]), tuple(hd[k] for k in NETS), T["actions"], T["rewards"], T["dones"], T["alpha"], c.gamma,
                            (o["dh1"], o["dh2"]), ((o["dw1"], o["db1"]), (o["dw2"], o["db2"])), o["scalars"], o["V"], o["y"])
    mod.sacd_actor_fwd_bwd((T["h_pi"], T["h_q1"], T["h_q2"]), (hd["pi"], hd["q1"], hd["q2"]), T["alpha"], c.target_entropy, o["dh"], o["dw"],
                           o["db"], o["e_rows"], o["actor_loss"])
    return o


# M x n of the issue's grids
HEAD_GRID = [(M, n) for M in (1, 5, 64) for n in (2, 6, 18)]
GPU_HEADS = [(1, 2), (5, 6), (9, 18), (64, 6), (64, 18), (1024, 2)]
GUARD_HEADS = [(1, 2), (5, 6), (64, 18), (1024, 2)]
GUARD_RINGS = [(1, 1), (2, 3), (7, 1)]
_T_KEYS = H_KEYS + ("actions", "rewards", "dones", "alpha", "noise") + tuple(p + k for k in NETS for p in ("w_", "b_"))


def bounds_head_case(M, n):
    """A ``bounds_cases.Case`` (not registered in ``bounds_cases.CASES``) over the three head entry points."""
    import bounds_cases as B

    def build():
        c = make_head_case(M, n)
        return dict({k: getattr(c, k) for k in _T_KEYS}, hp=(c.gamma, c.target_entropy))

    def run(mod, dev, T, K):
        c = SimpleNamespace(M=M, n=n, gamma=T["hp"][0], target_entropy=T["hp"][1], **{k: T[k] for k in _T_KEYS})
        K.stage("sac_atari heads")
        return run_heads(mod, c, dev, K)

    return B.Case(f"sac_atari heads M={M} n={n}", build, run, HEAD_OUTS, True, True, None, None)


def bounds_ring_case(slots, N):
    """A ``bounds_cases.Case`` over the two rings' add and gather: the rings, the staged step and the batch are carved."""
    import bounds_cases as B

    outs = ("ring_obs", "ring_next_obs", "ring_actions", "ring_rewards", "ring_dones", "frames", "actions", "rewards", "dones")

    def build():
        return dict(steps=ring_steps(slots, N, slots + 2))

    def run(mod, dev, T, K):
        K.stage("sac_atari ring")
        ring, _, _, out = run_ring(mod, dev, slots, N, T["steps"], K)
        return dict(zip(outs, ring + out))

    return B.Case(f"sac_atari ring slots={slots} N={N}", build, run, outs, False, True, None, None)


# ================================================================================================== the learner
def make_learner(dev, backend, M=8, slots=16, n=6, fill=False, seed=0, autotune=True, tau=1.0):
    """A ``SACAtariLearner`` on the script's own initialisation; ``fill``: rings that have wrapped, through ``store``."""
    from cleanrl_amd.agents import AtariSACActor, AtariSoftQNetwork
    from cleanrl_amd.learner_sac_atari import SACAtariLearner

    torch.manual_seed(6000 + seed)
    env = atari_env(n)
    actor = AtariSACActor(env).to(dev)
    qf1, qf2, t1, t2 = (AtariSoftQNetwork(env).to(dev) for _ in range(4))
    t1.load_state_dict(qf1.state_dict())
    t2.load_state_dict(qf2.state_dict())
    args = SimpleNamespace(buffer_size=slots, batch_size=M, policy_lr=3e-4, q_lr=3e-4, gamma=0.99, tau=tau, alpha=0.2, autotune=autotune,
                           target_entropy_scale=0.89, learning_starts=0)
    L = SACAtariLearner(actor, qf1, qf2, t1, t2, args, env, dev, backend=backend)
    if fill:
        for s in ring_steps(slots, 1, slots + 3, seed=seed):
            step = [x.numpy() for x in s]
            step[2] = step[2] % n
            L.store(*step)
    return L


def reference_update(L, bi, ei, dtype):
    """The reference's training lines on the fused learner's own rings and networks in ``dtype``, every gradient at the same weights
    (``update_kernels(adam=False)``) -> dict(scalars (5: the critic's four and actor_loss), critic_grads, actor_grads), the gradients
    as {parameter name: tensor}."""
    import copy

    a = L.args
    actor, qf1, qf2, t1, t2 = (copy.deepcopy(m).to("cpu", dtype) for m in (L.actor, *L.qfs, *L.qf_targets))
    for m in (actor, qf1, qf2):
        for p in m.parameters():
            p.grad = None
    fo, fn, actions, rewards, dones = (x.cpu() for x in L.ring)
    bi, ei = torch.as_tensor(bi), torch.as_tensor(ei)
    obs = fo[bi, ei].permute(0, 3, 1, 2).to(dtype)
    nxt = fn[bi, ei].permute(0, 3, 1, 2).to(dtype)
    act, rew, done = actions[bi, ei].reshape(-1, 1), rewards[bi, ei].to(dtype), dones[bi, ei].to(dtype)
    alpha = L.alpha_t.item() if L.fused else L.alpha
    with torch.no_grad():
        _, next_state_log_pi, next_state_action_probs = actor.get_action(nxt)
        min_qf_next_target = next_state_action_probs * (torch.min(t1(nxt), t2(nxt)) - alpha * next_state_log_pi)
        next_q_value = rew + (1 - done) * a.gamma * (min_qf_next_target.sum(dim=1))
    qf1_a_values = qf1(obs).gather(1, act).view(-1)
    qf2_a_values = qf2(obs).gather(1, act).view(-1)
    qf1_loss, qf2_loss = F.mse_loss(qf1_a_values, next_q_value), F.mse_loss(qf2_a_values, next_q_value)
    (qf1_loss + qf2_loss).backward()
    _, log_pi, action_probs = actor.get_action(obs)
    with torch.no_grad():
        min_qf_values = torch.min(qf1(obs), qf2(obs))
    actor_loss = (action_probs * ((alpha * log_pi) - min_qf_values)).mean()
    actor_loss.backward()
    sc = torch.stack([qf1_loss, qf2_loss, qf1_a_values.mean(), qf2_a_values.mean(), actor_loss]).detach()
    return dict(scalars=sc, critic_grads={f"qf{i + 1}.{k}": p.grad for i, m in enumerate((qf1, qf2)) for k, p in m.named_parameters()},
                actor_grads={"actor." + k: p.grad for k, p in actor.named_parameters()})


def learner_grads(L):
    """The fused learner's flat gradient cut into {parameter name: tensor} like ``reference_update``'s."""
    got = L.grads.detach().cpu()
    out = {}
    for i, (pre, m) in enumerate((("actor.", L.actor), ("qf1.", L.qfs[0]), ("qf2.", L.qfs[1]))):
        off = i * L.stride
        for k, p in m.named_parameters():
            out[pre + k] = got[off:off + p.numel()].view(p.shape)
            off += p.numel()
    return out
