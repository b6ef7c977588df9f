"""Shared case builders and references for the QDagger head kernels (csrc/qdagger.hip), their host twins and the learner
(cleanrl_amd/learner_qdagger.py): the reference is qdagger_dqn_atari_impalacnn.py's own lines (192-195, 294-306 / 403-415)."""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from offpolicy_cases import same, within_bar  # noqa: F401

HID = 256
HEAD_OUTS = ("act", "q", "dh", "dw", "db", "scalars", "target_q", "td_target")
# M x n of the issue's grid: one row, a ragged row tile, the script's batch; the smallest game, Pong's, the full action set
HEAD_GRID = [(M, n) for M in (1, 5, 32) for n in (2, 6, 18)]
TEMPS = (1.0, 0.7)
COEFFS = (0.0, 0.37, 1.0)
GPU_HEADS = [(M, n) for M in (1, 32, 1024) for n in (2, 18)]
GUARD_HEADS = [(1, 2), (5, 6), (32, 18), (1024, 2)]


def kl_divergence_with_logits(target_logits, prediction_logits):
    """qdagger_dqn_atari_impalacnn.py:192-195."""
    out = -F.softmax(target_logits, dim=-1) * (F.log_softmax(prediction_logits, dim=-1) - F.log_softmax(target_logits, dim=-1))
    return torch.sum(out)


def make_head_case(M, n, seed=0, gamma=0.99, temperature=1.0, coeff=0.37, tie=False):
    """Two heads from torch's own ``nn.Linear(256, n)`` initialisation on post-ReLU rows, a teacher's Q values of a trained network's
    scale, rewards with both done values.  ``tie``: actions 0 and 1 are exact copies in both heads.  With n > 2 the last action is
    never taken."""
    torch.manual_seed(5000 + 97 * seed + 7 * M + 3 * n)
    lin, lin_t = torch.nn.Linear(HID, n), torch.nn.Linear(HID, n)
    w, b, wt, bt = (t.detach().clone() for t in (lin.weight, lin.bias, lin_t.weight, lin_t.bias))
    if tie:
        for t in (w, b, wt, bt):
            t[1] = t[0]
    g = torch.Generator().manual_seed(seed + M)
    h, hn = torch.relu(torch.randn((M, HID), generator=g)), torch.relu(torch.randn((M, HID), generator=g))
    teacher_q = torch.randn((M, n), generator=g) * 2.0
    actions = torch.randint(0, n, (M,), generator=g)
    if n > 2:
        actions[actions == n - 1] = 0
    rewards = torch.randn(M, generator=g)
    dones = (torch.rand(M, generator=g) < 0.3).float()
    if M >= 2:
        dones[0], dones[1] = 0.0, 1.0
    return SimpleNamespace(M=M, n=n, h=h, h_next=hn, w=w, b=b, wt=wt, bt=bt, teacher_q=teacher_q, actions=actions, rewards=rewards, dones=dones,
                           gamma=gamma, temperature=temperature, coeff=coeff)


def reference_head(c, dtype):
    """The reference's training lines behind the hidden layer in ``dtype`` -> dict(q, scalars, dh, dw, db, target_q, td_target, act)."""
    h, w, b = (t.to(dtype).clone().requires_grad_() for t in (c.h, c.w, c.b))
    hn, wt, bt, rew, done, tq = (t.to(dtype) for t in (c.h_next, c.wt, c.bt, c.rewards, c.dones, c.teacher_q))
    with torch.no_grad():
        target_q = F.linear(hn, wt, bt)
        target_max, _ = target_q.max(dim=1)
        td_target = rew.flatten() + c.gamma * target_max * (1 - done.flatten())
    student_q_values = F.linear(h, w, b)
    old_val = student_q_values.gather(1, c.actions.reshape(-1, 1)).squeeze()
    q_loss = F.mse_loss(td_target, old_val.reshape(-1))
    distill_loss = torch.mean(kl_divergence_with_logits(tq / c.temperature, student_q_values / c.temperature))
    loss = q_loss + c.coeff * distill_loss
    loss.backward()
    return dict(q=student_q_values.detach(), act=torch.argmax(student_q_values.detach(), dim=1),
                scalars=torch.stack([loss.detach(), q_loss.detach(), distill_loss.detach(), old_val.mean().detach()]), dh=h.grad, dw=w.grad,
                db=b.grad, target_q=target_q, td_target=td_target)


def run_heads(mod, c, dev, K=None):
    """Both head entry points through ``mod`` (ops or host_ops) on ``dev`` -> dict of tensors.  ``K``: the allocator of the outputs
    (bounds_cases.Plain / Carved) when the case's tensors are already placed."""
    new = (lambda name, shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)) if K is None else K.new
    d = (lambda t: t.to(dev)) if K is None else (lambda t: t)
    M, n = c.M, c.n
    h, hn, w, b, wt, bt, tq, actions, rewards, dones = (d(t) for t in (c.h, c.h_next, c.w, c.b, c.wt, c.bt, c.teacher_q, c.actions, c.rewards,
                                                                        c.dones))
    act, q = new("actions", (M,), torch.int64), new("q", (M, n))
    mod.qdagger_head_act(h, w, b, act, q_out=q)
    dh, dw, db, sc = new("dh", (M, HID)), new("dw", (n, HID)), new("db", (n,)), new("scalars", (4,))
    target_q, td_target = new("target_q", (M, n)), new("td_target", (M,))
    mod.qdagger_head_fwd_bwd(h, hn, w, b, wt, bt, tq, actions, rewards, dones, c.gamma, c.temperature, c.coeff, dh, dw, db, sc, target_q,
                             td_target)
    return dict(act=act, q=q, dh=dh, dw=dw, db=db, scalars=sc, target_q=target_q, td_target=td_target)


def bounds_head_case(M, n):
    """A ``bounds_cases.Case`` (not registered in ``bounds_cases.CASES``) over the two head entry points."""
    import bounds_cases as B

    keys = ("h", "h_next", "w", "b", "wt", "bt", "teacher_q", "actions", "rewards", "dones")

    def build():
        c = make_head_case(M, n, temperature=0.7)
        return dict(dims=(M, n), hp=(c.gamma, c.temperature, c.coeff), **{k: getattr(c, k) for k in keys})

    def run(mod, dev, T, K):
        c = SimpleNamespace(M=M, n=n, gamma=T["hp"][0], temperature=T["hp"][1], coeff=T["hp"][2], **{k: T[k] for k in keys})
        K.stage("qdagger head")
        return run_heads(mod, c, dev, K)

    return B.Case(f"qdagger head M={M} n={n}", build, run, HEAD_OUTS, True, True, None, None)


# ================================================================================================== the learner
def make_learner(dev, backend, M=8, slots=16, n=6, temperature=0.7, fill=False, seed=0):
    """A ``QDaggerLearner`` on torch's own initialisation; ``fill``: a ring that has wrapped, through ``store``."""
    import dqn_atari_cases as A
    from cleanrl_amd.agents import AtariDQNNetwork, AtariImpalaQNetwork
    from cleanrl_amd.learner_qdagger import QDaggerLearner

    torch.manual_seed(6000 + seed)
    env = A.atari_env(n)
    q, t, teacher = AtariImpalaQNetwork(env).to(dev), AtariImpalaQNetwork(env).to(dev), AtariDQNNetwork(env).to(dev)
    args = SimpleNamespace(buffer_size=slots, batch_size=M, learning_rate=1e-4, gamma=0.99, tau=1.0, temperature=temperature)
    L = QDaggerLearner(q, t, teacher, args, env, dev, backend=backend)
    if fill:
        for s in A.ring_steps(slots, 1, slots + 3, seed=seed):
            step = [x.numpy() for x in s]
            step[2] = step[2] % n
            L.store(*step)
    return L


def reference_update(L, bi, ei, dtype, distill_coeff):
    """The reference's training lines on the fused learner's own ring and networks in ``dtype`` -> dict(scalars, grads)."""
    import copy

    a = L.args
    q, t, teacher = (copy.deepcopy(m).to("cpu", dtype) for m in (L.q_network, L.target_network, L.teacher))
    q.impala_backend = t.impala_backend = "torch"
    for p in q.parameters():
        p.grad = None
    frames, actions, rewards, dones = (x.cpu() for x in L.ring)
    bi, ei = torch.as_tensor(bi), torch.as_tensor(ei)
    obs = frames[bi, ei].permute(0, 3, 1, 2).to(dtype)
    nxt = frames[(bi + 1) % L.slots, ei].permute(0, 3, 1, 2).to(dtype)
    act, rew, done = actions[bi, ei], rewards[bi, ei].to(dtype), dones[bi, ei].to(dtype)
    with torch.no_grad():
        target_max, _ = t(nxt).max(dim=1)
        td_target = rew + a.gamma * target_max * (1 - done)
        teacher_q_values = teacher(obs) / a.temperature
    student_q_values = q(obs)
    old_val = student_q_values.gather(1, act.reshape(-1, 1)).squeeze(1)
    q_loss = F.mse_loss(td_target, old_val)
    distill_loss = torch.mean(kl_divergence_with_logits(teacher_q_values, student_q_values / a.temperature))
    loss = q_loss + distill_coeff * distill_loss
    loss.backward()
    return dict(scalars=torch.stack([loss.detach(), q_loss.detach(), distill_loss.detach(), old_val.mean().detach()]),
                grads=torch.cat([p.grad.reshape(-1) for p in q.parameters()]))
