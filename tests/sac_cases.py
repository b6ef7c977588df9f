"""Shared case builders and float64 references for the SAC kernels (csrc/sac.hip) and their host twins."""
import copy
from types import SimpleNamespace

import torch

import offpolicy_cases as C
from cleanrl_amd.agents import ActionValueNetwork, SoftActor
from cleanrl_amd.ops import offpolicy_counts, sac_actor_count

SHAPES = [(17, 6, 256), (376, 17, 256), (5, 1, 70), (512, 20, 9), (17, 6, 1)]
LOW, HIGH = -2.0, 1.0                     # asymmetric bounds: action_bias and a non-unit action_scale matter
ALPHA = 0.37
GAMMA = 0.99


def make_case(O, A, M, N=2, slots=37, seed=0, saturate=True, nan_row=None, tie_row=None):
    """Networks from torch's own initialisation (biases perturbed), a random ring, a random batch and three (M, A) draws.
    ``saturate``: fc_logstd's bias is raised so that std is near its maximum and eps entries of +-9 / +-30 in rows 0 and 1 give
    y = +-1 exactly.  ``nan_row``: that row's first eps is NaN.  ``tie_row``: both critics share parameters (q1 == q2 everywhere)."""
    torch.manual_seed(2000 + seed + O + A)
    env = C.fake_env(O, A, LOW, HIGH)
    nets = SimpleNamespace(actor=SoftActor(env), qfs=[ActionValueNetwork(env) for _ in range(2)],
                           qf_targets=[ActionValueNetwork(env) for _ in range(2)])
    g = torch.Generator().manual_seed(seed + M)
    with torch.no_grad():
        for m in [nets.actor] + nets.qfs + nets.qf_targets:
            for nm, p in m.named_parameters():
                if nm.endswith("bias"):
                    p.add_(torch.randn(p.shape, generator=g) * 0.1)
        if saturate:
            nets.actor.fc_logstd.bias.add_(3.0)
        if tie_row is not None:
            nets.qfs[1].load_state_dict(nets.qfs[0].state_dict())
    ring = (torch.randn((slots, N, O), generator=g), torch.randn((slots, N, O), generator=g),
            torch.rand((slots, N, A), generator=g) * (HIGH - LOW) + LOW, torch.randn((slots, N), generator=g),
            (torch.rand((slots, N), generator=g) < 0.3).float())
    bi, ei = torch.randint(0, slots, (M,), generator=g), torch.randint(0, N, (M,), generator=g)
    eps = [torch.randn((M, A), generator=g) for _ in range(3)]
    sat = []                                                    # (row, column, eps): +-9 and +-30, each where the shape has room
    if saturate:
        sat = [(0, 0, 9.0)] + ([(0, A - 1, -30.0)] if A > 1 else []) + ([(1, 0, -9.0 if A > 1 else -30.0)] if M > 1 else [])
        sat += [(1, A - 1, 30.0)] if M > 1 and A > 1 else []
        sat += [(2, 0, 30.0), (3, 0, -9.0)] if A == 1 and M > 3 else []
        for e in eps:
            for r, a, v in sat:
                e[r, a] = v
    if nan_row is not None:
        for e in eps:
            e[nan_row, 0] = float("nan")
    c = SimpleNamespace(O=O, A=A, M=M, N=N, slots=slots, nets=nets, ring=ring, bi=bi, ei=ei, eps=eps, sat=sat,
                        scale=nets.actor.action_scale.clone(), bias=nets.actor.action_bias.clone(), alpha=torch.tensor([ALPHA]),
                        target_entropy=-float(A))
    c.actor = C.flat(nets.actor)
    c.critics = torch.cat([C.flat(q) for q in nets.qfs])
    c.target_critics = torch.cat([C.flat(q) for q in nets.qf_targets])
    assert (c.actor.numel(), c.critics.numel()) == (sac_actor_count(O, A), 2 * offpolicy_counts(O, A)[1])
    return c


def _nets(c, dtype):
    n = copy.deepcopy(c.nets)
    for m in [n.actor] + n.qfs + n.qf_targets:
        m.to(dtype)
    return n


def _batch(c, dtype):
    obs, nxt, act, rew, done = (t.to(dtype) for t in c.ring)
    return obs[c.bi, c.ei], nxt[c.bi, c.ei], done[c.bi, c.ei], rew[c.bi, c.ei]


def reference_critic(c, y, dtype):
    """The reference's critic step in ``dtype`` on the SAC target ``y`` -> (flat gradient of qf1 | qf2, [mean q1, loss1, mean q2,
    loss2])."""
    n = _nets(c, dtype)
    obs, act = c.ring[0].to(dtype)[c.bi, c.ei], c.ring[2].to(dtype)[c.bi, c.ei]
    qv = [q(obs, act).view(-1) for q in n.qfs]
    losses = [torch.nn.functional.mse_loss(v, y.to(dtype)) for v in qv]
    (losses[0] + losses[1]).backward()
    grads = torch.cat([p.grad.reshape(-1) for q in n.qfs for p in q.parameters()])
    return grads, torch.stack([t for v, l in zip(qv, losses) for t in (v.mean(), l)]).detach()


def reference(c, dtype):
    """The reference's ops in ``dtype`` -> dict: the target block, the policy loss with autograd (flat gradient, gradients at mean
    and at fc_logstd's output u), the re-evaluated log_pi and the alpha loss with its Adam step."""
    n = _nets(c, dtype)
    obs, nxt, done, rew = _batch(c, dtype)
    alpha = torch.tensor(ALPHA, dtype=torch.float32).to(dtype).item() if dtype == torch.float32 else float(c.alpha.double().item())
    out = {}
    with torch.no_grad():
        na, nlp, _ = n.actor.get_action(nxt, c.eps[0].to(dtype))
        mq = torch.min(n.qf_targets[0](nxt, na), n.qf_targets[1](nxt, na)) - alpha * nlp
        out["y"] = rew.flatten() + (1 - done.flatten()) * GAMMA * mq.view(-1)
        out["next_actions"], out["next_log_pi"] = na, nlp.view(-1)
    # the policy loss, with hooks at the two heads' outputs
    a = n.actor
    h = torch.relu(a.fc2(torch.relu(a.fc1(obs))))
    mean, u = a.fc_mean(h), a.fc_logstd(h)
    mean.retain_grad(), u.retain_grad()
    log_std = -5 + 0.5 * (2 - -5) * (torch.tanh(u) + 1)
    std = log_std.exp()
    normal = torch.distributions.Normal(mean, std)
    x_t = mean + c.eps[1].to(dtype) * std
    y_t = torch.tanh(x_t)
    pi = y_t * a.action_scale + a.action_bias
    log_pi = normal.log_prob(x_t) - torch.log(a.action_scale * (1 - y_t.pow(2)) + 1e-6)
    log_pi = log_pi.sum(1, keepdim=True)
    loss = ((alpha * log_pi) - torch.min(n.qfs[0](obs, pi), n.qfs[1](obs, pi))).mean()
    loss.backward()
    out.update(log_pi=log_pi.detach().view(-1), pi=pi.detach(), y_t=y_t.detach(), actor_loss=loss.detach().reshape(1),
               actor_grads=torch.cat([p.grad.reshape(-1) for p in a.parameters()]), dmean=mean.grad, du=u.grad)
    with torch.no_grad():
        _, lp2, _ = a.get_action(obs, c.eps[2].to(dtype))
    log_alpha = torch.zeros(1, dtype=dtype, requires_grad=True)
    with torch.no_grad():
        log_alpha.fill_(-0.3)
    opt = torch.optim.Adam([log_alpha], lr=1e-3)
    al = (-log_alpha.exp() * (lp2 + c.target_entropy)).mean()
    al.backward()
    opt.step()
    out.update(log_pi2=lp2.view(-1), alpha_loss=al.detach().reshape(1), log_alpha=log_alpha.detach().clone())
    return out


def run_entry_points(mod, c, dev):
    """Every SAC entry point through ``mod`` (ops or host_ops) on ``dev`` -> dict of CPU tensors (names as ``reference``)."""
    d = lambda t: t.to(dev)  # noqa: E731
    z = lambda *s: torch.zeros(s, device=dev)  # noqa: E731
    ring = tuple(d(t) for t in c.ring)
    M, A = c.M, c.A
    bi, ei, actor, scale, bias, alpha = d(c.bi), d(c.ei), d(c.actor), d(c.scale), d(c.bias), d(c.alpha)
    y, na, nlp = z(M), z(M, A), z(M)
    mod.sac_target(ring, bi, ei, actor, d(c.target_critics), scale, bias, d(c.eps[0]), alpha, GAMMA, y, na, nlp)
    gq, sq = z(c.critics.numel()), z(4)
    mod.td3_critic_fwd_bwd(ring, bi, ei, d(c.critics), 2, y, gq, sq)         # the critic step on SAC's target, n_critics = 2
    ga, la, lp, dm, du = z(c.actor.numel()), z(1), z(M), z(M, A), z(M, A)
    mod.sac_actor_fwd_bwd(ring, bi, ei, actor, d(c.critics), scale, bias, d(c.eps[1]), alpha, ga, la, lp, dm, du)
    pi, lp1 = z(M, A), z(M)
    mod.sac_policy(ring[0], actor, scale, bias, d(c.eps[1]), actions_out=pi, log_pi_out=lp1, batch_inds=bi, env_inds=ei)
    lp2 = z(M)
    mod.sac_policy(ring[0], actor, scale, bias, d(c.eps[2]), log_pi_out=lp2, batch_inds=bi, env_inds=ei)
    dense = d(c.ring[0][c.bi, c.ei].contiguous())
    pid = z(M, A)
    mod.sac_policy(dense, actor, scale, bias, d(c.eps[1]), actions_out=pid)
    st = torch.tensor([-0.3, 0.0, 0.0, 0.0, 0.0], device=dev)
    s = [st[i:i + 1] for i in range(5)]
    mod.sac_alpha_(lp2, c.target_entropy, s[0], s[1], s[2], 1, 1e-3, s[3], s[4])
    return {k: v.cpu() for k, v in dict(critic_grads=gq, critic_scalars=sq, y=y, next_actions=na, next_log_pi=nlp, actor_grads=ga, actor_loss=la, log_pi=lp, dmean=dm, du=du,
                                        pi=pi, log_pi_policy=lp1, pi_dense=pid, log_pi2=lp2, log_alpha=s[0], alpha=s[3],
                                        alpha_loss=s[4], alpha_state=st).items()}
