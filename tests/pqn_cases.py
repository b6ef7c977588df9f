"""Shared cases of the PQN tests (tests/test_pqn_twins.py, tests/test_pqn_script.py on the host twins, tests/test_gpu_pqn.py on the
device kernels): the reference's lines as plain torch ops in any dtype (the yardsticks), random inputs, and a replay of the golden
iterations (tests/golden/pqn_iteration.npz, minted by tools/mint_pqn_goldens.py) through QNetwork / AtariQNetwork + PQNLearner."""
from __future__ import annotations

import json
import os
import random

import numpy as np
import torch
import torch.nn.functional as F

from cleanrl_amd import envs as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pqn_iteration.npz")


def reference_qlambda(rewards, dones, values, next_done, next_q, gamma, q_lambda):
    """The ``# Compute Q(lambda) targets`` loop of pqn.py, with ``next_q`` standing for ``q_network(next_obs)``."""
    T = rewards.shape[0]
    returns = torch.zeros_like(rewards)
    for t in reversed(range(T)):
        if t == T - 1:
            next_value, _ = torch.max(next_q, dim=-1)
            nextnonterminal = 1.0 - next_done
            returns[t] = rewards[t] + gamma * next_value * nextnonterminal
        else:
            nextnonterminal = 1.0 - dones[t + 1]
            next_value = values[t + 1]
            returns[t] = rewards[t] + gamma * (q_lambda * returns[t + 1] + (1 - q_lambda) * next_value) * nextnonterminal
    return returns


def reference_egreedy(q, random_actions, u, epsilon):
    max_actions = torch.argmax(q, dim=1)
    values = q[torch.arange(q.shape[0]), max_actions].flatten()
    explore = u < epsilon
    return torch.where(explore, random_actions, max_actions), values


def reference_td(q, mb_inds, b_actions, b_returns):
    """(loss, mean(old_val), d loss / d q) by autograd of gather + mse_loss in q's dtype."""
    q = q.detach().clone().requires_grad_(True)
    old_val = q.gather(1, b_actions[mb_inds].unsqueeze(-1).long()).squeeze(-1)
    loss = F.mse_loss(b_returns[mb_inds].to(q.dtype), old_val)
    loss.backward()
    return loss.detach(), old_val.detach().mean(), q.grad


def reference_mlp(params, O, A, dtype):
    """pqn.py's QNetwork in ``dtype`` with the given flat parameters (agent.parameters() order)."""
    from cleanrl_amd.agents import QNetwork

    env = type("Env", (), {"single_observation_space": E.Box(0, 1, (O,)), "single_action_space": E.Discrete(A)})()
    net = QNetwork(env).to(dtype)
    off = 0
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(params[off:off + p.numel()].reshape(p.shape).to(dtype))
            off += p.numel()
    return net


def reference_mlp_td(params, O, A, b_obs, mb_inds, b_actions, b_returns, dtype):
    """(q, loss, mean(old), flat gradient) of one pqn.py minibatch in ``dtype``."""
    net = reference_mlp(params, O, A, dtype)
    q = net(b_obs[mb_inds].to(dtype))
    old_val = q.gather(1, b_actions[mb_inds].unsqueeze(-1).long()).squeeze(-1)
    loss = F.mse_loss(b_returns[mb_inds].to(dtype), old_val)
    loss.backward()
    g = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
    return q.detach(), loss.detach(), old_val.detach().mean(), g


def within_bar(got, ref64, ref32, floor=2e-6):
    """The bar of the f32 reference: no more than twice its own error against float64, plus a floor."""
    got, ref64, ref32 = (t.detach().double().cpu() for t in (got, ref64, ref32))
    err = (got - ref64).abs().max().item()
    own = (ref32 - ref64).abs().max().item()
    return err <= 2 * own + floor * max(1.0, ref64.abs().max().item()), err, own


def random_mlp_params(O, A, seed, scale=1.0):
    """Flat parameters of the shape of QNetwork(O, A): orthogonal-like weights, non-trivial LayerNorm affines and biases."""
    from cleanrl_amd.ops import pqn_param_count

    g = torch.Generator().manual_seed(seed)
    p = torch.randn(pqn_param_count(O, A), generator=g) * 0.2 * scale
    n1, n2 = 120 * O, 84 * 120
    off = n1 + 120
    p[off:off + 120] = 1.0 + 0.2 * torch.randn(120, generator=g)                 # LayerNorm(120).weight
    off = n1 + 360 + n2 + 84
    p[off:off + 84] = 1.0 + 0.2 * torch.randn(84, generator=g)                   # LayerNorm(84).weight
    return p


# ------------------------------------------------------------------------------------------------ golden iterations
def golden_case(name):
    z = np.load(GOLDEN)
    pre = name + "/"
    return {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}


def replay(g, backend, device="cpu", force_actions=False):
    """Two iterations of the drop-in's loop (seeding, stand-in env, network, PQNLearner) with the golden's Args -> (records, metrics,
    net, learner).  ``force_actions`` feeds the golden's actions (teacher forcing)."""
    from cleanrl_amd.agents import AtariQNetwork, QNetwork
    from cleanrl_amd.learner_pqn import PQNLearner

    cfg = json.loads(bytes(g["config"]).decode())
    atari = cfg["script"] == "pqn_atari_envpool.py"
    if atari:
        from cleanrl_amd.pqn_atari_envpool import Args
    else:
        from cleanrl_amd.pqn import Args
    args = Args(**cfg["args"])
    args.batch_size = args.num_envs * args.num_steps
    args.minibatch_size = args.batch_size // args.num_minibatches
    args.total_timesteps = args.batch_size * cfg["iterations"]
    args.num_iterations = cfg["iterations"]
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    if atari:
        envs = E.SyntheticAtariVecEnv(args.num_envs, seed=args.seed, n_actions=4, api="gym")
        net = AtariQNetwork(envs).to(device)
    else:
        envs = E.CartPoleVecEnv(args.num_envs, seed=args.seed)
        net = QNetwork(envs).to(device)
    learner = PQNLearner(net, args, envs.single_observation_space.shape, envs.single_action_space.n, args.num_envs, device, mlp=not atari,
                         backend=backend)
    learner.reset(envs.reset() if atari else envs.reset(seed=args.seed)[0])
    recs, metrics = [], []
    for it in range(1, args.num_iterations + 1):
        learner.start_iteration(it)
        for step in range(args.num_steps):
            force = torch.from_numpy(g["actions"][it - 1][step]).long() if force_actions else None
            action = learner.act(step, force)
            out = envs.step(action.cpu().numpy())
            if atari:
                next_obs, reward, next_done, _ = out
            else:
                next_obs, reward, term, trunc, _ = out
                next_done = np.logical_or(term, trunc)
            learner.observe(step, next_obs, reward, next_done)
        learner.finish_rollout()
        rec = {k: getattr(learner, k).detach().cpu().clone() for k in ("actions", "values", "rewards", "dones", "returns")}
        rec["next_done"] = learner.next_done.detach().cpu().clone()
        recs.append(rec)
        metrics.append(learner.update())
    return recs, metrics, net, learner


def flat(net):
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()]).cpu()
