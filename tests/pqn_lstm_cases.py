"""Shared cases of the recurrent PQN tests (tests/test_pqn_lstm_twins.py and tests/test_pqn_lstm_script.py on the host twins,
tests/test_gpu_pqn_lstm.py on the device kernels).  Yardsticks are the reference's own ops -- ``nn.LSTM`` stepped as ``get_states``
does (``lstm_cases.reference_loop``), ``nn.functional.linear`` for ``q_func``, gather + ``mse_loss`` under autograd -- in float64
(truth) and float32 (the reference's own error), and ``pqn_cases.reference_egreedy``; plus a replay of the golden iterations
(tests/golden/pqn_lstm_iteration.npz, minted by tools/mint_pqn_lstm_goldens.py) through AtariLSTMQNetwork + LSTMPQNLearner."""
from __future__ import annotations

import json
import os
import random

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import lstm_cases as L
from cleanrl_amd import envs as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pqn_lstm_iteration.npz")
H = L.H
ACT_N = (1, 8, 65)
ACT_A = (1, 4, 18)
TD_M = (1, 256, 4096 + 3)


# ------------------------------------------------------------------------------------------------ one rollout step
def make_act_case(N, A, pattern, seed=0):
    """One step of N envs: ``lstm_cases.make_case`` at T = 1 (weights as the network initialises them, trunk-scaled input, random
    state, the done pattern) plus ``q_func`` (orthogonal, std sqrt(2), random bias) and the step's random draws."""
    c = L.make_case(1, N, pattern, seed=seed)
    gen = torch.Generator().manual_seed(seed * 7919 + N * 31 + A)
    wq = torch.empty(A, H)
    nn.init.orthogonal_(wq, float(np.sqrt(2)), generator=gen)
    c.update(wq=wq, bq=0.1 * torch.randn(A, generator=gen), rnd=torch.randint(0, A, (N,), generator=gen),
             u=torch.rand(N, generator=gen), gx=L.gx_of(c)[0].contiguous(), N=N, A=A)
    return c


def reference_act(c, dtype):
    """The reference's one-step ``get_states`` (on the case's f32 gx, as the kernel receives it) + ``q_func`` in ``dtype`` ->
    (h, c, q) as float64 tensors."""
    (h, hT, cT), _ = L.reference_loop(c, dtype, on_gx=True)
    q = F.linear(hT.to(dtype), c["wq"].to(dtype), c["bq"].to(dtype))
    return hT, cT, q.double()


def run_act(mod, c, device="cpu", bq=None, eps=0.3, alias=False, bootstrap=False):
    """``pqn_lstm_act`` of ``mod`` (host_ops or ops) on the case -> dict of CPU tensors."""
    to = lambda t: t.to(device)  # noqa: E731
    N, A = c["N"], c["A"]
    h_in, c_in = to(c["h0"]).clone(), to(c["c0"]).clone()
    q = torch.full((N, A), 7.0, device=device)
    args = (to(c["gx"]), to(c["w_hh"]), h_in, c_in, to(c["done"][0].contiguous()), to(c["wq"]), to(c["bq"] if bq is None else bq))
    if bootstrap:
        mod.pqn_lstm_act(*args, q_out=q)
        return dict(q=q.cpu(), h_in=h_in.cpu(), c_in=c_in.cpu())
    h_out, c_out = (h_in, c_in) if alias else (torch.empty((N, H), device=device), torch.empty((N, H), device=device))
    act, val = torch.empty(N, device=device), torch.empty(N, device=device)
    a64, drow = torch.empty(N, dtype=torch.int64, device=device), torch.empty(N, device=device)
    mod.pqn_lstm_act(*args, to(c["rnd"]), to(c["u"]), eps, h_out=h_out, c_out=c_out, q_out=q, actions_out=act, values_out=val,
                     action_i64_out=a64, done_row_out=drow)
    return {k: v.cpu() for k, v in dict(h=h_out, c=c_out, q=q, actions=act, values=val, a64=a64, done_row=drow).items()}


def same(a, b):
    """Bit equality that lets NaN equal NaN."""
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and torch.equal(a.isnan(), b.isnan()) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))


def check_egreedy(out, c, eps):
    """The step's actions / values EQUAL ``reference_egreedy`` applied to the kernel's own q."""
    from pqn_cases import reference_egreedy

    a, v = reference_egreedy(out["q"], c["rnd"], c["u"], eps)
    assert torch.equal(out["a64"], a) and torch.equal(out["actions"], a.float()) and same(out["values"], v)
    assert torch.equal(out["done_row"], c["done"][0])


def planted_bias(c):
    """A copy of ``bq`` that plants a NaN (and, with more than two actions, +inf and -inf) into columns of q."""
    bq = c["bq"].clone()
    A = c["A"]
    bq[A // 2] = float("nan")
    if A > 2:
        bq[0], bq[A - 1] = float("inf"), float("-inf")
    return bq


# ------------------------------------------------------------------------------------------------ one minibatch
def make_td_case(M, A, seed=0, envwise=None, actions=None):
    """h (M, H) like the scan's output (|h| < 1), ``q_func``, the flat batch and ``mb_inds``: random rows of a batch of M + 17, or
    with ``envwise=(T, N, envs)`` the update's pattern ``flatinds[:, envs].ravel()``.  ``actions``: the values that occur."""
    gen = torch.Generator().manual_seed(seed * 104729 + M * 13 + A)
    if envwise is None:
        B = M + 17
        mb = torch.randperm(B, generator=gen)[:M]
    else:
        T, N, envs = envwise
        B = T * N
        mb = torch.from_numpy(np.arange(B).reshape(T, N)[:, envs].ravel().copy())
        assert mb.numel() == M
    wq = torch.empty(A, H)
    nn.init.orthogonal_(wq, float(np.sqrt(2)), generator=gen)
    pool = torch.tensor(list(range(A)) if actions is None else list(actions))
    return dict(h=torch.tanh(torch.randn(M, H, generator=gen)), wq=wq, bq=0.1 * torch.randn(A, generator=gen), mb=mb,
                b_actions=pool[torch.randint(0, len(pool), (B,), generator=gen)].float(), b_returns=torch.randn(B, generator=gen) * 2,
                M=M, A=A)


def reference_td_head(c, dtype):
    """``q_func(h).gather(1, b_actions[mb_inds].long())`` + ``F.mse_loss(b_returns[mb_inds], old_val)`` under autograd in ``dtype`` ->
    dict(loss, mean_old, dh, dwq, dbq)."""
    h = c["h"].to(dtype).requires_grad_(True)
    wq, bq = c["wq"].to(dtype).requires_grad_(True), c["bq"].to(dtype).requires_grad_(True)
    old_val = F.linear(h, wq, bq).gather(1, c["b_actions"][c["mb"]].unsqueeze(-1).long()).squeeze(-1)
    loss = F.mse_loss(c["b_returns"][c["mb"]].to(dtype), old_val)
    loss.backward()
    return dict(loss=loss.detach().reshape(1), mean_old=old_val.detach().mean().reshape(1), dh=h.grad, dwq=wq.grad, dbq=bq.grad)


def run_td(mod, c, device="cpu", perm=None):
    to = lambda t: t.to(device)  # noqa: E731
    h, mb = (c["h"], c["mb"]) if perm is None else (c["h"][perm].contiguous(), c["mb"][perm].contiguous())
    dwq, dbq = torch.full((c["A"], H), 3.0, device=device), torch.full((c["A"],), 3.0, device=device)      # OVERWRITTEN, not added to
    dh, sc = mod.pqn_lstm_td_fwd_bwd(to(h), to(mb), to(c["b_actions"]), to(c["b_returns"]), to(c["wq"]), to(c["bq"]), dwq, dbq)
    return dict(loss=sc[0:1].cpu(), mean_old=sc[1:2].cpu(), dh=dh.cpu(), dwq=dwq.cpu(), dbq=dbq.cpu(), scalars=sc.cpu())


# ------------------------------------------------------------------------------------------------ golden iterations
def golden_case():
    z = np.load(GOLDEN)
    return {k[len("lstm/"):]: z[k] for k in z.files}


def golden_args(g):
    from cleanrl_amd.pqn_atari_envpool_lstm import Args

    cfg = json.loads(bytes(g["config"]).decode())
    args = Args(**cfg["args"])
    args.batch_size = args.num_envs * args.num_steps
    args.minibatch_size = args.batch_size // args.num_minibatches
    args.total_timesteps = args.batch_size * cfg["iterations"]
    args.num_iterations = cfg["iterations"]
    return args, cfg


def golden_envs(args, cfg):
    return E.SyntheticAtariVecEnv(args.num_envs, seed=args.seed, n_actions=4, api="gym", frames=1, done_p=cfg["done_p"])


def replay(g, backend, device="cpu", force_actions=False):
    """The golden's iterations of the drop-in's loop (seeding, stand-in env, network, LSTMPQNLearner) -> (records, metrics, net,
    learner).  ``force_actions`` feeds the golden's actions (teacher forcing)."""
    from cleanrl_amd.agents import AtariLSTMQNetwork
    from cleanrl_amd.learner_pqn_lstm import LSTMPQNLearner

    args, cfg = golden_args(g)
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    envs = golden_envs(args, cfg)
    net = AtariLSTMQNetwork(envs).to(device)
    learner = LSTMPQNLearner(net, args, envs.single_observation_space.shape, envs.single_action_space.n, args.num_envs, device,
                             backend=backend)
    learner.reset(envs.reset())
    recs, metrics = [], []
    for it in range(1, args.num_iterations + 1):
        learner.start_iteration(it)
        for step in range(args.num_steps):
            force = torch.from_numpy(g["actions"][it - 1][step]).long() if force_actions else None
            action = learner.act(step, force)
            next_obs, reward, next_done, _ = envs.step(action.cpu().numpy())
            learner.observe(step, next_obs, reward, next_done)
        learner.finish_rollout()
        rec = {k: getattr(learner, k).detach().cpu().clone() for k in ("actions", "values", "rewards", "dones", "returns")}
        rec["next_done"] = learner.next_done.detach().cpu().clone()
        rec["initial_h"], rec["initial_c"] = (t.detach().cpu().clone() for t in learner.initial_lstm_state)
        recs.append(rec)
        metrics.append(learner.update())
    return recs, metrics, net, learner


def flat(net):
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()]).cpu()
