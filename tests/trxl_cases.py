"""Shared cases of the TrXL memory-attention tests (tests/test_trxl_attn_twins.py on the host twins, tests/test_gpu_trxl.py on
the device kernels).

``reference_window_attention`` transcribes the reference's window path (cleanrl/ppo_trxl/ppo_trxl.py: ``batched_index_select``
of the window, ``Transformer.forward``'s ``memories + pos_embedding``, ``TransformerLayer.forward``'s ``norm_kv``, then
``MultiHeadAttention.forward``'s keys / values projections, einsum energy, ``masked_fill(-1e20)``, ``/ embed_dim ** 0.5``,
softmax and weighted sum) in plain torch ops for any dtype; run in float64 it is the yardstick, run in float32 it measures
what the reference's own arithmetic loses.  ``fused_window_attention`` is the same result through ``TrXLMemoryAttention``:
q~ = q @ keys.weight, u from the kernel, then ``values``.
"""
from __future__ import annotations

import math

import torch

from cleanrl_amd import ops


def positional_table(D: int, P: int, dtype=torch.float32) -> torch.Tensor:
    """``PositionalEncoding(D)(P)``: reversed positions, sin | cos halves (ppo_trxl.py)."""
    freqs = torch.arange(0, D, 2.0)
    inv = 1e4 ** (-freqs / D)
    seq = torch.arange(P - 1, -1, -1.0)
    inp = seq[:, None] * inv[None, :]
    return torch.cat((inp.sin(), inp.cos()), dim=-1).to(dtype)


def reference_window_attention(memory, layer, ep, rows, pos, mask, pe, gamma, beta, q, w_k, w_v):
    """(B, H, d) ``attention`` before ``fc_out``, by the reference's ops in the inputs' dtype.  ``q`` (B, H, d) are the
    projected queries (``self.queries(query)``), ``w_k`` / ``w_v`` the (d, d) ``keys`` / ``values`` weights."""
    B, L = rows.shape
    H, d = q.shape[1], q.shape[2]
    D = H * d
    win = memory[ep][torch.arange(B)[:, None], rows]              # batched_index_select(stored_memories[ep], 1, rows)
    if pe is not None:
        win = win + pe[pos].unsqueeze(2)
    x = torch.nn.functional.layer_norm(win[:, :, layer], (D,), gamma, beta, 1e-5)
    x = x.reshape(B, L, H, d)
    values = x @ w_v.T
    keys = x @ w_k.T
    energy = torch.einsum("nqhd,nkhd->nhqk", [q.unsqueeze(1), keys])
    energy = energy.masked_fill(mask.unsqueeze(1).unsqueeze(1) == 0, float("-1e20"))
    att = torch.softmax(energy / (D ** (1 / 2)), dim=3)
    return torch.einsum("nhql,nlhd->nqhd", [att, values]).reshape(B, H, d)


def fused_window_attention(memory, layer, ep, rows, pos, mask, pe, gamma, beta, q, w_k, w_v):
    qt = q @ w_k                                                   # q~ = W_k^T q per head
    u = ops.TrXLMemoryAttention.apply(qt, gamma, beta, memory, layer, ep, rows, pos, mask, pe)
    return u @ w_v.T


MASKS = ("none", "all", "tril", "random")


def make_case(D: int, H: int, L: int, B: int, mask_kind: str, pe_kind: str, seed: int = 0, layers: int = 2, layer: int = 1,
              device="cpu"):
    """Random inputs of one call: an episode pool with fewer episodes than samples, windows of the reference's sliding
    shape (``memory_indices`` rows), positions != rows, and the named mask pattern."""
    g = torch.Generator().manual_seed(seed * 7919 + D * 31 + H * 7 + L)
    E = max(1, B // 3 + 1)
    T = L + 5
    P = T + 3
    memory = torch.randn((E, T, layers, D), generator=g) * 1.5 + 0.25
    ep = torch.randint(0, E, (B,), generator=g)
    start = torch.randint(0, T - L + 1, (B,), generator=g)
    rows = start[:, None] + torch.arange(L)[None, :]
    pos = (rows + torch.randint(1, 3, (B, 1), generator=g)) % P   # positions differ from rows (the bootstrap's case)
    if mask_kind == "none":
        mask = torch.ones((B, L), dtype=torch.bool)
    elif mask_kind == "all":
        mask = torch.zeros((B, L), dtype=torch.bool)
    elif mask_kind == "tril":                                      # the reference's per-step rows: step k keeps rows < k
        tri = torch.tril(torch.ones((L, L)), diagonal=-1).bool()
        mask = tri[torch.randint(0, L, (B,), generator=g)]
    else:
        mask = torch.rand((B, L), generator=g) < 0.6
    pe = positional_table(D, P) if pe_kind == "absolute" else None
    gamma = 1.0 + 0.3 * torch.randn(D, generator=g)
    beta = 0.2 * torch.randn(D, generator=g)
    d = D // H
    q = torch.randn((B, H, d), generator=g)
    w_k = torch.randn((d, d), generator=g) / math.sqrt(d)
    w_v = torch.randn((d, d), generator=g) / math.sqrt(d)
    dout = torch.randn((B, H, d), generator=g)
    c = dict(memory=memory, layer=layer, ep=ep, rows=rows, pos=pos, mask=mask, pe=pe, gamma=gamma, beta=beta, q=q, w_k=w_k, w_v=w_v,
             dout=dout)
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in c.items()}


_GRAD = ("q", "gamma", "beta")


def run(fn, case, dtype):
    """Output and d(out . dout)/d(q, gamma, beta) of ``fn`` with the float inputs in ``dtype``."""
    args = {}
    for k, v in case.items():
        if k == "dout":
            continue
        if isinstance(v, torch.Tensor) and v.is_floating_point():
            v = v.to(dtype)
            if k in _GRAD:
                v = v.detach().requires_grad_(True)
        args[k] = v
    out = fn(**args)
    (out * case["dout"].to(dtype)).sum().backward()
    return [out.detach()] + [args[k].grad.detach() for k in _GRAD]


def errors(fn, case):
    """Max abs error of ``fn`` (f32) and of the reference's f32 ops against float64, per result (out, dq, dgamma, dbeta), and the
    float64 results' magnitudes."""
    gold = run(reference_window_attention, case, torch.float64)
    ref32 = run(reference_window_attention, case, torch.float32)
    got = run(fn, case, torch.float32)
    e_got = [(a.double().cpu() - b.cpu()).abs().max().item() for a, b in zip(got, gold)]
    e_ref = [(a.double().cpu() - b.cpu()).abs().max().item() for a, b in zip(ref32, gold)]
    scale = [b.abs().max().item() for b in gold]
    return e_got, e_ref, scale


def within_bar(e_got, e_ref, scale, floor: float = 2e-6):
    """The bar, set from the host twins before any device run: at most twice the reference f32 error, plus a floor of a few
    f32 ulps of the result's magnitude (the reference can be exact by luck on a small case)."""
    return all(eg <= 2.0 * er + floor * max(1.0, s) for eg, er, s in zip(e_got, e_ref, scale))


# ------------------------------------------------------------------------------------------- whole iterations (goldens)
def golden_case(name: str):
    from conftest import load_golden

    return load_golden("trxl_iteration")[name]


def replay(g, device="cpu", backend="torch", force_actions=False):
    """One golden case through ``TrXLLearner``: the same seeds, stand-in env and update seeds as the minting run
    (tools/mint_trxl_goldens.py).  ``force_actions`` feeds the recorded actions instead of sampling (teacher forcing).
    Returns (per-iteration rollout records, per-iteration metrics, the agent, the learner)."""
    import json
    import random
    from types import SimpleNamespace

    import numpy as np

    from cleanrl_amd import envs as E
    from cleanrl_amd.agents import TrXLAgent
    from cleanrl_amd.learner_trxl import TrXLLearner
    from cleanrl_amd.ppo_trxl import Args, action_space_shape_of, max_episode_steps_of

    cfg = json.loads(bytes(g["config"]).decode())
    args = Args(**{k: v for k, v in cfg["args"].items()})
    args = SimpleNamespace(**vars(args))
    args.batch_size = args.num_envs * args.num_steps
    args.minibatch_size = args.batch_size // args.num_minibatches
    envs = E.SyntheticMemoryVecEnv(cfg["env_id"], args.num_envs, **cfg["env"])
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    shape = action_space_shape_of(envs.single_action_space)
    mes = max_episode_steps_of(envs)
    args.trxl_memory_length = min(args.trxl_memory_length, mes)
    agent = TrXLAgent(args, envs.single_observation_space, shape, mes)
    agent.trxl_backend = backend
    agent = agent.to(device)
    learner = TrXLLearner(agent, args, envs.single_observation_space, shape, args.num_envs, mes, device)
    obs, _ = envs.reset(seed=args.seed)
    learner.reset(obs)
    recs, metrics = [], []
    for it in range(g["actions"].shape[0]):
        learner.start_iteration()
        for step in range(args.num_steps):
            forced = torch.from_numpy(g["actions"][it, step]).to(device) if force_actions else None
            action = learner.act(step, forced)
            next_obs, reward, term, trunc, _ = envs.step(action.cpu().numpy())
            learner.observe(step, next_obs, reward, term, trunc)
        learner.finish_rollout()
        recs.append({k: getattr(learner, k).detach().cpu().clone() for k in
                     ("actions", "log_probs", "values", "rewards", "dones", "stored_memory_masks", "stored_memory_indices",
                      "stored_memory_index", "advantages", "returns", "next_done")})
        torch.manual_seed(int(g["update_seed"]) + it + 1)
        m = learner.update()
        m["num_episodes"] = learner.pool.shape[0]
        metrics.append(m)
    return recs, metrics, agent, learner


SCALAR_KEYS = (("pg_loss", "policy_loss"), ("v_loss", "value_loss"), ("entropy_loss", "entropy"), ("loss", "loss"),
               ("r_loss", "reconstruction_loss"), ("old_approx_kl", "old_approx_kl"), ("approx_kl", "approx_kl"),
               ("clipfrac", "clipfrac"), ("explained_var", "explained_variance"), ("lr", "learning_rate"),
               ("ent_coef", "entropy_coefficient"), ("actual_max_episode_steps", "actual_max_episode_steps"),
               ("num_episodes", "num_episodes"), ("value_mean", "value_mean"), ("advantage_mean", "advantage_mean"))
