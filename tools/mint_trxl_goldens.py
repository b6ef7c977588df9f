"""Mint the ppo_trxl fixtures from the reference's own lines.

    python tools/mint_trxl_goldens.py

Build-container tool: it needs the reference checkout (``oracle.ref_extract.REFERENCE_ROOT``); nothing on the GPU machine
runs it.  Like ``oracle/ref_extract.py`` it stores no reference text: it ``ast``-compiles ``layer_init``,
``batched_index_select``, ``PositionalEncoding``, ``MultiHeadAttention``, ``TransformerLayer``, ``Transformer`` and ``Agent``
of cleanrl/ppo_trxl/ppo_trxl.py and ``exec``s the main loop's blocks, located by their comments, against the synthetic memory
task of cleanrl_amd/envs.py on one CPU thread:

* setup   -- from ``observation_space = envs.single_observation_space`` to the ``for iteration`` line (spaces, max episode
             steps, ``Agent``, ``AdamW``, storage, ``next_memory``, ``memory_mask``, ``memory_indices``, ``envs.reset``);
* rollout -- the iteration body up to ``# Flatten the batch`` (annealing, the episode list, action logic, episode ends,
             bootstrap and GAE);
* update  -- ``# Flatten the batch`` up to the print line (trim, minibatch loss, AdamW, ``target_kl``, explained variance,
             episode statistics).

``torch.manual_seed(update_seed + iteration)`` precedes each update block, so a test can replay the minibatch permutations
without replaying the sampler.  Writes tests/golden/trxl_iteration.npz and tests/golden/trxl_cli_surface.json.
"""
from __future__ import annotations

import ast
import json
import os
import random
import sys
import textwrap
import time
from collections import deque
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn
import torch.optim as optim
from torch.distributions import Categorical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cleanrl_amd import envs as E  # noqa: E402
from oracle import ref_extract as R  # noqa: E402

SCRIPT = os.path.join("ppo_trxl", "ppo_trxl.py")
OUT = os.path.join(ROOT, "tests", "golden")
STRIDE = 37
ITERATIONS = 2
UPDATE_SEED = 1000

# name -> (env id, stand-in settings, Args overrides).  T = 16, N = 4 throughout.
CASES = {
    # episodes end mid-rollout and at the last step; windows reach past the memory length (no trim)
    "vec_discrete": ("MemoryVector-v0", dict(max_episode_steps=12, min_len=2, max_len=14),
                     dict(trxl_memory_length=8, trxl_positional_encoding="absolute")),
    # long episodes against a long window: the trim is taken; no positional encoding; normalised advantages, target_kl
    "vec_multidiscrete": ("MemoryVector-MultiDiscrete-v0", dict(max_episode_steps=40, min_len=6, max_len=44),
                          dict(trxl_memory_length=32, trxl_positional_encoding="", norm_adv=True, target_kl=0.002)),
    # (84, 84, 3) images through the NatureCNN, learned positional encoding, the reconstruction head
    "image": ("MiniGrid-MemoryImage-v0", dict(max_episode_steps=10, min_len=2, max_len=12),
              dict(trxl_memory_length=4, trxl_positional_encoding="learned", reconstruction_coef=0.1)),
}
COMMON = dict(num_envs=4, num_steps=16, num_minibatches=2, update_epochs=2, trxl_dim=64, trxl_num_heads=4, trxl_num_layers=2,
              anneal_steps=256, seed=3)


def _lines():
    return R._read(SCRIPT)


def _find(lines, needle, start=0):
    return R._find(lines, needle, start)


def reference_args_defaults() -> dict:
    """The reference's ``Args`` fields and defaults, as data (``exp_name`` left out)."""
    tree = ast.parse("\n".join(_lines()))
    (cls,) = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Args"]
    out = {}
    for b in cls.body:
        if isinstance(b, ast.AnnAssign) and b.target.id != "exp_name":
            v = b.value
            try:
                out[b.target.id] = ast.literal_eval(v)
            except ValueError:                                     # `32 * 512 * 10000`
                out[b.target.id] = eval(compile(ast.Expression(v), "<args>", "eval"), {})
    return out


def load_reference_network():
    """The reference's network classes, compiled from its source."""
    from einops import rearrange

    tree = ast.parse("\n".join(_lines()))
    names = ("layer_init", "batched_index_select", "PositionalEncoding", "MultiHeadAttention", "TransformerLayer", "Transformer", "Agent")
    wanted = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert {n.name for n in wanted} == set(names)
    ns = {"np": np, "torch": torch, "nn": nn, "Categorical": Categorical, "rearrange": rearrange}
    exec(compile(ast.Module(body=wanted, type_ignores=[]), "<reference:ppo_trxl.py>", "exec"), ns)
    return ns


def _block(lines, lo, hi):
    return compile(textwrap.dedent("\n".join(lines[lo:hi])), "<reference:ppo_trxl.py>", "exec")


def blocks():
    L = _lines()
    s0 = _find(L, "observation_space = envs.single_observation_space")
    s1 = _find(L, "for iteration in range(1, args.num_iterations + 1):", s0)
    r1 = _find(L, "# Flatten the batch", s1)
    u1 = _find(L, "print(", r1)
    return _block(L, s0, s1), _block(L, s1 + 1, r1), _block(L, r1, u1)


def make_args(overrides):
    d = reference_args_defaults()
    d.update(COMMON)
    d.update(overrides)
    d["batch_size"] = d["num_envs"] * d["num_steps"]
    d["minibatch_size"] = d["batch_size"] // d["num_minibatches"]
    d["num_iterations"] = ITERATIONS
    return SimpleNamespace(**d)


def flat_params(agent):
    return torch.cat([p.detach().reshape(-1) for p in agent.parameters()])


def mint_case(name):
    env_id, env_kw, over = CASES[name]
    args = make_args(over)
    setup, rollout, update = blocks()
    net = load_reference_network()
    envs = E.SyntheticMemoryVecEnv(env_id, args.num_envs, **env_kw)
    ns = dict(net)
    ns.update(args=args, envs=envs, device=torch.device("cpu"), torch=torch, np=np, nn=nn, optim=optim, time=time, deque=deque,
              gym=SimpleNamespace(spaces=SimpleNamespace(Discrete=E.Discrete)))
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    exec(setup, ns)
    agent = ns["agent"]
    rec = {"init_params_sub": flat_params(agent)[::STRIDE].numpy(), "init_checksum": np.float64(flat_params(agent).double().sum()),
           "max_episode_steps": np.int64(ns["max_episode_steps"]), "memory_length": np.int64(args.trxl_memory_length)}
    per = {k: [] for k in ("actions", "log_probs", "values", "rewards", "dones", "stored_memory_masks", "stored_memory_indices",
                           "stored_memory_index", "advantages", "returns", "next_done")}
    sc = {k: [] for k in ("pg_loss", "v_loss", "entropy_loss", "loss", "r_loss", "old_approx_kl", "approx_kl", "clipfrac",
                          "explained_var", "lr", "ent_coef", "actual_max_episode_steps", "num_episodes", "r_mean", "l_mean",
                          "value_mean", "advantage_mean")}
    for iteration in range(1, ITERATIONS + 1):
        ns["iteration"] = iteration
        exec(rollout, ns)
        for k in per:
            per[k].append(ns[k].detach().clone().numpy())
        torch.manual_seed(UPDATE_SEED + iteration)
        exec(update, ns)
        sm = ns["stored_memory_indices"] * ns["stored_memory_masks"]
        for k in ("pg_loss", "v_loss", "entropy_loss", "loss", "r_loss", "old_approx_kl", "approx_kl"):
            sc[k].append(float(ns[k].item()))
        sc["clipfrac"].append(float(np.mean(ns["clipfracs"])))
        sc["explained_var"].append(float(ns["explained_var"]))
        sc["lr"].append(float(ns["lr"]))
        sc["ent_coef"].append(float(ns["ent_coef"]))
        sc["actual_max_episode_steps"].append(float(sm.max().item() + 1))
        sc["num_episodes"].append(float(ns["stored_memories"].shape[0]))
        er = ns["episode_result"]
        sc["r_mean"].append(float(er.get("r_mean", np.nan)))
        sc["l_mean"].append(float(er.get("l_mean", np.nan)))
        sc["value_mean"].append(float(torch.mean(ns["values"]).item()))
        sc["advantage_mean"].append(float(torch.mean(ns["advantages"]).item()))
    for k, v in per.items():
        rec[k] = np.stack(v)
    for k, v in sc.items():
        rec["s_" + k] = np.asarray(v, np.float64)
    final = flat_params(agent)
    rec["final_params_sub"] = final[::STRIDE].numpy()
    rec["final_checksum"] = np.float64(final.double().sum())
    rec["stride"] = np.int64(STRIDE)
    rec["update_seed"] = np.int64(UPDATE_SEED)
    rec["config"] = np.frombuffer(json.dumps({"env_id": env_id, "env": env_kw, "args": {**COMMON, **over}}).encode(), np.uint8)
    print(f"{name}: episodes {sc['num_episodes']}, actual_max_episode_steps {sc['actual_max_episode_steps']} "
          f"(memory length {args.trxl_memory_length}), last-step ends {[int(d.sum()) for d in per['next_done']]}, "
          f"mid dones {[int(d[1:].sum()) for d in per['dones']]}")
    return rec


def main():
    assert R.available(), "needs the reference checkout"
    torch.set_num_threads(1)
    out = {}
    for name in CASES:
        for k, v in mint_case(name).items():
            out[f"{name}/{k}"] = v
    np.savez_compressed(os.path.join(OUT, "trxl_iteration.npz"), **out)
    with open(os.path.join(OUT, "trxl_cli_surface.json"), "w") as fh:
        json.dump({"args": reference_args_defaults()}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", os.path.join(OUT, "trxl_iteration.npz"), os.path.getsize(os.path.join(OUT, "trxl_iteration.npz")), "bytes")


if __name__ == "__main__":
    main()
