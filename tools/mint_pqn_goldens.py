"""Mint the pqn / pqn_atari_envpool fixtures from the reference's own lines.

    python tools/mint_pqn_goldens.py

Build-container tool: it needs the reference checkout (``oracle.ref_extract.REFERENCE_ROOT``); nothing on the GPU machine runs it.
Like ``oracle/ref_extract.py`` it stores no reference text: it ``ast``-compiles ``layer_init``, ``QNetwork`` and ``linear_schedule`` of
cleanrl/pqn.py and cleanrl/pqn_atari_envpool.py and ``exec``s the main loop's blocks, located by their lines, against the stand-ins
of cleanrl_amd/envs.py (``CartPoleVecEnv``; ``SyntheticAtariVecEnv(api="gym")``) on one CPU thread:

* setup   -- from ``q_network = QNetwork(envs)`` to the ``for iteration`` line (network, RAdam, storage, reset);
* rollout -- the iteration body up to ``# flatten the batch`` (annealing, action logic, env steps, Q(lambda) targets);
* update  -- ``# flatten the batch`` up to the ``losses/td_loss`` line (shuffled minibatches, TD loss, clip, RAdam).

Seeding is the reference's (``random`` / ``numpy`` / ``torch`` with ``args.seed`` before the env and the network), so a replay
that draws in the reference's order meets the same random stream.  Writes tests/golden/pqn_iteration.npz and
tests/golden/pqn_cli_surface.json.
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
import torch.nn.functional as F
import torch.optim as optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cleanrl_amd import envs as E  # noqa: E402
from oracle import ref_extract as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
ITERATIONS = 2
ATARI_STRIDE = 101

# name -> (script, Args overrides).  start_e below 1 so that greedy actions occur from the first step on.
CASES = {
    "pqn": ("pqn.py", dict(num_envs=4, num_steps=16, num_minibatches=4, update_epochs=2, start_e=0.5, end_e=0.05,
                           exploration_fraction=0.5, seed=3)),
    "atari": ("pqn_atari_envpool.py", dict(num_envs=4, num_steps=8, num_minibatches=4, update_epochs=2, start_e=0.5, end_e=0.01,
                                           exploration_fraction=0.5, seed=5)),
}


def reference_args_defaults(script) -> dict:
    """The reference's ``Args`` fields and defaults, as data (``exp_name`` left out)."""
    tree = ast.parse("\n".join(R._read(script)))
    (cls,) = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Args"]
    return {b.target.id: ast.literal_eval(b.value) for b in cls.body if isinstance(b, ast.AnnAssign) and b.target.id != "exp_name"}


def load_reference_network(script):
    tree = ast.parse("\n".join(R._read(script)))
    names = ("layer_init", "QNetwork", "linear_schedule")
    wanted = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert {n.name for n in wanted} == set(names)
    ns = {"np": np, "torch": torch, "nn": nn}
    exec(compile(ast.Module(body=wanted, type_ignores=[]), f"<reference:{script}>", "exec"), ns)
    return ns


def blocks(script):
    L = R._read(script)
    s0 = R._find(L, "q_network = QNetwork(envs)")
    s1 = R._find(L, "for iteration in range(1, args.num_iterations + 1):", s0)
    r1 = R._find(L, "# flatten the batch", s1)
    u1 = R._find(L, 'writer.add_scalar("losses/td_loss"', r1)

    def block(lo, hi):
        return compile(textwrap.dedent("\n".join(L[lo:hi])), f"<reference:{script}>", "exec")

    return block(s0, s1), block(s1 + 1, r1), block(r1, u1)


class _Writer:
    def add_scalar(self, *a, **k):
        pass


def make_args(script, over):
    d = reference_args_defaults(script)
    d.update(over)
    d["batch_size"] = d["num_envs"] * d["num_steps"]
    d["minibatch_size"] = d["batch_size"] // d["num_minibatches"]
    d["total_timesteps"] = d["batch_size"] * ITERATIONS
    d["num_iterations"] = ITERATIONS
    return SimpleNamespace(**d)


def make_envs(name, args):
    if name == "pqn":
        return E.CartPoleVecEnv(args.num_envs, seed=args.seed)
    return E.SyntheticAtariVecEnv(args.num_envs, seed=args.seed, n_actions=4, api="gym")


def flat_params(net):
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()])


def mint_case(name):
    script, over = CASES[name]
    args = make_args(script, over)
    setup, rollout, update = blocks(script)
    ns = load_reference_network(script)
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    envs = make_envs(name, args)
    ns.update(args=args, envs=envs, device=torch.device("cpu"), torch=torch, np=np, nn=nn, F=F, optim=optim, time=time, deque=deque,
              writer=_Writer())
    exec(setup, ns)
    net = ns["q_network"]
    init = flat_params(net)
    rec = {}
    if name == "pqn":
        rec["init_params"] = init.numpy()
    else:
        rec["init_params_sub"] = init[::ATARI_STRIDE].numpy()
        rec["stride"] = np.int64(ATARI_STRIDE)
    rec["init_checksum"] = np.float64(init.double().sum())
    per = {k: [] for k in ("actions", "values", "rewards", "dones", "returns", "next_done")}
    sc = {"td_loss": [], "q_values": [], "global_step": []}
    for iteration in range(1, ITERATIONS + 1):
        ns["iteration"] = iteration
        exec(rollout, ns)
        for k in per:
            per[k].append(ns[k].detach().clone().numpy())
        exec(update, ns)
        sc["td_loss"].append(float(ns["loss"].item()))
        sc["q_values"].append(float(ns["old_val"].mean().item()))
        sc["global_step"].append(float(ns["global_step"]))
    for k, v in per.items():
        rec[k] = np.stack(v)
    for k, v in sc.items():
        rec["s_" + k] = np.asarray(v, np.float64)
    final = flat_params(net)
    if name == "pqn":
        rec["final_params"] = final.numpy()
    else:
        rec["final_params_sub"] = final[::ATARI_STRIDE].numpy()
    rec["final_checksum"] = np.float64(final.double().sum())
    rec["config"] = np.frombuffer(json.dumps({"script": script, "args": over, "iterations": ITERATIONS}).encode(), np.uint8)
    a = rec["actions"]
    print(f"{name}: actions {np.bincount(a.astype(np.int64).ravel())}, dones {int(rec['dones'].sum())}, "
          f"next_done {int(rec['next_done'].sum())}, td_loss {sc['td_loss']}")
    return rec


def main():
    assert R.available(), "needs the reference checkout"
    torch.set_num_threads(1)
    out = {}
    for name in CASES:
        for k, v in mint_case(name).items():
            out[f"{name}/{k}"] = v
    path = os.path.join(OUT, "pqn_iteration.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(OUT, "pqn_cli_surface.json"), "w") as fh:
        json.dump({name: reference_args_defaults(script) for name, (script, _) in CASES.items()}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
