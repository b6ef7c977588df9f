"""Mint the pqn_atari_envpool_lstm fixtures from the reference's own lines.

    python tools/mint_pqn_lstm_goldens.py

Build-container tool, built like tools/mint_pqn_goldens.py (whose helpers it imports): it needs the reference checkout
(``oracle.ref_extract.REFERENCE_ROOT``), stores no reference text, ``ast``-compiles ``layer_init``, ``QNetwork`` and
``linear_schedule`` of cleanrl/pqn_atari_envpool_lstm.py and ``exec``s the main loop's setup / rollout / update blocks, found by
the same four anchor lines, against ``SyntheticAtariVecEnv(api="gym", frames=1)`` on one CPU thread.  The setup block creates
``next_lstm_state``; the rollout block starts with the ``initial_lstm_state`` clone.

The case ends episodes often (``done_p=0.1``), so that both iterations reset the state in mid-rollout, the second iteration
starts from a non-zero state and the bootstrap sees ``next_done``.  Writes tests/golden/pqn_lstm_iteration.npz (storage of two
iterations, the state at the start of each iteration and at the end, scalars, parameters subsampled at a stride with checksums)
and tests/golden/pqn_lstm_cli_surface.json.
"""
from __future__ import annotations

import json
import os
import random
import sys
import time
from collections import deque

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.optim as optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mint_pqn_goldens as M  # noqa: E402
from cleanrl_amd import envs as E  # noqa: E402
from oracle import ref_extract as R  # noqa: E402

SCRIPT = "pqn_atari_envpool_lstm.py"
STRIDE = 101
DONE_P = 0.1
ARGS = dict(num_envs=4, num_steps=8, num_minibatches=2, update_epochs=2, start_e=0.5, end_e=0.01, exploration_fraction=0.5, seed=5)


def make_envs(args):
    return E.SyntheticAtariVecEnv(args.num_envs, seed=args.seed, n_actions=4, api="gym", frames=1, done_p=DONE_P)


def mint():
    args = M.make_args(SCRIPT, ARGS)
    setup, rollout, update = M.blocks(SCRIPT)
    ns = M.load_reference_network(SCRIPT)
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    envs = make_envs(args)
    ns.update(args=args, envs=envs, device=torch.device("cpu"), torch=torch, np=np, nn=nn, F=F, optim=optim, time=time, deque=deque,
              writer=M._Writer())
    exec(setup, ns)
    net = ns["q_network"]
    init = M.flat_params(net)
    rec = {"init_params_sub": init[::STRIDE].numpy(), "stride": np.int64(STRIDE), "init_checksum": np.float64(init.double().sum())}
    per = {k: [] for k in ("actions", "values", "rewards", "dones", "returns", "next_done", "initial_h", "initial_c")}
    sc = {"td_loss": [], "q_values": [], "global_step": []}
    for iteration in range(1, M.ITERATIONS + 1):
        ns["iteration"] = iteration
        exec(rollout, ns)
        for k in ("actions", "values", "rewards", "dones", "returns", "next_done"):
            per[k].append(ns[k].detach().clone().numpy())
        per["initial_h"].append(ns["initial_lstm_state"][0].detach().clone().numpy())
        per["initial_c"].append(ns["initial_lstm_state"][1].detach().clone().numpy())
        exec(update, ns)
        sc["td_loss"].append(float(ns["loss"].item()))
        sc["q_values"].append(float(ns["old_val"].mean().item()))
        sc["global_step"].append(float(ns["global_step"]))
    for k, v in per.items():
        rec[k] = np.stack(v)
    for k, v in sc.items():
        rec["s_" + k] = np.asarray(v, np.float64)
    rec["final_h"] = ns["next_lstm_state"][0].detach().clone().numpy()
    rec["final_c"] = ns["next_lstm_state"][1].detach().clone().numpy()
    final = M.flat_params(net)
    rec["final_params_sub"] = final[::STRIDE].numpy()
    rec["final_checksum"] = np.float64(final.double().sum())
    rec["config"] = np.frombuffer(json.dumps({"script": SCRIPT, "args": ARGS, "iterations": M.ITERATIONS, "done_p": DONE_P}).encode(),
                                  np.uint8)
    print(f"lstm: actions {np.bincount(rec['actions'].astype(np.int64).ravel())}, dones at t >= 1 per iteration "
          f"{[int(d[1:].sum()) for d in rec['dones']]}, next_done {[int(d.sum()) for d in rec['next_done']]}, "
          f"|initial_h| {[float(np.abs(h).max()) for h in rec['initial_h']]}, td_loss {sc['td_loss']}")
    return rec


def main():
    assert R.available(), "needs the reference checkout"
    torch.set_num_threads(1)
    out = {f"lstm/{k}": v for k, v in mint().items()}
    path = os.path.join(M.OUT, "pqn_lstm_iteration.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(M.OUT, "pqn_lstm_cli_surface.json"), "w") as fh:
        json.dump({"lstm": M.reference_args_defaults(SCRIPT)}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
