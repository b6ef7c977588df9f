"""Mint the dqn_atari / c51_atari fixtures from the reference's own lines.

    python tools/mint_dqn_atari_goldens.py

Build-container tool: it needs the reference checkout (``oracle.ref_extract.REFERENCE_ROOT``); nothing on the GPU machine runs it.
It stores no reference text: as tools/mint_dqn_goldens.py does, it ``ast``-compiles ``QNetwork`` and ``linear_schedule`` of the two
scripts and ``ReplayBuffer`` of cleanrl_utils/buffers.py -- built by the scripts' own setup lines with ``optimize_memory_usage=True`` --
and ``exec``s each script's setup, step and train blocks, located by their lines, against ``AtariReplayVecEnv`` (6 actions, horizon 10)
on one CPU thread.  Frames are never stored: both sides regenerate them from the seed.  A float64 copy of the networks runs the
``train`` block in lockstep on the float32 run's batches; the float32 reference's maximum deviation from it, per compared quantity,
goes to tests/golden/dqn_atari_iteration_ref_sensitivity.json.  Final parameters are stored at a stride.  Writes
tests/golden/dqn_atari_iteration.npz and tests/golden/dqn_atari_cli_surface.json.
"""
from __future__ import annotations

import ast
import json
import os
import random
import sys
import textwrap
import time
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.optim as optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mint_td3_goldens as T  # noqa: E402
from cleanrl_amd import envs as E  # noqa: E402
from oracle import ref_extract as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
STEPS = 40
STRIDE = 997
N_ACTIONS = 6
HORIZON = 10

_COMMON = dict(buffer_size=16, batch_size=8, learning_starts=8, train_frequency=2, target_network_frequency=6)
# name -> (script, Args overrides)
CASES = {
    "dqn_atari": ("dqn_atari.py", dict(_COMMON, seed=3, exploration_fraction=0.5, end_e=0.3)),
    "c51_atari": ("c51_atari.py", dict(_COMMON, seed=5, n_atoms=51, exploration_fraction=0.5, end_e=0.3)),
    "c51_small": ("c51_atari.py", dict(_COMMON, seed=6, n_atoms=5, v_min=-2, v_max=2, exploration_fraction=0.5, end_e=0.3)),
}
SCALARS = ("loss", "q_values")


def load_reference_classes(script):
    ns = T.load_reference_classes(script)                       # QNetwork and ReplayBuffer
    tree = ast.parse("\n".join(R._read(script)))
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "linear_schedule"]
    exec(compile(ast.Module(body=fn, type_ignores=[]), f"<reference:{script}>", "exec"), ns)
    return ns


def blocks(script):
    L = R._read(script)
    s0 = R._find(L, "q_network = QNetwork(envs")
    s1 = R._find(L, "start_time = time.time()", s0)
    b0 = R._find(L, "# ALGO LOGIC: put action logic here", s1)
    t0 = R._find(L, "if global_step % args.train_frequency == 0:", b0)
    b1 = R._find(L, "if args.save_model:", t0)

    def block(lo, hi):
        return compile(textwrap.dedent("\n".join(L[lo:hi])), f"<reference:{script}>", "exec")

    return block(s0, s1), block(b0, b1), block(t0, b1)


def make_args(script, over):
    d = T.reference_args_defaults(script)
    d.update(over)
    d["total_timesteps"] = STEPS
    return SimpleNamespace(**d)


class _Rb64:
    def __init__(self, rb):
        self.rb, self.inds = rb, None

    def sample(self, batch_size):
        bi, ei = self.inds
        rb = self.rb
        t = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
        return T.Samples(t(rb.observations[bi, ei, :]), torch.tensor(rb.actions[bi, ei, :]), t(rb.observations[(bi + 1) % rb.buffer_size, ei, :]),
                         t(rb.dones[bi, ei].reshape(-1, 1)), t(rb.rewards[bi, ei].reshape(-1, 1)))


def _namespace(args, envs, classes):
    ns = dict(classes)
    ns.update(args=args, envs=envs, device=torch.device("cpu"), torch=torch, np=np, nn=nn, F=F, optim=optim, time=time, random=random,
              writer=T._Writer())
    return ns


def _scalars(ns, c51):
    loss = ns["loss"]
    if c51:
        q = (ns["old_pmfs"] * ns["q_network"].atoms).sum(1).mean()      # the reference's logging line
    else:
        q = ns["old_val"].mean()
    return float(loss.item()), float(q.item())


def mint_case(name):
    script, over = CASES[name]
    c51 = script.startswith("c51")
    assert ("optimize_memory_usage=True" in "".join(R._read(script)))
    args = make_args(script, over)
    setup, step, train = blocks(script)
    classes = load_reference_classes(script)
    nets = ("q_network", "target_network")

    def seeded_setup():
        random.seed(args.seed)
        np.random.seed(args.seed)
        torch.manual_seed(args.seed)
        envs = E.AtariReplayVecEnv(1, seed=args.seed, n_actions=N_ACTIONS, horizon=HORIZON)
        ns = _namespace(args, envs, classes)
        exec(setup, ns)
        return ns

    ns64 = seeded_setup()
    for k in nets:
        ns64[k].double()
    ns = seeded_setup()                                          # the float32 run owns the global random streams from here on
    rb64 = _Rb64(ns["rb"])
    ns64.update(rb=rb64)
    envs = ns["envs"]
    B = args.batch_size
    rec = {"init_checksum": np.float64(T.flat(ns["q_network"]).double().sum())}
    per = {k: [] for k in ("actions", "batch_inds", "env_inds", "random_branch", "target_update") + SCALARS}
    dev = {k: 0.0 for k in SCALARS}
    ns["obs"], _ = envs.reset(seed=args.seed)
    truncs = terms = 0
    for global_step in range(STEPS):
        ns["global_step"] = ns64["global_step"] = global_step
        np_state, py_state = np.random.get_state(), random.getstate()
        pos, full = ns["rb"].pos, ns["rb"].full
        exec(step, ns)
        truncs += int(np.asarray(ns["truncations"]).sum())
        terms += int(np.asarray(ns["terminations"]).sum())
        per["actions"].append(np.asarray(ns["actions"], np.int64).reshape(1))
        pr = random.Random()
        pr.setstate(py_state)
        per["random_branch"].append(np.int64(pr.random() < ns["epsilon"]))
        learning = global_step > args.learning_starts
        trained = learning and global_step % args.train_frequency == 0
        bi, ei = np.full(B, -1, np.int64), np.full(B, -1, np.int64)
        sc = {k: np.nan for k in SCALARS}
        if trained:
            rs = np.random.RandomState()
            rs.set_state(np_state)
            pos, full = (pos + 1) % ns["rb"].buffer_size, full or pos + 1 == ns["rb"].buffer_size      # rb.add ran before rb.sample
            size = ns["rb"].buffer_size                                # the memory-optimised sample: never slot pos once full
            bi = (rs.randint(1, size, size=B) + pos) % size if full else rs.randint(0, pos, size=B)
            ei = rs.randint(0, high=1, size=(B,))
            rb64.inds = (bi, ei)
            # the recovered draws must be the run's own: check the batch against the buffer
            assert torch.equal(ns["data"].observations, torch.tensor(ns["rb"].observations[bi, ei, :])), "index recovery is off"
        if learning:
            exec(train, ns64)
        if trained:
            for k, v32, v64 in zip(SCALARS, _scalars(ns, c51), _scalars(ns64, c51)):
                sc[k] = v32
                dev[k] = max(dev[k], abs(v32 - v64))
        per["batch_inds"].append(bi), per["env_inds"].append(ei)
        per["target_update"].append(np.int64(learning and global_step % args.target_network_frequency == 0))
        for k in SCALARS:
            per[k].append(sc[k])
    for k, v in per.items():
        rec[k] = np.stack(v) if k in ("actions", "batch_inds", "env_inds") else np.asarray(v)
    for nm, key in (("online", "q_network"), ("target", "target_network")):
        f32, f64 = T.flat(ns[key]), T.flat(ns64[key])
        rec[f"final_{nm}_sub"] = f32[::STRIDE].numpy()
        rec[f"final_{nm}_checksum"] = np.float64(f32.double().sum())
        dev[f"final_{nm}"] = float((f32.double() - f64).abs().max())
    rec["stride"] = np.int64(STRIDE)
    rec["config"] = np.frombuffer(json.dumps({"script": script, "args": over, "steps": STEPS, "horizon": HORIZON, "n_actions": N_ACTIONS}).encode(), np.uint8)
    rb = rec["random_branch"]
    assert truncs >= 1 and ns["rb"].full, "the horizon must cross a truncation and the ring must wrap"
    assert 0 < rb.sum() < STEPS, "both action branches must occur"
    print(f"{name}: truncations {truncs}, terminations {terms}, random actions {int(rb.sum())}, trained steps "
          f"{int((rec['batch_inds'][:, 0] >= 0).sum())}, target updates {int(rec['target_update'].sum())}, deviations {dev}")
    return rec, dev


def main():
    assert R.available(), "needs the reference checkout"
    torch.set_num_threads(1)
    out, sens = {}, {}
    for name in CASES:
        rec, dev = mint_case(name)
        sens[name] = dev
        for k, v in rec.items():
            out[f"{name}/{k}"] = v
    path = os.path.join(OUT, "dqn_atari_iteration.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(OUT, "dqn_atari_iteration_ref_sensitivity.json"), "w") as fh:
        json.dump(sens, fh, indent=1, sort_keys=True)
        fh.write("\n")
    with open(os.path.join(OUT, "dqn_atari_cli_surface.json"), "w") as fh:
        surf = {s[: -len(".py")]: {"defaults": T.reference_args_defaults(s), "order": T.reference_args_order(s)}
                for s in sorted({c[0] for c in CASES.values()})}
        json.dump(surf, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
