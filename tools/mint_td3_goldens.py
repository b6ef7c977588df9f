"""Mint the ddpg_continuous_action / td3_continuous_action fixtures from the reference's own lines.

    python tools/mint_td3_goldens.py

Build-container tool: it needs the reference checkout (``oracle.ref_extract.REFERENCE_ROOT``); nothing on the GPU machine runs it.
It stores no reference text: it ``ast``-compiles ``Actor`` / ``QNetwork`` of the two scripts and the classes and helpers of
cleanrl_utils/buffers.py (whose ``gymnasium.spaces`` import is served by a stand-in module built from cleanrl_amd/envs.py's spaces)
and ``exec``s each script's blocks, located by their lines, against ``SyntheticReplayVecEnv`` on one CPU thread:

* setup -- from ``actor = Actor(envs)`` to ``start_time`` (networks, targets, the two Adams, the ReplayBuffer);
* step  -- the loop body from ``# ALGO LOGIC: put action logic here`` to the ``global_step % 100`` line (action, env step,
  ``final_observation``, ``rb.add``, the training block);
* train -- the training block alone, from ``data = rb.sample`` on.

Per case a second copy of the networks is held in float64 and runs the ``train`` block in lockstep on the float32 run's batches
(same indices, same target noise): the float32 reference's maximum deviation from it, per compared quantity, goes to
tests/golden/td3_iteration_ref_sensitivity.json.  Writes tests/golden/td3_iteration.npz and tests/golden/td3_cli_surface.json.
"""
from __future__ import annotations

import ast
import json
import os
import random
import sys
import textwrap
import time
import types
from collections import namedtuple
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
STEPS = 100
STRIDE = 101
HORIZON = 30

# name -> (script, Args overrides, n_envs)
CASES = {
    "td3": ("td3_continuous_action.py", dict(num_envs=1, buffer_size=64, batch_size=32, learning_starts=8, seed=3)),
    "td3_n2": ("td3_continuous_action.py", dict(num_envs=2, buffer_size=64, batch_size=32, learning_starts=8, seed=4)),
    "ddpg": ("ddpg_continuous_action.py", dict(buffer_size=64, batch_size=32, learning_starts=8, seed=5)),
}
SCALARS = ("qf1_values", "qf1_loss", "qf2_values", "qf2_loss", "actor_loss")


def reference_args_defaults(script) -> dict:
    tree = ast.parse("\n".join(R._read(script)))
    (cls,) = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Args"]
    out = {}
    for b in cls.body:
        if isinstance(b, ast.AnnAssign) and b.target.id != "exp_name":
            out[b.target.id] = eval(compile(ast.Expression(b.value), "<args>", "eval"), {"int": int})
    return out


def reference_args_order(script) -> list:
    tree = ast.parse("\n".join(R._read(script)))
    (cls,) = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Args"]
    return [b.target.id for b in cls.body if isinstance(b, ast.AnnAssign)]


def load_reference_classes(script):
    tree = ast.parse("\n".join(R._read(script)))
    wanted = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in ("Actor", "QNetwork")]
    ns = {"np": np, "torch": torch, "nn": nn, "F": F}
    exec(compile(ast.Module(body=wanted, type_ignores=[]), f"<reference:{script}>", "exec"), ns)
    spaces = types.ModuleType("gymnasium.spaces")
    spaces.Box, spaces.Discrete, spaces.MultiDiscrete, spaces.Space = E.Box, E.Discrete, E.MultiDiscrete, object
    spaces.MultiBinary = spaces.Dict = type("_Absent", (), {})
    gym = types.ModuleType("gymnasium")
    gym.spaces = spaces
    saved = {k: sys.modules.get(k) for k in ("gymnasium", "gymnasium.spaces")}
    sys.modules["gymnasium"], sys.modules["gymnasium.spaces"] = gym, spaces
    try:
        with open(os.path.join(R.REFERENCE_ROOT, "cleanrl_utils", "buffers.py")) as fh:
            btree = ast.parse(fh.read())
        bns = {"__name__": "reference_buffers"}
        exec(compile(btree, "<reference:buffers.py>", "exec"), bns)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    ns["ReplayBuffer"] = bns["ReplayBuffer"]
    return ns


def blocks(script):
    L = R._read(script)
    s0 = R._find(L, "actor = Actor(envs).to(device)")
    s1 = R._find(L, "start_time = time.time()", s0)
    b0 = R._find(L, "# ALGO LOGIC: put action logic here", s1)
    t0 = R._find(L, "data = rb.sample(args.batch_size)", b0)
    b1 = R._find(L, "if global_step % 100 == 0:", t0)

    def block(lo, hi):
        return compile(textwrap.dedent("\n".join(L[lo:hi])), f"<reference:{script}>", "exec")

    return block(s0, s1), block(b0, b1), block(t0, b1)


class _Writer:
    def add_scalar(self, *a, **k):
        pass


def make_args(script, over):
    d = reference_args_defaults(script)
    d.update(over)
    d["total_timesteps"] = STEPS
    return SimpleNamespace(**d)


def flat(*nets):
    return torch.cat([p.detach().reshape(-1) for n in nets for p in n.parameters()])


class _TorchShim:
    """``torch`` with ``randn_like`` returning the float32 run's draw (in float64)."""

    def __init__(self):
        self.noise = None

    def __getattr__(self, k):
        return getattr(torch, k)

    def randn_like(self, *a, **k):
        return self.noise


Samples = namedtuple("Samples", "observations actions next_observations dones rewards")


class _Rb64:
    def __init__(self, rb):
        self.rb, self.inds = rb, None

    def sample(self, batch_size):
        bi, ei = self.inds
        rb = self.rb
        t = lambda a: torch.tensor(a, dtype=torch.float64)  # noqa: E731
        return Samples(t(rb.observations[bi, ei, :]), t(rb.actions[bi, ei, :]), t(rb.next_observations[bi, ei, :]),
                       t(rb.dones[bi, ei].reshape(-1, 1)), t(rb.rewards[bi, ei].reshape(-1, 1)))


def _namespace(args, envs, classes):
    ns = dict(classes)
    ns.update(args=args, envs=envs, device=torch.device("cpu"), torch=torch, np=np, nn=nn, F=F, optim=optim, time=time, writer=_Writer())
    return ns


def mint_case(name):
    script, over = CASES[name]
    td3 = script.startswith("td3")
    args = make_args(script, over)
    N = getattr(args, "num_envs", 1)
    setup, step, train = blocks(script)
    classes = load_reference_classes(script)
    nets = ("actor", "qf1", "qf2") if td3 else ("actor", "qf1")
    all_nets = nets + ("target_actor", "qf1_target") + (("qf2_target",) if td3 else ())

    def seeded_setup():
        random.seed(args.seed)
        np.random.seed(args.seed)
        torch.manual_seed(args.seed)
        envs = E.SyntheticReplayVecEnv(N, seed=args.seed, horizon=HORIZON)
        ns = _namespace(args, envs, classes)
        exec(setup, ns)
        return ns

    ns64 = seeded_setup()
    for k in all_nets:
        ns64[k].double()
    shim, rb64 = _TorchShim(), None
    ns = seeded_setup()                                          # the float32 run owns the global random streams from here on
    rb64 = _Rb64(ns["rb"])
    ns64.update(torch=shim, rb=rb64)
    envs = ns["envs"]
    A = envs.single_action_space.shape[0]
    B = args.batch_size
    rec = {"init_checksum": np.float64(flat(*[ns[k] for k in nets]).double().sum())}
    per = {k: [] for k in ("actions", "batch_inds", "env_inds", "noise", "policy_update") + SCALARS}
    dev = {k: 0.0 for k in SCALARS}
    ns["obs"], _ = envs.reset(seed=args.seed)
    truncs = 0
    for global_step in range(STEPS):
        ns["global_step"] = ns64["global_step"] = global_step
        np_state, t_state = np.random.get_state(), torch.get_rng_state()
        pos, full = ns["rb"].pos, ns["rb"].full
        exec(step, ns)
        truncs += int(np.asarray(ns["truncations"]).sum())
        per["actions"].append(np.asarray(ns["actions"], np.float32).reshape(N, A))
        trained = global_step > args.learning_starts
        bi, ei, nz = np.full(B, -1, np.int64), np.full(B, -1, np.int64), np.zeros((B, A), np.float32)
        sc = {k: np.nan for k in SCALARS}
        if trained:
            rs = np.random.RandomState()
            rs.set_state(np_state)
            pos, full = (pos + 1) % ns["rb"].buffer_size, full or pos + 1 == ns["rb"].buffer_size      # rb.add ran before rb.sample
            bi = rs.randint(0, ns["rb"].buffer_size if full else pos, size=B)
            ei = rs.randint(0, high=N, size=(B,))
            g = torch.Generator()
            g.set_state(t_state)
            if global_step >= args.learning_starts:
                torch.normal(torch.zeros_like(ns["actor"].action_scale), ns["actor"].action_scale * args.exploration_noise, generator=g)
            if td3:
                nz = torch.randn((B, A), generator=g).numpy()
            rb64.inds, shim.noise = (bi, ei), torch.from_numpy(nz).double()
            exec(train, ns64)
            for k in SCALARS:
                src = {"qf1_values": "qf1_a_values", "qf2_values": "qf2_a_values"}.get(k, k)
                if src in ns and (k != "actor_loss" or "actor_loss" in ns):
                    v32, v64 = ns[src], ns64[src]
                    v32, v64 = (v.mean() if v.dim() else v for v in (v32, v64))
                    sc[k] = float(v32.item())
                    dev[k] = max(dev[k], abs(float(v32.item()) - float(v64.item())))
        per["batch_inds"].append(bi), per["env_inds"].append(ei), per["noise"].append(nz)
        per["policy_update"].append(np.int64(trained and global_step % args.policy_frequency == 0))
        for k in SCALARS:
            per[k].append(sc[k])
    # the recovered draws must be the run's own: check the last batch against the buffer
    data = ns["data"]
    assert torch.equal(data.observations, torch.tensor(ns["rb"].observations[bi, ei, :])), "index recovery is off"
    for k, v in per.items():
        rec[k] = np.stack(v) if k in ("actions", "batch_inds", "env_inds", "noise") else np.asarray(v)
    fa, fq = flat(ns["actor"]), flat(*[ns[k] for k in nets[1:]])
    fa64, fq64 = flat(ns64["actor"]), flat(*[ns64[k] for k in nets[1:]])
    ft, ft64 = flat(*[ns[k] for k in all_nets[len(nets):]]), flat(*[ns64[k] for k in all_nets[len(nets):]])
    for nm, f32, f64 in (("actor", fa, fa64), ("critics", fq, fq64), ("targets", ft, ft64)):
        rec[f"final_{nm}_sub"] = f32[::STRIDE].numpy()
        rec[f"final_{nm}_checksum"] = np.float64(f32.double().sum())
        dev[f"final_{nm}"] = float((f32.double() - f64).abs().max())
    rec["stride"] = np.int64(STRIDE)
    rec["config"] = np.frombuffer(json.dumps({"script": script, "args": over, "steps": STEPS, "horizon": HORIZON}).encode(), np.uint8)
    assert truncs >= 1 and ns["rb"].full, "the horizon must cross a truncation and the ring must wrap"
    print(f"{name}: truncations {truncs}, trained steps {int((rec['batch_inds'][:, 0] >= 0).sum())}, deviations {dev}")
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
    path = os.path.join(OUT, "td3_iteration.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(OUT, "td3_iteration_ref_sensitivity.json"), "w") as fh:
        json.dump(sens, fh, indent=1, sort_keys=True)
        fh.write("\n")
    with open(os.path.join(OUT, "td3_cli_surface.json"), "w") as fh:
        surf = {s[: -len(".py")]: {"defaults": reference_args_defaults(s), "order": reference_args_order(s)}
                for s in sorted({c[0] for c in CASES.values()})}
        json.dump(surf, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
