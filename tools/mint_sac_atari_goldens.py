"""Mint the sac_atari fixtures from the reference's own lines.

    python tools/mint_sac_atari_goldens.py

Build-container tool: it needs the reference checkout (``oracle.ref_extract.REFERENCE_ROOT``); nothing on the GPU machine runs it.
It stores no reference text: as tools/mint_dqn_atari_goldens.py does, it ``ast``-compiles ``Actor``, ``SoftQNetwork`` and ``layer_init``
of cleanrl/sac_atari.py and ``ReplayBuffer`` of cleanrl_utils/buffers.py -- built by the script's own setup lines, without
``optimize_memory_usage`` -- and ``exec``s the script's setup, step and train blocks, located by their lines, against
``AtariReplayVecEnv`` (6 actions, horizon 10) on one CPU thread.  Frames are never stored: both sides regenerate them from the seed.
A float64 copy of the five networks and ``log_alpha`` runs the train block in lockstep on the float32 run's batches (its
``Categorical.sample`` draws nothing: the update discards the sampled actions); the float32 reference's maximum deviation from it, per
compared quantity, goes to tests/golden/sac_atari_iteration_ref_sensitivity.json.  Final parameters are stored at a stride.  Writes
tests/golden/sac_atari_iteration.npz, sac_atari_cli_surface.json and sac_atari_network_init.npz.
"""
from __future__ import annotations

import ast
import json
import os
import random
import re
import sys
import textwrap
import time
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.optim as optim
from torch.distributions.categorical import Categorical

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import mint_td3_goldens as T  # noqa: E402
from cleanrl_amd import envs as E  # noqa: E402
from oracle import ref_extract as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SCRIPT = "sac_atari.py"
STEPS = 40
STRIDE = 1999
N_ACTIONS = 6
HORIZON = 10

_COMMON = dict(buffer_size=16, batch_size=4, learning_starts=8, update_frequency=4, target_network_frequency=8)
CASES = {
    "sac_atari": dict(_COMMON, seed=3),
    "sac_atari_fixed": dict(_COMMON, seed=4, autotune=False),
    "sac_atari_polyak": dict(_COMMON, seed=5, tau=0.5),
}
SCALARS = ("qf1_values", "qf2_values", "qf1_loss", "qf2_loss", "qf_loss", "actor_loss", "alpha_loss", "alpha")
SOURCE = {"qf1_values": "qf1_a_values", "qf2_values": "qf2_a_values"}
NETS = ("actor", "qf1", "qf2")
TARGETS = ("qf1_target", "qf2_target")
GROUPS = (("actor", ("actor",)), ("critics", ("qf1", "qf2")), ("targets", TARGETS))
PROBES = (0, 1, 8191, 8192, 77777, 1684127)          # flat elements of a network recorded beside its checksum


class _QuietCategorical(Categorical):
    """``Categorical`` whose ``sample`` draws nothing (the float64 copy must leave torch's generator to the float32 run)."""

    def sample(self, sample_shape=torch.Size()):
        return self.probs.argmax(-1)


def load_classes(categorical):
    tree = ast.parse("\n".join(R._read(SCRIPT)))
    body = [n for n in tree.body if (isinstance(n, ast.ClassDef) and n.name in ("Actor", "SoftQNetwork"))
            or (isinstance(n, ast.FunctionDef) and n.name == "layer_init")]
    ns = {"np": np, "torch": torch, "nn": nn, "F": F, "Categorical": categorical}
    exec(compile(ast.Module(body=body, type_ignores=[]), f"<reference:{SCRIPT}>", "exec"), ns)
    ns["ReplayBuffer"] = T.load_reference_classes("td3_continuous_action.py")["ReplayBuffer"]
    return ns


def blocks():
    L = R._read(SCRIPT)
    s0 = R._find(L, "actor = Actor(envs).to(device)")
    s1 = R._find(L, "start_time = time.time()", s0)
    b0 = R._find(L, "# ALGO LOGIC: put action logic here", s1)
    t0 = R._find(L, "if global_step % args.update_frequency == 0:", b0)
    b1 = R._find(L, "if global_step % 100 == 0:", t0)

    def block(lo, hi):
        return compile(textwrap.dedent("\n".join(L[lo:hi])), f"<reference:{SCRIPT}>", "exec")

    return block(s0, s1), block(b0, b1), block(t0, b1)


def logged_tags():
    return re.findall(r'writer\.add_scalar\("([^"]+)"', "\n".join(R._read(SCRIPT)))


def make_args(over):
    d = T.reference_args_defaults(SCRIPT)
    d.update(over)
    d["total_timesteps"] = STEPS
    return SimpleNamespace(**d)


def _namespace(args, envs, classes):
    ns = dict(classes)
    ns.update(args=args, envs=envs, device=torch.device("cpu"), torch=torch, np=np, nn=nn, F=F, optim=optim, time=time, random=random,
              writer=T._Writer())
    return ns


def mint_case(name):
    over = CASES[name]
    assert "optimize_memory_usage" not in "".join(R._read(SCRIPT))
    args = make_args(over)
    B = args.batch_size
    setup, step, train = blocks()

    def seeded_setup(classes):
        random.seed(args.seed)
        np.random.seed(args.seed)
        torch.manual_seed(args.seed)
        envs = E.AtariReplayVecEnv(1, seed=args.seed, n_actions=N_ACTIONS, horizon=HORIZON)
        ns = _namespace(args, envs, classes)
        exec(setup, ns)
        return ns

    ns64 = seeded_setup(load_classes(_QuietCategorical))
    for k in NETS + TARGETS:
        ns64[k].double()
    if args.autotune:
        ns64["log_alpha"] = torch.zeros(1, requires_grad=True, dtype=torch.float64)
        ns64["alpha"] = ns64["log_alpha"].exp().item()
        ns64["a_optimizer"] = optim.Adam([ns64["log_alpha"]], lr=args.q_lr, eps=1e-4)
    ns = seeded_setup(load_classes(Categorical))                 # the float32 run owns the global random streams from here on
    rb64 = T._Rb64(ns["rb"])
    ns64.update(rb=rb64)
    envs = ns["envs"]
    rec = {"init_checksum": np.float64(T.flat(*[ns[k] for k in NETS]).double().sum())}
    per = {k: [] for k in ("actions", "batch_inds", "env_inds", "target_update") + SCALARS}
    dev = {k: 0.0 for k in SCALARS}
    ns["obs"], _ = envs.reset(seed=args.seed)
    truncs = dones_in_batch = 0
    for global_step in range(STEPS):
        ns["global_step"] = ns64["global_step"] = global_step
        np_state = np.random.get_state()
        pos, full = ns["rb"].pos, ns["rb"].full
        exec(step, ns)
        truncs += int(np.asarray(ns["truncations"]).sum())
        per["actions"].append(np.asarray(ns["actions"], np.int64).reshape(1))
        learning = global_step > args.learning_starts
        trained = learning and global_step % args.update_frequency == 0
        bi, ei = np.full(B, -1, np.int64), np.full(B, -1, np.int64)
        sc = {k: np.nan for k in SCALARS}
        if trained:
            rs = np.random.RandomState()
            rs.set_state(np_state)
            pos, full = (pos + 1) % ns["rb"].buffer_size, full or pos + 1 == ns["rb"].buffer_size      # rb.add ran before rb.sample
            bi = rs.randint(0, ns["rb"].buffer_size if full else pos, size=B)
            ei = rs.randint(0, high=1, size=(B,))
            rb64.inds = (bi, ei)
            # the recovered draws must be the run's own: check the batch against the buffer
            assert torch.equal(ns["data"].observations, torch.tensor(ns["rb"].observations[bi, ei, :])), "index recovery is off"
            assert torch.equal(ns["data"].next_observations, torch.tensor(ns["rb"].next_observations[bi, ei, :]))
            dones_in_batch += int(ns["data"].dones.sum().item())
        if learning:
            exec(train, ns64)
        if trained:
            for k in SCALARS:
                src = SOURCE.get(k, k)
                if src in ns:
                    v32, v64 = (float(v.mean().item()) if torch.is_tensor(v) else float(v) for v in (ns[src], ns64[src]))
                    sc[k] = v32
                    dev[k] = max(dev[k], abs(v32 - v64))
        per["batch_inds"].append(bi), per["env_inds"].append(ei)
        per["target_update"].append(np.int64(learning and global_step % args.target_network_frequency == 0))
        for k in SCALARS:
            per[k].append(sc[k])
    for k, v in per.items():
        rec[k] = np.stack(v) if k in ("actions", "batch_inds", "env_inds") else np.asarray(v)
    for nm, keys in GROUPS:
        f32, f64 = T.flat(*[ns[k] for k in keys]), T.flat(*[ns64[k] for k in keys])
        rec[f"final_{nm}_sub"] = f32[::STRIDE].numpy()
        rec[f"final_{nm}_checksum"] = np.float64(f32.double().sum())
        dev[f"final_{nm}"] = float((f32.double() - f64).abs().max())
    la32 = float(ns["log_alpha"].item()) if args.autotune else float(np.log(args.alpha))
    la64 = float(ns64["log_alpha"].item()) if args.autotune else float(np.log(args.alpha))
    rec["final_log_alpha"] = np.float64(la32)
    dev["final_log_alpha"] = abs(la32 - la64)
    rec["stride"] = np.int64(STRIDE)
    rec["config"] = np.frombuffer(json.dumps({"script": SCRIPT, "args": over, "steps": STEPS, "horizon": HORIZON, "n_actions": N_ACTIONS}).encode(),
                                  np.uint8)
    assert truncs >= 1 and ns["rb"].full, "the horizon must cross a truncation and the ring must wrap"
    print(f"{name}: truncations {truncs}, dones in batches {dones_in_batch}, trained steps {int((rec['batch_inds'][:, 0] >= 0).sum())}, "
          f"target updates {int(rec['target_update'].sum())}, deviations {dev}")
    return rec, dev


def mint_network_init():
    """Seeded constructions of both classes, in the script's order: checksums, a few probed elements and the state-dict keys."""
    classes = load_classes(Categorical)
    out = {}
    for n_actions, seed in ((6, 1), (18, 7)):
        torch.manual_seed(seed)
        envs = E.AtariReplayVecEnv(1, seed=seed, n_actions=n_actions, horizon=HORIZON)
        for key, cls in (("actor", "Actor"), ("qf1", "SoftQNetwork"), ("qf2", "SoftQNetwork")):
            net = classes[cls](envs)
            f = T.flat(net)
            pre = f"n{n_actions}_seed{seed}/{key}"
            out[pre + "/bits_checksum"] = np.int64(f.view(torch.int32).to(torch.int64).sum())     # of the f32 bit patterns: exact in any order
            out[pre + "/abs_checksum"] = np.float64(f.double().abs().sum())
            out[pre + "/probes"] = f[list(PROBES)].numpy()
            out[pre + "/count"] = np.int64(f.numel())
            out[pre + "/keys"] = np.frombuffer(json.dumps(list(net.state_dict().keys())).encode(), np.uint8)
    out["probe_index"] = np.asarray(PROBES, np.int64)
    return out


def main():
    assert R.available(), "needs the reference checkout"
    torch.set_num_threads(1)
    out, sens = {}, {}
    for name in CASES:
        rec, dev = mint_case(name)
        sens[name] = dev
        for k, v in rec.items():
            out[f"{name}/{k}"] = v
    path = os.path.join(OUT, "sac_atari_iteration.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(OUT, "sac_atari_iteration_ref_sensitivity.json"), "w") as fh:
        json.dump(sens, fh, indent=1, sort_keys=True)
        fh.write("\n")
    with open(os.path.join(OUT, "sac_atari_cli_surface.json"), "w") as fh:
        surf = {SCRIPT[: -len(".py")]: {"defaults": T.reference_args_defaults(SCRIPT), "order": T.reference_args_order(SCRIPT),
                                        "tags": logged_tags()}}
        json.dump(surf, fh, indent=1, sort_keys=True)
        fh.write("\n")
    init = os.path.join(OUT, "sac_atari_network_init.npz")
    np.savez_compressed(init, **mint_network_init())
    for p in (path, init):
        print("wrote", p, os.path.getsize(p), "bytes")


if __name__ == "__main__":
    main()
