"""Mint the sac_continuous_action fixtures from the reference's own lines.

    python tools/mint_sac_goldens.py

Build-container tool, modelled on tools/mint_td3_goldens.py (whose block finder, ``Args`` readers and float64 replay buffer it
imports): it needs the reference checkout; nothing on the GPU machine runs it.  It stores no reference text: it ``ast``-compiles
``Actor`` / ``SoftQNetwork`` and ``exec``s the script's setup, step and train blocks, located by their lines, against
``SyntheticReplayVecEnv`` on one CPU thread.

The draws themselves are not stored (271 draws of 32 x 6 floats per case do not compress): the file keeps the generator state in
front of the first step, the draws' offsets per step and one float64 checksum per draw, and tests/sac_replay.py regenerates them in
the run's order.  Every standard normal draw of the run is recovered from the generator state in front of each step (the rollout's ``(N, A)``, then per
training step the target's ``(B, A)`` and per policy iteration the actor's and the re-evaluation's) and checked by comparing the
generator's state after the replayed draws with the run's.  A second copy of the networks and of ``log_alpha`` is held in float64 and
runs the train block in lockstep on the float32 run's batches and draws (its ``Normal.rsample`` pops them): the float32 reference's
maximum deviation from it, per compared quantity, goes to tests/golden/sac_iteration_ref_sensitivity.json.  Writes
tests/golden/sac_iteration.npz and tests/golden/sac_cli_surface.json.
"""
from __future__ import annotations

import ast
import json
import os
import random
import sys

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
SCRIPT = "sac_continuous_action.py"
STEPS, STRIDE, HORIZON = T.STEPS, T.STRIDE, T.HORIZON
BASE = dict(buffer_size=64, batch_size=32, learning_starts=8)
CASES = {
    "sac": dict(BASE, num_envs=1, seed=3),
    "sac_n2": dict(BASE, num_envs=2, seed=4),
    "sac_fixed": dict(BASE, num_envs=1, seed=5, autotune=False),
    "sac_tnf2": dict(BASE, num_envs=1, seed=6, target_network_frequency=2),
}
SCALARS = ("qf1_values", "qf1_loss", "qf2_values", "qf2_loss", "qf_loss", "actor_loss", "alpha_loss", "alpha")
SOURCE = {"qf1_values": "qf1_a_values", "qf2_values": "qf2_a_values"}
NETS = ("actor", "qf1", "qf2")
TARGETS = ("qf1_target", "qf2_target")


class _Normal64(torch.distributions.Normal):
    """``Normal`` whose ``rsample`` pops the float32 run's draw."""

    queue: list = []

    def rsample(self, sample_shape=torch.Size()):
        return self.loc + _Normal64.queue.pop(0) * self.scale


class _Dist:
    Normal = _Normal64


class _TorchShim:
    distributions = _Dist

    def __getattr__(self, k):
        return getattr(torch, k)


def load_classes(torch_mod):
    tree = ast.parse("\n".join(R._read(SCRIPT)))
    body = [n for n in tree.body if (isinstance(n, ast.ClassDef) and n.name in ("Actor", "SoftQNetwork"))
            or (isinstance(n, ast.Assign) and n.targets[0].id in ("LOG_STD_MAX", "LOG_STD_MIN"))]
    ns = {"np": np, "torch": torch_mod, "nn": nn, "F": F}
    exec(compile(ast.Module(body=body, type_ignores=[]), f"<reference:{SCRIPT}>", "exec"), ns)
    ns["ReplayBuffer"] = T.load_reference_classes("td3_continuous_action.py")["ReplayBuffer"]
    return ns


def mint_case(name):
    over = CASES[name]
    args = T.make_args(SCRIPT, over)
    N, B = args.num_envs, args.batch_size
    setup, step, train = T.blocks(SCRIPT)
    shim = _TorchShim()

    def seeded_setup(classes):
        random.seed(args.seed)
        np.random.seed(args.seed)
        torch.manual_seed(args.seed)
        envs = E.SyntheticReplayVecEnv(N, seed=args.seed, horizon=HORIZON)
        ns = T._namespace(args, envs, classes)
        exec(setup, ns)
        return ns

    ns64 = seeded_setup(load_classes(shim))
    for k in NETS + TARGETS:
        ns64[k].double()
    if args.autotune:
        ns64["log_alpha"] = torch.zeros(1, requires_grad=True, dtype=torch.float64)
        ns64["a_optimizer"] = optim.Adam([ns64["log_alpha"]], lr=args.q_lr)
    ns = seeded_setup(load_classes(torch))                       # the float32 run owns the global random streams from here on
    rb64 = T._Rb64(ns["rb"])
    ns64.update(torch=shim, rb=rb64)
    envs = ns["envs"]
    A = envs.single_action_space.shape[0]
    rec = {"init_checksum": np.float64(T.flat(*[ns[k] for k in NETS]).double().sum())}
    per = {k: [] for k in ("actions", "batch_inds", "env_inds", "policy_update", "target_update") + SCALARS}
    noise, offsets = [], [0]
    dev = {k: 0.0 for k in SCALARS}
    ns["obs"], _ = envs.reset(seed=args.seed)
    rec["rng_state"] = torch.get_rng_state().numpy().copy()      # every later draw of the run follows from it (tests/sac_replay.py)
    truncs = 0
    for global_step in range(STEPS):
        ns["global_step"] = ns64["global_step"] = global_step
        np_state, t_state = np.random.get_state(), torch.get_rng_state()
        pos, full = ns["rb"].pos, ns["rb"].full
        exec(step, ns)
        truncs += int(np.asarray(ns["truncations"]).sum())
        per["actions"].append(np.asarray(ns["actions"], np.float32).reshape(N, A))
        trained = global_step > args.learning_starts
        pu = trained and global_step % args.policy_frequency == 0
        bi, ei = np.full(B, -1, np.int64), np.full(B, -1, np.int64)
        sc = {k: np.nan for k in SCALARS}
        g = torch.Generator()
        g.set_state(t_state)
        if global_step >= args.learning_starts:
            torch.randn((N, A), generator=g)                     # the rollout's get_action
        draws = []
        if trained:
            rs = np.random.RandomState()
            rs.set_state(np_state)
            pos, full = (pos + 1) % ns["rb"].buffer_size, full or pos + 1 == ns["rb"].buffer_size      # rb.add ran before rb.sample
            bi = rs.randint(0, ns["rb"].buffer_size if full else pos, size=B)
            ei = rs.randint(0, high=N, size=(B,))
            count = 1 + (args.policy_frequency * (2 if args.autotune else 1) if pu else 0)
            draws = [torch.randn((B, A), generator=g) for _ in range(count)]
        assert torch.equal(g.get_state(), torch.get_rng_state()), "noise recovery is off"
        if trained:
            rb64.inds, _Normal64.queue = (bi, ei), [d.double() for d in draws]
            exec(train, ns64)
            assert not _Normal64.queue
            for k in SCALARS:
                src = SOURCE.get(k, k)
                if src in ns:
                    v32, v64 = ns[src], ns64[src]
                    v32, v64 = (float(v.mean().item()) if torch.is_tensor(v) else float(v) for v in (v32, v64))
                    sc[k] = v32
                    dev[k] = max(dev[k], abs(v32 - v64))
        noise += [d.numpy() for d in draws]
        offsets.append(len(noise))
        per["batch_inds"].append(bi), per["env_inds"].append(ei)
        per["policy_update"].append(np.int64(pu))
        per["target_update"].append(np.int64(trained and global_step % args.target_network_frequency == 0))
        for k in SCALARS:
            per[k].append(sc[k])
    data = ns["data"]
    assert torch.equal(data.observations, torch.tensor(ns["rb"].observations[bi, ei, :])), "index recovery is off"
    for k, v in per.items():
        rec[k] = np.stack(v) if k in ("actions", "batch_inds", "env_inds") else np.asarray(v)
    rec["noise_checksums"] = np.asarray([d.astype(np.float64).sum() for d in noise], np.float64)
    rec["noise_offsets"] = np.asarray(offsets, np.int64)
    groups = (("actor", ("actor",)), ("critics", ("qf1", "qf2")), ("targets", TARGETS))
    for nm, keys in groups:
        f32, f64 = T.flat(*[ns[k] for k in keys]), T.flat(*[ns64[k] for k in keys])
        rec[f"final_{nm}_sub"] = f32[::STRIDE].numpy()
        rec[f"final_{nm}_checksum"] = np.float64(f32.double().sum())
        dev[f"final_{nm}"] = float((f32.double() - f64).abs().max())
    la32 = float(ns["log_alpha"].item()) if args.autotune else float(np.log(args.alpha))
    la64 = float(ns64["log_alpha"].item()) if args.autotune else float(np.log(args.alpha))
    rec["final_log_alpha"] = np.float64(la32)
    dev["final_log_alpha"] = abs(la32 - la64)
    rec["stride"] = np.int64(STRIDE)
    rec["config"] = np.frombuffer(json.dumps({"script": SCRIPT, "args": over, "steps": STEPS, "horizon": HORIZON}).encode(), np.uint8)
    assert truncs >= 1 and ns["rb"].full, "the horizon must cross a truncation and the ring must wrap"
    print(f"{name}: truncations {truncs}, trained steps {int((rec['batch_inds'][:, 0] >= 0).sum())}, draws {len(noise)}, deviations {dev}")
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
    path = os.path.join(OUT, "sac_iteration.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(OUT, "sac_iteration_ref_sensitivity.json"), "w") as fh:
        json.dump(sens, fh, indent=1, sort_keys=True)
        fh.write("\n")
    with open(os.path.join(OUT, "sac_cli_surface.json"), "w") as fh:
        surf = {SCRIPT[: -len(".py")]: {"defaults": T.reference_args_defaults(SCRIPT), "order": T.reference_args_order(SCRIPT)}}
        json.dump(surf, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
