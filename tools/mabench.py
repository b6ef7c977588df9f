"""Time both backends (MI355PPO_MA_ATARI=torch | fused) of the PPO learner behind ppo_pettingzoo_ma_atari.py on one GPU.  Each leg runs
in a child process of its own under a time limit, with both backends in that one process and in alternation (torch, fused, torch, ...),
so that a drift of the machine falls on both sides; the first leg that fails or runs out of time ends the run.

    python tools/mabench.py [--reps 20] [--sizes 16x128,256x128] [--leg-timeout 300] [--json out.json]

Legs, per size (envs N x steps T, (84, 84, 6) observations, 6 actions, the script's 4 minibatches and 4 epochs):

    rollout_step_us    one rollout step on device frames: the store of the N incoming observations and the policy step on them
    minibatch_us       one minibatch: gather, forward, fused loss, backward, clip + Adam (eager launches on both sides)
    update_us          one whole ``update()``: 16 minibatches and the diagnostics -- as ``runner.train`` runs it: eager launches on the
                       default backend, captured graphs on the fused one (the graph policy of ppo_atari.py)

Times are medians over ``--reps`` runs (the update: a quarter of them, at least 3), synchronised, in microseconds.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEGS = ("rollout_step_us", "minibatch_us", "update_us")


def _alternate(fns, reps):
    """Medians (us) of several sides timed in alternation: one run of each per repetition, each synchronised."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[i].append((time.perf_counter() - t0) * 1e6)
    return [statistics.median(t) for t in ts]


def _learner(backend, N, T, dev, graphs):
    from cleanrl_amd import envs as E
    from cleanrl_amd.agents import MAAtariAgent
    from cleanrl_amd.learner import PPOLearner
    from cleanrl_amd.learner_smoke import default_args

    os.environ["MI355PPO_MA_ATARI"] = backend                 # read when the learner is built
    torch.manual_seed(1)
    envs = type("S", (), dict(single_observation_space=E.Box(0, 255, (84, 84, 6), np.uint8), single_action_space=E.Discrete(6)))
    args = default_args(num_steps=T, num_minibatches=4, update_epochs=4, clip_coef=0.1)
    L = PPOLearner(MAAtariAgent(envs).to(dev), args, envs.single_observation_space, envs.single_action_space, N, dev, sample_seed=1)
    assert L.hip and L.ma_fused == (backend == "fused")
    # a filled rollout: every slot stored through the learner's own store, behaviour arrays as a rollout leaves them
    env = E.SyntheticMAAtariVecEnv(N, seed=2)
    frames = [torch.from_numpy(env.reset()).to(dev)] + [torch.from_numpy(env.step(None)[0]).to(dev) for _ in range(3)]
    zeros = torch.zeros(N, device=dev)
    for step in range(T + 1):
        L.observe(step, frames[step % 4], zeros)
    gen = torch.Generator(device=dev).manual_seed(3)
    L.actions.copy_(torch.randint(0, 6, L.actions.shape, generator=gen, device=dev).float())
    L.logprobs.fill_(float(-np.log(6.0)))
    L.rewards.copy_(torch.randn(L.rewards.shape, generator=gen, device=dev).clamp_(-1, 1))
    L.values.copy_(0.1 * torch.randn(L.values.shape, generator=gen, device=dev))
    L.finish_rollout()
    if graphs and L.fused_cnn:
        L.capture_update()
    return L, frames


def child(leg, N, T, reps):
    dev = torch.device("cuda")
    sides = [_learner(b, N, T, dev, leg == "update_us") for b in ("torch", "fused")]
    zeros = torch.zeros(N, device=dev)
    if leg == "rollout_step_us":
        def run(L, frames):
            L.observe(1, frames[1], zeros)
            L.act(1)
    elif leg == "minibatch_us":
        idx = torch.from_numpy(np.random.RandomState(4).permutation(N * T)[:N * T // 4].astype(np.int64)).to(dev)

        def run(L, frames):
            sc = torch.zeros(7, device=dev)
            L._minibatch_hip(idx, L.obs.reshape((-1,) + L.obs_shape), L.actions.reshape(-1), L.logprobs.reshape(-1), L.advantages.reshape(-1),
                             L.returns.reshape(-1), L.values.reshape(-1), 0.0, sc)
    else:
        reps = max(3, reps // 4)

        def run(L, frames):
            np.random.seed(5)
            L.update(0.0)
    fns = [lambda L=L, fr=fr: run(L, fr) for L, fr in sides]
    for (L, _), t in zip(sides, _alternate(fns, reps)):
        print(json.dumps({"envs": N, "steps": T, "rows": N * T, "leg": leg, "backend": "fused" if L.ma_fused else "torch",
                          "graphs": L._update_graphs is not None, "us": round(t, 1), "reps": reps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="16x128,256x128", help="envs x steps, comma separated")
    ap.add_argument("--leg-timeout", type=int, default=300, help="seconds one leg (one child process) may take")
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", nargs=3, metavar=("LEG", "N", "T"), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], int(a.child[1]), int(a.child[2]), a.reps)
        return 0
    rows = []
    for size in a.sizes.split(","):
        N, T = (int(v) for v in size.split("x"))
        for leg in LEGS:
            cmd = ["timeout", "-k", "10", str(a.leg_timeout), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--child", leg, str(N),
                   str(T)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            if r.returncode != 0:                              # a failed or hung leg ends the run: nothing more is started on the GPU
                sys.stderr.write(r.stderr[-4000:])
                print(json.dumps({"leg": leg, "envs": N, "failed": r.returncode}), flush=True)
                return 1
            rows += [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
