"""Time both PQN backends (MI355PPO_PQN=torch | fused) on one GPU: one rollout step, the Q(lambda) scan, one minibatch and one
``update()`` of PQNLearner / LSTMPQNLearner, at each script's defaults and at a larger env count.

    python tools/pqnbench.py [--reps 20] [--scripts pqn,atari,lstm] [--json out.json]

The recurrent script (``lstm``) builds both learners in one process and times them in alternation (torch, fused, torch, ...), so
that a drift of the machine falls on both sides.

A rollout step here is the learner's ``act`` plus the action's copy to the host (the env is left out); ``minibatch_us`` is one
``update()`` (update_epochs x num_minibatches of forward + TD loss + backward + clip + RAdam, plus the shuffles) divided by its
minibatch count.  Times are medians over ``--reps`` runs, synchronised, in microseconds.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cleanrl_amd import envs as E  # noqa: E402
from cleanrl_amd.agents import AtariLSTMQNetwork, AtariQNetwork, QNetwork  # noqa: E402
from cleanrl_amd.learner_pqn import PQNLearner  # noqa: E402
from cleanrl_amd.learner_pqn_lstm import LSTMPQNLearner  # noqa: E402


def _time(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(ts)


def bench(script, N, backend, reps, dev):
    if script == "pqn":
        from cleanrl_amd.pqn import Args

        env = E.CartPoleVecEnv(N, seed=1)
        net, mlp = QNetwork(env).to(dev), True
        obs = env.reset(seed=1)[0]
    else:
        from cleanrl_amd.pqn_atari_envpool import Args

        env = E.SyntheticAtariVecEnv(N, seed=1, api="gym")
        net, mlp = AtariQNetwork(env).to(dev), False
        obs = env.reset()
    args = Args(num_envs=N)
    args.batch_size = N * args.num_steps
    args.minibatch_size = args.batch_size // args.num_minibatches
    args.num_iterations = args.total_timesteps // args.batch_size
    L = PQNLearner(net, args, env.single_observation_space.shape, env.single_action_space.n, N, dev, mlp=mlp, backend=backend)
    L.reset(obs)
    L.start_iteration(1)
    for step in range(args.num_steps):                       # fill the storage once (random rewards / dones)
        L.act(step)
        L.observe(step, obs, np.random.randn(N), np.random.rand(N) < 0.02)
    out = {"script": script, "N": N, "backend": backend}
    out["rollout_step_us"] = _time(lambda: L.act(0).cpu(), reps)
    out["qlambda_us"] = _time(L.finish_rollout, reps)
    out["update_us"] = _time(L.update, max(3, reps // 4))
    out["minibatch_us"] = out["update_us"] / (args.update_epochs * args.num_minibatches)
    out["batch"] = args.batch_size
    return out


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


def bench_lstm(N, reps, dev):
    """pqn_atari_envpool_lstm.py at N envs: both backends in this process, alternating -> [torch row, fused row]."""
    from cleanrl_amd.pqn_atari_envpool_lstm import Args

    args = Args(num_envs=N)
    args.batch_size = N * args.num_steps
    args.minibatch_size = args.batch_size // args.num_minibatches
    args.num_iterations = args.total_timesteps // args.batch_size
    learners = []
    for backend in ("torch", "fused"):
        torch.manual_seed(1)
        np.random.seed(1)
        env = E.SyntheticAtariVecEnv(N, seed=1, api="gym", frames=1)
        obs = env.reset()
        L = LSTMPQNLearner(AtariLSTMQNetwork(env).to(dev), args, env.single_observation_space.shape, env.single_action_space.n, N, dev,
                           backend=backend)
        L.reset(obs)
        L.start_iteration(1)
        for step in range(args.num_steps):                   # fill the storage once (random rewards / dones)
            L.act(step)
            L.observe(step, obs, np.random.randn(N), np.random.rand(N) < 0.02)
        learners.append(L)
    rows = [{"script": "lstm", "N": N, "backend": L.backend} for L in learners]
    for key, fns, r in (("rollout_step_us", [lambda L=L: L.act(1).cpu() for L in learners], reps),
                        ("qlambda_us", [L.finish_rollout for L in learners], reps),
                        ("update_us", [L.update for L in learners], max(3, reps // 4))):
        for row, t in zip(rows, _alternate(fns, r)):
            row[key] = t
    for row in rows:
        row["minibatch_us"] = row["update_us"] / (args.update_epochs * args.num_minibatches)
        row["batch"] = args.batch_size
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--scripts", default="pqn,atari,lstm")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda")
    rows = []
    show = lambda r: print(json.dumps({k: (round(v, 1) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)  # noqa: E731
    scripts = a.scripts.split(",")
    for script, Ns in (("pqn", (4, 1024)), ("atari", (8, 128))):
        if script not in scripts:
            continue
        for N in Ns:
            for backend in ("torch", "fused"):
                torch.manual_seed(1)
                np.random.seed(1)
                r = bench(script, N, backend, a.reps, dev)
                rows.append(r)
                show(r)
    if "lstm" in scripts:
        for N in (8, 64):
            for r in bench_lstm(N, a.reps, dev):
                rows.append(r)
                show(r)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    main()
