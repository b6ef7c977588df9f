"""Time both RND backends (MI355PPO_RND=torch | fused) of RNDPPOLearner on one GPU, in one process and in alternation (torch, fused,
torch, ...), so that a drift of the machine falls on both sides.

    python tools/rndbench.py [--reps 20] [--sizes 128x128,32x32] [--json out.json]

Legs, per size (envs x steps, 4 minibatches, 4 epochs as the script):

    curiosity_us       one ``curiosity(step)``: statistics -> RND input -> both networks -> intrinsic reward
    finish_rollout_us  ``finish_rollout``: reward filter + running variance + scaling, bootstrap values, two GAE launches
    stats_norm_us      the statistics-plus-normalise part of ``update``: observation moments of the batch, ``obs_rms``, and the RND
                       input of the whole batch (torch: one tensor for the batch; fused: one normalise launch per minibatch)
    minibatch_us       one minibatch: gather, networks, losses, backward, clip + Adam
    update_us          one whole ``update``
    peak_mem_mb        ``torch.cuda.max_memory_allocated`` over the backend's ``update`` (reset before it)

Times are medians over ``--reps`` runs, synchronised, in microseconds.

    python tools/rndbench.py --trunk [--reps 20] [--sizes 128x128,32x32] [--leg-timeout 300] [--breakdown] [--json out.json]

The trunk axis: ``MI355PPO_RND=fused`` on both sides, ``MI355PPO_RND_TRUNK=torch | fused`` in alternation.  Every leg is a child process
under its own time limit; the first leg that fails or runs out of time ends the run.  Legs, per size: ``act_us`` (one ``act(step)``),
``curiosity_us``, ``minibatch_us``, ``update_us`` and, from the update's child, ``peak_mem_mb``.  ``--breakdown`` adds one child that times
every library call of one fused-trunk minibatch (synchronised around each launch: what a call costs alone, not what it costs in the queue).
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

from cleanrl_amd import envs as E  # noqa: E402
from cleanrl_amd.agents import RNDAgent, RNDModel  # noqa: E402
from cleanrl_amd.learner_rnd import RNDPPOLearner  # noqa: E402
from cleanrl_amd.learner_smoke import default_args  # noqa: E402
from cleanrl_amd.rnd_ops import rnd_mean_var  # noqa: E402


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


def _learner(backend, N, T, dev, trunk="torch"):
    os.environ["MI355PPO_RND"] = backend                      # read when the learner is built
    os.environ["MI355PPO_RND_TRUNK"] = trunk
    torch.manual_seed(1)
    np.random.seed(1)
    envs = type("S", (), dict(single_observation_space=E.Box(0, 255, (4, 84, 84), np.uint8), single_action_space=E.Discrete(6)))
    agent, rnd = RNDAgent(envs).to(dev), RNDModel(4, envs.single_action_space.n).to(dev)
    args = default_args(num_steps=T, num_minibatches=4, update_epochs=4, gamma=0.999, int_gamma=0.99, clip_coef=0.1, ent_coef=0.001,
                        update_proportion=0.25, int_coef=1.0, ext_coef=2.0, learning_rate=1e-4)
    L = RNDPPOLearner(agent, rnd, args, envs.single_observation_space, envs.single_action_space, N, dev, sample_seed=1)
    assert L.rnd_fused == (backend == "fused") and L.rnd_trunk_fused == (trunk == "fused")
    rs = np.random.RandomState(2)
    L.obs_rms.update(rs.randint(0, 256, size=(64, 1, 84, 84)).astype(np.float64))
    if L.rnd_fused:
        L.refresh_obs_stats()
    frame = lambda: rs.randint(0, 256, size=(N, 4, 84, 84)).astype(np.uint8)      # noqa: E731
    L.observe(0, frame(), np.zeros(N, np.float32))
    for step in range(T):                                    # fill the storage once (random frames / rewards / dones)
        L.act(step)
        L.store_reward(step, rs.randn(N).astype(np.float32))
        L.observe(step + 1, frame(), (rs.rand(N) < 0.02).astype(np.float32))
        L.curiosity(step)
    L.finish_rollout()
    return L


def _stats_norm(L):
    """The statistics-plus-normalise part of ``update`` alone, on copies of the running statistics."""
    B, M = L.batch_size, L.minibatch_size
    b_obs = L.obs.reshape((-1,) + L.obs_shape)
    keep = (L.obs_rms.mean.copy(), L.obs_rms.var.copy(), L.obs_rms.count)
    if L.rnd_fused:
        mean, var = rnd_mean_var(L.ops.rnd_obs_moments(b_obs, L._rnd_sums), B)
        L.obs_rms.update_from_moments(mean.reshape(1, 1, 84, 84), var.reshape(1, 1, 84, 84), B)
        L.refresh_obs_stats()
        idx = torch.arange(B, device=L.device)
        out = torch.empty((M, 1, 84, 84), device=L.device)
        for start in range(0, B, M):
            L.ops.rnd_normalize(b_obs, L._rnd_mean, L._rnd_sd, idx=idx[start:start + M], out=out)
    else:
        newest = L._newest_frame(b_obs)
        d = newest.double()
        L.obs_rms.update_from_moments(d.mean(0).cpu().numpy(), d.var(0, unbiased=False).cpu().numpy(), d.shape[0])
        del d
        mean = torch.from_numpy(L.obs_rms.mean).to(L.device)
        var = torch.from_numpy(L.obs_rms.var).to(L.device)
        ((newest - mean) / torch.sqrt(var)).clip(-5, 5).float()
    L.obs_rms.mean, L.obs_rms.var, L.obs_rms.count = keep


def _one_minibatch(L):
    """The first minibatch of an ``update`` (rows 0 .. M-1), with what ``update`` prepares before its loop built once and kept."""
    a, M = L.args, L.minibatch_size
    if not hasattr(L, "_bench_mb"):
        b_obs = L.obs.reshape((-1,) + L.obs_shape)
        rnd_next_obs = None
        if not L.rnd_fused:
            mean, var = torch.from_numpy(L.obs_rms.mean).to(L.device), torch.from_numpy(L.obs_rms.var).to(L.device)
            rnd_next_obs = ((L._newest_frame(b_obs) - mean) / torch.sqrt(var)).clip(-5, 5).float()
        L._bench_mb = (torch.arange(M, device=L.device), b_obs, rnd_next_obs, L.actions.reshape(-1), L.logprobs.reshape(-1),
                       L.int_advantages.reshape(-1) * a.int_coef + L.advantages.reshape(-1) * a.ext_coef, L.returns.reshape(-1),
                       L.int_returns.reshape(-1), L.values.reshape(-1))
    L._minibatch_rnd_hip(*L._bench_mb, 1e-4, 0)


def bench(N, T, reps, dev):
    learners = [_learner(b, N, T, dev) for b in ("torch", "fused")]
    rows = [{"N": N, "T": T, "batch": L.batch_size, "backend": "fused" if L.rnd_fused else "torch"} for L in learners]

    def finish(L):
        raw = L.curiosity_rewards.clone()

        def run():
            L.curiosity_rewards.copy_(raw)                   # the method scales in place: start from the same rewards every time
            L.finish_rollout()
        return run

    upd = max(3, reps // 4)
    for key, fns, r in (("curiosity_us", [lambda L=L: L.curiosity(1) for L in learners], reps),
                        ("finish_rollout_us", [finish(L) for L in learners], reps),
                        ("stats_norm_us", [lambda L=L: _stats_norm(L) for L in learners], upd),
                        ("minibatch_us", [lambda L=L: _one_minibatch(L) for L in learners], reps),
                        ("update_us", [lambda L=L: L.update(1e-4) for L in learners], upd)):
        for row, t in zip(rows, _alternate(fns, r)):
            row[key] = t
    for row, L in zip(rows, learners):
        L.__dict__.pop("_bench_mb", None)                     # the torch side's whole-batch RND input must not count as resident
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        L.update(1e-4)
        torch.cuda.synchronize()
        row["peak_mem_mb"] = torch.cuda.max_memory_allocated(dev) / 2**20
        row["peak_over_resident_mb"] = (torch.cuda.max_memory_allocated(dev) - base) / 2**20
    return rows


TRUNK_LEGS = ("act_us", "curiosity_us", "minibatch_us", "update_us")


def _peak(L, dev):
    L.__dict__.pop("_bench_mb", None)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    L.update(1e-4)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(dev) / 2**20


def trunk_child(leg, N, T, reps):
    """One leg of the trunk axis: both learners under ``MI355PPO_RND=fused``, the two trunks timed in alternation."""
    dev = torch.device("cuda")
    sides = [_learner("fused", N, T, dev, trunk) for trunk in ("torch", "fused")]
    base = {"envs": N, "steps": T, "minibatch_rows": sides[0].minibatch_size, "leg": leg}
    if leg == "breakdown":
        for row in _breakdown(sides[1], reps):
            print(json.dumps({**base, "trunk": "fused", **row}), flush=True)
        return
    run = {"act_us": lambda L: L.act(1), "curiosity_us": lambda L: L.curiosity(1), "minibatch_us": _one_minibatch,
           "update_us": lambda L: L.update(1e-4)}[leg]
    r = max(3, reps // 4) if leg == "update_us" else reps
    for L, t in zip(sides, _alternate([lambda L=L: run(L) for L in sides], r)):
        row = {**base, "trunk": "fused" if L.rnd_trunk_fused else "torch", "us": round(t, 1), "reps": r}
        if leg == "update_us":
            row["peak_mem_mb"] = round(_peak(L, dev), 1)
        print(json.dumps(row), flush=True)


def _breakdown(L, reps):
    """Median time of every library call of one minibatch of ``L``, in call order, each launch synchronised on both sides."""
    from cleanrl_amd import ops

    real = ops._launch
    mods = [m for n, m in sorted(sys.modules.items()) if n.startswith("cleanrl_amd") and m is not None and getattr(m, "_launch", None) is real]
    calls = []

    def timed(name, dev, *args):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        real(name, dev, *args)
        torch.cuda.synchronize()
        calls.append((name, (time.perf_counter() - t0) * 1e6))

    _one_minibatch(L)
    torch.cuda.synchronize()
    runs = []
    for m in mods:
        m._launch = timed
    try:
        for _ in range(max(3, reps // 4)):
            calls.clear()
            _one_minibatch(L)
            runs.append(list(calls))
    finally:
        for m in mods:
            m._launch = real
    assert all([n for n, _ in r] == [n for n, _ in runs[0]] for r in runs), "the minibatch's launches changed between runs"
    return [{"call": k, "entry": name, "us": round(statistics.median(r[k][1] for r in runs), 1)} for k, (name, _) in enumerate(runs[0])]


def trunk_main(a):
    rows = []
    for size in a.sizes.split(","):
        N, T = (int(v) for v in size.split("x"))
        for leg in TRUNK_LEGS + (("breakdown",) if a.breakdown else ()):
            cmd = ["timeout", "-k", "10", str(a.leg_timeout), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--trunk-child", leg,
                   str(N), str(T)]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="128x128,32x32", help="envs x steps, comma separated")
    ap.add_argument("--json", default=None)
    ap.add_argument("--trunk", action="store_true", help="the MI355PPO_RND_TRUNK axis under MI355PPO_RND=fused, one child process per leg")
    ap.add_argument("--breakdown", action="store_true", help="with --trunk: the time per library call of one fused-trunk minibatch")
    ap.add_argument("--leg-timeout", type=int, default=300, help="with --trunk: seconds one leg (one child process) may take")
    ap.add_argument("--trunk-child", nargs=3, metavar=("LEG", "N", "T"), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.trunk_child:
        trunk_child(a.trunk_child[0], int(a.trunk_child[1]), int(a.trunk_child[2]), a.reps)
        return 0
    if a.trunk:
        return trunk_main(a)
    dev = torch.device("cuda")
    rows = []
    for size in a.sizes.split(","):
        N, T = (int(v) for v in size.split("x"))
        for r in bench(N, T, a.reps, dev):
            rows.append(r)
            print(json.dumps({k: (round(v, 1) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)


if __name__ == "__main__":
    sys.exit(main())
