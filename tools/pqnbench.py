"""Time both PQN backends (MI355PPO_PQN=torch | fused) on one GPU: one rollout step, the Q(lambda) scan, one minibatch and one
``update()`` of PQNLearner / LSTMPQNLearner, at each script's defaults and at a larger env count.

    python tools/pqnbench.py [--reps 20] [--scripts pqn,atari,lstm,trunk,lstm_trunk] [--json out.json] [--leg-seconds 60] [--breakdown]

The recurrent script (``lstm``) builds both learners in one process and times them in alternation (torch, fused, torch, ...), so
that a drift of the machine falls on both sides.  ``trunk`` is the Atari script's trunk axis (MI355PPO_PQN=fused with
MI355PPO_PQN_TRUNK=torch | fused): both learners in one process, alternating, every leg (rollout step, Q(lambda), update) under its own
time limit of ``--leg-seconds`` -- a leg that runs out stops repeating and reports the medians of what it has; the rows also carry the
bytes of ``learner.obs``.  ``--breakdown`` adds, per env count, the synchronised median time of every library call of one fused-trunk
minibatch (forward + backward), in call order.  ``lstm_trunk`` is the same axis for the recurrent script (LSTMPQNLearner on one-frame
observations; the rows add ``minibatch_us`` of one minibatch timed on its own); it asserts that the fused trunk's ``learner.obs`` is exactly
a quarter of the f32 storage's bytes.

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


def _alternate_limited(fns, reps, limit_s):
    """``_alternate`` that stops repeating once the leg has used ``limit_s`` seconds (always one warm-up and one timed round)."""
    t_leg = time.perf_counter()
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
        if time.perf_counter() - t_leg > limit_s:
            break
    return [statistics.median(t) for t in ts], len(ts[0])


def _atari_learner(N, trunk, dev):
    from cleanrl_amd.pqn_atari_envpool import Args

    args = Args(num_envs=N)
    args.batch_size = N * args.num_steps
    args.minibatch_size = args.batch_size // args.num_minibatches
    args.num_iterations = args.total_timesteps // args.batch_size
    torch.manual_seed(1)
    np.random.seed(1)
    env = E.SyntheticAtariVecEnv(N, seed=1, api="gym")
    obs = env.reset()
    L = PQNLearner(AtariQNetwork(env).to(dev), args, env.single_observation_space.shape, env.single_action_space.n, N, dev, mlp=False,
                   backend="fused", trunk=trunk, obs_space=env.single_observation_space)
    L.reset(obs)
    L.start_iteration(1)
    for step in range(args.num_steps):                       # fill the storage once (random rewards / dones)
        L.act(step)
        L.observe(step, obs, np.random.randn(N), np.random.rand(N) < 0.02)
    return L, args


def bench_atari_trunks(N, reps, dev, leg_seconds):
    """pqn_atari_envpool.py at N envs on MI355PPO_PQN=fused: the torch trunk and the fused trunk in this process, alternating ->
    [torch-trunk row, fused-trunk row]."""
    learners = [_atari_learner(N, trunk, dev) for trunk in ("torch", "fused")]
    args = learners[0][1]
    learners = [L for L, _ in learners]
    rows = [{"script": "atari", "N": N, "backend": "fused", "trunk": L.trunk, "obs_bytes": L.obs.numel() * L.obs.element_size()} for L in learners]
    for key, fns, r in (("rollout_step_us", [lambda L=L: L.act(1).cpu() for L in learners], reps),
                        ("qlambda_us", [L.finish_rollout for L in learners], reps),
                        ("update_us", [L.update for L in learners], max(3, reps // 4))):
        meds, n = _alternate_limited(fns, r, leg_seconds)
        for row, t in zip(rows, meds):
            row[key] = t
            row[key[:-3] + "_reps"] = n
    for row in rows:
        row["minibatch_us"] = row["update_us"] / (args.update_epochs * args.num_minibatches)
        row["batch"], row["minibatch_rows"] = args.batch_size, args.minibatch_size
    return rows, learners[1], args


def trunk_breakdown(L, args, reps, minibatch=None):
    """The library calls of ONE fused-trunk minibatch (forward, TD loss, backward) of learner ``L``, each synchronised and timed: ->
    [(call, median us)] in call order.  The calls are timed in place of the node's own bindings, which are restored afterwards.
    ``minibatch``: the minibatch to run (default: PQNLearner's)."""
    from cleanrl_amd import cnn, ln_cnn

    spots = [(ln_cnn, n) for n in ("conv1q_pre_fwd", "conv1q1_pre_fwd", "layernorm_relu_fwd", "conv_pre_packed", "fc_pre", "layernorm_relu_bwd",
                                   "conv1p1_wgrad")] + \
            [(cnn, n) for n in ("fc_wgrad", "fc_dgrad_mask_packed", "conv_wgrad", "conv_dgrad_packed")]
    log = []

    def timed(name, fn):
        def call(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **k)
            torch.cuda.synchronize()
            log.append((name, (time.perf_counter() - t0) * 1e6))
            return out
        return call

    mb = torch.randperm(args.batch_size)[:args.minibatch_size].to(L.device)

    def own_minibatch():
        q = L._q(L.obs.view(-1, 84, 84, 4), mb)
        dq, _ = L.g.pqn_td_loss(q.detach().contiguous(), mb, L.actions.reshape(-1), L.returns.reshape(-1))
        q.backward(dq)
        L.flat.grads.zero_()

    minibatch = own_minibatch if minibatch is None else minibatch
    minibatch()
    saved = [(m, n, getattr(m, n)) for m, n in spots]
    try:
        for m, n, fn in saved:
            setattr(m, n, timed(n, fn))
        runs = []
        for _ in range(reps):
            log.clear()
            minibatch()
            runs.append(list(log))
    finally:
        for m, n, fn in saved:
            setattr(m, n, fn)
    return [(runs[0][i][0], statistics.median(r[i][1] for r in runs)) for i in range(len(runs[0]))]


def _lstm_learner(N, trunk, dev):
    from cleanrl_amd.pqn_atari_envpool_lstm import Args

    args = Args(num_envs=N)
    args.batch_size = N * args.num_steps
    args.minibatch_size = args.batch_size // args.num_minibatches
    args.num_iterations = args.total_timesteps // args.batch_size
    torch.manual_seed(1)
    np.random.seed(1)
    env = E.SyntheticAtariVecEnv(N, seed=1, api="gym", frames=1)
    obs = env.reset()
    L = LSTMPQNLearner(AtariLSTMQNetwork(env).to(dev), args, env.single_observation_space.shape, env.single_action_space.n, N, dev,
                       backend="fused", trunk=trunk, obs_space=env.single_observation_space)
    L.reset(obs)
    L.start_iteration(1)
    for step in range(args.num_steps):                       # fill the storage once (random rewards / dones)
        L.act(step)
        L.observe(step, obs, np.random.randn(N), np.random.rand(N) < 0.02)
    L.finish_rollout()
    return L, args


def _lstm_minibatch(L, args):
    """One minibatch of ``LSTMPQNLearner.update`` (the first ``N / num_minibatches`` envs, time-major rows): trunk + gx, the scan, the TD
    kernel, the backward; the gradients are zeroed instead of stepped."""
    envs = np.arange(L.N // int(args.num_minibatches))
    mb = torch.from_numpy(np.arange(L.T * L.N).reshape(L.T, L.N)[:, envs].ravel().copy()).to(L.device)
    env = torch.from_numpy(envs).to(L.device)
    net, b_dones = L.net, L.dones.reshape(-1)
    b_obs = L.obs.view(-1, 84, 84) if L.fused_trunk else L.obs.reshape((-1,) + L.obs_shape)

    def minibatch():
        state = (L.initial_lstm_state[0][:, env], L.initial_lstm_state[1][:, env])
        if L.fused_trunk:
            h, _ = net.states_from_gates(L._gates(b_obs, mb), state, b_dones[mb])
        else:
            h, _ = net.states_fused(b_obs[mb], state, b_dones[mb])
        dh, _ = L.g.pqn_lstm_td_fwd_bwd(h.detach(), mb, L.actions.reshape(-1), L.returns.reshape(-1), net.q_func.weight.detach(),
                                        net.q_func.bias.detach(), net.q_func.weight.grad, net.q_func.bias.grad)
        h.backward(dh)
        L.flat.grads.zero_()

    return minibatch


def bench_lstm_trunks(N, reps, dev, leg_seconds):
    """pqn_atari_envpool_lstm.py at N envs on MI355PPO_PQN=fused: the torch trunk and the fused trunk in this process, alternating ->
    ([torch-trunk row, fused-trunk row], the fused learner, args)."""
    learners = [_lstm_learner(N, trunk, dev) for trunk in ("torch", "fused")]
    args = learners[0][1]
    learners = [L for L, _ in learners]
    rows = [{"script": "lstm", "N": N, "backend": "fused", "trunk": L.trunk, "obs_bytes": L.obs.numel() * L.obs.element_size()} for L in learners]
    assert learners[1].obs.dtype == torch.uint8 and 4 * rows[1]["obs_bytes"] == rows[0]["obs_bytes"], rows      # a quarter of the f32 storage
    for key, fns, r in (("rollout_step_us", [lambda L=L: L.act(1).cpu() for L in learners], reps),
                        ("qlambda_us", [L.finish_rollout for L in learners], reps),
                        ("minibatch_us", [_lstm_minibatch(L, args) for L in learners], reps),
                        ("update_us", [L.update for L in learners], max(3, reps // 4))):
        meds, n = _alternate_limited(fns, r, leg_seconds)
        for row, t in zip(rows, meds):
            row[key] = t
            row[key[:-3] + "_reps"] = n
    for row in rows:
        row["batch"], row["minibatch_rows"] = args.batch_size, args.minibatch_size
    return rows, learners[1], args


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
    ap.add_argument("--leg-seconds", type=float, default=60.0, help="time limit of each leg of the trunk axis")
    ap.add_argument("--breakdown", action="store_true", help="trunk axis: also time every library call of one fused-trunk minibatch")
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
    if "trunk" in scripts:
        for N in (8, 128):
            trunk_rows, fused_learner, targs = bench_atari_trunks(N, a.reps, dev, a.leg_seconds)
            for r in trunk_rows:
                rows.append(r)
                show(r)
            if a.breakdown:
                r = {"script": "atari", "N": N, "trunk": "fused", "minibatch_rows": targs.minibatch_size,
                     "calls_us": [[n, round(t, 1)] for n, t in trunk_breakdown(fused_learner, targs, max(3, a.reps // 2))]}
                rows.append(r)
                show(r)
            del trunk_rows, fused_learner
            torch.cuda.empty_cache()
    if "lstm_trunk" in scripts:
        for N in (8, 128):
            trunk_rows, fused_learner, targs = bench_lstm_trunks(N, a.reps, dev, a.leg_seconds)
            for r in trunk_rows:
                rows.append(r)
                show(r)
            if a.breakdown:
                calls = trunk_breakdown(fused_learner, targs, max(3, a.reps // 2), _lstm_minibatch(fused_learner, targs))
                r = {"script": "lstm", "N": N, "trunk": "fused", "minibatch_rows": targs.minibatch_size, "calls_us": [[n, round(t, 1)] for n, t in calls]}
                rows.append(r)
                show(r)
            del trunk_rows, fused_learner
            torch.cuda.empty_cache()
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
