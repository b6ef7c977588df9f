"""ppo_atari_lstm.py's recurrence on one MI355X with both LSTM backends (``torch``: the reference's per-step nn.LSTM loop,
``fused``: the sequence scans of csrc/lstm.hip); JSON lines to stdout and to --out.

    python tools/lstmbench.py [--seq] [--update] [--trunk [--lstm fused|torch]] [--out FILE]

  --seq     forward + backward of the T = 128 sequence (input projection, recurrence, every LSTM gradient) at
            B in {1, 2, 8, 64, 256, 1024}; CUDA-event time per call, median of --reps after warm-up
  --update  one LSTMPPOLearner.update() (host wall, ends in the metrics' device -> host copy) after a rollout on random frames,
            at the script's defaults (8 envs x 128 steps, 4 minibatches, 4 epochs) and at 64 envs; median of --reps
  --trunk   MI355PPO_LSTM_TRUNK=torch against =fused (only with --trunk): one rollout step, finish_rollout, one minibatch forward + backward
            and one update() at the script's defaults (8 envs x 128 steps: 256-row minibatches) and at 128 envs (4,096 rows).  Every leg is
            a child process under its own time limit (--leg-timeout) that builds BOTH learners and times them in alternation (torch, fused,
            torch, ...), each call ending in a device synchronise (host clock); medians of --reps rounds, fewer once a leg has used
            --leg-seconds.  --lstm picks the recurrence behind both trunks.  A leg that fails ends the run: nothing is started after it.
"""
import argparse
import json
import os
import subprocess
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cleanrl_amd import envs as E, ops  # noqa: E402
from cleanrl_amd.agents import AtariLSTMAgent  # noqa: E402
from cleanrl_amd.learner_lstm import LSTMPPOLearner  # noqa: E402
from cleanrl_amd.learner_smoke import default_args  # noqa: E402

DEV = torch.device("cuda:0")
H = 128


def _emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def _event_time(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def bench_seq(reps, out, T=128):
    torch.manual_seed(0)
    lstm = nn.LSTM(512, H).to(DEV)
    for B in (1, 2, 8, 64, 256, 1024):
        x = torch.relu(torch.randn(T, B, 512, device=DEV))
        done = (torch.rand(T, B, device=DEV) < 0.01).float()
        h0, c0 = torch.zeros(1, B, H, device=DEV), torch.zeros(1, B, H, device=DEV)
        dh = torch.randn(T, B, H, device=DEV)

        def loop():                                          # cleanrl/ppo_atari_lstm.py:140-158 + its autograd
            state, hs = (h0, c0), []
            for t in range(T):
                keep = (1.0 - done[t]).view(1, -1, 1)
                h, state = lstm(x[t:t + 1], (keep * state[0], keep * state[1]))
                hs.append(h)
            torch.autograd.backward(torch.cat(hs), dh)

        def fused():
            gx = nn.functional.linear(x, lstm.weight_ih_l0, lstm.bias_ih_l0 + lstm.bias_hh_l0)
            h, _, _ = ops.LSTMSeq.apply(gx, lstm.weight_hh_l0, h0[0], c0[0], done)
            torch.autograd.backward(h, dh)

        gx = nn.functional.linear(x, lstm.weight_ih_l0, lstm.bias_ih_l0 + lstm.bias_hh_l0).detach().contiguous()
        w = lstm.weight_hh_l0.detach().contiguous()
        rec = ops.lstm_seq_forward(gx, w, h0[0], c0[0], done, record=True)[3]
        kf = _event_time(lambda: ops.lstm_seq_forward(gx, w, h0[0], c0[0], done, record=True), reps)
        kb = _event_time(lambda: ops.lstm_seq_backward(dh, None, None, rec, w, done), reps)
        for name, fn in (("torch", loop), ("fused", fused)):
            med, best = _event_time(fn, reps)
            lstm.zero_grad(set_to_none=True)
            _emit(dict(bench="lstm_seq_fwd_bwd", backend=name, T=T, B=B, us_median=round(med, 1), us_min=round(best, 1)), out)
        _emit(dict(bench="lstm_seq_kernels", T=T, B=B, fwd_us_median=round(kf[0], 1), bwd_us_median=round(kb[0], 1)), out)


def bench_update(reps, out):
    envs = SimpleNamespace(single_observation_space=E.Box(0, 255, (1, 84, 84), np.uint8), single_action_space=E.Discrete(4))
    for N in (8, 64):
        for backend in ("torch", "fused"):
            torch.manual_seed(0)
            np.random.seed(0)
            agent = AtariLSTMAgent(envs).to(DEV)
            agent.lstm_backend = backend
            args = default_args(num_steps=128, num_minibatches=4, update_epochs=4)           # ppo_atari_lstm.py's defaults
            L = LSTMPPOLearner(agent, args, envs.single_observation_space, envs.single_action_space, N, DEV, sample_seed=1)
            rs = np.random.RandomState(0)
            L.observe(0, rs.randint(0, 256, (N, 1, 84, 84)).astype(np.uint8), np.zeros(N, np.float32))
            t0 = time.perf_counter()
            for step in range(L.T):
                L.act(step)
                L.store_reward(step, rs.randint(-1, 2, N).astype(np.float32))
                L.observe(step + 1, rs.randint(0, 256, (N, 1, 84, 84)).astype(np.uint8), (rs.random_sample(N) < 0.01).astype(np.float32))
            L.finish_rollout()
            torch.cuda.synchronize()
            rollout_ms = (time.perf_counter() - t0) * 1e3
            ts = []
            for i in range(reps + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m = L.update(2.5e-4)
                ts.append((time.perf_counter() - t0) * 1e3)
            ts = ts[1:]                                            # the first call pays allocations / MIOpen lookups
            _emit(dict(bench="lstm_update", backend=backend, num_envs=N, num_steps=128, minibatches=m["num_updates"],
                       update_ms_median=round(float(np.median(ts)), 2), update_ms_min=round(float(np.min(ts)), 2),
                       rollout_ms=round(rollout_ms, 1), loss=m["loss"]), out)


TRUNK_LEGS = ("rollout_step", "finish_rollout", "minibatch", "update")
TRUNK_ENVS = (8, 128)


def _trunk_learner(N, trunk, lstm):
    """LSTMPPOLearner at the script's defaults on ``N`` envs with the given trunk, its storage filled by one rollout on random frames."""
    envs = SimpleNamespace(single_observation_space=E.Box(0, 255, (1, 84, 84), np.uint8), single_action_space=E.Discrete(4))
    torch.manual_seed(0)
    agent = AtariLSTMAgent(envs).to(DEV)
    agent.lstm_backend = lstm
    args = default_args(num_steps=128, num_minibatches=4, update_epochs=4)
    os.environ["MI355PPO_LSTM_TRUNK"] = trunk                     # read by the learner's constructor
    L = LSTMPPOLearner(agent, args, envs.single_observation_space, envs.single_action_space, N, DEV, sample_seed=1)
    assert L.trunk == trunk
    rs = np.random.RandomState(0)
    L.observe(0, rs.randint(0, 256, (N, 1, 84, 84)).astype(np.uint8), np.zeros(N, np.float32))
    for step in range(L.T):
        L.act(step)
        L.store_reward(step, rs.randint(-1, 2, N).astype(np.float32))
        L.observe(step + 1, rs.randint(0, 256, (N, 1, 84, 84)).astype(np.uint8), (rs.random_sample(N) < 0.01).astype(np.float32))
    L.finish_rollout()
    return L


def _trunk_minibatch(L):
    """One minibatch's forward + backward as update() runs it (all T steps of the first N / 4 envs, time-major); the gradient buffer is
    zeroed inside the call on both sides (no optimizer step follows here)."""
    T, N = L.T, L.N
    env_idx = torch.arange(N // int(L.args.num_minibatches), device=DEV)
    idx = torch.arange(T * N, device=DEV).reshape(T, N).index_select(1, env_idx).reshape(-1)
    b_obs = L.obs.reshape((-1,) + L.obs_shape)
    flat = [t.reshape(-1) for t in (L.logprobs, L.advantages, L.returns, L.values, L.dones)]
    b_actions = L.actions.reshape((-1,) + L.act_shape)

    def minibatch():
        L._mb_state = (L.initial_lstm_state[0].index_select(1, env_idx), L.initial_lstm_state[1].index_select(1, env_idx))
        L._mb_dones = flat[4].index_select(0, idx)
        L.flat.grads.zero_()
        L.forward_backward_hip(idx, b_obs, b_actions, flat[0], flat[1], flat[2], flat[3], L._scalars[0])

    return minibatch, idx.numel()


def trunk_leg(leg, N, lstm, reps, leg_seconds, out):
    """One leg in this process: both learners, alternating."""
    learners = [_trunk_learner(N, trunk, lstm) for trunk in ("torch", "fused")]
    rows = T_rows = learners[0].T * N // int(learners[0].args.num_minibatches)
    if leg == "rollout_step":
        fns, rows = [lambda L=L: L.act(1) for L in learners], N
    elif leg == "finish_rollout":
        fns, rows = [L.finish_rollout for L in learners], N
    elif leg == "minibatch":
        fns = [_trunk_minibatch(L)[0] for L in learners]
    else:
        fns, reps = [lambda L=L: L.update(2.5e-4) for L in learners], max(3, reps // 4)
    t_leg = time.perf_counter()
    for _ in range(2):                                            # warm-up: every shape of the timed window, packs, allocations
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts[i].append((time.perf_counter() - t0) * 1e6)
        if time.perf_counter() - t_leg > leg_seconds:
            break
    for L, t in zip(learners, ts):
        _emit(dict(bench="lstm_trunk", leg=leg, trunk=L.trunk, lstm=lstm, num_envs=N, num_steps=L.T, rows=rows, minibatch_rows=T_rows,
                   us_median=round(float(np.median(t)), 1), us_min=round(float(np.min(t)), 1), reps=len(t)), out)


def bench_trunk(a):
    """Every (envs, leg) as a child process of its own under ``timeout``; the first failure ends the run."""
    for N in TRUNK_ENVS:
        for leg in TRUNK_LEGS:
            cmd = ["timeout", "-k", "10", str(a.leg_timeout), sys.executable, os.path.abspath(__file__), "--trunk-leg", leg, "--num-envs", str(N),
                   "--lstm", a.lstm, "--reps", str(a.reps), "--leg-seconds", str(a.leg_seconds)] + (["--out", a.out] if a.out else [])
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                _emit(dict(bench="lstm_trunk", leg=leg, num_envs=N, lstm=a.lstm, error=f"child exit status {rc}"), a.out)
                return rc
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seq", action="store_true")
    ap.add_argument("--update", action="store_true")
    ap.add_argument("--trunk", action="store_true")
    ap.add_argument("--trunk-leg", choices=TRUNK_LEGS, default=None, help="(the child of --trunk: one leg in this process)")
    ap.add_argument("--num-envs", type=int, default=8)
    ap.add_argument("--lstm", choices=("torch", "fused"), default="fused")
    ap.add_argument("--leg-seconds", type=float, default=30.0)
    ap.add_argument("--leg-timeout", type=int, default=240)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.trunk:                                   # the parent never opens the GPU: its children do, one at a time
        sys.exit(bench_trunk(a))
    assert torch.cuda.is_available(), "lstmbench needs a GPU"
    if a.trunk_leg:
        trunk_leg(a.trunk_leg, a.num_envs, a.lstm, a.reps, a.leg_seconds, a.out)
        return
    if not (a.seq or a.update):
        a.seq = a.update = True
    if a.seq:
        bench_seq(a.reps, a.out)
    if a.update:
        bench_update(max(3, a.reps // 3), a.out)


if __name__ == "__main__":
    main()
