"""ppo_atari_lstm.py's recurrence on one MI355X with both LSTM backends (``torch``: the reference's per-step nn.LSTM loop,
``fused``: the sequence scans of csrc/lstm.hip); JSON lines to stdout and to --out.

    python tools/lstmbench.py [--seq] [--update] [--out FILE]

  --seq     forward + backward of the T = 128 sequence (input projection, recurrence, every LSTM gradient) at
            B in {1, 2, 8, 64, 256, 1024}; CUDA-event time per call, median of --reps after warm-up
  --update  one LSTMPPOLearner.update() (host wall, ends in the metrics' device -> host copy) after a rollout on random frames,
            at the script's defaults (8 envs x 128 steps, 4 minibatches, 4 epochs) and at 64 envs; median of --reps
"""
import argparse
import json
import os
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seq", action="store_true")
    ap.add_argument("--update", action="store_true")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not (a.seq or a.update):
        a.seq = a.update = True
    assert torch.cuda.is_available(), "lstmbench needs a GPU"
    if a.seq:
        bench_seq(a.reps, a.out)
    if a.update:
        bench_update(max(3, a.reps // 3), a.out)


if __name__ == "__main__":
    main()
