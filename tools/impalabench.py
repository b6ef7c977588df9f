"""The IMPALA-CNN trunk of ppo_procgen.py / ppg_procgen.py on one MI355X with both backends (``torch``: the reference's
ConvSequence modules on MIOpen, ``fused``: the trunk kernels of csrc/impala.hip), timed in one process, alternating the two;
JSON lines to stdout and to --out.

    python tools/impalabench.py [--trunk] [--update] [--reps N] [--out FILE]

  --trunk   the trunk forward at B = 64 (one rollout step, no autograd) and forward + backward (all 30 parameter gradients,
            from a fixed upstream gradient) at B = 1,024 (one PPG auxiliary minibatch) and 2,048 (one ppo_procgen minibatch at the
            defaults); CUDA-event time per call, median of --reps after warm-up.  The fused time includes the in-call weight
            repack.  Each record carries the FLOP and the minimum HBM bytes of the pass, computed from shapes.
  --update  one PPOLearner.update() at ppo_procgen's defaults (64 envs x 256 steps, 8 minibatches, 3 epochs) after a rollout of
            random frames; host wall time ending in the metrics' device -> host copy, median of --reps
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cleanrl_amd import envs as E, ops  # noqa: E402
from cleanrl_amd.agents import ProcgenAgent  # noqa: E402
from cleanrl_amd.learner import PPOLearner  # noqa: E402
from cleanrl_amd.learner_smoke import default_args  # noqa: E402

DEV = torch.device("cuda:0")
LAYERS = [(3, 16, 64), (16, 16, 32), (16, 16, 32), (16, 16, 32), (16, 16, 32),
          (16, 32, 32), (32, 32, 16), (32, 32, 16), (32, 32, 16), (32, 32, 16),
          (32, 32, 16), (32, 32, 8), (32, 32, 8), (32, 32, 8), (32, 32, 8)]      # (C_in, C_out, H = W) per conv


def flop(B, backward):
    """2 x multiply-adds of the 15 convolutions (forward; + data gradient except layer 1's, + weight gradient)."""
    f = sum(2 * 9 * ci * co * h * h for ci, co, h in LAYERS)
    if backward:
        f += sum(2 * 9 * ci * co * h * h for ci, co, h in LAYERS[1:]) + f
    return f * B


def hbm_bytes(B, backward):
    """Minimum traffic of the fused path: frames in, every saved activation written once (and read back once by the
    backward, which also writes and reads its gradient planes), the pre-pool planes through the pool."""
    frames = 64 * 64 * 3 * 4
    saved = 4 * (5 * 32 * 32 * 16 + 5 * 16 * 16 * 32 + 4 * 8 * 8 * 32)
    prepool = 4 * (64 * 64 * 16 + 32 * 32 * 32 + 16 * 16 * 32)
    fwd = frames + saved + 2 * prepool
    if not backward:
        return fwd * B
    return (fwd + frames + 2 * saved + 4 * prepool) * B


def _emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def _agent():
    envs = SimpleNamespace(single_observation_space=E.Box(0, 255, (64, 64, 3), np.uint8), single_action_space=E.Discrete(15))
    torch.manual_seed(0)
    return ProcgenAgent(envs).to(DEV), envs


def _events(fn, reps, warm=3):
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
        ts.append(e0.elapsed_time(e1))
    return ts


def bench_trunk(reps, out):
    agent, _ = _agent()
    params = [p for i in range(3) for p in agent.network[i].parameters()]
    for B, backward in ((64, False), (1024, True), (2048, True)):
        x = torch.rand((B, 64, 64, 3), device=DEV)
        dy = torch.randn((B, 8, 8, 32), device=DEV)

        def run_torch():
            if not backward:
                with torch.no_grad():
                    agent.network[:3](x.permute(0, 3, 1, 2))
                return
            y = agent.network[:3](x.permute(0, 3, 1, 2))
            torch.autograd.grad(y, params, dy.permute(0, 3, 1, 2))

        def run_fused():
            if not backward:
                with torch.no_grad():
                    ops.impala_trunk(x, params)
                return
            y = ops.ImpalaTrunk.apply(x, *params)
            torch.autograd.grad(y, params, dy)

        ts = {"torch": [], "fused": []}
        for rnd in range(4):                                   # alternate the backends in rounds
            for name, fn in (("torch", run_torch), ("fused", run_fused)) if rnd % 2 == 0 else (("fused", run_fused), ("torch", run_torch)):
                ts[name] += _events(fn, max(1, reps // 4))
        for name in ("torch", "fused"):
            ms = float(np.median(ts[name]))
            rec = {"bench": "impala_trunk", "pass": "fwd+bwd" if backward else "fwd", "B": B, "backend": name, "ms": round(ms, 4),
                   "min_ms": round(float(np.min(ts[name])), 4), "n": len(ts[name]), "gflop": round(flop(B, backward) / 1e9, 3),
                   "tflops": round(flop(B, backward) / ms / 1e9, 2), "min_hbm_mb": round(hbm_bytes(B, backward) / 1e6, 1)}
            _emit(rec, out)


def bench_update(reps, out):
    res = {}
    for rnd in range(2):
        for backend in ("torch", "fused") if rnd == 0 else ("fused", "torch"):
            agent, envs = _agent()
            agent.impala_backend = backend
            args = default_args(num_steps=256, num_minibatches=8, update_epochs=3, clip_coef=0.2, learning_rate=5e-4)
            L = PPOLearner(agent, args, envs.single_observation_space, envs.single_action_space, 64, DEV, sample_seed=1)
            L.obs.copy_(torch.randint(0, 256, L.obs.shape, dtype=torch.uint8, device=DEV))
            L.actions.copy_(torch.randint(0, 15, L.actions.shape, device=DEV).to(L.actions.dtype))
            L.logprobs.fill_(-2.7)
            L.advantages.normal_()
            L.returns.normal_()
            L.values.normal_()
            L.update(5e-4)
            torch.cuda.synchronize()
            for _ in range(max(1, reps // 2)):
                t0 = time.perf_counter()
                L.update(5e-4)
                torch.cuda.synchronize()
                res.setdefault(backend, []).append((time.perf_counter() - t0) * 1e3)
            del L, agent
            torch.cuda.empty_cache()
    for backend, ts in res.items():
        _emit({"bench": "procgen_update", "backend": backend, "envs": 64, "steps": 256, "minibatches": 8, "epochs": 3,
               "ms": round(float(np.median(ts)), 2), "min_ms": round(float(np.min(ts)), 2), "n": len(ts)}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trunk", action="store_true")
    ap.add_argument("--update", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("impalabench: no GPU (timings are only meaningful on the device)")
    if not (a.trunk or a.update):
        a.trunk = a.update = True
    if a.trunk:
        bench_trunk(a.reps, a.out)
    if a.update:
        bench_update(a.reps, a.out)


if __name__ == "__main__":
    main()
