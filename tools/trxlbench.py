"""ppo_trxl.py's memory attention on one MI355X with both TrXL backends (``torch``: the reference's whole-episode gather and
attention ops, ``fused``: the episodic-memory attention of csrc/trxl_attn.hip); JSON lines to stdout and to --out.

    python tools/trxlbench.py [--minibatch] [--update] [--kernel] [--out FILE]

  --minibatch  forward + backward of one minibatch through TrXLAgent at the script's defaults (2,048 samples, 3 layers,
               D = 384, H = 4, window 119) over an episode pool of T_ep = 512; CUDA-event time, median of --reps
  --update     one TrXLLearner.update() (3 epochs x 8 minibatches of 32 envs x 512 steps, T_ep = 1024: a Memory Gym env
               without a step limit) on a synthetic rollout; host wall time ending in the metrics' device -> host copies,
               median of --reps
  --kernel     the attention kernels alone (forward, backward) at the update size (B = 2,048) and the rollout size (B = 32)
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cleanrl_amd import envs as E, ops  # noqa: E402
from cleanrl_amd.agents import MemoryWindow, TrXLAgent  # noqa: E402
from cleanrl_amd.learner_trxl import TrXLLearner  # noqa: E402
from cleanrl_amd.ppo_trxl import Args  # noqa: E402

DEV = torch.device("cuda:0")


def _emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        with open(out, "a") as f:
            f.write(line + "\n")


def _event_time(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def _agent(backend, T_ep, seed=1):
    args = Args()
    torch.manual_seed(seed)
    agent = TrXLAgent(args, E.Box(0, 255, (84, 84, 3), np.uint8), (4,), T_ep)
    agent.trxl_backend = backend
    return args, agent.to(DEV)


def _windows(args, T_ep, E_, B, g):
    L = args.trxl_memory_length
    ep = torch.randint(0, E_, (B,), generator=g)
    step = torch.randint(0, T_ep, (B,), generator=g)
    tri = torch.tril(torch.ones((L, L)), diagonal=-1)
    rep = torch.arange(L).repeat(L - 1, 1)
    idx = torch.cat((rep, torch.stack([torch.arange(i, i + L) for i in range(T_ep - L + 1)])))
    return ep.to(DEV), idx[step].to(DEV), tri[step.clamp(max=L - 1)].bool().to(DEV)


def bench_minibatch(reps, out, T_ep=512, E_=64, B=2048):
    g = torch.Generator().manual_seed(0)
    for backend in ("torch", "fused"):
        args, agent = _agent(backend, T_ep)
        pool = torch.randn((E_, T_ep, args.trxl_num_layers, args.trxl_dim), generator=g).to(DEV)
        ep, idx, mask = _windows(args, T_ep, E_, B, g)
        obs = torch.randint(0, 256, (B, 84, 84, 3), generator=g).float().to(DEV)
        act = torch.randint(0, 4, (B, 1), generator=g).to(DEV)

        def step():
            if backend == "fused":
                win = MemoryWindow(pool, ep, idx)
            else:                                                # the reference's minibatch: whole episodes, then the windows
                from cleanrl_amd.agents import batched_index_select
                win = batched_index_select(pool[ep], 1, idx)
            _, lp, ent, v, _ = agent.get_action_and_value(obs, win, mask, idx, act)
            (lp.sum() + ent.sum() + v.sum()).backward()

        med, mn = _event_time(step, reps)
        _emit({"bench": "trxl_minibatch_fwd_bwd", "backend": backend, "B": B, "T_ep": T_ep, "episodes": E_, "ms_median": med,
               "ms_min": mn}, out)
        del agent, pool
        torch.cuda.empty_cache()


def bench_update(reps, out, T_ep=1024):
    g = torch.Generator().manual_seed(1)
    for backend in ("torch", "fused"):
        args, agent = _agent(backend, T_ep)
        N, T = args.num_envs, args.num_steps
        L = TrXLLearner(agent, args, E.Box(0, 255, (84, 84, 3), np.uint8), (4,), N, T_ep, DEV)
        L.start_iteration()
        # a synthetic rollout: every env runs one episode of random length through the iteration
        steps = torch.randint(0, T_ep - T, (N,), generator=g)
        for t in range(T):
            L.env_current_episode_step.copy_((steps + t).to(DEV))
            L.stored_memory_masks[t] = L.memory_mask[torch.clip(L.env_current_episode_step, 0, L.L - 1)]
            L.stored_memory_indices[t] = L.memory_indices[L.env_current_episode_step]
        L.next_memory.copy_(torch.randn(L.next_memory.shape, generator=g).to(DEV))
        L.obs.copy_(torch.randint(0, 256, L.obs.shape, generator=g).float().to(DEV))
        L.actions.copy_(torch.randint(0, 4, L.actions.shape, generator=g).to(DEV))
        L.log_probs.fill_(-np.log(4.0))
        L.values.copy_(torch.randn(L.values.shape, generator=g).to(DEV))
        L.advantages = torch.randn(L.values.shape, generator=g).to(DEV)
        L.returns = L.advantages + L.values
        ts = []
        for _ in range(reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            L.update()
            ts.append(time.perf_counter() - t0)
        _emit({"bench": "trxl_update", "backend": backend, "N": N, "T": T, "T_ep": T_ep, "s_median": float(np.median(ts[1:])),
               "s_min": float(np.min(ts[1:]))}, out)
        del agent, L
        torch.cuda.empty_cache()


def bench_kernel(reps, out, T_ep=512, E_=64):
    g = torch.Generator().manual_seed(2)
    args = Args()
    D, H = args.trxl_dim, args.trxl_num_heads
    pool = torch.randn((E_, T_ep, args.trxl_num_layers, D), generator=g).to(DEV)
    pe = torch.randn((T_ep, D), generator=g).to(DEV)
    gamma, beta = torch.ones(D, device=DEV), torch.zeros(D, device=DEV)
    for B in (2048, 32):
        ep, idx, mask = _windows(args, T_ep, E_, B, g)
        mask = mask.to(torch.uint8)
        q = torch.randn((B, H, D // H), generator=g).to(DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        u, st = ops.trxl_attn_forward(pool, 1, ep, idx, idx, mask, pe, gamma, beta, q)
        fwd = _event_time(lambda: ops.trxl_attn_forward(pool, 1, ep, idx, idx, mask, pe, gamma, beta, q, err=err), reps)
        bwd = _event_time(lambda: ops.trxl_attn_backward(pool, 1, ep, idx, idx, mask, pe, gamma, beta, q, u, st, u, err=err), reps)
        _emit({"bench": "trxl_attn_kernel", "B": B, "L": args.trxl_memory_length, "D": D, "H": H, "fwd_ms_median": fwd[0],
               "bwd_ms_median": bwd[0], "fwd_ms_min": fwd[1], "bwd_ms_min": bwd[1]}, out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minibatch", action="store_true")
    ap.add_argument("--update", action="store_true")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    everything = not (a.minibatch or a.update or a.kernel)
    if a.kernel or everything:
        bench_kernel(max(a.reps, 20), a.out)
    if a.minibatch or everything:
        bench_minibatch(a.reps, a.out)
    if a.update or everything:
        bench_update(a.reps, a.out)


if __name__ == "__main__":
    main()
