"""Time both auxiliary-phase backends (MI355PPO_PPG=torch | fused) of PPGLearner on one GPU.  Each leg runs in a child process of its
own under a time limit, with both backends in that one process and in alternation (torch, fused, torch, ...), so that a drift of the
machine falls on both sides; the first leg that fails or runs out of time ends the run.

    python tools/ppgbench.py [--reps 20] [--sizes 256x4,64x4] [--phase-rollouts 64] [--leg-timeout 300] [--json out.json]

Legs, per size (steps T x rollouts per minibatch, 64 x 64 x 3 frames, 15 actions):

    old_minibatch_us   the old-policy pass of one minibatch: gather, u8 -> f32, trunk, normalised logits into aux_pi
    aux_minibatch_us   one auxiliary minibatch with its optimiser step: gather, trunk, heads, losses, backward, clip + Adam
                       (the torch side restates the lines of ``PPGLearner.aux_phase`` around one fixed minibatch)
    aux_phase_us       one whole ``aux_phase`` over ``--phase-rollouts`` stored rollouts (old-policy pass + e_auxiliary = 6 epochs)

Times are medians over ``--reps`` runs (the phase: a quarter of them, at least 3), synchronised, in microseconds.
"""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEGS = ("old_minibatch_us", "aux_minibatch_us", "aux_phase_us")


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


def _learner(backend, T, nr, R, dev):
    from cleanrl_amd import envs as E
    from cleanrl_amd.agents import PPGAgent
    from cleanrl_amd.learner_ppg import PPGLearner
    from cleanrl_amd.learner_smoke import default_args

    os.environ["MI355PPO_PPG"] = backend                      # read when the learner is built
    torch.manual_seed(1)
    envs = type("S", (), dict(single_observation_space=E.Box(0, 255, (64, 64, 3), np.uint8), single_action_space=E.Discrete(15)))
    args = default_args(num_steps=T, num_minibatches=8, gamma=0.999, clip_coef=0.2, adv_norm_fullbatch=True, e_policy=1, e_auxiliary=6,
                        beta_clone=1.0, num_aux_rollouts=nr, n_aux_grad_accum=1, aux_batch_rollouts=R, n_iteration=1, learning_rate=5e-4)
    L = PPGLearner(PPGAgent(envs).to(dev), args, envs.single_observation_space, envs.single_action_space, R, dev, sample_seed=1)
    assert L.hip and L.ppg_fused == (backend == "fused")
    gen = torch.Generator(device=dev).manual_seed(2)          # a filled auxiliary buffer, as after n_iteration policy updates
    L.aux_obs.copy_(torch.randint(0, 256, L.aux_obs.shape, generator=gen, device=dev, dtype=torch.uint8))
    L.aux_returns.copy_(torch.randn(L.aux_returns.shape, generator=gen, device=dev))
    L._aux_update = 1
    return L


def _old_minibatch(L, cols_np, aux_pi):
    from cleanrl_amd.learner_ppg import unflatten01

    if L.ppg_fused:
        cols = torch.from_numpy(cols_np).to(L.device)
        with torch.no_grad():
            L.ops.ppg_old_logits_(L._aux_hidden(cols).contiguous(), L.agent.actor.weight.data, L.agent.actor.bias.data, cols, aux_pi)
        return
    with torch.no_grad():                                     # learner_ppg.py, the body of aux_phase's first loop
        logits = L._aux_forward(L._aux_rows(cols_np))[0]
        logits = logits - logits.logsumexp(dim=-1, keepdim=True)
        aux_pi[:, torch.from_numpy(cols_np).to(aux_pi.device)] = unflatten01(logits, (L.T, len(cols_np))).to(aux_pi.device)


def _aux_minibatch(L, cols_np, aux_pi):
    import torch.distributions as td
    from torch.distributions.categorical import Categorical

    from cleanrl_amd.learner_ppg import flatten01

    a, ag = L.args, L.agent
    if L.ppg_fused:
        cols = torch.from_numpy(cols_np).to(L.device)
        heads = [p for m in (ag.actor, ag.critic, ag.aux_critic) for p in (m.weight, m.bias)]
        hidden = L._aux_hidden(cols)
        _, dh = L.ops.ppg_aux_fwd_bwd(hidden.detach(), [p.data for p in heads], aux_pi, L.aux_returns, cols, float(a.beta_clone), 1.0,
                                      [p.grad for p in heads], False)
        hidden.backward(dh)
        L._aux_step_fused(5e-4)
        return
    cols = torch.from_numpy(cols_np).to(L.aux_obs.device)     # learner_ppg.py, the body of aux_phase's minibatch loop
    m_aux_returns = flatten01(L.aux_returns.index_select(1, cols)).to(torch.float32).to(L.device)
    logits, new_values, new_aux_values = L._aux_forward(L._aux_rows(cols))
    new_values, new_aux_values = new_values.view(-1), new_aux_values.view(-1)
    old_pi = Categorical(logits=flatten01(aux_pi.index_select(1, cols)).to(L.device))
    kl_loss = td.kl_divergence(old_pi, Categorical(logits=logits)).mean()
    real_value_loss = 0.5 * ((new_values - m_aux_returns) ** 2).mean()
    aux_value_loss = 0.5 * ((new_aux_values - m_aux_returns) ** 2).mean()
    ((aux_value_loss + a.beta_clone * kl_loss + real_value_loss) / a.n_aux_grad_accum).backward()
    L._aux_step_hip(5e-4)


def child(leg, T, nr, R, reps):
    dev = torch.device("cuda")
    learners = [_learner(b, T, nr, R, dev) for b in ("torch", "fused")]
    cols_np = np.random.RandomState(3).permutation(R)[:nr].astype(np.int64)
    if leg == "aux_phase_us":
        def run(L):
            L._aux_update = 1
            np.random.seed(4)
            with contextlib.redirect_stdout(io.StringIO()):
                L.aux_phase()
        fns, reps = [lambda L=L: run(L) for L in learners], max(3, reps // 4)
    else:
        body = _old_minibatch if leg == "old_minibatch_us" else _aux_minibatch
        pis = [torch.zeros((T, R, 15), device=dev) for _ in learners]
        for L, pi in zip(learners, pis):                       # a normalised old policy for the minibatch leg
            _old_minibatch(L, cols_np, pi)
        fns = [lambda L=L, pi=pi: body(L, cols_np, pi) for L, pi in zip(learners, pis)]
    for L, t in zip(learners, _alternate(fns, reps)):
        print(json.dumps({"T": T, "rollouts_per_minibatch": nr, "rows": T * nr, "stored_rollouts": R, "leg": leg,
                          "backend": "fused" if L.ppg_fused else "torch", "us": round(t, 1), "reps": reps}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", default="256x4,64x4", help="steps x rollouts per minibatch, comma separated")
    ap.add_argument("--phase-rollouts", type=int, default=64, help="stored rollouts R of the whole-phase leg")
    ap.add_argument("--leg-timeout", type=int, default=300, help="seconds one leg (one child process) may take")
    ap.add_argument("--json", default=None)
    ap.add_argument("--child", nargs=4, metavar=("LEG", "T", "NR", "R"), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], int(a.child[1]), int(a.child[2]), int(a.child[3]), a.reps)
        return 0
    rows = []
    for size in a.sizes.split(","):
        T, nr = (int(v) for v in size.split("x"))
        for leg in LEGS:
            R = a.phase_rollouts if leg == "aux_phase_us" else 2 * nr
            cmd = ["timeout", "-k", "10", str(a.leg_timeout), sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--child", leg, str(T),
                   str(nr), str(R)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            if r.returncode != 0:                              # a failed or hung leg ends the run: nothing more is started on the GPU
                sys.stderr.write(r.stderr[-4000:])
                print(json.dumps({"leg": leg, "T": T, "failed": r.returncode}), flush=True)
                return 1
            rows += [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
