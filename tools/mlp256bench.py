"""A/B timing of ppo_continuous_action_isaacgym.py's learner on the K8 kernels (MI355PPO_MLP256=fused) against the torch modules, in the
mould of tools/mabench.py: the two backends alternate, every leg is a child process under its own time limit, medians are reported.

    python tools/mlp256bench.py [--rounds 3] [--out profiles/mlp256bench.jsonl]

Legs, at 4,096 x 16 (the script's defaults) and 256 x 16: one rollout step (forward + sampling), the bootstrap value, one minibatch
(forward + loss + backward + optimizer step), one whole ``update()``.  Times are device-synchronised host clocks around ``reps`` calls.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((4096, 16), (256, 16))


def leg(num_envs, num_steps, reps):
    sys.path.insert(0, ROOT)
    import torch

    from cleanrl_amd import envs as E, ppo_continuous_action_isaacgym as script
    from cleanrl_amd.learner import PPOLearner

    dev = torch.device("cuda")
    args = script.Args(num_envs=num_envs, num_steps=num_steps)
    args.batch_size = num_envs * num_steps
    args.minibatch_size = args.batch_size // args.num_minibatches
    torch.manual_seed(1)
    env = E.DeviceLinearContinuousVecEnv(num_envs, dev, seed=1)
    agent = script.Agent(env).to(dev)
    L = PPOLearner(agent, args, env.single_observation_space, env.single_action_space, num_envs, dev, sample_seed=1)
    L.device_randperm = True
    L.observe(0, env.obs(), torch.zeros(num_envs, device=dev))
    for step in range(num_steps):                           # a real rollout: the update's operands
        obs, r, d = env.step(L.act(step))
        L.store_reward(step, r)
        L.observe(step + 1, obs, d)
    L.finish_rollout()
    b = lambda t, s=(): t.reshape((-1,) + tuple(s))      # noqa: E731
    idx = torch.randperm(args.batch_size, device=dev)[:args.minibatch_size]
    scal = torch.zeros(7, device=dev)

    def minibatch():
        L._minibatch_hip(idx, b(L.obs, L.obs_shape), b(L.actions, L.act_shape), b(L.logprobs), b(L.advantages), b(L.returns), b(L.values), 1e-5, scal)

    out = {"backend": "fused" if L.mlp256 is not None else "torch", "num_envs": num_envs, "num_steps": num_steps}
    for name, fn in (("rollout_step", lambda: L.act(0)), ("bootstrap_value", L.finish_rollout), ("minibatch", minibatch), ("update", lambda: L.update(1e-5))):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out[name + "_us"] = (time.perf_counter() - t0) / reps * 1e6
    print("MLP256BENCH " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=120)
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", nargs=2, type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg[0], a.leg[1], a.reps)
    rows = []
    for _ in range(a.rounds):
        for n, t in SIZES:
            for backend in ("torch", "fused"):
                env = dict(os.environ, MI355PPO_MLP256=backend)
                r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--leg", str(n), str(t), "--reps", str(a.reps)],
                                   env=env, capture_output=True, text=True)
                if r.returncode != 0:                        # a leg that failed ends the run: nothing more is started on the device
                    sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                    raise SystemExit(f"leg {backend} {n} x {t} ended with status {r.returncode}")
                rows.append(json.loads(next(l for l in r.stdout.splitlines() if l.startswith("MLP256BENCH "))[12:]))
    summary = []
    for n, t in SIZES:
        for backend in ("torch", "fused"):
            mine = [r for r in rows if (r["backend"], r["num_envs"], r["num_steps"]) == (backend, n, t)]
            summary.append({"backend": backend, "num_envs": n, "num_steps": t, "rounds": len(mine),
                            **{k: round(statistics.median(r[k] for r in mine), 1) for k in mine[0] if k.endswith("_us")}})
    for s in summary:
        print(json.dumps(s))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows + summary:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
