"""ddpg_continuous_action.py / td3_continuous_action.py / sac_continuous_action.py with both ``MI355PPO_OFFPOLICY`` backends, in one
process, alternating.

    python tools/offpolicybench.py [--reps 20] [--scripts td3 ddpg sac dqn dqn_atari rainbow rainbow_buffer sac_atari qdagger]

Times, at each script's defaults (batch 256) on a HalfCheetah-shaped (obs 17 / act 6) and a Humanoid-shaped (376 / 17) task:
one rollout step including the action's copy to the host, one critic-only training step and one step with the delayed policy
update.  The comparison is the ``torch`` backend on the same box in the same process; medians of ``--reps`` after a warm-up.
Prints one JSON line per (script, shape).  ``--scripts dqn`` times dqn.py and c51.py (batch 128) at a CartPole-shaped (obs 4 / 2
actions) and a LunarLander-shaped (8 / 4) task: one greedy rollout step, one DQN update and one C51 update (101 atoms).
``--scripts rainbow`` times rainbow_atari.py (batch 32, 51 atoms) for a 4-action and an 18-action game: one rollout step, one update
and the three noise compositions.  ``--scripts rainbow_buffer`` times rainbow_atari.py's prioritized replay at batch 32 (cleanrl_amd/rainbow_replay.py): the host buffer
by the reference's rules (NumPy tree walk, batch upload, ``loss_per_sample`` read back) against the device buffer, per add, per
sample and per priority update; and the four NoisyLinear layers' ``mu + sigma * eps`` by torch against the one-launch compose, for a
4-action and an 18-action game.  ``--scripts sac_atari`` times sac_atari.py at its batch of 64 for a 4-action and an 18-action game: one rollout
step (the policy's sample) and one update (critics, actor, temperature).  ``--scripts qdagger`` times qdagger_dqn_atari_impalacnn.py at batch 32
for a 4-action and an 18-action game: one greedy step of the student, one offline update (``distill_coeff`` 1) and one online update
(``distill_coeff`` 0.37); the ``fused`` side runs the IMPALA trunk kernels too (``impala_backend`` fused).  Every family but
``rainbow_buffer`` also has a ``store`` leg: 64 back-to-back ``store``s with one synchronisation behind them, in microseconds per store
(the other legs synchronise around every call, so a wait inside ``store`` for an earlier copy would not show in them).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cleanrl_amd import envs as E  # noqa: E402
from cleanrl_amd.agents import ActionValueNetwork, Actor, SoftActor  # noqa: E402
from cleanrl_amd.learner_offpolicy import OffPolicyLearner  # noqa: E402
from cleanrl_amd.learner_sac import SACLearner  # noqa: E402

SHAPES = {"halfcheetah": (17, 6), "humanoid": (376, 17)}
DQN_SHAPES = {"cartpole": (4, 2), "lunarlander": (8, 4)}


def make_dqn(c51, O, n, backend, dev, fill=4096):
    from cleanrl_amd.agents import C51Network, DQNNetwork
    from cleanrl_amd.learner_dqn import DQNLearner

    torch.manual_seed(1)
    np.random.seed(1)
    rng = np.random.RandomState(1)
    env = SimpleNamespace(single_observation_space=SimpleNamespace(shape=(O,)), single_action_space=E.SamplingDiscrete(n), num_envs=1)
    mk = (lambda: C51Network(env).to(dev)) if c51 else (lambda: DQNNetwork(env).to(dev))
    q, t = mk(), mk()
    t.load_state_dict(q.state_dict())
    args = SimpleNamespace(buffer_size=fill * 2, batch_size=128, learning_rate=2.5e-4, gamma=0.99, tau=1.0, n_atoms=101, v_min=-100, v_max=100)
    L = DQNLearner(q, t, args, env, dev, c51=c51, backend=backend)
    obs = rng.standard_normal((1, O)).astype(np.float32)
    for i in range(fill):
        nxt = rng.standard_normal((1, O)).astype(np.float32)
        L.store(obs, nxt, np.array([env.single_action_space.sample()]), np.ones(1), np.array([i % 20 == 19]))
        obs = nxt
    return L, obs


def bench_dqn(a, dev):
    for shape, (O, n) in DQN_SHAPES.items():
        learners = {(alg, b): make_dqn(alg == "c51", O, n, b, dev) for alg in ("dqn", "c51") for b in ("torch", "fused")}
        legs = {"rollout_step": ("dqn", lambda L, obs: L.act(obs, 1, 0.0)), "dqn_update": ("dqn", lambda L, obs: L.train_step()),
                "c51_update": ("c51", lambda L, obs: L.train_step()), "store": ("dqn", store_leg(*learners[("dqn", "torch")]))}
        times = {leg: {b: [] for b in ("torch", "fused")} for leg in legs}
        for rep in range(a.warmup + a.reps):
            for leg, (alg, fn) in legs.items():
                for b in ("torch", "fused"):                             # alternating: both backends see the same box state
                    L, obs = learners[(alg, b)]
                    us = timed(lambda: fn(L, obs), dev)
                    if rep >= a.warmup:
                        times[leg][b].append(us)
        row = {"script": "dqn", "shape": shape, "obs_dim": O, "n_actions": n, "n_atoms": 101, "batch": 128, "device": str(dev), "reps": a.reps}
        for leg in legs:
            for b in ("torch", "fused"):
                row[f"{leg}_{b}_us"] = round(statistics.median(times[leg][b]), 1)
            row[f"{leg}_speedup"] = round(row[f"{leg}_torch_us"] / row[f"{leg}_fused_us"], 2)
        emit(row)


ATARI_SHAPES = {"4-action": 4, "18-action": 18}


def make_dqn_atari(c51, n, backend, dev, fill=256):
    from cleanrl_amd.agents import AtariC51Network, AtariDQNNetwork
    from cleanrl_amd.learner_dqn_atari import AtariDQNLearner

    torch.manual_seed(1)
    np.random.seed(1)
    envs = E.AtariReplayVecEnv(1, seed=1, n_actions=n)
    mk = (lambda: AtariC51Network(envs).to(dev)) if c51 else (lambda: AtariDQNNetwork(envs).to(dev))
    q, t = mk(), mk()
    t.load_state_dict(q.state_dict())
    args = SimpleNamespace(buffer_size=fill * 2, batch_size=32, learning_rate=1e-4, gamma=0.99, tau=1.0, n_atoms=51, v_min=-10, v_max=10)
    return fill_ring(AtariDQNLearner(q, t, args, envs, dev, c51=c51, backend=backend), envs, fill)


def bench_dqn_atari(a, dev):
    """dqn_atari.py / c51_atari.py at batch 32: one greedy rollout step, one DQN update, one C51 update (51 atoms)."""
    for shape, n in ATARI_SHAPES.items():
        learners = {(alg, b): make_dqn_atari(alg == "c51", n, b, dev) for alg in ("dqn", "c51") for b in ("torch", "fused")}
        legs = {"rollout_step": ("dqn", lambda L, obs: L.act(obs, 1, 0.0)), "dqn_update": ("dqn", lambda L, obs: L.train_step()),
                "c51_update": ("c51", lambda L, obs: L.train_step()), "store": ("dqn", store_leg(*learners[("dqn", "torch")]))}
        times = {leg: {b: [] for b in ("torch", "fused")} for leg in legs}
        for rep in range(a.warmup + a.reps):
            for leg, (alg, fn) in legs.items():
                for b in ("torch", "fused"):                             # alternating: both backends see the same box state
                    L, obs = learners[(alg, b)]
                    us = timed(lambda: fn(L, obs), dev)
                    if rep >= a.warmup:
                        times[leg][b].append(us)
        row = {"script": "dqn_atari", "shape": shape, "n_actions": n, "n_atoms": 51, "batch": 32, "device": str(dev), "reps": a.reps}
        for leg in legs:
            for b in ("torch", "fused"):
                row[f"{leg}_{b}_us"] = round(statistics.median(times[leg][b]), 1)
            row[f"{leg}_speedup"] = round(row[f"{leg}_torch_us"] / row[f"{leg}_fused_us"], 2)
        emit(row)


def make_rainbow(n, backend, dev, fill=256):
    from cleanrl_amd.agents import NoisyDuelingDistributionalNetwork
    from cleanrl_amd.learner_rainbow import RainbowLearner

    torch.manual_seed(1)
    np.random.seed(1)
    envs = E.AtariReplayVecEnv(1, seed=1, n_actions=n)
    q, t = (NoisyDuelingDistributionalNetwork(envs, 51, -10, 10).to(dev) for _ in range(2))
    t.load_state_dict(q.state_dict())
    args = SimpleNamespace(buffer_size=fill * 2, batch_size=32, learning_rate=6.25e-5, gamma=0.99, tau=1.0, n_step=3, n_atoms=51, v_min=-10,
                           v_max=10, prioritized_replay_alpha=0.5, prioritized_replay_beta=0.4, prioritized_replay_eps=1e-6)
    L = RainbowLearner(q, t, args, envs, dev, backend=backend)
    obs, _ = envs.reset(seed=1)
    for _ in range(fill):
        act = np.array([envs.single_action_space.sample()])
        nxt, r, term, trunc, _ = envs.step(act)
        L.store(obs, act, r, nxt, term)
        obs = nxt
    return L, obs


def bench_rainbow(a, dev):
    """rainbow_atari.py at batch 32: one rollout step, one update, and the three noise compositions (after ``reset_noise``: both
    networks; after Adam: online; after ``sync_target``: target).  The ``torch`` side of a compose leg is what its forward passes
    pay instead: ``mu + sigma * eps`` of the same layers by torch's ops."""
    for shape, n in ATARI_SHAPES.items():
        learners = {b: make_rainbow(n, b, dev) for b in ("torch", "fused")}

        def composes(L, online, target):
            if L.fused:
                return L.compose(online, target)
            with torch.no_grad():
                nets = [net for net, on in ((L.q_network, online), (L.target_network, target)) if on]
                return [t for net in nets for l in net.noisy_layers()
                        for t in (l.weight_mu + l.weight_sigma * l.weight_epsilon, l.bias_mu + l.bias_sigma * l.bias_epsilon)]

        legs = {"rollout_step": lambda L, obs: L.act(obs), "update": lambda L, obs: L.train_step(),
                "compose_both": lambda L, obs: composes(L, True, True), "compose_online": lambda L, obs: composes(L, True, False),
                "compose_target": lambda L, obs: composes(L, False, True), "store": store_leg(*learners["torch"], rainbow=True)}
        times = {leg: {b: [] for b in learners} for leg in legs}
        for rep in range(a.warmup + a.reps):
            for leg, fn in legs.items():
                for b, (L, obs) in learners.items():                     # alternating: both backends see the same box state
                    us = timed(lambda: fn(L, obs), dev)
                    if rep >= a.warmup:
                        times[leg][b].append(us)
        row = {"script": "rainbow", "shape": shape, "n_actions": n, "n_atoms": 51, "batch": 32, "device": str(dev), "reps": a.reps}
        for leg in legs:
            for b in learners:
                row[f"{leg}_{b}_us"] = round(statistics.median(times[leg][b]), 1)
            row[f"{leg}_speedup"] = round(row[f"{leg}_torch_us"] / row[f"{leg}_fused_us"], 2)
        emit(row)


def bench_rainbow_buffer(a, dev, slots=4096, B=32):
    from cleanrl_amd import ops
    from cleanrl_amd.agents import NoisyDuelingDistributionalNetwork
    from cleanrl_amd.rainbow_replay import DevicePrioritizedReplay, HostPrioritizedReplay

    g = ops.twins(dev)
    for shape, n in ATARI_SHAPES.items():
        torch.manual_seed(1)
        np.random.seed(1)
        envs = E.AtariReplayVecEnv(1, seed=1, n_actions=n)
        bufs = {"torch": HostPrioritizedReplay(slots, (4, 84, 84), 3, 0.99, 0.5, 0.4, 1e-6), "fused": DevicePrioritizedReplay(slots, dev, 3, 0.99, 0.5)}
        obs, _ = envs.reset(seed=1)
        steps = []
        for _ in range(slots // 4):
            act = np.array([envs.single_action_space.sample()])
            nxt, r, term, trunc, _ = envs.step(act)
            steps.append((obs, act, r, nxt, term))
            for rb in bufs.values():
                rb.add(*steps[-1])
            obs = nxt
        net = NoisyDuelingDistributionalNetwork(envs, 51, -10, 10).to(dev)
        layers = net.noisy_layers()
        params = torch.cat([p.detach().reshape(-1) for l in layers for p in (l.weight_mu, l.weight_sigma, l.bias_mu, l.bias_sigma)])
        eps = torch.cat([b.reshape(-1) for l in layers for b in (l.weight_epsilon, l.bias_epsilon)])
        eff = torch.zeros_like(eps)
        loss = torch.rand(B, device=dev)
        last = {}

        def host_sample(rb):
            b = rb.sample(B)
            last["torch"] = b["indices"]
            return [torch.from_numpy(b[k]).to(dev) for k in ("observations", "next_observations", "actions", "rewards", "dones", "weights")]

        def dev_sample(rb):
            last["fused"] = rb.sample(B)["indices"]

        k = [0]

        def add(rb):
            k[0] += 1
            rb.add(*steps[k[0] % len(steps)])

        def torch_compose():
            with torch.no_grad():
                return [t for l in layers for t in (l.weight_mu + l.weight_sigma * l.weight_epsilon, l.bias_mu + l.bias_sigma * l.bias_epsilon)]

        legs = {"add": {"torch": lambda: add(bufs["torch"]), "fused": lambda: add(bufs["fused"])},
                "sample": {"torch": lambda: host_sample(bufs["torch"]), "fused": lambda: dev_sample(bufs["fused"])},
                "priority_update": {"torch": lambda: bufs["torch"].update_priorities(last["torch"], loss.cpu().numpy()),
                                    "fused": lambda: bufs["fused"].update_priorities(last["fused"], loss)},
                "compose": {"torch": torch_compose, "fused": lambda: g.rainbow_noisy_compose(params, eps, eff, n, 51)}}
        times = {leg: {b: [] for b in ("torch", "fused")} for leg in legs}
        for rep in range(a.warmup + a.reps):
            for leg, fns in legs.items():
                for b in ("torch", "fused"):                             # alternating: both see the same box state
                    us = timed(fns[b], dev)
                    if rep >= a.warmup:
                        times[leg][b].append(us)
        row = {"script": "rainbow_buffer", "shape": shape, "n_actions": n, "n_atoms": 51, "batch": B, "slots": slots, "device": str(dev), "reps": a.reps}
        for leg in legs:
            for b in ("torch", "fused"):
                row[f"{leg}_{b}_us"] = round(statistics.median(times[leg][b]), 1)
            row[f"{leg}_speedup"] = round(row[f"{leg}_torch_us"] / row[f"{leg}_fused_us"], 2)
        emit(row)


def make_sac_atari(n, backend, dev, fill=256):
    from cleanrl_amd.agents import AtariSACActor, AtariSoftQNetwork
    from cleanrl_amd.learner_sac_atari import SACAtariLearner

    torch.manual_seed(1)
    np.random.seed(1)
    envs = E.AtariReplayVecEnv(1, seed=1, n_actions=n)
    actor = AtariSACActor(envs).to(dev)
    qs = [AtariSoftQNetwork(envs).to(dev) for _ in range(4)]
    qs[2].load_state_dict(qs[0].state_dict()), qs[3].load_state_dict(qs[1].state_dict())
    args = SimpleNamespace(buffer_size=fill * 2, batch_size=64, q_lr=3e-4, policy_lr=3e-4, gamma=0.99, tau=1.0, learning_starts=0, alpha=0.2,
                           autotune=True, target_entropy_scale=0.89)
    return fill_ring(SACAtariLearner(actor, *qs, args, envs, dev, backend=backend), envs, fill)


def bench_sac_atari(a, dev):
    """sac_atari.py at batch 64: one rollout step (``get_action``'s sample, with its copy to the host) and one update."""
    for shape, n in ATARI_SHAPES.items():
        learners = {b: make_sac_atari(n, b, dev) for b in ("torch", "fused")}
        legs = {"rollout_step": lambda L, obs: L.act(obs, 1), "update": lambda L, obs: L.train_step(), "store": store_leg(*learners["torch"])}
        times = {leg: {b: [] for b in learners} for leg in legs}
        for rep in range(a.warmup + a.reps):
            for leg, fn in legs.items():
                for b, (L, obs) in learners.items():                     # alternating: both backends see the same box state
                    us = timed(lambda: fn(L, obs), dev)
                    if rep >= a.warmup:
                        times[leg][b].append(us)
        row = {"script": "sac_atari", "shape": shape, "n_actions": n, "batch": 64, "device": str(dev), "reps": a.reps}
        for leg in legs:
            for b in learners:
                row[f"{leg}_{b}_us"] = round(statistics.median(times[leg][b]), 1)
            row[f"{leg}_speedup"] = round(row[f"{leg}_torch_us"] / row[f"{leg}_fused_us"], 2)
        emit(row)


def make_qdagger(n, backend, dev, fill=256):
    from cleanrl_amd.agents import AtariDQNNetwork, AtariImpalaQNetwork
    from cleanrl_amd.learner_qdagger import QDaggerLearner

    torch.manual_seed(1)
    np.random.seed(1)
    envs = E.AtariReplayVecEnv(1, seed=1, n_actions=n)
    q, t = AtariImpalaQNetwork(envs).to(dev), AtariImpalaQNetwork(envs).to(dev)
    q.impala_backend = t.impala_backend = backend
    t.load_state_dict(q.state_dict())
    args = SimpleNamespace(buffer_size=fill * 2, batch_size=32, learning_rate=1e-4, gamma=0.99, tau=1.0, temperature=1.0)
    return fill_ring(QDaggerLearner(q, t, AtariDQNNetwork(envs).to(dev), args, envs, dev, backend=backend), envs, fill)


def bench_qdagger(a, dev):
    """qdagger_dqn_atari_impalacnn.py at batch 32: one greedy step of the student, one offline and one online update."""
    for shape, n in ATARI_SHAPES.items():
        learners = {b: make_qdagger(n, b, dev) for b in ("torch", "fused")}
        legs = {"greedy_step": lambda L, obs: L.act(obs, 1, 0.0), "offline_update": lambda L, obs: L.train_step(1.0),
                "online_update": lambda L, obs: L.train_step(0.37), "store": store_leg(*learners["torch"])}
        times = {leg: {b: [] for b in learners} for leg in legs}
        for rep in range(a.warmup + a.reps):
            for leg, fn in legs.items():
                for b, (L, obs) in learners.items():                     # alternating: both backends see the same box state
                    us = timed(lambda: fn(L, obs), dev)
                    if rep >= a.warmup:
                        times[leg][b].append(us)
        row = {"script": "qdagger", "shape": shape, "n_actions": n, "batch": 32, "device": str(dev), "reps": a.reps}
        for leg in legs:
            for b in learners:
                row[f"{leg}_{b}_us"] = round(statistics.median(times[leg][b]), 1)
            row[f"{leg}_speedup"] = round(row[f"{leg}_torch_us"] / row[f"{leg}_fused_us"], 2)
        emit(row)


def make(script, O, A, backend, dev, fill=4096):
    td3 = script == "td3"
    torch.manual_seed(1)
    np.random.seed(1)
    envs = E.SyntheticReplayVecEnv(1, seed=1, obs_dim=O, act_dim=A)
    if script == "sac":
        qs = [ActionValueNetwork(envs).to(dev) for _ in range(4)]
        qs[2].load_state_dict(qs[0].state_dict()), qs[3].load_state_dict(qs[1].state_dict())
        args = SimpleNamespace(buffer_size=fill * 2, batch_size=256, q_lr=1e-3, policy_lr=3e-4, gamma=0.99, tau=0.005, learning_starts=0,
                               policy_frequency=2, target_network_frequency=1, alpha=0.2, autotune=True)
        return fill_ring(SACLearner(SoftActor(envs).to(dev), *qs, args, envs, dev, backend=backend), envs, fill)
    nets = [Actor(envs, batched_space=not td3).to(dev)] + [ActionValueNetwork(envs).to(dev) for _ in range(2 if td3 else 1)]
    tgts = [Actor(envs, batched_space=not td3).to(dev)] + [ActionValueNetwork(envs).to(dev) for _ in range(2 if td3 else 1)]
    for n, t in zip(nets, tgts):
        t.load_state_dict(n.state_dict())
    args = SimpleNamespace(buffer_size=fill * 2, batch_size=256, learning_rate=3e-4, gamma=0.99, tau=0.005, policy_noise=0.2, noise_clip=0.5,
                           exploration_noise=0.1, learning_starts=0)
    return fill_ring(OffPolicyLearner(nets[0], nets[1:], tgts[0], tgts[1:], args, envs, dev, td3=td3, backend=backend), envs, fill)


def fill_ring(L, envs, fill):
    obs, _ = envs.reset(seed=1)
    for _ in range(fill):
        a = np.array([envs.single_action_space.sample()])
        nxt, r, term, trunc, _ = envs.step(a)
        L.store(obs, nxt, a, r, term)
        obs = nxt
    return L, obs


STORES = 64


def store_leg(L, obs, rainbow=False):
    """The ``store`` leg of ``L``'s family: 64 back-to-back ``store``s of pre-generated transitions shaped like ``obs``, with no
    synchronisation but the one ``timed`` puts behind them, so whatever a ``store`` waits for is in the time."""
    rng = np.random.RandomState(2)
    obs = np.asarray(obs)
    new = (lambda: rng.randint(0, 256, obs.shape).astype(np.uint8)) if obs.dtype == np.uint8 else (lambda: rng.standard_normal(obs.shape).astype(np.float32))
    steps = [(new(), new(), np.array([L.space.sample()]), rng.standard_normal(1).astype(np.float32), np.array([i % 20 == 19])) for i in range(STORES)]
    if rainbow:                                                  # RainbowLearner.store(obs, actions, rewards, real_next_obs, terminations)
        steps = [(o, a, r, nxt, d) for o, nxt, a, r, d in steps]

    def run(L, obs):
        for step in steps:
            L.store(*step)

    return run


def emit(row):
    """Prints the row; the ``store`` leg's medians become microseconds per store."""
    for k in ("store_torch_us", "store_fused_us"):
        if k in row:
            row[k] = round(row[k] / STORES, 2)
    print(json.dumps(row), flush=True)


def timed(fn, dev):
    if dev.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--scripts", nargs="+", default=["td3", "ddpg"])
    ap.add_argument("--no-cuda", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda" if torch.cuda.is_available() and not a.no_cuda else "cpu")
    for script in a.scripts:
        if script == "dqn":
            bench_dqn(a, dev)
            continue
        if script == "dqn_atari":
            bench_dqn_atari(a, dev)
            continue
        if script == "rainbow":
            bench_rainbow(a, dev)
            continue
        if script == "rainbow_buffer":
            bench_rainbow_buffer(a, dev)
            continue
        if script == "sac_atari":
            bench_sac_atari(a, dev)
            continue
        if script == "qdagger":
            bench_qdagger(a, dev)
            continue
        for shape, (O, A) in SHAPES.items():
            learners = {b: make(script, O, A, b, dev) for b in ("torch", "fused")}
            extra = (True,) if script == "sac" else ()          # SAC's target update runs every step (target_network_frequency 1)
            legs = {"rollout_step": lambda L, obs: L.act(obs, 1), "critic_step": lambda L, obs: L.train_step(False, *extra),
                    "policy_step": lambda L, obs: L.train_step(True, *extra), "store": store_leg(*learners["torch"])}
            times = {leg: {b: [] for b in learners} for leg in legs}
            for rep in range(a.warmup + a.reps):
                for leg, fn in legs.items():
                    for b, (L, obs) in learners.items():                 # alternating: both backends see the same box state
                        us = timed(lambda: fn(L, obs), dev)
                        if rep >= a.warmup:
                            times[leg][b].append(us)
            row = {"script": script, "shape": shape, "obs_dim": O, "act_dim": A, "batch": 256, "device": str(dev), "reps": a.reps}
            for leg in legs:
                for b in learners:
                    row[f"{leg}_{b}_us"] = round(statistics.median(times[leg][b]), 1)
                row[f"{leg}_speedup"] = round(row[f"{leg}_torch_us"] / row[f"{leg}_fused_us"], 2)
            emit(row)


if __name__ == "__main__":
    main()
