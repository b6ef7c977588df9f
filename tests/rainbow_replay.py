"""The host and the device buffer of cleanrl_amd.rainbow_replay driven side by side (the device one on the CPU runs the host twins), and
``RainbowLearner``'s two backends driven side by side."""
from types import SimpleNamespace

import numpy as np
import torch

import rainbow_cases as R
from cleanrl_amd.rainbow_replay import DevicePrioritizedReplay, HostPrioritizedReplay


def _frames(g):
    return torch.randint(0, 256, (1, 4, 84, 84), dtype=torch.uint8, generator=g).numpy()


LOCKSTEP = [(1, 1, 0.5), (5, 5, 0.6), (37, 32, 0.5), (16, 8, 0.6)]


def lockstep(device, slots, B, alpha):
    """Same calls, same ``np.random`` seed: ring contents, n-step returns, max_priority and size equal; leaves within 1 ulp and inner
    nodes what the leaves determine; on equal trees the same indices and weights within 4 ulp; ``np.random`` is left where the host
    buffer's ``uniform`` calls leave it."""
    g = torch.Generator().manual_seed(slots + B)
    host = HostPrioritizedReplay(slots, (4, 84, 84), 3, 0.99, alpha, 0.4, 1e-6)
    dev = DevicePrioritizedReplay(slots, device, 3, 0.99, alpha, 0.4, 1e-6)
    rng = np.random.default_rng(slots)
    obs = _frames(g)
    states, compared = [], 0
    for t in range(slots + 9):
        nxt, a, r, dn = _frames(g), np.array([rng.integers(0, 6)]), np.array([rng.standard_normal()]), np.array([t % 7 == 6])
        assert host.add(obs, a, r, nxt, dn) == dev.add(obs, a, r, nxt, dn)
        obs = nxt
        assert (host.pos, host.size) == (dev.pos, dev.size) and dev.buf[7].item() == dev.size
        if host.size and t % 2:
            beta = 0.4 + 0.05 * t
            host.beta = dev.beta = beta
            equal_trees = R.same_bits(dev.tree, torch.from_numpy(host.sum_tree.tree))
            for rb in (host, dev):
                np.random.seed(50 + t)
                batch = rb.sample(B)
                if rb is dev:
                    batch = {k: v.cpu() for k, v in batch.items()}
                states.append(np.random.get_state()[1].copy())
                if rb is host:
                    want = batch
            assert np.array_equal(states[-1], states[-2])
            if equal_trees:
                compared += 1
                assert batch["indices"].tolist() == list(want["indices"])
                assert int(R.ulps(batch["weights"], want["weights"]).max()) <= 4
                hw = lambda a: torch.from_numpy(a).permute(0, 2, 3, 1)  # noqa: E731
                assert torch.equal(batch["frames"][:B], hw(want["observations"])) and torch.equal(batch["frames"][B:], hw(want["next_observations"]))
                assert torch.equal(batch["actions"], torch.from_numpy(want["actions"]))
                assert R.same_bits(batch["rewards"], torch.from_numpy(want["rewards"]))
                assert torch.equal(batch["dones"], torch.from_numpy(want["dones"]).float())
            loss = torch.randn(B, generator=g) * (3.0 if t % 3 == 0 else 0.2)
            host.update_priorities(want["indices"], loss.numpy())
            dev.update_priorities(torch.as_tensor(want["indices"]).to(device), loss.to(device))
        R.tree_matches(dev.tree, host.sum_tree.tree, slots, f"step {t}")
        assert np.float32(host.max_priority) == np.float32(dev.max_priority)
    assert compared >= 1, "no sample was drawn from bit-equal trees: the indices and the batch were never compared"
    hwc = lambda a: torch.from_numpy(a).permute(0, 2, 3, 1)  # noqa: E731
    buf = [t.cpu() for t in dev.buf]
    assert torch.equal(dev.buf[0].cpu(), hwc(host.obs)) and torch.equal(buf[1], hwc(host.next_obs))
    assert torch.equal(buf[2], torch.from_numpy(host.actions)) and R.same_bits(buf[3], torch.from_numpy(host.rewards))
    assert torch.equal(buf[4], torch.from_numpy(host.dones).float()) and dev.buf[6][1].item() == np.float32(host.beta)


# ================================================================================================== the learner
CPU = torch.device("cpu")


def make_args(**over):
    d = dict(buffer_size=16, batch_size=8, learning_rate=6.25e-5, gamma=0.99, tau=1.0, n_step=3, prioritized_replay_alpha=0.5,
             prioritized_replay_beta=0.4, prioritized_replay_eps=1e-6, n_atoms=5, v_min=-2.0, v_max=2.0)
    d.update(over)
    return SimpleNamespace(**d)


def make_learner(dev, backend, n=6, seed=0, **over):
    from cleanrl_amd.agents import NoisyDuelingDistributionalNetwork
    from cleanrl_amd.envs import SamplingDiscrete

    args = make_args(**over)
    env = SimpleNamespace(single_observation_space=SimpleNamespace(shape=(4, 84, 84)), single_action_space=SamplingDiscrete(n), num_envs=1)
    torch.manual_seed(9000 + seed)
    q = NoisyDuelingDistributionalNetwork(env, args.n_atoms, args.v_min, args.v_max).to(dev)
    t = NoisyDuelingDistributionalNetwork(env, args.n_atoms, args.v_min, args.v_max).to(dev)
    t.load_state_dict(q.state_dict())
    from cleanrl_amd.learner_rainbow import RainbowLearner

    return RainbowLearner(q, t, args, env, dev, backend=backend)


def fill(L, steps, n=6, seed=0):
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    obs = torch.randint(0, 256, (1, 4, 84, 84), dtype=torch.uint8, generator=g).numpy()
    for t in range(steps):
        nxt = torch.randint(0, 256, (1, 4, 84, 84), dtype=torch.uint8, generator=g).numpy()
        L.store(obs, np.array([rng.integers(0, n)]), np.array([rng.standard_normal()]), nxt, np.array([t % 7 == 6]))
        obs = nxt
    return obs


def noise_for(L, seed):
    E = sum(b.numel() for l in L.q_network.noisy_layers() for b in (l.weight_epsilon, l.bias_epsilon))
    g = torch.Generator().manual_seed(seed)
    return torch.randn(E, generator=g).to(L.device), torch.randn(E, generator=g).to(L.device)


def lockstep_updates(dev, n_atoms, updates=4):
    """``fused`` on ``dev`` beside ``torch`` on the CPU, the same transitions, noise and draws: -> per update the two backends'
    (loss, q_values, loss_per_sample) and the sampled indices."""
    T, F = make_learner(CPU, "torch", n_atoms=n_atoms), make_learner(dev, "fused", n_atoms=n_atoms)
    for L in (T, F):
        fill(L, 22)
    out = []
    rng = np.random.default_rng(4)
    for k in range(updates):
        u = rng.random(8)
        noise = noise_for(T, 100 + k)
        for L in (T, F):
            L.beta = 0.4 + 0.1 * k
            L.train_step(indices=u, noise=tuple(x.to(L.device) for x in noise))
            if k == 1:
                L.sync_target()
        mt, mf = T.metrics(), F.metrics()
        out.append((mt, mf, T.loss_per_sample.cpu().clone(), F.loss_per_sample.cpu().clone(), list(T.last[3]), F.rb._batch["indices"].cpu().tolist()))
    return T, F, out


def assert_lockstep(out):
    """The family's bar on ``loss``, ``q_values`` and ``loss_per_sample``: rtol 1e-3, atol 1e-4."""
    for k, (mt, mf, lt, lf, it, i_f) in enumerate(out):
        print(f"update {k}: loss {mt['loss']:.6f} / {mf['loss']:.6f}  q {mt['q_values']:.6f} / {mf['q_values']:.6f}  "
              f"max |d loss_per_sample| {(lt - lf).abs().max().item():.2e}")
        assert it == i_f, k
        for name in ("loss", "q_values"):
            assert abs(mt[name] - mf[name]) <= 1e-4 + 1e-3 * abs(mt[name]), (k, name, mt[name], mf[name])
        assert torch.allclose(lf, lt, rtol=1e-3, atol=1e-4), k


# ================================================================================================== the minted whole runs
import json  # noqa: E402
import os  # noqa: E402
import random  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RUNS = ("rainbow_atari", "rainbow_small")
RTOL, ATOL = 1e-3, 1e-4                                          # the family's bar on loss, q_values and loss_per_sample


def golden_run(name):
    d = np.load(os.path.join(GOLDEN, "rainbow_iteration.npz"))
    return {k.split("/", 1)[1]: d[k] for k in d.files if k.startswith(name + "/")}


def surface():
    with open(os.path.join(GOLDEN, "rainbow_cli_surface.json")) as fh:
        return json.load(fh)["rainbow_atari"]


def replay_run(name, backend, device=CPU, forced=None, on_first_update=None):
    """The minted run's steps as ``rainbow_atari.main``'s loop runs them -> dict of per-step arrays, the tree and the final parameters.
    Frames and noise are regenerated from the seed.  Free-running (``torch`` by default): the learner's own actions, noise and draws.
    ``forced``: the golden actions and draws ``u``, and the noise drawn on the CPU from the seeded generator in ``reset_noise()``'s order
    (a device's own generator would draw other numbers)."""
    from cleanrl_amd import envs as E
    from cleanrl_amd import rainbow_atari
    from cleanrl_amd.agents import NoisyDuelingDistributionalNetwork
    from cleanrl_amd.learner_rainbow import RainbowLearner

    g = golden_run(name)
    cfg = json.loads(bytes(g["config"]).decode())
    args = rainbow_atari.Args(**cfg["args"])
    args.total_timesteps = cfg["steps"]
    forced = backend == "fused" if forced is None else forced
    random.seed(args.seed), np.random.seed(args.seed), torch.manual_seed(args.seed)
    envs = E.AtariReplayVecEnv(1, seed=args.seed, n_actions=cfg["n_actions"], horizon=cfg["horizon"])
    q_network = NoisyDuelingDistributionalNetwork(envs, args.n_atoms, args.v_min, args.v_max)
    target_network = NoisyDuelingDistributionalNetwork(envs, args.n_atoms, args.v_min, args.v_max)
    init_checksum = torch.cat([p.detach().reshape(-1) for p in q_network.parameters()]).double().sum().item()
    target_network.load_state_dict(q_network.state_dict())
    L = RainbowLearner(q_network.to(device), target_network.to(device), args, envs, device, backend=backend)
    first_grad = []
    if backend == "fused":                                       # the pre-Adam flat gradient of the first update (the Adam launch consumes it)
        adam = L._adam
        L._adam = lambda segs, *a, **k: (first_grad or first_grad.append(segs[1].detach().cpu().double().clone()), adam(segs, *a, **k))[1]
    shapes = [tuple(b.shape) for l in q_network.noisy_layers() for b in (l.weight_epsilon, l.bias_epsilon)]

    def cpu_noise():
        return tuple(torch.cat([torch.empty(s).normal_().reshape(-1) for s in shapes]).to(device) for _ in range(2))

    B = args.batch_size
    out = {k: [] for k in ("actions", "beta", "indices", "weights", "loss_per_sample", "loss", "q_values")}
    obs, _ = envs.reset(seed=args.seed)
    for global_step in range(args.total_timesteps):
        L.beta = min(1.0, args.prioritized_replay_beta + global_step * (1.0 - args.prioritized_replay_beta) / args.total_timesteps)
        actions = L.act(obs)
        out["actions"].append(np.asarray(actions, np.int64).reshape(1))
        if forced:
            actions = g["actions"][global_step]
        next_obs, rewards, terminations, truncations, infos = envs.step(actions)
        real_next_obs = next_obs.copy()
        for idx, trunc in enumerate(truncations):
            if trunc:
                real_next_obs[idx] = infos["final_observation"][idx]
        L.store(obs, actions, rewards, real_next_obs, terminations)
        obs = next_obs
        row = dict(indices=np.full(B, -1, np.int64), weights=np.full(B, np.nan, np.float32), loss_per_sample=np.full(B, np.nan, np.float32),
                   loss=np.nan, q_values=np.nan)
        if global_step > args.learning_starts:
            if global_step % args.train_frequency == 0:
                if forced:
                    L.train_step(indices=g["u"][global_step], noise=cpu_noise())
                else:
                    L.train_step()
                if on_first_update is not None:
                    on_first_update(L)
                    on_first_update = None
                idx, w = (L.last[3], L.last[4]) if L.last[0] == "torch" else (L.rb._batch["indices"].cpu().numpy().copy(), L.rb._batch["weights"].cpu().numpy().copy())
                row.update(indices=np.asarray(idx, np.int64), weights=np.asarray(w, np.float32),
                           loss_per_sample=L.loss_per_sample.detach().cpu().numpy().copy(), **L.metrics())
            if global_step % args.target_network_frequency == 0:
                L.sync_target()
        out["beta"].append(float(L.beta))
        for k, v in row.items():
            out[k].append(v)
    out = {k: np.stack(v) if isinstance(v[0], np.ndarray) else np.asarray(v) for k, v in out.items()}
    out["final_online"], out["final_target"] = (t.cpu() for t in L.flat_params())
    out["tree"] = L.rb.sum_tree.tree.copy() if backend == "torch" else L.rb.tree.cpu().numpy()
    out["init_checksum"], out["learner"], out["golden"] = init_checksum, L, g
    out["first_grad"] = first_grad[0] if first_grad else None
    return out


def assert_run_within_bar(rec):
    """``loss``, ``q_values`` and ``loss_per_sample`` of every update at rtol 1e-3, atol 1e-4 against the minted run; the sampled indices
    equal and the weights within 4 ulp, so that the updates compared are the same updates.  -> the number of updates compared."""
    import rainbow_cases as R

    g = rec["golden"]
    trained = g["trained"].astype(bool)
    assert np.array_equal(~np.isnan(rec["loss"]), trained)
    assert np.array_equal(rec["indices"][trained], g["indices"][trained])
    assert int(R.ulps(rec["weights"][trained], g["weights"][trained]).max()) <= 4
    for k in ("loss", "q_values", "loss_per_sample"):
        got, want = rec[k][trained].astype(np.float64), g[k][trained].astype(np.float64)
        worst = np.abs(got - want).max()
        print(f"{k}: max deviation from the minted run {worst:.3e}")
        assert (np.abs(got - want) <= ATOL + RTOL * np.abs(want)).all(), (k, worst)
    return int(trained.sum())
