"""What the replays of the minted off-policy runs share (td3_replay.py, sac_replay.py, dqn_replay.py): the loaders of a family's
golden files, the seeding, the flat-parameter helper, the script's main loop around the family's own action choice and training
step, and the comparison against the goldens at the sensitivity bar."""
import json
import os
import random

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cache = {}                                                      # prefix -> the arrays of <prefix>_iteration.npz; the modules add keys of their own


def flat(*nets):
    return torch.cat([p.detach().reshape(-1) for n in nets for p in n.parameters()]).cpu()


def seed_all(seed):
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def case_config(g):
    return json.loads(bytes(g["config"]).decode())


def run_loop(g, args, envs, L, scalars, forced, choose_action, train, action_dtype=np.float32, action_shape=None):
    """The script's main loop: the golden actions (``forced``) or ``choose_action(obs, global_step)``, the env step,
    ``real_next_obs``, ``store`` and, past ``learning_starts``, ``train(global_step)`` -> the step's scalars (an empty dict when the
    step does not train).  Returns the per-step actions and scalars (NaN where a step has none) as arrays."""
    shape = (envs.num_envs, -1) if action_shape is None else action_shape
    out = {k: [] for k in ("actions",) + tuple(scalars)}
    obs, _ = envs.reset(seed=args.seed)
    for global_step in range(args.total_timesteps):
        actions = g["actions"][global_step].copy() if forced else choose_action(obs, global_step)
        out["actions"].append(np.asarray(actions, action_dtype).reshape(shape))
        next_obs, rewards, terminations, truncations, infos = envs.step(actions)
        real_next_obs = next_obs.copy()
        for idx, trunc in enumerate(truncations):
            if trunc:
                real_next_obs[idx] = infos["final_observation"][idx]
        L.store(obs, real_next_obs, actions, rewards, terminations)
        obs = next_obs
        sc = train(global_step) if global_step > args.learning_starts else {}
        for k in scalars:
            out[k].append(sc.get(k, np.nan))
    return {k: np.asarray(v) for k, v in out.items()}


class Goldens:
    """One family's minted files ``<prefix>_iteration.npz``, ``<prefix>_iteration_ref_sensitivity.json`` and
    ``<prefix>_cli_surface.json``, and the comparison of a replay's record against them: ``scalars`` per step, ``final`` flat
    parameters at the golden stride, ``extra(rec, g)`` -> further deviations."""

    def __init__(self, prefix, scalars, final, extra=None):
        self.prefix, self.scalars, self.final, self.extra = prefix, scalars, final, extra

    def _json(self, suffix):
        with open(os.path.join(GOLDEN_DIR, self.prefix + suffix)) as fh:
            return json.load(fh)

    def golden_case(self, name):
        if self.prefix not in _cache:
            z = np.load(os.path.join(GOLDEN_DIR, self.prefix + "_iteration.npz"))
            _cache[self.prefix] = {k: z[k] for k in z.files}
        return {k.split("/", 1)[1]: v for k, v in _cache[self.prefix].items() if k.startswith(name + "/")}

    def sensitivity(self, name):
        return self._json("_iteration_ref_sensitivity.json")[name]

    def surface(self):
        return self._json("_cli_surface.json")

    def deviations(self, name, rec):
        g = self.golden_case(name)
        dev = {}
        for k in self.scalars:
            a, b = rec[k], g[k]
            m = ~np.isnan(b)
            assert np.array_equal(np.isnan(a), np.isnan(b)), k
            dev[k] = float(np.abs(a[m] - b[m]).max()) if m.any() else 0.0
        s = int(g["stride"])
        for k in self.final:
            dev["final_" + k] = float((rec["final_" + k][::s] - torch.from_numpy(g[f"final_{k}_sub"])).abs().max())
        if self.extra is not None:
            dev.update(self.extra(rec, g))
        return dev

    def assert_within_sensitivity(self, name, rec):
        """Every compared quantity within twice the float32 reference's own recorded deviation from float64, plus 2e-6."""
        dev, sens = self.deviations(name, rec), self.sensitivity(name)
        print(name, {k: f"{v:.3e} (bar {2 * sens[k] + 2e-6:.3e})" for k, v in dev.items()})
        bad = {k: (v, 2 * sens[k] + 2e-6) for k, v in dev.items() if not v <= 2 * sens[k] + 2e-6}
        assert not bad, bad
