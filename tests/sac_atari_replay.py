"""Replay of the minted discrete-SAC runs (tests/golden/sac_atari_iteration.npz, tools/mint_sac_atari_goldens.py) through the drop-in's
own classes: free-running for the ``torch`` backend (it must meet the reference's random streams, ``Categorical.sample`` included),
teacher-forced (the golden actions and indices) for ``fused``.  The loop and the comparison are tests/replay_harness.py's."""
import numpy as np
import torch

import replay_harness as H
from cleanrl_amd import envs as E
from cleanrl_amd.agents import AtariSACActor, AtariSoftQNetwork
from cleanrl_amd.learner_sac_atari import SACAtariLearner

CASES = ("sac_atari", "sac_atari_fixed", "sac_atari_polyak")
SCALARS = ("qf1_values", "qf2_values", "qf1_loss", "qf2_loss", "qf_loss", "actor_loss", "alpha_loss", "alpha")
FINAL = ("actor", "critics", "targets")
_G = H.Goldens("sac_atari", SCALARS, FINAL, extra=lambda rec, g: {"final_log_alpha": abs(rec["final_log_alpha"] - float(g["final_log_alpha"]))})
golden_case, sensitivity, surface, deviations, assert_within_sensitivity = (
    _G.golden_case, _G.sensitivity, _G.surface, _G.deviations, _G.assert_within_sensitivity)


def build(name, backend, device=torch.device("cpu")):
    """The case's seeded environment, networks and learner, as the script's ``main`` builds them."""
    from cleanrl_amd import sac_atari as mod

    g = golden_case(name)
    cfg = H.case_config(g)
    args = mod.Args(**cfg["args"])
    args.total_timesteps = cfg["steps"]
    H.seed_all(args.seed)
    envs = E.AtariReplayVecEnv(1, seed=args.seed, n_actions=cfg["n_actions"], horizon=cfg["horizon"])
    actor = AtariSACActor(envs).to(device)
    qf1 = AtariSoftQNetwork(envs).to(device)
    qf2 = AtariSoftQNetwork(envs).to(device)
    qf1_target = AtariSoftQNetwork(envs).to(device)
    qf2_target = AtariSoftQNetwork(envs).to(device)
    qf1_target.load_state_dict(qf1.state_dict())
    qf2_target.load_state_dict(qf2.state_dict())
    init_checksum = H.flat(actor, qf1, qf2).double().sum().item()
    L = SACAtariLearner(actor, qf1, qf2, qf1_target, qf2_target, args, envs, device, backend=backend)
    return g, args, envs, L, init_checksum


def replay(name, backend, device=torch.device("cpu"), forced=None, on_update=None):
    """Runs the case's steps as the script's main loop does -> dict of per-step arrays and final flat parameters.  ``on_update(L,
    global_step, indices)`` is called in front of every update (tests)."""
    g, args, envs, L, init_checksum = build(name, backend, device)
    forced = backend == "fused" if forced is None else forced

    def train(global_step):
        sc = {}
        if global_step % args.update_frequency == 0:
            idx = (g["batch_inds"][global_step], g["env_inds"][global_step]) if forced else None
            if on_update is not None:
                on_update(L, global_step, idx)
            L.train_step(indices=idx)
            sc = L.metrics()
        if global_step % args.target_network_frequency == 0:
            L.sync_target()
        return sc

    out = H.run_loop(g, args, envs, L, SCALARS, forced, L.act, train, action_dtype=np.int64, action_shape=(1,))
    out["final_actor"], out["final_critics"], out["final_targets"] = H.flat(L.actor), H.flat(*L.qfs), H.flat(*L.qf_targets)
    out["final_log_alpha"] = L.log_alpha_value()
    out["init_checksum"] = init_checksum
    out["learner"] = L
    return out
