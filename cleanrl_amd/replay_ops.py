"""The replay-ring operators, each defined once for the HIP entry point and its host twin.

The C ABI makes one definition enough: a ``*_cpu`` twin takes its device entry point's arguments minus the tail ``(stream)`` or
``(workspace, workspace_bytes, stream)``.  So every operator below validates its arguments once and makes one call through its first
parameter ``s``, a ``Side``, which holds the only two differences between the paths:

* ``s.chk(t, dtype, name, shape=None)`` -- a tensor on this side's kind of device, of that dtype, contiguous, of exactly that shape:
  ``TypeError`` for a non-tensor, the wrong kind of device or a wrong dtype, ``ValueError`` for a non-contiguous tensor or a wrong
  shape.  Nothing is coerced or copied, and every check runs before the C call.
* ``s.launch(name, dev, *args)`` / ``s.launch_ws(name, dev, ws_bytes, dims, *args)`` -- the device side calls ``name`` with ``args``,
  then (``launch_ws``) the workspace of ``ws_bytes(*dims)`` bytes and its size, then ``dev``'s current stream; the host side calls
  ``name + "_cpu"`` with ``args`` alone and never asks for the workspace's size.

``cleanrl_amd.ops`` and ``cleanrl_amd.host_ops`` each build their side and ``bind`` it once at import: ``ops.X`` and ``host_ops.X``
are the function ``X`` below bound to that side, under one name, signature and docstring.  ``sac_alpha_`` holds the one entry point
whose twin differs in the middle of its argument list.  This module imports neither of the two.
"""
from __future__ import annotations

import ctypes
import types
from collections import namedtuple

import torch

Side = namedtuple("Side", "host chk launch launch_ws")

OPERATORS = (
    "replay_add", "ddpg_act", "td3_target", "td3_critic_fwd_bwd", "td3_actor_fwd_bwd", "polyak_",
    "sac_policy", "sac_target", "sac_actor_fwd_bwd", "sac_alpha_",
    "dqn_act", "dqn_td_fwd_bwd", "c51_fwd_bwd",
    "replay_add_u8", "replay_gather_u8", "dqn_head_act", "dqn_head_td_fwd_bwd", "c51_head_fwd_bwd",
    "qdagger_head_act", "qdagger_head_fwd_bwd",
    "rainbow_per_add_u8", "rainbow_per_sample", "rainbow_per_gather_u8", "rainbow_per_update", "rainbow_noisy_compose",
    "rainbow_noisy_grad", "rainbow_head_act", "rainbow_head_fwd_bwd",
    "replay_add2_u8", "replay_gather2_u8", "sacd_head_act", "sacd_critic_fwd_bwd", "sacd_actor_fwd_bwd",
)


def bind(side: Side, namespace: dict) -> None:
    """Put every operator, bound to ``side``, into ``namespace`` (a module's globals) under its own name."""
    for name in OPERATORS:
        namespace[name] = types.MethodType(globals()[name], side)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------- DDPG / TD3 (csrc/offpolicy.hip)
OFFPOLICY_MAX_OBS, OFFPOLICY_MAX_ACT, OFFPOLICY_HIDDEN = 512, 20, 256


def offpolicy_counts(obs_dim: int, act_dim: int):
    """(actor, critic) parameter counts of the two scripts' ``Actor`` / ``QNetwork`` (hidden width 256)."""
    h = OFFPOLICY_HIDDEN
    return h * obs_dim + h + h * h + h + act_dim * h + act_dim, h * (obs_dim + act_dim) + h + h * h + h + h + 1


def _ring_dims(s, ring):
    """ring = (obs, next_obs, actions, rewards, dones), each (slots, n_envs, .) f32 -> (slots, N, O, A)."""
    obs, nxt, act, rew, done = ring
    slots, N, O = obs.shape
    A = act.shape[-1]
    for t, nm, shape in ((obs, "ring obs", (slots, N, O)), (nxt, "ring next_obs", (slots, N, O)), (act, "ring actions", (slots, N, A)),
                         (rew, "ring rewards", (slots, N)), (done, "ring dones", (slots, N))):
        s.chk(t, torch.float32, nm, shape)
    return slots, N, O, A


def _batch_inds(s, batch_inds, env_inds):
    (M,) = batch_inds.shape
    s.chk(batch_inds, torch.int64, "batch_inds", (M,))
    s.chk(env_inds, torch.int64, "env_inds", (M,))
    return M


def replay_add(s, ring, pos: int, obs, next_obs, actions, rewards, dones):
    """``ReplayBuffer.add``: one step's N transitions into slot ``pos`` of the device ring (one launch)."""
    slots, N, O, A = _ring_dims(s, ring)
    s.chk(obs, torch.float32, "obs", (N, O))
    s.chk(next_obs, torch.float32, "next_obs", (N, O))
    s.chk(actions, torch.float32, "actions", (N, A))
    s.chk(rewards, torch.float32, "rewards", (N,))
    s.chk(dones, torch.float32, "dones", (N,))
    s.launch("mi355ppo_replay_add_f32", obs.device, _ptr(obs), _ptr(next_obs), _ptr(actions), _ptr(rewards), _ptr(dones),
             *[_ptr(t) for t in ring], int(pos), slots, N, O, A)


def ddpg_act(s, obs, actor_params, action_scale, action_bias, noise_row, low, high, actions_out):
    """The rollout's action in one launch: ``actor(obs) + noise_row`` clipped to ``low`` / ``high`` -> actions_out (N, A)."""
    chk = s.chk
    N, O = obs.shape
    (A,) = action_scale.shape
    chk(obs, torch.float32, "obs")
    chk(actor_params, torch.float32, "actor_params", (offpolicy_counts(O, A)[0],))
    for t, nm in ((action_scale, "action_scale"), (action_bias, "action_bias"), (low, "low"), (high, "high")):
        chk(t, torch.float32, nm, (A,))
    if noise_row is not None:
        chk(noise_row, torch.float32, "noise_row", (A,))
    chk(actions_out, torch.float32, "actions_out", (N, A))
    s.launch("mi355ppo_ddpg_act_f32", obs.device, _ptr(obs), _ptr(actor_params), _ptr(action_scale), _ptr(action_bias), _ptr(noise_row),
             _ptr(low), _ptr(high), _ptr(actions_out), N, O, A)
    return actions_out


def td3_target(s, ring, batch_inds, env_inds, target_actor, target_critics, n_critics: int, action_scale, action_bias, noise,
               policy_noise: float, noise_clip: float, low0: float, high0: float, gamma: float, next_q_value, next_actions_out=None):
    """The ``with torch.no_grad()`` block of the training step in one launch -> next_q_value (M,).  ``noise`` None: DDPG."""
    chk = s.chk
    slots, N, O, A = _ring_dims(s, ring)
    M = _batch_inds(s, batch_inds, env_inds)
    pa, pq = offpolicy_counts(O, A)
    chk(target_actor, torch.float32, "target_actor", (pa,))
    chk(target_critics, torch.float32, "target_critics", (int(n_critics) * pq,))
    chk(action_scale, torch.float32, "action_scale", (A,))
    chk(action_bias, torch.float32, "action_bias", (A,))
    if noise is not None:
        chk(noise, torch.float32, "noise", (M, A))
    chk(next_q_value, torch.float32, "next_q_value", (M,))
    if next_actions_out is not None:
        chk(next_actions_out, torch.float32, "next_actions_out", (M, A))
    s.launch("mi355ppo_td3_target_f32", batch_inds.device, _ptr(ring[1]), _ptr(ring[3]), _ptr(ring[4]), _ptr(batch_inds), _ptr(env_inds), slots,
             N, _ptr(target_actor), _ptr(target_critics), int(n_critics), _ptr(action_scale), _ptr(action_bias), _ptr(noise),
             float(policy_noise), float(noise_clip), float(low0), float(high0), float(gamma), _ptr(next_q_value), _ptr(next_actions_out),
             M, O, A)
    return next_q_value


def td3_critic_fwd_bwd(s, ring, batch_inds, env_inds, critics, n_critics: int, next_q_value, grads, scalars):
    """Critic forward, ``mse_loss`` and backward in two launches.  OVERWRITES ``grads`` (flat, ``list(qf1.parameters()) +
    list(qf2.parameters())`` order); scalars (2 * n_critics,) = {mean q1, qf1_loss, mean q2, qf2_loss}."""
    slots, N, O, A = _ring_dims(s, ring)
    M = _batch_inds(s, batch_inds, env_inds)
    P = int(n_critics) * offpolicy_counts(O, A)[1]
    s.chk(critics, torch.float32, "critics", (P,))
    s.chk(next_q_value, torch.float32, "next_q_value", (M,))
    s.chk(grads, torch.float32, "grads", (P,))
    s.chk(scalars, torch.float32, "scalars", (2 * int(n_critics),))
    s.launch_ws("mi355ppo_td3_critic_fwd_bwd_f32", batch_inds.device, "mi355ppo_td3_critic_workspace_bytes", (M, O, A, int(n_critics)),
                _ptr(ring[0]), _ptr(ring[2]), _ptr(batch_inds), _ptr(env_inds), slots, N, _ptr(critics), int(n_critics), _ptr(next_q_value),
                _ptr(grads), _ptr(scalars), M, O, A)
    return scalars


def td3_actor_fwd_bwd(s, ring, batch_inds, env_inds, actor, qf1, action_scale, action_bias, grads, actor_loss, dq_daction_out=None):
    """``actor_loss = -qf1(obs, actor(obs)).mean()`` and its gradient w.r.t. the actor in two launches.  OVERWRITES ``grads``."""
    chk = s.chk
    slots, N, O, A = _ring_dims(s, ring)
    M = _batch_inds(s, batch_inds, env_inds)
    pa, pq = offpolicy_counts(O, A)
    chk(actor, torch.float32, "actor", (pa,))
    chk(qf1, torch.float32, "qf1", (pq,))
    chk(action_scale, torch.float32, "action_scale", (A,))
    chk(action_bias, torch.float32, "action_bias", (A,))
    chk(grads, torch.float32, "grads", (pa,))
    chk(actor_loss, torch.float32, "actor_loss", (1,))
    if dq_daction_out is not None:
        chk(dq_daction_out, torch.float32, "dq_daction_out", (M, A))
    s.launch_ws("mi355ppo_td3_actor_fwd_bwd_f32", batch_inds.device, "mi355ppo_td3_actor_workspace_bytes", (M, O, A), _ptr(ring[0]),
                _ptr(batch_inds), _ptr(env_inds), slots, N, _ptr(actor), _ptr(qf1), _ptr(action_scale), _ptr(action_bias), _ptr(grads),
                _ptr(actor_loss), _ptr(dq_daction_out), M, O, A)
    return actor_loss


def polyak_(s, params, target_params, tau: float):
    """``target = tau * param + (1 - tau) * target`` over flat buffers, in place on ``target_params`` (one launch)."""
    n = params.numel()
    s.chk(params, torch.float32, "params", (n,))
    s.chk(target_params, torch.float32, "target_params", (n,))
    s.launch("mi355ppo_polyak_f32", params.device, _ptr(params), _ptr(target_params), n, float(tau))
    return target_params


# ------------------------------------------------------------------------------------------- SAC (csrc/sac.hip)
def sac_actor_count(obs_dim: int, act_dim: int) -> int:
    """Parameter count of sac_continuous_action.py's ``Actor`` (fc1, fc2, fc_mean, fc_logstd; hidden width 256)."""
    h = OFFPOLICY_HIDDEN
    return h * obs_dim + h + h * h + h + 2 * (act_dim * h + act_dim)


def sac_policy(s, obs, actor, action_scale, action_bias, eps, actions_out=None, log_pi_out=None, batch_inds=None, env_inds=None):
    """``actor.get_action`` forward in one launch.  ``obs`` is a dense (rows, O) array, or with ``batch_inds`` / ``env_inds`` a ring
    array (slots, n_envs, O) gathered through them; ``eps`` (rows, A) is the standard normal draw."""
    chk = s.chk
    rows, A = eps.shape
    chk(eps, torch.float32, "eps", (rows, A))
    if batch_inds is None:
        slots, N, O = 0, 0, obs.shape[-1]
        chk(obs, torch.float32, "obs", (rows, O))
    else:
        slots, N, O = obs.shape
        chk(obs, torch.float32, "obs", (slots, N, O))
        assert _batch_inds(s, batch_inds, env_inds) == rows
    chk(actor, torch.float32, "actor", (sac_actor_count(O, A),))
    chk(action_scale, torch.float32, "action_scale", (A,))
    chk(action_bias, torch.float32, "action_bias", (A,))
    if actions_out is not None:
        chk(actions_out, torch.float32, "actions_out", (rows, A))
    if log_pi_out is not None:
        chk(log_pi_out, torch.float32, "log_pi_out", (rows,))
    s.launch("mi355ppo_sac_policy_f32", eps.device, _ptr(obs), _ptr(batch_inds), _ptr(env_inds), slots, N, _ptr(actor), _ptr(action_scale),
             _ptr(action_bias), _ptr(eps), _ptr(actions_out), _ptr(log_pi_out), rows, O, A)
    return actions_out, log_pi_out


def sac_target(s, ring, batch_inds, env_inds, actor, target_critics, action_scale, action_bias, eps, alpha, gamma: float, next_q_value,
               next_actions_out=None, log_pi_out=None):
    """The ``with torch.no_grad()`` block of SAC's training step in one launch -> next_q_value (M,).  ``alpha``: one device float."""
    chk = s.chk
    slots, N, O, A = _ring_dims(s, ring)
    M = _batch_inds(s, batch_inds, env_inds)
    chk(actor, torch.float32, "actor", (sac_actor_count(O, A),))
    chk(target_critics, torch.float32, "target_critics", (2 * offpolicy_counts(O, A)[1],))
    chk(action_scale, torch.float32, "action_scale", (A,))
    chk(action_bias, torch.float32, "action_bias", (A,))
    chk(eps, torch.float32, "eps", (M, A))
    chk(alpha, torch.float32, "alpha", (1,))
    chk(next_q_value, torch.float32, "next_q_value", (M,))
    if next_actions_out is not None:
        chk(next_actions_out, torch.float32, "next_actions_out", (M, A))
    if log_pi_out is not None:
        chk(log_pi_out, torch.float32, "log_pi_out", (M,))
    s.launch("mi355ppo_sac_target_f32", batch_inds.device, _ptr(ring[1]), _ptr(ring[3]), _ptr(ring[4]), _ptr(batch_inds), _ptr(env_inds), slots,
             N, _ptr(actor), _ptr(target_critics), _ptr(action_scale), _ptr(action_bias), _ptr(eps), _ptr(alpha), float(gamma),
             _ptr(next_q_value), _ptr(next_actions_out), _ptr(log_pi_out), M, O, A)
    return next_q_value


def sac_actor_fwd_bwd(s, ring, batch_inds, env_inds, actor, critics, action_scale, action_bias, eps, alpha, grads, actor_loss,
                      log_pi_out=None, dmean_out=None, du_out=None):
    """``actor_loss = ((alpha * log_pi) - min(qf1_pi, qf2_pi)).mean()`` and its gradient w.r.t. the actor in two launches.
    OVERWRITES ``grads``."""
    chk = s.chk
    slots, N, O, A = _ring_dims(s, ring)
    M = _batch_inds(s, batch_inds, env_inds)
    pa = sac_actor_count(O, A)
    chk(actor, torch.float32, "actor", (pa,))
    chk(critics, torch.float32, "critics", (2 * offpolicy_counts(O, A)[1],))
    chk(action_scale, torch.float32, "action_scale", (A,))
    chk(action_bias, torch.float32, "action_bias", (A,))
    chk(eps, torch.float32, "eps", (M, A))
    chk(alpha, torch.float32, "alpha", (1,))
    chk(grads, torch.float32, "grads", (pa,))
    chk(actor_loss, torch.float32, "actor_loss", (1,))
    if log_pi_out is not None:
        chk(log_pi_out, torch.float32, "log_pi_out", (M,))
    for t, nm in ((dmean_out, "dmean_out"), (du_out, "du_out")):
        if t is not None:
            chk(t, torch.float32, nm, (M, A))
    s.launch_ws("mi355ppo_sac_actor_fwd_bwd_f32", batch_inds.device, "mi355ppo_sac_actor_workspace_bytes", (M, O, A), _ptr(ring[0]),
                _ptr(batch_inds), _ptr(env_inds), slots, N, _ptr(actor), _ptr(critics), _ptr(action_scale), _ptr(action_bias), _ptr(eps),
                _ptr(alpha), _ptr(grads), _ptr(actor_loss), _ptr(log_pi_out), _ptr(dmean_out), _ptr(du_out), M, O, A)
    return actor_loss


def sac_alpha_(s, log_pi, target_entropy: float, log_alpha, exp_avg, exp_avg_sq, step: int, lr: float, alpha_out, alpha_loss_out, sched2=None,
               beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8):
    """``alpha_loss``, its gradient and the Adam step on ``log_alpha`` in one launch; writes ``alpha_out = exp(log_alpha)``.  With
    ``sched2`` (2 device floats, ``adam_schedule`` values) the step is read from device memory: capturable.  The host twin takes the
    Adam step count by value and refuses ``sched2``: the one entry point whose twin differs in the middle of the argument list."""
    chk = s.chk
    if s.host and sched2 is not None:
        raise ValueError("sac_alpha_: the host twin takes `step` and `lr`; a schedule tensor is the device path's (cleanrl_amd.ops)")
    (M,) = log_pi.shape
    chk(log_pi, torch.float32, "log_pi", (M,))
    for t, nm in ((log_alpha, "log_alpha"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq"), (alpha_out, "alpha_out"),
                  (alpha_loss_out, "alpha_loss_out")):
        chk(t, torch.float32, nm, (1,))
    if sched2 is not None:
        chk(sched2, torch.float32, "sched2", (2,))
    if s.host:
        s.launch("mi355ppo_sac_alpha_f32", log_pi.device, _ptr(log_pi), M, float(target_entropy), _ptr(log_alpha), _ptr(exp_avg), _ptr(exp_avg_sq),
                 float(lr), float(beta1), float(beta2), float(eps), int(step), _ptr(alpha_out), _ptr(alpha_loss_out))
    else:
        s.launch("mi355ppo_sac_alpha_f32", log_pi.device, _ptr(log_pi), M, float(target_entropy), _ptr(log_alpha), _ptr(exp_avg), _ptr(exp_avg_sq),
                 float(lr), float(beta1), float(beta2), float(eps), int(step), _ptr(sched2), _ptr(alpha_out), _ptr(alpha_loss_out))
    return alpha_out


# ------------------------------------------------------------------------------------------- DQN / C51 (csrc/dqn.hip)
DQN_MAX_OBS, DQN_MAX_ACT, DQN_MAX_ATOMS, DQN_MAX_OUT, DQN_HIDDEN = 512, 18, 101, 512, (120, 84)


def dqn_counts(obs_dim: int, n_actions: int, n_atoms: int = 1) -> int:
    """Parameter count of dqn.py's / c51.py's ``QNetwork`` (120 - 84 - n_actions * n_atoms)."""
    h1, h2 = DQN_HIDDEN
    J = n_actions * n_atoms
    return h1 * obs_dim + h1 + h2 * h1 + h2 + J * h2 + J


def dqn_limits_ok(obs_dim: int, n_actions: int, n_atoms: int = 1) -> bool:
    """What the fused Q networks take (anything else is ``MI355PPO_EINVAL`` from the C ABI)."""
    return (1 <= obs_dim <= DQN_MAX_OBS and 2 <= n_actions <= DQN_MAX_ACT and 1 <= n_atoms <= DQN_MAX_ATOMS
            and n_actions * n_atoms <= DQN_MAX_OUT)


def _dqn_ring(s, ring):
    slots, N, O, A = _ring_dims(s, ring)
    if A != 1:
        raise ValueError(f"ring actions: the DQN / C51 ring stores one action index per env, got width {A}")
    return slots, N, O


def dqn_act(s, obs, params, n_actions: int, actions_out, atoms=None, q_out=None):
    """The greedy action in one launch: ``argmax(q_network(obs), dim=1)`` or, with ``atoms`` (n_atoms,), C51's ``get_action`` ->
    actions_out (N,) int64.  ``q_out`` (N, n_actions) optionally receives the q values."""
    N, O = obs.shape
    na = 1 if atoms is None else atoms.numel()
    s.chk(obs, torch.float32, "obs")
    s.chk(params, torch.float32, "params", (dqn_counts(O, n_actions, na),))
    if atoms is not None:
        s.chk(atoms, torch.float32, "atoms", (na,))
    s.chk(actions_out, torch.int64, "actions_out", (N,))
    if q_out is not None:
        s.chk(q_out, torch.float32, "q_out", (N, n_actions))
    s.launch("mi355ppo_dqn_act_f32", obs.device, _ptr(obs), _ptr(params), _ptr(atoms), _ptr(actions_out), _ptr(q_out), N, O, int(n_actions), na)
    return actions_out


def dqn_td_fwd_bwd(s, ring, batch_inds, env_inds, online, target, n_actions: int, gamma: float, grads, scalars, target_q_out=None,
                   td_target_out=None):
    """dqn.py's update up to the optimizer in two launches.  OVERWRITES ``grads`` (flat, ``q_network.parameters()`` order);
    scalars (2,) = {td_loss, mean old_val}."""
    chk = s.chk
    slots, N, O = _dqn_ring(s, ring)
    M = _batch_inds(s, batch_inds, env_inds)
    P = dqn_counts(O, n_actions)
    for t, nm in ((online, "online"), (target, "target"), (grads, "grads")):
        chk(t, torch.float32, nm, (P,))
    chk(scalars, torch.float32, "scalars", (2,))
    if target_q_out is not None:
        chk(target_q_out, torch.float32, "target_q_out", (M, n_actions))
    if td_target_out is not None:
        chk(td_target_out, torch.float32, "td_target_out", (M,))
    s.launch_ws("mi355ppo_dqn_td_fwd_bwd_f32", batch_inds.device, "mi355ppo_dqn_td_workspace_bytes", (M, O, int(n_actions)),
                *[_ptr(t) for t in ring], _ptr(batch_inds), _ptr(env_inds), slots, N, _ptr(online), _ptr(target), float(gamma), _ptr(grads),
                _ptr(scalars), _ptr(target_q_out), _ptr(td_target_out), M, O, int(n_actions))
    return scalars


def c51_fwd_bwd(s, ring, batch_inds, env_inds, online, target, atoms, n_actions: int, gamma: float, v_min: float, v_max: float, grads, scalars,
                next_pmfs_out=None, target_pmfs_out=None):
    """c51.py's update up to the optimizer in two launches (target ``get_action``, projection, loss, backward).  OVERWRITES
    ``grads``; scalars (2,) = {loss, mean (old_pmfs * atoms).sum(1)}."""
    chk = s.chk
    slots, N, O = _dqn_ring(s, ring)
    M = _batch_inds(s, batch_inds, env_inds)
    na = atoms.numel()
    P = dqn_counts(O, n_actions, na)
    for t, nm in ((online, "online"), (target, "target"), (grads, "grads")):
        chk(t, torch.float32, nm, (P,))
    chk(atoms, torch.float32, "atoms", (na,))
    chk(scalars, torch.float32, "scalars", (2,))
    for t, nm in ((next_pmfs_out, "next_pmfs_out"), (target_pmfs_out, "target_pmfs_out")):
        if t is not None:
            chk(t, torch.float32, nm, (M, na))
    s.launch_ws("mi355ppo_c51_fwd_bwd_f32", batch_inds.device, "mi355ppo_c51_workspace_bytes", (M, O, int(n_actions), na),
                *[_ptr(t) for t in ring], _ptr(batch_inds), _ptr(env_inds), slots, N, _ptr(online), _ptr(target), _ptr(atoms), float(gamma),
                float(v_min), float(v_max), _ptr(grads), _ptr(scalars), _ptr(next_pmfs_out), _ptr(target_pmfs_out), M, O, int(n_actions), na)
    return scalars


# ------------------------------------------------------------------------------------------- Atari DQN / C51 (csrc/dqn_atari.hip)
DQN_HEAD_HIDDEN, DQN_HEAD_MAX_OUT, DQN_HEAD_MAX_ROWS, ATARI_FRAME = 512, 1024, 1024, (84, 84, 4)


def dqn_head_limits_ok(n_actions: int, n_atoms: int = 1, rows: int = 1) -> bool:
    """What the fused Q heads take (anything else is ``MI355PPO_EINVAL`` from the C ABI)."""
    return (2 <= n_actions <= DQN_MAX_ACT and 1 <= n_atoms <= DQN_MAX_ATOMS and n_actions * n_atoms <= DQN_HEAD_MAX_OUT
            and 1 <= rows <= DQN_HEAD_MAX_ROWS)


def _frame_ring(s, ring):
    """ring = (frames (slots, n_envs, 84, 84, 4) u8, actions (slots, n_envs) int64, rewards, dones (slots, n_envs) f32) -> (slots, N)."""
    frames, act, rew, done = ring
    slots, N = frames.shape[:2]
    s.chk(frames, torch.uint8, "ring frames", (slots, N) + ATARI_FRAME)
    s.chk(act, torch.int64, "ring actions", (slots, N))
    s.chk(rew, torch.float32, "ring rewards", (slots, N))
    s.chk(done, torch.float32, "ring dones", (slots, N))
    return slots, N


def _step_u8(s, N, obs, next_obs, actions, rewards, dones):
    """One step's N transitions as the frame rings take them: ``obs`` / ``next_obs`` (N, 4, 84, 84) u8 channels-last."""
    H, W, C = ATARI_FRAME
    s.chk(obs, torch.uint8, "obs", (N, C, H, W))
    s.chk(next_obs, torch.uint8, "next_obs", (N, C, H, W))
    s.chk(actions, torch.int64, "actions", (N,))
    s.chk(rewards, torch.float32, "rewards", (N,))
    s.chk(dones, torch.float32, "dones", (N,))


def _batch_u8(s, M, frames_out, actions_out, rewards_out, dones_out):
    """A gathered batch of M transitions: frames_out (2M, 84, 84, 4) u8, actions_out (M,) int64, rewards_out / dones_out (M,) f32."""
    s.chk(frames_out, torch.uint8, "frames_out", (2 * M,) + ATARI_FRAME)
    s.chk(actions_out, torch.int64, "actions_out", (M,))
    s.chk(rewards_out, torch.float32, "rewards_out", (M,))
    s.chk(dones_out, torch.float32, "dones_out", (M,))


def replay_add_u8(s, ring, pos: int, obs, next_obs, actions, rewards, dones):
    """The memory-optimised ``ReplayBuffer.add``: ``obs`` / ``next_obs`` (N, 4, 84, 84) u8 channels-last into slot ``pos`` and slot
    ``(pos + 1) % slots`` of the device frame ring, actions / rewards / dones into slot ``pos`` (one launch)."""
    slots, N = _frame_ring(s, ring)
    _step_u8(s, N, obs, next_obs, actions, rewards, dones)
    s.launch("mi355ppo_replay_add_u8", obs.device, _ptr(obs), _ptr(next_obs), _ptr(actions), _ptr(rewards), _ptr(dones), *[_ptr(t) for t in ring],
             int(pos), slots, N)


def replay_gather_u8(s, ring, batch_inds, env_inds, frames_out, actions_out, rewards_out, dones_out):
    """A batch out of the frame ring in one launch: frames_out (2M, 84, 84, 4) u8 = the M observation stacks, then the M stacks at
    ``(batch_inds + 1) % slots``; actions_out (M,) int64, rewards_out / dones_out (M,) f32."""
    slots, N = _frame_ring(s, ring)
    M = _batch_inds(s, batch_inds, env_inds)
    _batch_u8(s, M, frames_out, actions_out, rewards_out, dones_out)
    s.launch("mi355ppo_replay_gather_u8", batch_inds.device, *[_ptr(t) for t in ring], _ptr(batch_inds), _ptr(env_inds), slots, N,
             _ptr(frames_out), _ptr(actions_out), _ptr(rewards_out), _ptr(dones_out), M)
    return frames_out


def _head(s, h, w, b):
    M, hidden = h.shape
    J = b.numel()
    s.chk(h, torch.float32, "h", (M, hidden))
    s.chk(w, torch.float32, "w", (J, hidden))
    s.chk(b, torch.float32, "b", (J,))
    return M, hidden, J


def dqn_head_act(s, h, w, b, n_actions: int, actions_out, atoms=None, q_out=None):
    """The greedy action on ``h`` (N, 512): ``Linear(512, n_actions * n_atoms)`` and ``dqn_act``'s argmax -> actions_out (N,) int64."""
    N, hidden, J = _head(s, h, w, b)
    na = 1 if atoms is None else atoms.numel()
    if J != n_actions * na:
        raise ValueError(f"w: expected {n_actions * na} output rows, got {J}")
    if atoms is not None:
        s.chk(atoms, torch.float32, "atoms", (na,))
    s.chk(actions_out, torch.int64, "actions_out", (N,))
    if q_out is not None:
        s.chk(q_out, torch.float32, "q_out", (N, n_actions))
    s.launch_ws("mi355ppo_dqn_head_act_f32", h.device, "mi355ppo_dqn_head_act_workspace_bytes", (N, int(n_actions), na), _ptr(h), _ptr(w),
                _ptr(b), _ptr(atoms), _ptr(actions_out), _ptr(q_out), N, hidden, int(n_actions), na)
    return actions_out


def _head_update_args(s, h, h_next, w, b, w_target, b_target, actions, rewards, dones, dh, dw, db, scalars, n_actions, na, aux):
    """``aux``: (optional f32 output, its name, its columns or None for a vector) each."""
    chk = s.chk
    M, hidden, J = _head(s, h, w, b)
    if J != n_actions * na:
        raise ValueError(f"w: expected {n_actions * na} output rows, got {J}")
    chk(h_next, torch.float32, "h_next", (M, hidden))
    chk(w_target, torch.float32, "w_target", (J, hidden))
    chk(b_target, torch.float32, "b_target", (J,))
    chk(actions, torch.int64, "actions", (M,))
    chk(rewards, torch.float32, "rewards", (M,))
    chk(dones, torch.float32, "dones", (M,))
    chk(dh, torch.float32, "dh", (M, hidden))
    chk(dw, torch.float32, "dw", (J, hidden))
    chk(db, torch.float32, "db", (J,))
    chk(scalars, torch.float32, "scalars", (2,))
    for t, nm, cols in aux:
        if t is not None:
            chk(t, torch.float32, nm, (M,) if cols is None else (M, cols))
    return M, hidden


def dqn_head_td_fwd_bwd(s, h, h_next, w, b, w_target, b_target, actions, rewards, dones, n_actions: int, gamma: float, dh, dw, db, scalars,
                        target_q_out=None, td_target_out=None):
    """dqn_atari.py's update behind the trunks in three launches.  OVERWRITES ``dh`` (M, 512), ``dw`` / ``db`` (the head's gradient,
    e.g. views of the flat gradient); scalars (2,) = {td_loss, mean old_val}."""
    M, hidden = _head_update_args(s, h, h_next, w, b, w_target, b_target, actions, rewards, dones, dh, dw, db, scalars, n_actions, 1,
                                  ((target_q_out, "target_q_out", n_actions), (td_target_out, "td_target_out", None)))
    s.launch_ws("mi355ppo_dqn_head_td_fwd_bwd_f32", h.device, "mi355ppo_dqn_head_workspace_bytes", (M, int(n_actions), 1), _ptr(h), _ptr(h_next),
                _ptr(w), _ptr(b), _ptr(w_target), _ptr(b_target), _ptr(actions), _ptr(rewards), _ptr(dones), float(gamma), _ptr(dh), _ptr(dw),
                _ptr(db), _ptr(scalars), _ptr(target_q_out), _ptr(td_target_out), M, hidden, int(n_actions))
    return scalars


def c51_head_fwd_bwd(s, h, h_next, w, b, w_target, b_target, atoms, actions, rewards, dones, n_actions: int, gamma: float, v_min: float,
                     v_max: float, dh, dw, db, scalars, next_pmfs_out=None, target_pmfs_out=None):
    """c51_atari.py's update behind the trunks in three launches (target ``get_action``, projection, loss, the head's backward).
    OVERWRITES ``dh``, ``dw`` / ``db``; scalars (2,) = {loss, mean (old_pmfs * atoms).sum(1)}."""
    na = atoms.numel()
    s.chk(atoms, torch.float32, "atoms", (na,))
    M, hidden = _head_update_args(s, h, h_next, w, b, w_target, b_target, actions, rewards, dones, dh, dw, db, scalars, n_actions, na,
                                  ((next_pmfs_out, "next_pmfs_out", na), (target_pmfs_out, "target_pmfs_out", na)))
    s.launch_ws("mi355ppo_c51_head_fwd_bwd_f32", h.device, "mi355ppo_dqn_head_workspace_bytes", (M, int(n_actions), na), _ptr(h), _ptr(h_next),
                _ptr(w), _ptr(b), _ptr(w_target), _ptr(b_target), _ptr(atoms), _ptr(actions), _ptr(rewards), _ptr(dones), float(gamma),
                float(v_min), float(v_max), _ptr(dh), _ptr(dw), _ptr(db), _ptr(scalars), _ptr(next_pmfs_out), _ptr(target_pmfs_out), M, hidden,
                int(n_actions), na)
    return scalars


# ------------------------------------------------------------------------------------------- QDagger head (csrc/qdagger.hip)
QDAGGER_HIDDEN, QDAGGER_MAX_ROWS = 256, 1024


def qdagger_head_limits_ok(n_actions: int, rows: int = 1, hidden: int = QDAGGER_HIDDEN) -> bool:
    """What the QDagger head kernels take (anything else is ``MI355PPO_EINVAL`` from the C ABI)."""
    return hidden == QDAGGER_HIDDEN and 2 <= n_actions <= DQN_MAX_ACT and 1 <= rows <= QDAGGER_MAX_ROWS


def qdagger_head_act(s, h, w, b, actions_out, q_out=None):
    """The student's greedy action on ``h`` (N, 256): ``Linear(256, n)`` and ``dqn_act``'s argmax -> actions_out (N,) int64."""
    N, hidden, n = _head(s, h, w, b)
    s.chk(actions_out, torch.int64, "actions_out", (N,))
    if q_out is not None:
        s.chk(q_out, torch.float32, "q_out", (N, n))
    s.launch_ws("mi355ppo_qdagger_head_act_f32", h.device, "mi355ppo_qdagger_head_act_workspace_bytes", (N, n), _ptr(h), _ptr(w), _ptr(b),
                _ptr(actions_out), _ptr(q_out), N, hidden, n)
    return actions_out


def qdagger_head_fwd_bwd(s, h, h_next, w, b, w_target, b_target, teacher_q, actions, rewards, dones, gamma: float, temperature: float,
                         distill_coeff: float, dh, dw, db, scalars, target_q_out=None, td_target_out=None):
    """qdagger_dqn_atari_impalacnn.py's update behind the student's hidden layer in three launches: the TD loss against the target
    network plus ``distill_coeff`` x the KL against the teacher's softmax (``teacher_q`` (M, n): its raw Q values), summed over the
    batch.  OVERWRITES ``dh`` (M, 256), ``dw`` / ``db`` (e.g. views of the flat gradient); scalars (4,) = {loss, q_loss, distill_loss,
    mean old_val}."""
    chk = s.chk
    M, hidden, n = _head(s, h, w, b)
    chk(h_next, torch.float32, "h_next", (M, hidden))
    chk(w_target, torch.float32, "w_target", (n, hidden))
    chk(b_target, torch.float32, "b_target", (n,))
    chk(teacher_q, torch.float32, "teacher_q", (M, n))
    chk(actions, torch.int64, "actions", (M,))
    chk(rewards, torch.float32, "rewards", (M,))
    chk(dones, torch.float32, "dones", (M,))
    chk(dh, torch.float32, "dh", (M, hidden))
    chk(dw, torch.float32, "dw", (n, hidden))
    chk(db, torch.float32, "db", (n,))
    chk(scalars, torch.float32, "scalars", (4,))
    if target_q_out is not None:
        chk(target_q_out, torch.float32, "target_q_out", (M, n))
    if td_target_out is not None:
        chk(td_target_out, torch.float32, "td_target_out", (M,))
    s.launch_ws("mi355ppo_qdagger_head_fwd_bwd_f32", h.device, "mi355ppo_qdagger_head_workspace_bytes", (M, n), _ptr(h), _ptr(h_next), _ptr(w),
                _ptr(b), _ptr(w_target), _ptr(b_target), _ptr(teacher_q), _ptr(actions), _ptr(rewards), _ptr(dones), float(gamma),
                float(temperature), float(distill_coeff), _ptr(dh), _ptr(dw), _ptr(db), _ptr(scalars), _ptr(target_q_out), _ptr(td_target_out),
                M, hidden, n)
    return scalars


# ------------------------------------------------------------------------------------------- Rainbow (csrc/rainbow.hip)
RAINBOW_MAX_BATCH = 1024


def rainbow_noisy_limits_ok(n_actions: int, n_atoms: int) -> bool:
    """What the noisy dueling head's compose / grad kernels take (anything else is ``MI355PPO_EINVAL`` from the C ABI)."""
    return 2 <= n_actions <= DQN_MAX_ACT and 2 <= n_atoms <= DQN_MAX_ATOMS and (n_actions + 1) * n_atoms <= DQN_HEAD_MAX_OUT


def rainbow_noisy_counts(n_actions: int, n_atoms: int):
    """(elements of the effective buffer and of eps, elements of the head's flat parameters) of the four NoisyLinear layers."""
    if not rainbow_noisy_limits_ok(n_actions, n_atoms):
        raise ValueError(f"n_actions={n_actions} n_atoms={n_atoms}: 2 <= n_actions <= {DQN_MAX_ACT}, 2 <= n_atoms <= {DQN_MAX_ATOMS}, "
                         f"(n_actions + 1) * n_atoms <= {DQN_HEAD_MAX_OUT}")
    hid, fc_in, J = DQN_HEAD_HIDDEN, 3136, (n_actions + 1) * n_atoms
    E = 2 * hid * fc_in + 2 * hid + J * hid + J
    return E, 2 * E


def rainbow_new_buffer(slots: int, device, beta: float = 0.4):
    """The prioritized buffer's tensors on ``device``: (ring_obs, ring_next_obs (slots, 84, 84, 4) u8, actions (slots,) int64, rewards,
    dones (slots,) f32, tree (2 * slots - 1,) f32, state (2,) f32 = {max_priority = 1, beta}, size (1,) int64)."""
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=device)  # noqa: E731
    state = torch.tensor([1.0, beta], dtype=torch.float32, device=device)
    return (z((slots,) + ATARI_FRAME, torch.uint8), z((slots,) + ATARI_FRAME, torch.uint8), z((slots,), torch.int64), z((slots,), torch.float32),
            z((slots,), torch.float32), z((2 * slots - 1,), torch.float32), state, z((1,), torch.int64))


def _per_buffer(s, buf):
    chk = s.chk
    ring_obs, ring_next, act, rew, done, tree, state, size = buf
    slots = ring_obs.shape[0]
    chk(ring_obs, torch.uint8, "ring obs", (slots,) + ATARI_FRAME)
    chk(ring_next, torch.uint8, "ring next_obs", (slots,) + ATARI_FRAME)
    chk(act, torch.int64, "ring actions", (slots,))
    chk(rew, torch.float32, "ring rewards", (slots,))
    chk(done, torch.float32, "ring dones", (slots,))
    chk(tree, torch.float32, "tree", (2 * slots - 1,))
    chk(state, torch.float32, "state", (2,))
    chk(size, torch.int64, "size", (1,))
    return slots


def rainbow_per_add_u8(s, buf, pos: int, obs, next_obs, action, reward, done, alpha: float):
    """``PrioritizedReplayBuffer.add`` behind the n-step accumulator: one transition into slot ``pos`` of both frame rings, its leaf at
    ``max_priority ** alpha`` and the leaf's ancestors (one launch)."""
    slots = _per_buffer(s, buf)
    H, W, C = ATARI_FRAME
    s.chk(obs, torch.uint8, "obs", (1, C, H, W))
    s.chk(next_obs, torch.uint8, "next_obs", (1, C, H, W))
    s.chk(action, torch.int64, "action", (1,))
    s.chk(reward, torch.float32, "reward", (1,))
    s.chk(done, torch.float32, "done", (1,))
    s.launch("mi355ppo_rainbow_per_add_u8", obs.device, _ptr(obs), _ptr(next_obs), _ptr(action), _ptr(reward), _ptr(done), *[_ptr(t) for t in buf],
             int(pos), slots, float(alpha))


def rainbow_per_sample(s, buf, u, indices_out, weights_out):
    """``PrioritizedReplayBuffer.sample``'s indices (B,) int64 and weights (B,) f32 from the draws ``u`` (B,) f64; the tree, ``size``
    and ``beta`` are read from device memory (one launch)."""
    slots = _per_buffer(s, buf)
    (B,) = u.shape
    s.chk(u, torch.float64, "u", (B,))
    s.chk(indices_out, torch.int64, "indices_out", (B,))
    s.chk(weights_out, torch.float32, "weights_out", (B,))
    s.launch("mi355ppo_rainbow_per_sample", u.device, _ptr(u), _ptr(buf[5]), _ptr(buf[6]), _ptr(buf[7]), slots, _ptr(indices_out),
             _ptr(weights_out), B)
    return indices_out, weights_out


def rainbow_per_gather_u8(s, buf, indices, frames_out, actions_out, rewards_out, dones_out):
    """A batch out of the two frame rings in one launch: frames_out (2M, 84, 84, 4) u8 = the M obs frames, then the M next_obs frames;
    actions_out (M,) int64, rewards_out / dones_out (M,) f32."""
    slots = _per_buffer(s, buf)
    (M,) = indices.shape
    s.chk(indices, torch.int64, "indices", (M,))
    _batch_u8(s, M, frames_out, actions_out, rewards_out, dones_out)
    s.launch("mi355ppo_rainbow_per_gather_u8", indices.device, *[_ptr(t) for t in buf[:5]], _ptr(indices), slots, _ptr(frames_out),
             _ptr(actions_out), _ptr(rewards_out), _ptr(dones_out), M)
    return frames_out


def rainbow_per_update(s, buf, indices, loss_per_sample, alpha: float, eps: float):
    """``PrioritizedReplayBuffer.update_priorities`` on device tensors: the running maximum, the leaves and their ancestors (one
    launch, no read-back of ``loss_per_sample``)."""
    slots = _per_buffer(s, buf)
    (B,) = indices.shape
    s.chk(indices, torch.int64, "indices", (B,))
    s.chk(loss_per_sample, torch.float32, "loss_per_sample", (B,))
    s.launch("mi355ppo_rainbow_per_update", indices.device, _ptr(indices), _ptr(loss_per_sample), _ptr(buf[5]), _ptr(buf[6]), slots, float(alpha),
             float(eps), B)


def rainbow_noisy_compose(s, params, eps, effective, n_actions: int, n_atoms: int):
    """``mu + sigma * eps`` of the four NoisyLinear layers into the effective buffer (layouts: include/mi355ppo.h), one launch."""
    E, P = rainbow_noisy_counts(n_actions, n_atoms)
    s.chk(params, torch.float32, "params", (P,))
    s.chk(eps, torch.float32, "eps", (E,))
    s.chk(effective, torch.float32, "effective", (E,))
    s.launch("mi355ppo_rainbow_noisy_compose_f32", params.device, _ptr(params), _ptr(eps), _ptr(effective), int(n_actions), int(n_atoms))
    return effective


def rainbow_noisy_grad(s, effective_grad, eps, grads, n_actions: int, n_atoms: int):
    """The effective buffer's gradient back onto the parameters: ``dmu = g``, ``dsigma = g * eps``; OVERWRITES ``grads``, one launch."""
    E, P = rainbow_noisy_counts(n_actions, n_atoms)
    s.chk(effective_grad, torch.float32, "effective_grad", (E,))
    s.chk(eps, torch.float32, "eps", (E,))
    s.chk(grads, torch.float32, "grads", (P,))
    s.launch("mi355ppo_rainbow_noisy_grad_f32", grads.device, _ptr(effective_grad), _ptr(eps), _ptr(grads), int(n_actions), int(n_atoms))
    return grads


RAINBOW_HEAD_IN = 2 * DQN_HEAD_HIDDEN            # h (rows, 1024): the value stream's 512 hidden columns, then the advantage stream's


def rainbow_head_limits_ok(n_actions: int, n_atoms: int, rows: int = 1) -> bool:
    """What the fused dueling distributional head takes (anything else is ``MI355PPO_EINVAL`` from the C ABI)."""
    return rainbow_noisy_limits_ok(n_actions, n_atoms) and 1 <= rows <= DQN_HEAD_MAX_ROWS


def _rainbow_head(s, h, w_out, b_out, support, n_actions, nm=""):
    M = h.shape[0]
    na = support.numel()
    J = (int(n_actions) + 1) * na
    s.chk(h, torch.float32, nm + "h", (M, RAINBOW_HEAD_IN))
    s.chk(w_out, torch.float32, nm + "w_out", (J, DQN_HEAD_HIDDEN))
    s.chk(b_out, torch.float32, nm + "b_out", (J,))
    s.chk(support, torch.float32, "support", (na,))
    return M, na, J


def rainbow_head_act(s, h, w_out, b_out, support, n_actions: int, actions_out, q_out=None):
    """The greedy action of the noisy dueling head on ``h`` (N, 1024) -> actions_out (N,) int64 (two launches)."""
    N, na, J = _rainbow_head(s, h, w_out, b_out, support, n_actions)
    s.chk(actions_out, torch.int64, "actions_out", (N,))
    if q_out is not None:
        s.chk(q_out, torch.float32, "q_out", (N, n_actions))
    s.launch_ws("mi355ppo_rainbow_head_act_f32", h.device, "mi355ppo_rainbow_head_act_workspace_bytes", (N, int(n_actions), na), _ptr(h),
                _ptr(w_out), _ptr(b_out), _ptr(support), _ptr(actions_out), _ptr(q_out), N, int(n_actions), na)
    return actions_out


def _rainbow_head_update_args(s, h, h_next, h_next_target, w_out, b_out, w_out_target, b_out_target, support, actions, rewards, dones, weights,
                              n_actions, dh, dw_out, db_out, scalars, loss_per_sample, best_actions_out, next_pmfs_out, target_pmfs_out):
    chk = s.chk
    M, na, J = _rainbow_head(s, h, w_out, b_out, support, n_actions)
    _rainbow_head(s, h_next, w_out_target, b_out_target, support, n_actions, "target ")
    chk(h_next_target, torch.float32, "h_next_target", (M, RAINBOW_HEAD_IN))
    chk(h_next, torch.float32, "h_next", (M, RAINBOW_HEAD_IN))
    chk(actions, torch.int64, "actions", (M,))
    for t, nm in ((rewards, "rewards"), (dones, "dones"), (weights, "weights"), (loss_per_sample, "loss_per_sample")):
        chk(t, torch.float32, nm, (M,))
    chk(dh, torch.float32, "dh", (M, RAINBOW_HEAD_IN))
    chk(dw_out, torch.float32, "dw_out", (J, DQN_HEAD_HIDDEN))
    chk(db_out, torch.float32, "db_out", (J,))
    chk(scalars, torch.float32, "scalars", (2,))
    if best_actions_out is not None:
        chk(best_actions_out, torch.int64, "best_actions_out", (M,))
    for t, nm in ((next_pmfs_out, "next_pmfs_out"), (target_pmfs_out, "target_pmfs_out")):
        if t is not None:
            chk(t, torch.float32, nm, (M, na))
    return M, na


def rainbow_head_fwd_bwd(s, h, h_next, h_next_target, w_out, b_out, w_out_target, b_out_target, support, actions, rewards, dones, weights,
                         n_actions: int, gamma_n: float, v_min: float, v_max: float, dh, dw_out, db_out, scalars, loss_per_sample,
                         best_actions_out=None, next_pmfs_out=None, target_pmfs_out=None):
    """rainbow_atari.py's update behind the trunks in three launches: online(obs), online(next_obs) and target(next_obs) through the
    effective output layers, double-Q selection, the n-step projection (``gamma_n = gamma ** n_step``), the importance-weighted loss and
    the head's backward.  OVERWRITES ``dh`` (M, 1024), ``dw_out`` / ``db_out``, ``loss_per_sample`` (M,); scalars (2,) = {loss, q_values}."""
    M, na = _rainbow_head_update_args(s, h, h_next, h_next_target, w_out, b_out, w_out_target, b_out_target, support, actions, rewards, dones,
                                      weights, n_actions, dh, dw_out, db_out, scalars, loss_per_sample, best_actions_out, next_pmfs_out,
                                      target_pmfs_out)
    s.launch_ws("mi355ppo_rainbow_head_fwd_bwd_f32", h.device, "mi355ppo_rainbow_head_workspace_bytes", (M, int(n_actions), na), _ptr(h),
                _ptr(h_next), _ptr(h_next_target), _ptr(w_out), _ptr(b_out), _ptr(w_out_target), _ptr(b_out_target), _ptr(support), _ptr(actions),
                _ptr(rewards), _ptr(dones), _ptr(weights), float(gamma_n), float(v_min), float(v_max), _ptr(dh), _ptr(dw_out), _ptr(db_out),
                _ptr(scalars), _ptr(loss_per_sample), _ptr(best_actions_out), _ptr(next_pmfs_out), _ptr(target_pmfs_out), M, int(n_actions), na)
    return scalars


# ------------------------------------------------------------------------------------------- discrete SAC on Atari (csrc/sac_atari.hip)
def sacd_limits_ok(n_actions: int, rows: int = 1) -> bool:
    """What the fused discrete-SAC heads take (anything else is ``MI355PPO_EINVAL`` from the C ABI)."""
    return dqn_head_limits_ok(n_actions, 1, rows)


def _frame_ring2(s, ring):
    """ring = (obs frames, next_obs frames (slots, n_envs, 84, 84, 4) u8, actions (slots, n_envs) int64, rewards, dones (slots, n_envs)
    f32) -> (slots, N)."""
    obs, nxt, act, rew, done = ring
    slots, N = obs.shape[:2]
    s.chk(obs, torch.uint8, "ring obs", (slots, N) + ATARI_FRAME)
    s.chk(nxt, torch.uint8, "ring next_obs", (slots, N) + ATARI_FRAME)
    s.chk(act, torch.int64, "ring actions", (slots, N))
    s.chk(rew, torch.float32, "ring rewards", (slots, N))
    s.chk(done, torch.float32, "ring dones", (slots, N))
    return slots, N


def replay_add2_u8(s, ring, pos: int, obs, next_obs, actions, rewards, dones):
    """The plain ``ReplayBuffer.add`` of sac_atari.py: ``obs`` / ``next_obs`` (N, 4, 84, 84) u8 channels-last into slot ``pos`` of the
    obs ring and of the next_obs ring, actions / rewards / dones into slot ``pos`` (one launch)."""
    slots, N = _frame_ring2(s, ring)
    _step_u8(s, N, obs, next_obs, actions, rewards, dones)
    s.launch("mi355ppo_replay_add2_u8", obs.device, _ptr(obs), _ptr(next_obs), _ptr(actions), _ptr(rewards), _ptr(dones), *[_ptr(t) for t in ring],
             int(pos), slots, N)


def replay_gather2_u8(s, ring, batch_inds, env_inds, frames_out, actions_out, rewards_out, dones_out):
    """A batch out of the two frame rings in one launch: frames_out (2M, 84, 84, 4) u8 = the M observation stacks, then the M next
    observation stacks of the same slots; actions_out (M,) int64, rewards_out / dones_out (M,) f32."""
    slots, N = _frame_ring2(s, ring)
    M = _batch_inds(s, batch_inds, env_inds)
    _batch_u8(s, M, frames_out, actions_out, rewards_out, dones_out)
    s.launch("mi355ppo_replay_gather2_u8", batch_inds.device, *[_ptr(t) for t in ring], _ptr(batch_inds), _ptr(env_inds), slots, N,
             _ptr(frames_out), _ptr(actions_out), _ptr(rewards_out), _ptr(dones_out), M)
    return frames_out


def _sacd_heads(s, hs, heads):
    """``hs``: the heads' inputs (rows, 512); ``heads``: one (w (n, 512), b (n,)) per input -> (rows, hidden, n)."""
    M, hidden = hs[0].shape
    n = heads[0][1].numel()
    if len(hs) != len(heads):
        raise ValueError(f"{len(hs)} inputs for {len(heads)} heads")
    for i, (h, (w, b)) in enumerate(zip(hs, heads)):
        s.chk(h, torch.float32, f"h[{i}]", (M, hidden))
        s.chk(w, torch.float32, f"w[{i}]", (n, hidden))
        s.chk(b, torch.float32, f"b[{i}]", (n,))
    return M, hidden, n


def sacd_head_act(s, h, w, b, noise_exp1, actions_out, probs_out=None):
    """``Actor.get_action``'s sample on ``h`` (N, 512): ``Linear(512, n)``, the softmax and argmax ``probs / noise_exp1`` (the caller's
    Exp(1) draws (N, n)) -> actions_out (N,) int64; probs_out (N, n) optional."""
    N, hidden, n = _sacd_heads(s, (h,), ((w, b),))
    s.chk(noise_exp1, torch.float32, "noise_exp1", (N, n))
    s.chk(actions_out, torch.int64, "actions_out", (N,))
    if probs_out is not None:
        s.chk(probs_out, torch.float32, "probs_out", (N, n))
    s.launch_ws("mi355ppo_sacd_head_act_f32", h.device, "mi355ppo_sacd_head_act_workspace_bytes", (N, n), _ptr(h), _ptr(w), _ptr(b),
                _ptr(noise_exp1), _ptr(actions_out), _ptr(probs_out), N, hidden, n)
    return actions_out


def sacd_critic_fwd_bwd(s, hs, heads, actions, rewards, dones, alpha, gamma: float, dhs, grads, scalars, v_out=None, y_out=None):
    """sac_atari.py's critic update behind the trunks in four launches.  ``hs`` = (qf1, qf2 on obs; actor, qf1_target, qf2_target on
    next_obs), ``heads`` their (w, b) in that order; ``alpha`` (1,) in device memory.  OVERWRITES ``dhs`` = (dh1, dh2) (M, 512) and
    ``grads`` = ((dw1, db1), (dw2, db2)); scalars (4,) = {qf1_loss, qf2_loss, mean qf1_a_values, mean qf2_a_values}."""
    chk = s.chk
    M, hidden, n = _sacd_heads(s, hs, heads)
    if len(hs) != 5:
        raise ValueError(f"the critic update takes five heads, got {len(hs)}")
    chk(actions, torch.int64, "actions", (M,))
    chk(rewards, torch.float32, "rewards", (M,))
    chk(dones, torch.float32, "dones", (M,))
    chk(alpha, torch.float32, "alpha", (1,))
    for i in range(2):
        chk(dhs[i], torch.float32, f"dh{i + 1}", (M, hidden))
        chk(grads[i][0], torch.float32, f"dw{i + 1}", (n, hidden))
        chk(grads[i][1], torch.float32, f"db{i + 1}", (n,))
    chk(scalars, torch.float32, "scalars", (4,))
    for t, nm in ((v_out, "v_out"), (y_out, "y_out")):
        if t is not None:
            chk(t, torch.float32, nm, (M,))
    s.launch_ws("mi355ppo_sacd_critic_fwd_bwd_f32", hs[0].device, "mi355ppo_sacd_critic_workspace_bytes", (M, n), *[_ptr(h) for h in hs],
                *[_ptr(t) for wb in heads for t in wb], _ptr(actions), _ptr(rewards), _ptr(dones), _ptr(alpha), float(gamma), _ptr(dhs[0]),
                _ptr(dhs[1]), *[_ptr(t) for wb in grads for t in wb], _ptr(scalars), _ptr(v_out), _ptr(y_out), M, hidden, n)
    return scalars


def sacd_actor_fwd_bwd(s, hs, heads, alpha, target_entropy: float, dh, dw, db, entropy_rows, actor_loss):
    """sac_atari.py's actor update behind the trunks in three launches.  ``hs`` = (actor, qf1, qf2 on obs), ``heads`` their (w, b).
    OVERWRITES ``dh`` (M, 512), ``dw`` / ``db`` (the actor head's gradient), ``entropy_rows`` (M,) (what ``sac_alpha_`` takes with a
    target entropy of 0) and ``actor_loss`` (1,)."""
    M, hidden, n = _sacd_heads(s, hs, heads)
    if len(hs) != 3:
        raise ValueError(f"the actor update takes three heads, got {len(hs)}")
    s.chk(alpha, torch.float32, "alpha", (1,))
    s.chk(dh, torch.float32, "dh", (M, hidden))
    s.chk(dw, torch.float32, "dw", (n, hidden))
    s.chk(db, torch.float32, "db", (n,))
    s.chk(entropy_rows, torch.float32, "entropy_rows", (M,))
    s.chk(actor_loss, torch.float32, "actor_loss", (1,))
    s.launch_ws("mi355ppo_sacd_actor_fwd_bwd_f32", hs[0].device, "mi355ppo_sacd_actor_workspace_bytes", (M, n), *[_ptr(h) for h in hs],
                *[_ptr(t) for wb in heads for t in wb], _ptr(alpha), float(target_entropy), _ptr(dh), _ptr(dw), _ptr(db), _ptr(entropy_rows),
                _ptr(actor_loss), M, hidden, n)
    return actor_loss
