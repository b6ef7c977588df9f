"""The replay buffer, action logic and training step of ``dqn.py`` and ``c51.py`` (reference: cleanrl/dqn.py, cleanrl/c51.py and
``ReplayBuffer`` of cleanrl_utils/buffers.py).

====================================================  ==============================================================
reference                                              here
====================================================  ==============================================================
``optim.Adam(q_network.parameters(), ...)``,           ``DQNLearner.__init__``: ``torch`` -- ``HostReplayBuffer`` (int64 actions) + the torch
``ReplayBuffer(..., handle_timeout_termination=        optimizer; ``fused`` -- the ring in device memory with an action width of 1 (the index
False)``                                               as f32), flat parameter / gradient / Adam buffers the modules' parameters are views of
``random.random() < epsilon``, then                    ``act``: the same two draws in the same order; the greedy branch on ``fused`` is one
``single_action_space.sample()`` per env or            launch (``mi355ppo_dqn_act_f32``) on the staged obs
``argmax(q_network(obs))`` / ``get_action(obs)``
``real_next_obs`` / ``rb.add(...)``                    ``store`` (``DeviceRing``): one staged copy + ``mi355ppo_replay_add_f32``
``rb.sample`` (``np.random.randint`` twice)            ``sample_indices`` (``DeviceRing``)
dqn.py: ``target_max`` / ``td_target`` /               ``train_step``: ``mi355ppo_dqn_td_fwd_bwd_f32`` (2 launches) + ``mi355ppo_clip_adam_f32``
``old_val`` / ``mse_loss`` / ``backward`` /            (grad_scale 1, max_grad_norm inf, eps 1e-8: 2 launches)
``optimizer.step``
c51.py: target ``get_action``, the projection          ``train_step``: ``mi355ppo_c51_fwd_bwd_f32`` (2 launches) + ``mi355ppo_clip_adam_f32``
loop, ``old_pmfs``, the loss, ``backward``,            with eps ``0.01 / batch_size``
``optimizer.step``
dqn.py: the ``tau`` Polyak loop                        ``sync_target``: ``mi355ppo_polyak_f32`` over the flat buffers (1 launch)
c51.py: ``target_network.load_state_dict``             ``sync_target``: one flat ``target.copy_(online)`` (a copy keeps ``-0.0`` and does not
                                                       read the old target, which ``polyak_(tau=1)`` would)
``losses/*``                                           ``metrics`` (one device -> host copy when the script logs)
====================================================  ==============================================================

Backend: ``MI355PPO_OFFPOLICY=torch|fused``, default ``torch``.  Both backends draw the reference's random
streams in its order.  The backend switch, the ring, the flat-buffer helpers and the Adam helper are the base class's (``DeviceRing``,
cleanrl_amd/learner_offpolicy.py).  A fused step is 6 library launches (act 1, add 1, update 2, Adam 2), 7 on a target-update step of dqn.py.

``QLearner`` and ``project`` are what this learner shares with ``learner_dqn_atari.AtariDQNLearner`` and
``learner_rainbow.RainbowLearner``: the online / target flat buffers, the target update, the torch update of dqn.py / c51.py, the
logged scalars, and the categorical projection of all three torch backends.
"""
from __future__ import annotations

import random

import numpy as np
import torch
import torch.nn.functional as F
import torch.optim as optim

from . import ops
from .learner_offpolicy import DeviceRing


def project(next_pmfs, rewards, dones, support, delta_z, gamma, v_min, v_max, n_atoms, l_eq_b: bool):
    """``target_pmfs`` of c51.py / c51_atari.py (``l_eq_b`` False) and of rainbow_atari.py (True: its own ``(l == b)``, and ``gamma`` is
    ``gamma ** n_step``), op for op: ``support`` and ``delta_z`` are the network's own (a tensor or a float)."""
    next_atoms = rewards + gamma * support * (1 - dones.float())
    tz = next_atoms.clamp(v_min, v_max)
    b = (tz - v_min) / delta_z
    l = b.floor().clamp(0, n_atoms - 1)  # noqa: E741
    u = b.ceil().clamp(0, n_atoms - 1)
    d_m_l = (u.float() + (l == b).float() - b if l_eq_b else u + (l == u).float() - b) * next_pmfs
    d_m_u = (b - l) * next_pmfs
    target_pmfs = torch.zeros_like(next_pmfs)
    for i in range(target_pmfs.size(0)):
        target_pmfs[i].index_add_(0, l[i].long(), d_m_l[i])
        target_pmfs[i].index_add_(0, u[i].long(), d_m_u[i])
    return target_pmfs


class QLearner(DeviceRing):
    """What the Q learners on a replay ring share (``DQNLearner``, ``AtariDQNLearner``, ``RainbowLearner``).  A subclass sets ``n`` /
    ``n_atoms`` (and ``c51``) before ``__init__``.  ``torch``: the optimizer.  ``fused``: ``online`` / ``target`` flat buffers the two
    networks' parameters are views of, the greedy actions and the two logged scalars in device memory."""

    c51 = False

    def __init__(self, q_network, target_network, args, envs, device, backend, adam_eps):
        super().__init__(args, envs, device, backend, 1, act_dtype=np.int64)
        self.q_network, self.target_network = q_network, target_network
        self.eps = adam_eps
        self.step = 0
        if not self.fused:
            self.optimizer = optim.Adam(q_network.parameters(), lr=args.learning_rate, eps=self.eps)
            return
        dev = self.device
        total = sum(p.numel() for p in q_network.parameters())
        self._alloc_flat(total)
        self.target = torch.zeros(total, dtype=torch.float32, device=dev)
        self._adopt([q_network], self.online)
        self._adopt([target_network], self.target)
        self._greedy = torch.zeros(self.N, dtype=torch.int64, device=dev)
        self._sc = torch.zeros(2, dtype=torch.float32, device=dev)

    @staticmethod
    def _param_offsets(net):
        off = 0
        for p in net.parameters():
            yield p, off
            off += p.numel()

    def _weights_changed(self, online: bool, target: bool):
        """``fused``: the flat parameters of the online / the target network were written (Adam, ``sync_target``).  The Atari learners
        tell their trunks, Rainbow composes its noisy layers again."""

    def _train_torch(self, bi, ei):
        """The update of dqn.py / dqn_atari.py, or of c51.py / c51_atari.py (``c51``), in the reference's ops."""
        a = self.args
        observations, actions, next_observations, dones, rewards = self.rb.gather(bi, ei)
        q_network, target_network = self.q_network, self.target_network
        if self.c51:
            with torch.no_grad():
                _, next_pmfs = target_network.get_action(next_observations)
                atoms = target_network.atoms
                target_pmfs = project(next_pmfs, rewards, dones, atoms, atoms[1] - atoms[0], a.gamma, a.v_min, a.v_max, a.n_atoms, False)
            _, old_pmfs = q_network.get_action(observations, actions.flatten())
            loss = (-(target_pmfs * old_pmfs.clamp(min=1e-5, max=1 - 1e-5).log()).sum(-1)).mean()
            old_val = (old_pmfs * q_network.atoms).sum(1)
        else:
            with torch.no_grad():
                target_max, _ = target_network(next_observations).max(dim=1)
                td_target = rewards.flatten() + a.gamma * target_max * (1 - dones.flatten())
            old_val = q_network(observations).gather(1, actions).squeeze()
            loss = F.mse_loss(td_target, old_val)
        self.optimizer.zero_grad()
        loss.backward()
        self.optimizer.step()
        self.step += 1
        self.last = ("torch", loss.detach(), old_val.detach())
        return self

    def sync_target(self):
        """The target update: the scripts' ``tau`` loop, or ``load_state_dict`` of c51.py / c51_atari.py (``c51``)."""
        if self.fused:
            if self.c51:
                self.target.copy_(self.online)
            else:
                self.g.polyak_(self.online, self.target, self.args.tau)
            self._weights_changed(False, True)
            return
        if self.c51:
            self.target_network.load_state_dict(self.q_network.state_dict())
            return
        tau = self.args.tau
        for target_network_param, q_network_param in zip(self.target_network.parameters(), self.q_network.parameters()):
            target_network_param.data.copy_(tau * q_network_param.data + (1.0 - tau) * target_network_param.data)

    def metrics(self) -> dict:
        """The last update's scalars as Python floats: ``loss`` (``losses/td_loss`` or ``losses/loss``) and ``q_values``."""
        if self.last[0] == "torch":
            return {"loss": self.last[1].item(), "q_values": self.last[2].mean().item()}
        sc = self._sc.tolist()
        return {"loss": sc[0], "q_values": sc[1]}

    def flat_params(self):
        """(online, target) flat parameters, detached copies (tests)."""
        return self._flat([self.q_network]), self._flat([self.target_network])


class DQNLearner(QLearner):
    """``c51``: the networks are ``C51Network`` (atoms, ``get_action``) and the update is the categorical one."""

    def __init__(self, q_network, target_network, args, envs, device, c51: bool, backend=None):
        self.c51 = bool(c51)
        self.n = int(envs.single_action_space.n)
        self.n_atoms = int(args.n_atoms) if self.c51 else 1
        super().__init__(q_network, target_network, args, envs, device, backend, 0.01 / args.batch_size if self.c51 else 1e-8)
        if self.fused:
            self.atoms = q_network.atoms.detach().to(self.device).contiguous() if self.c51 else None

    def _check_sizes(self):
        if not ops.dqn_limits_ok(self.O, self.n, self.n_atoms) or (self.c51 and self.n_atoms < 2):
            raise ValueError(f"MI355PPO_OFFPOLICY=fused: the fused Q networks take obs_dim <= {ops.DQN_MAX_OBS}, 2 <= n_actions <= "
                             f"{ops.DQN_MAX_ACT}, n_atoms <= {ops.DQN_MAX_ATOMS} (at least 2 for c51) and n_actions * n_atoms <= "
                             f"{ops.DQN_MAX_OUT}, not {self.O} / {self.n} / {self.n_atoms}; use MI355PPO_OFFPOLICY=torch")

    # ------------------------------------------------------------------ rollout
    def act(self, obs, global_step: int, epsilon: float):
        """The step's actions (N,) int64: ``random.random() < epsilon`` first, then ``sample()`` per env or the greedy action."""
        if random.random() < epsilon:
            return np.array([self.space.sample() for _ in range(self.N)])
        with torch.no_grad():
            if not self.fused:
                x = torch.Tensor(obs).to(self.device)
                if self.c51:
                    actions, _ = self.q_network.get_action(x)
                else:
                    actions = torch.argmax(self.q_network(x), dim=1)
                return actions.cpu().numpy()
            self.g.dqn_act(self._stage_obs(obs), self.online, self.n, self._greedy, atoms=self.atoms)
            return self._copy_out(self._greedy)

    # ------------------------------------------------------------------ training
    def train_step(self, indices=None):
        """One ``# ALGO LOGIC: training.`` block up to the optimizer step.  ``indices`` replaces the draws (teacher forcing)."""
        M = int(self.args.batch_size)
        bi, ei = self.sample_indices(M) if indices is None else indices
        if not self.fused:
            return self._train_torch(bi, ei)
        idx = self._stage_indices(bi, ei)
        self.update_kernels(idx[0], idx[1])
        self.last = ("fused",)
        return self

    def update_kernels(self, bi, ei, adam: bool = True, sched=None):
        """The update's library launches on device-resident indices (what a graph capture records).  With ``sched``, a (2,) float32
        device tensor holding ``adam_schedule()``, Adam reads its step size and bias correction from it (``clip_adam_sched_``) and
        the caller advances ``step``."""
        a, g = self.args, self.g
        if self.c51:
            g.c51_fwd_bwd(self.ring, bi, ei, self.online, self.target, self.atoms, self.n, a.gamma, a.v_min, a.v_max, self.grads, self._sc)
        else:
            g.dqn_td_fwd_bwd(self.ring, bi, ei, self.online, self.target, self.n, a.gamma, self.grads, self._sc)
        if adam:
            if sched is None:
                self.step += 1
            self._adam(self._flats, self.step if sched is None else sched, a.learning_rate, self.eps)

    def adam_schedule(self):
        """(2,) host tensor: the library's (step size, bias correction) of the NEXT Adam step."""
        return torch.tensor(ops.adam_schedule(self.args.learning_rate, self.step + 1), dtype=torch.float32)
