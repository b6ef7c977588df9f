"""The replay buffer, action logic and training step of ``sac_continuous_action.py`` (reference: cleanrl/sac_continuous_action.py and
``ReplayBuffer`` of cleanrl_utils/buffers.py).  The backend switch, ``HostReplayBuffer``, the ring with its staging and the helpers
of the flat parameter buffers are the base class's (``DeviceRing``, cleanrl_amd/learner_offpolicy.py).

====================================================  ==============================================================
reference                                              here
====================================================  ==============================================================
``optim.Adam`` x 3 (``q_lr``, ``policy_lr``,           ``SACLearner.__init__``: ``torch`` -- ``HostReplayBuffer`` + torch optimizers; ``fused``
``q_lr`` on ``log_alpha``), ``ReplayBuffer``           -- the device ring, flat ``actor | critics`` buffers, a target buffer for the critics,
                                                       ``log_alpha`` / its moments / ``alpha`` in device memory
``single_action_space.sample()`` before                ``act``: ``fused`` -- one launch (``mi355ppo_sac_policy_f32``) on the staged obs and the
``learning_starts``, else ``actor.get_action``         ``(N, A)`` standard normal
``with torch.no_grad():`` target block                 ``mi355ppo_sac_target_f32`` (the online actor, the target critics, ``alpha`` from
                                                       device memory)
critic losses, ``backward``, ``q_optimizer.step``      ``mi355ppo_td3_critic_fwd_bwd_f32`` (2 launches) + ``mi355ppo_clip_adam_f32`` (2)
``policy_frequency`` x (``actor_loss``,                per iteration: ``mi355ppo_sac_actor_fwd_bwd_f32`` (2) + ``mi355ppo_clip_adam_f32`` (2)
``actor_optimizer.step``, ``alpha_loss``,              + ``mi355ppo_sac_policy_f32`` (the ``no_grad`` re-evaluation, 1) +
``a_optimizer.step``, ``log_alpha.exp().item()``)      ``mi355ppo_sac_alpha_f32`` (1); ``alpha`` never leaves the device
the two Polyak loops                                   ``mi355ppo_polyak_f32`` over the critics' segment (1 launch)
``losses/*``                                           ``metrics`` (device -> host copies only when the script logs)
====================================================  ==============================================================

Random streams, both backends, in the reference's order: ``single_action_space.sample()``; ``np.random.randint`` for ``batch_inds`` and
then ``env_indices``; one ``(rows, A)`` standard normal per ``get_action`` call on the learner's device -- per training step the
target's, then per policy iteration the actor's and (``autotune``) the re-evaluation's.  On ``fused`` a critic-only step is 8 library
launches (add, target, critic 2, Adam 2, Polyak, act) and a step with the policy update 8 + ``policy_frequency`` x 6 = 20.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F
import torch.optim as optim

from . import ops
from .learner_offpolicy import DeviceRing


class SACLearner(DeviceRing):
    """``store`` (``rb.add``) and ``sample_indices`` (``rb.sample``'s two ``np.random`` draws) are the base class's."""

    def __init__(self, actor, qf1, qf2, qf1_target, qf2_target, args, envs, device, backend=None):
        super().__init__(args, envs, device, backend, int(np.prod(envs.single_action_space.shape)))
        self.actor, self.qfs, self.qf_targets = actor, [qf1, qf2], [qf1_target, qf2_target]
        self.q_step = self.actor_step = self.alpha_step = 0
        self.autotune = bool(args.autotune)
        dev = self.device
        if self.autotune:
            self.target_entropy = -torch.prod(torch.Tensor(self.space.shape).to(dev)).item()
        if not self.fused:
            self.q_optimizer = optim.Adam(list(qf1.parameters()) + list(qf2.parameters()), lr=args.q_lr)
            self.actor_optimizer = optim.Adam(list(actor.parameters()), lr=args.policy_lr)
            if self.autotune:
                self.log_alpha = torch.zeros(1, requires_grad=True, device=dev)
                self.alpha = self.log_alpha.exp().item()
                self.a_optimizer = optim.Adam([self.log_alpha], lr=args.q_lr)
            else:
                self.alpha = args.alpha
            return
        self.pa, self.pq = ops.sac_actor_count(self.O, self.A), ops.offpolicy_counts(self.O, self.A)[1]
        self.q_off = (self.pa + 3) // 4 * 4                      # the critics start 16-byte aligned (the Adam kernel's float4s)
        self._alloc_flat(self.q_off + 2 * self.pq)
        self.target = torch.zeros(2 * self.pq, dtype=torch.float32, device=dev)          # SAC has no target actor
        self._adopt([actor], self.online)
        self._adopt(self.qfs, self.online, self.q_off)
        self._adopt(self.qf_targets, self.target)
        self.scale = actor.action_scale.detach().reshape(-1).to(dev).contiguous()
        self.bias = actor.action_bias.detach().reshape(-1).to(dev).contiguous()
        M = int(args.batch_size)
        self._y = torch.zeros(M, dtype=torch.float32, device=dev)
        self._lp = torch.zeros(M, dtype=torch.float32, device=dev)
        self._qsc = torch.zeros(4, dtype=torch.float32, device=dev)
        self._asc = torch.zeros(1, dtype=torch.float32, device=dev)
        # log_alpha | exp_avg | exp_avg_sq | alpha | alpha_loss: --no-autotune leaves args.alpha in the alpha slot and never launches the step
        self.alpha_state = torch.tensor([0.0, 0.0, 0.0, 1.0 if self.autotune else float(args.alpha), 0.0], dtype=torch.float32, device=dev)
        self.log_alpha_t, self._am, self._av, self.alpha_t, self._alsc = (self.alpha_state[i:i + 1] for i in range(5))

    # ------------------------------------------------------------------ views of the flat buffers
    def _seg(self, flat, which):
        return flat[:self.pa] if which == "actor" else flat[self.q_off:self.q_off + 2 * self.pq]

    def noise_count(self, policy_update: bool) -> int:
        """Standard normal draws of one training step: the target's, then per policy iteration the actor's and the re-evaluation's."""
        return 1 + (int(self.args.policy_frequency) * (2 if self.autotune else 1) if policy_update else 0)

    # ------------------------------------------------------------------ rollout
    def act(self, obs, global_step: int):
        """The step's action (N, A) as a float32 numpy array."""
        if global_step < self.args.learning_starts:
            return np.array([self.space.sample() for _ in range(self.N)])
        with torch.no_grad():
            if not self.fused:
                actions, _, _ = self.actor.get_action(torch.Tensor(obs).to(self.device))
                return actions.detach().cpu().numpy()
            eps = torch.randn((self.N, self.A), dtype=torch.float32, device=self.device)
            self.g.sac_policy(self._stage_obs(obs), self._seg(self.online, "actor"), self.scale, self.bias, eps, actions_out=self._act)
            return self._copy_out(self._act)

    # ------------------------------------------------------------------ training
    def train_step(self, policy_update: bool, target_update: bool, indices=None, noise=None):
        """One ``# ALGO LOGIC: training.`` block.  ``indices`` and ``noise`` (a list of ``noise_count`` (M, A) tensors) replace the
        draws (teacher forcing)."""
        M = int(self.args.batch_size)
        bi, ei = self.sample_indices(M) if indices is None else indices
        if not self.fused:
            return self._train_torch(bi, ei, policy_update, target_update, noise)
        dev = self.device
        if noise is None:                                        # drawn in the reference's order; nothing between them draws from torch
            noise = [torch.randn((M, self.A), dtype=torch.float32, device=dev) for _ in range(self.noise_count(policy_update))]
        idx = self._stage_indices(bi, ei)
        self.update_kernels(idx[0], idx[1], noise, policy_update, target_update)
        self.last = "fused"
        return self

    def update_kernels(self, bi, ei, noise, policy_update: bool, target_update: bool, adam: bool = True, sched=None):
        """The step's library launches on device-resident indices and noises (what a graph capture records).  With ``sched``, a
        (1 + 2 * policy_frequency, 2) float32 device tensor holding ``adam_schedules()``, every Adam step (the scalar one too) reads
        its step size and bias correction from it and the caller advances ``q_step`` / ``actor_step`` / ``alpha_step``.  ``sched`` is
        for a device only: the host twins take the step as an argument and refuse a schedule pointer."""
        a, g = self.args, self.g
        actor, critics = self._seg(self.online, "actor"), self._seg(self.online, "critics")
        g.sac_target(self.ring, bi, ei, actor, self.target, self.scale, self.bias, noise[0], self.alpha_t, a.gamma, self._y)
        g.td3_critic_fwd_bwd(self.ring, bi, ei, critics, 2, self._y, self._seg(self.grads, "critics"), self._qsc)
        if adam:
            if sched is None:
                self.q_step += 1
            self._adam_seg("critics", self.q_step if sched is None else sched[0], a.q_lr)
        if policy_update:
            k = 1
            for i in range(int(a.policy_frequency)):
                g.sac_actor_fwd_bwd(self.ring, bi, ei, actor, critics, self.scale, self.bias, noise[k], self.alpha_t,
                                    self._seg(self.grads, "actor"), self._asc)
                k += 1
                if adam:
                    if sched is None:
                        self.actor_step += 1
                    self._adam_seg("actor", self.actor_step if sched is None else sched[1 + 2 * i], a.policy_lr)
                if self.autotune:
                    g.sac_policy(self.ring[0], actor, self.scale, self.bias, noise[k], log_pi_out=self._lp, batch_inds=bi, env_inds=ei)
                    k += 1
                    if sched is None:
                        self.alpha_step += 1
                    g.sac_alpha_(self._lp, self.target_entropy, self.log_alpha_t, self._am, self._av, max(self.alpha_step, 1), a.q_lr,
                                 self.alpha_t, self._alsc, sched2=None if sched is None else sched[2 + 2 * i])
        if target_update:
            g.polyak_(critics, self.target, a.tau)

    def _adam_seg(self, which, step, lr):
        self._adam([self._seg(f, which) for f in self._flats], step, lr)

    def adam_schedules(self):
        """(1 + 2 * policy_frequency, 2) host tensor: the library's (step size, bias correction) of the NEXT critic step and, per policy
        iteration, of the next actor and ``log_alpha`` steps."""
        a = self.args
        rows = [ops.adam_schedule(a.q_lr, self.q_step + 1)]
        for i in range(int(a.policy_frequency)):
            rows += [ops.adam_schedule(a.policy_lr, self.actor_step + 1 + i), ops.adam_schedule(a.q_lr, self.alpha_step + 1 + i)]
        return torch.tensor(rows, dtype=torch.float32)

    def _train_torch(self, bi, ei, policy_update, target_update, noise):
        a = self.args
        nz = iter(noise) if noise is not None else None
        draw = (lambda: next(nz)) if nz is not None else (lambda: None)
        obs, actions, next_obs, dones, rewards = self.rb.gather(bi, ei)
        qf1, qf2 = self.qfs
        with torch.no_grad():
            next_state_actions, next_state_log_pi, _ = self.actor.get_action(next_obs, draw())
            qf1_next_target = self.qf_targets[0](next_obs, next_state_actions)
            qf2_next_target = self.qf_targets[1](next_obs, next_state_actions)
            min_qf_next_target = torch.min(qf1_next_target, qf2_next_target) - self.alpha * next_state_log_pi
            next_q_value = rewards.flatten() + (1 - dones.flatten()) * a.gamma * (min_qf_next_target).view(-1)
        qf1_a_values = qf1(obs, actions).view(-1)
        qf2_a_values = qf2(obs, actions).view(-1)
        qf1_loss = F.mse_loss(qf1_a_values, next_q_value)
        qf2_loss = F.mse_loss(qf2_a_values, next_q_value)
        qf_loss = qf1_loss + qf2_loss
        self.q_optimizer.zero_grad()
        qf_loss.backward()
        self.q_optimizer.step()
        self.q_step += 1
        if policy_update:
            for _ in range(int(a.policy_frequency)):
                pi, log_pi, _ = self.actor.get_action(obs, draw())
                min_qf_pi = torch.min(qf1(obs, pi), qf2(obs, pi))
                actor_loss = ((self.alpha * log_pi) - min_qf_pi).mean()
                self.actor_optimizer.zero_grad()
                actor_loss.backward()
                self.actor_optimizer.step()
                self.actor_step += 1
                self._actor_loss = actor_loss.detach()
                if self.autotune:
                    with torch.no_grad():
                        _, log_pi, _ = self.actor.get_action(obs, draw())
                    alpha_loss = (-self.log_alpha.exp() * (log_pi + self.target_entropy)).mean()
                    self.a_optimizer.zero_grad()
                    alpha_loss.backward()
                    self.a_optimizer.step()
                    self.alpha_step += 1
                    self.alpha = self.log_alpha.exp().item()
                    self._alpha_loss = alpha_loss.detach()
        if target_update:
            for net, tgt in zip(self.qfs, self.qf_targets):
                for param, target_param in zip(net.parameters(), tgt.parameters()):
                    target_param.data.copy_(a.tau * param.data + (1 - a.tau) * target_param.data)
        self.last = ("torch", (qf1_a_values, qf2_a_values), (qf1_loss, qf2_loss), qf_loss)
        self.next_q_value = next_q_value
        return self

    def metrics(self) -> dict:
        """The last step's scalars as Python floats (the script's ``losses/*``); ``actor_loss`` / ``alpha_loss`` are the last policy
        update's.  On ``fused`` this is where ``alpha`` reaches the host."""
        out = {}
        if self.last != "fused":
            _, q_values, q_losses, qf_loss = self.last
            for i in range(2):
                out[f"qf{i + 1}_values"] = q_values[i].mean().item()
                out[f"qf{i + 1}_loss"] = q_losses[i].item()
            out["qf_loss"] = qf_loss.item()
            if self.actor_step:
                out["actor_loss"] = self._actor_loss.item()
            out["alpha"] = self.alpha
            if self.alpha_step:
                out["alpha_loss"] = self._alpha_loss.item()
            return out
        sc = self._qsc.tolist()
        for i in range(2):
            out[f"qf{i + 1}_values"], out[f"qf{i + 1}_loss"] = sc[2 * i], sc[2 * i + 1]
        out["qf_loss"] = float(np.float32(sc[1]) + np.float32(sc[3]))
        if self.actor_step:
            out["actor_loss"] = self._asc.item()
        st = self.alpha_state.tolist()
        out["alpha"] = st[3]
        if self.alpha_step:
            out["alpha_loss"] = st[4]
        return out

    def log_alpha_value(self) -> float:
        return (self.log_alpha_t if self.fused else self.log_alpha.detach()).item() if self.autotune else math.log(self.args.alpha)

    def flat_params(self):
        """(actor, critics, critic targets) flat parameters, detached copies (tests)."""
        return self._flat([self.actor]), self._flat(self.qfs), self._flat(self.qf_targets)
