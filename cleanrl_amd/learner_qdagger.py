"""The replay buffers, action logic and training steps of ``qdagger_dqn_atari_impalacnn.py`` (reference:
cleanrl/qdagger_dqn_atari_impalacnn.py and ``ReplayBuffer(..., optimize_memory_usage=True, handle_timeout_termination=False)``).

====================================================  ==============================================================
reference                                              here
====================================================  ==============================================================
``teacher_rb`` / ``rb``                                the ring of ``AtariDQNLearner`` (``torch``: ``HostFrameBuffer``; ``fused``: the u8 frame
                                                       ring in device memory).  ``start_online_phase`` takes a fresh one for the online phase:
                                                       ``torch`` a new buffer; ``fused`` the SAME device memory with ``pos`` / ``full`` reset --
                                                       the reference never reads ``teacher_rb`` after the offline phase, so the teacher's ring is
                                                       given up in place and never two rings are resident
teacher phase: ``argmax(teacher_model(obs))``          ``act(..., teacher=True)``: ``cnn.NatureTrunk`` + ``LinearReLUHwcFn`` +
                                                       ``mi355ppo_dqn_head_act_f32`` on a GPU
online phase: ``argmax(q_network(obs))``               ``act``: ``mi355ppo_impala84_fwd_u8`` on the staged bytes, torch's ``Linear(3872, 256)``,
                                                       ``mi355ppo_qdagger_head_act_f32``
the update (offline: ``distill_coeff`` 1.0)            ``train_step(distill_coeff)``: ``mi355ppo_replay_gather_u8``; under ``no_grad`` the target's
                                                       trunk + FC on the next rows and the teacher's trunk + FC + ``dqn_head_act(q_out=)`` on the
                                                       observation rows; the student's trunk + FC under autograd;
                                                       ``mi355ppo_qdagger_head_fwd_bwd_f32`` (3 launches); ``h.backward(dh)`` into the flat
                                                       gradient (``mi355ppo_impala84_bwd_u8`` below torch's FC); ``mi355ppo_clip_adam_f32``
the ``tau`` loop                                       ``sync_target`` (inherited): ``mi355ppo_polyak_f32``
====================================================  ==============================================================

Backend: ``MI355PPO_OFFPOLICY=torch|fused``, default ``torch``; the student's trunk follows the network's
``impala_backend`` (``MI355PPO_IMPALA``).  Both backends draw ``random``, ``np.random`` and the action space's stream in the reference's
order.  On the CPU ``fused`` runs the host twins.
"""
from __future__ import annotations

import random

import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from .learner_dqn_atari import AtariDQNLearner


def kl_divergence_with_logits(target_logits, prediction_logits):
    """Implementation of on-policy distillation loss (qdagger_dqn_atari_impalacnn.py:192-195)."""
    out = -F.softmax(target_logits, dim=-1) * (F.log_softmax(prediction_logits, dim=-1) - F.log_softmax(target_logits, dim=-1))
    return torch.sum(out)


class QDaggerLearner(AtariDQNLearner):
    """``q_network`` / ``target_network``: ``agents.AtariImpalaQNetwork``; ``teacher_model``: ``agents.AtariDQNNetwork`` (frozen)."""

    def __init__(self, q_network, target_network, teacher_model, args, envs, device, backend=None):
        self.teacher = teacher_model
        for p in teacher_model.parameters():
            p.requires_grad_(False)
        super().__init__(q_network, target_network, args, envs, device, c51=False, backend=backend)
        if not self.fused:
            return
        M, H = int(args.batch_size), ops.QDAGGER_HIDDEN
        self.head_off = self.online.numel() - self.n * H - self.n
        self._dh = torch.zeros((M, H), dtype=torch.float32, device=self.device)
        self._sc = torch.zeros(4, dtype=torch.float32, device=self.device)
        self._teacher_q = torch.zeros((M, self.n), dtype=torch.float32, device=self.device)
        self._teacher_act = torch.zeros(M, dtype=torch.int64, device=self.device)

    def _check_sizes(self):
        if not ops.qdagger_head_limits_ok(self.n, int(self.args.batch_size)):
            raise ValueError(f"MI355PPO_OFFPOLICY=fused: the QDagger head takes 2 <= n_actions <= {ops.DQN_MAX_ACT} and batch_size <= "
                             f"{ops.QDAGGER_MAX_ROWS}, not {self.n} / {self.args.batch_size}; use MI355PPO_OFFPOLICY=torch")

    def start_online_phase(self, envs=None):
        """The reference's second ``ReplayBuffer``: an empty ring.  ``fused`` reuses the teacher ring's device memory (a slot is read
        only after the online phase wrote it: ``sample_indices`` stays below ``pos`` until the ring is full).  ``envs``: the
        environments the reference makes again for this phase; the random branch samples from THEIR action space."""
        self.pos, self.full = 0, False
        if envs is not None:
            self.space = envs.single_action_space
        if not self.fused:
            self.rb = self._host_buffer(np.int64)

    # ------------------------------------------------------------------ the networks below the heads
    def _hidden(self, net, frames_hwc):
        """The student's ``Linear(3872, 256)`` ReLU output on (rows, 84, 84, 4) u8 rows (the trunk per ``net.impala_backend``); the
        teacher's ``Linear(3136, 512)`` output through the base class."""
        if net is self.teacher:
            return super()._hidden(net, frames_hwc)
        return net.hidden_hwc(frames_hwc)

    def _head(self, flat):
        H = ops.QDAGGER_HIDDEN
        return flat[self.head_off:self.head_off + self.n * H].view(self.n, H), flat[self.head_off + self.n * H:]

    def _teacher_head(self, rows, actions_out, q_out=None):
        last = self.teacher.network[-1]
        h = self._hidden(self.teacher, rows).contiguous()
        self.g.dqn_head_act(h, last.weight.detach().contiguous(), last.bias.detach().contiguous(), self.n, actions_out, q_out=q_out)

    # ------------------------------------------------------------------ rollout
    def act(self, obs, global_step: int, epsilon: float, teacher: bool = False):
        """The step's actions (N,) int64: ``random.random() < epsilon`` first, then ``sample()`` per env or the greedy action of the
        student (``teacher``: of the teacher model)."""
        if random.random() < epsilon:
            return np.array([self.space.sample() for _ in range(self.N)])
        with torch.no_grad():
            if not self.fused:
                q_values = (self.teacher if teacher else self.q_network)(torch.Tensor(obs).to(self.device))
                return torch.argmax(q_values, dim=1).cpu().numpy()
            rows = self._stage_frames(obs)
            if teacher:
                self._teacher_head(rows, self._greedy)
            else:
                w, b = self._head(self.online)
                self.g.qdagger_head_act(self._hidden(self.q_network, rows).contiguous(), w, b, self._greedy)
            return self._copy_out(self._greedy)

    # ------------------------------------------------------------------ training
    def train_step(self, distill_coeff: float = 1.0, indices=None):
        """One training block up to the optimizer step (the offline phase's with ``distill_coeff`` 1.0).  ``indices`` replaces the
        draws (teacher forcing)."""
        M = int(self.args.batch_size)
        bi, ei = self.sample_indices(M) if indices is None else indices
        if not self.fused:
            return self._train_qdagger_torch(np.asarray(bi), np.asarray(ei), distill_coeff)
        idx = self._stage_indices(bi, ei)
        self.update_kernels(idx[0], idx[1], distill_coeff=distill_coeff)
        self.last = ("fused",)
        return self

    def _train_qdagger_torch(self, bi, ei, distill_coeff):
        """qdagger_dqn_atari_impalacnn.py:294-310 / 403-430 in the reference's ops."""
        a = self.args
        observations, actions, next_observations, dones, rewards = self.rb.gather(bi, ei)
        q_network, target_network, teacher_model = self.q_network, self.target_network, self.teacher
        with torch.no_grad():
            target_max, _ = target_network(next_observations).max(dim=1)
            td_target = rewards.flatten() + a.gamma * target_max * (1 - dones.flatten())
            teacher_q_values = teacher_model(observations) / a.temperature
        student_q_values = q_network(observations)
        old_val = student_q_values.gather(1, actions).squeeze()
        q_loss = F.mse_loss(td_target, old_val)
        student_q_values = student_q_values / a.temperature
        distill_loss = torch.mean(kl_divergence_with_logits(teacher_q_values, student_q_values))
        loss = q_loss + distill_coeff * distill_loss
        self.optimizer.zero_grad()
        loss.backward()
        self.optimizer.step()
        self.step += 1
        self.last = ("torch", loss.detach(), q_loss.detach(), distill_loss.detach(), old_val.detach())
        return self

    def update_kernels(self, bi, ei, adam: bool = True, aux=None, distill_coeff: float = 1.0):
        """The update on device-resident indices: gather, the three networks below their heads, the QDagger head kernels, the backward
        below the head, Adam.  ``aux``: an optional pair of tensors for ``target_q`` / ``td_target`` (tests)."""
        a, g = self.args, self.g
        M = bi.numel()
        frames, actions, rewards, dones = self._batch
        g.replay_gather_u8(self.ring, bi, ei, frames, actions, rewards, dones)
        with torch.no_grad():
            h_next = self._hidden(self.target_network, frames[M:]).contiguous()
            self._teacher_head(frames[:M], self._teacher_act, q_out=self._teacher_q)
        h = self._hidden(self.q_network, frames[:M])
        hd = h.detach().contiguous()
        (w, b), (wt, bt), (dw, db) = self._head(self.online), self._head(self.target), self._head(self.grads)
        self.grads[:self.head_off].zero_()
        g.qdagger_head_fwd_bwd(hd, h_next, w, b, wt, bt, self._teacher_q, actions, rewards, dones, a.gamma, a.temperature, distill_coeff,
                               self._dh, dw, db, self._sc, *(aux or (None, None)))
        h.backward(self._dh)
        if adam:
            self.step += 1
            self._adam(self._flats, self.step, a.learning_rate, self.eps)
            self._weights_changed(True, False)

    def metrics(self) -> dict:
        """The last update's scalars as Python floats: ``loss``, ``q_loss`` (``losses/td_loss``), ``distill_loss`` and ``q_values``."""
        if self.last[0] == "torch":
            return {"loss": self.last[1].item(), "q_loss": self.last[2].item(), "distill_loss": self.last[3].item(),
                    "q_values": self.last[4].mean().item()}
        return dict(zip(("loss", "q_loss", "distill_loss", "q_values"), self._sc.tolist()))
