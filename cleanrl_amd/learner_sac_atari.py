"""The replay buffer, action logic and training step of ``sac_atari.py`` (reference: cleanrl/sac_atari.py and the plain
``ReplayBuffer(..., handle_timeout_termination=False)`` of cleanrl_utils/buffers.py -- sac_atari.py does not pass
``optimize_memory_usage``).

====================================================  ==============================================================
reference                                              here
====================================================  ==============================================================
``ReplayBuffer`` (separate ``observations`` and        ``torch`` -- ``HostFrameBuffer2`` (two u8 arrays, the reference's add / sample rules);
``next_observations``)                                 ``fused`` -- two u8 frame rings in device memory, channels-last, pinned staging
``optim.Adam`` x 3 (``q_lr``, ``policy_lr``,           ``fused`` -- one flat ``actor | qf1 | qf2`` buffer with its gradient and Adam moments,
``q_lr`` on ``log_alpha``; eps 1e-4)                   a flat ``qf1_t | qf2_t``; ``log_alpha`` / its moments / ``alpha`` in device memory
``single_action_space.sample()`` before                ``act``: ``fused`` -- the actor's trunk and ``Linear(3136, 512)`` on this library's
``learning_starts``, else ``actor.get_action``         kernels, then ``mi355ppo_sacd_head_act_f32`` on Exponential(1) noise drawn here
``rb.add(obs, real_next_obs, ...)``                    ``store``: one staged copy + ``mi355ppo_replay_add2_u8``
``rb.sample``                                          ``sample_indices`` (``DeviceRing``: ``randint(0, slots if full else pos)``, ``env_indices``)
``# CRITIC training`` up to ``q_optimizer.step``       ``mi355ppo_replay_gather2_u8``; the actor's and both targets' trunks on next_obs under
                                                       ``no_grad``, both critics' trunks on obs under autograd;
                                                       ``mi355ppo_sacd_critic_fwd_bwd_f32`` (4 launches); ``h.backward(dh)`` twice into the flat
                                                       gradient; ``mi355ppo_clip_adam_f32`` on ``qf1 | qf2`` (2)
``# ACTOR training`` up to                             both critics' trunks on obs again under ``no_grad`` (the new weights, as the reference);
``actor_optimizer.step``                               the actor's trunk on obs under autograd; ``mi355ppo_sacd_actor_fwd_bwd_f32`` (3);
                                                       ``h.backward(dh)``; ``mi355ppo_clip_adam_f32`` on the actor (2)
``alpha_loss`` ... ``log_alpha.exp().item()``          ``mi355ppo_sac_alpha_f32`` on the actor kernel's ``e_r`` rows (1); ``alpha`` never
                                                       leaves the device
the two ``tau`` loops                                  ``sync_target``: one flat copy at ``tau == 1``, ``mi355ppo_polyak_f32`` otherwise
``losses/*``                                           ``metrics`` (device -> host copies only when the script logs)
====================================================  ==============================================================

Backend: ``MI355PPO_OFFPOLICY=torch|fused``, default ``torch``.  ``torch`` draws the reference's random streams
in its order, ``Categorical.sample`` on torch's generator included (the two ``get_action`` calls of an update sample and discard).  ``fused``
draws ``space.sample()`` and ``np.random`` alike, but its policy samples come from Exponential(1) noise: the same distribution on another
stream, so whole-run tests of ``fused`` are teacher-forced.  On the CPU ``fused`` runs the host twins around torch's convolutions.
"""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F
import torch.optim as optim

from . import ops
from .learner_dqn_atari import FRAME, FrameRing, Trunks, check_frames
from .learner_offpolicy import DeviceRing, advance

ADAM_EPS = 1e-4          # "TRY NOT TO MODIFY: eps=1e-4 increases numerical stability"


class HostFrameBuffer2:
    """The plain ``ReplayBuffer`` on u8 frames: ``observations`` and ``next_observations`` are separate arrays, both written at ``pos``."""

    def __init__(self, buffer_size: int, device, n_envs: int = 1):
        self.slots, self.n_envs, self.device = max(int(buffer_size) // n_envs, 1), n_envs, device
        self.observations = np.zeros((self.slots, n_envs) + FRAME, np.uint8)
        self.next_observations = np.zeros((self.slots, n_envs) + FRAME, np.uint8)
        self.actions = np.zeros((self.slots, n_envs, 1), np.int64)
        self.rewards = np.zeros((self.slots, n_envs), np.float32)
        self.dones = np.zeros((self.slots, n_envs), np.float32)
        self.pos, self.full = 0, False

    def add(self, obs, next_obs, action, reward, done):
        self.observations[self.pos] = np.array(obs)
        self.next_observations[self.pos] = np.array(next_obs)
        self.actions[self.pos] = np.array(action).reshape(self.n_envs, 1)
        self.rewards[self.pos] = np.array(reward)
        self.dones[self.pos] = np.array(done)
        advance(self)

    def gather(self, bi, ei):
        t = lambda a: torch.tensor(a, device=self.device)  # noqa: E731
        return (t(self.observations[bi, ei, :]), t(self.actions[bi, ei, :]), t(self.next_observations[bi, ei, :]),
                t(self.dones[bi, ei].reshape(-1, 1)), t(self.rewards[bi, ei].reshape(-1, 1)))


class SACAtariLearner(FrameRing, DeviceRing):
    """``sample_indices`` (``rb.sample``'s two ``np.random`` draws) is ``DeviceRing``'s; the two rings, their staging and ``store`` are
    ``FrameRing``'s."""

    NETS = ("actor", "qf1", "qf2")
    FRAME_ARRAYS = 2

    def __init__(self, actor, qf1, qf2, qf1_target, qf2_target, args, envs, device, backend=None):
        self.n = int(envs.single_action_space.n)
        check_frames(envs)
        super().__init__(args, envs, device, backend, 1, act_dtype=np.int64)
        self.actor, self.qfs, self.qf_targets = actor, [qf1, qf2], [qf1_target, qf2_target]
        self.q_step = self.actor_step = self.alpha_step = 0
        self.autotune = bool(args.autotune)
        dev = self.device
        if self.autotune:
            self.target_entropy = -args.target_entropy_scale * torch.log(1 / torch.tensor(envs.single_action_space.n))
        if not self.fused:
            self.q_optimizer = optim.Adam(list(qf1.parameters()) + list(qf2.parameters()), lr=args.q_lr, eps=ADAM_EPS)
            self.actor_optimizer = optim.Adam(list(actor.parameters()), lr=args.policy_lr, eps=ADAM_EPS)
            if self.autotune:
                self.log_alpha = torch.zeros(1, requires_grad=True, device=dev)
                self.alpha = self.log_alpha.exp().item()
                self.a_optimizer = optim.Adam([self.log_alpha], lr=args.q_lr, eps=ADAM_EPS)
            else:
                self.alpha = args.alpha
            return
        self.P = sum(p.numel() for p in actor.parameters())          # the three classes have the same parameter count
        self.stride = (self.P + 3) // 4 * 4                          # every network starts 16-byte aligned (the Adam kernel's float4s)
        self._alloc_flat(3 * self.stride)
        self.target = torch.zeros(2 * self.stride, dtype=torch.float32, device=dev)
        for i, net in enumerate((actor, qf1, qf2)):
            self._adopt([net], self.online, i * self.stride)
            off = i * self.stride
            for p in net.parameters():                               # autograd accumulates into the flat gradient
                p.grad = self.grads[off:off + p.numel()].view(p.shape)
                off += p.numel()
        for i, net in enumerate(self.qf_targets):
            self._adopt([net], self.target, i * self.stride)
        M, Hd = int(args.batch_size), ops.DQN_HEAD_HIDDEN
        self._dh = tuple(torch.zeros((M, Hd), dtype=torch.float32, device=dev) for _ in range(3))       # dh1 | dh2 | the actor's
        self._er = torch.zeros(M, dtype=torch.float32, device=dev)
        self._qsc = torch.zeros(4, dtype=torch.float32, device=dev)
        self._asc = torch.zeros(1, dtype=torch.float32, device=dev)
        self._sampled = torch.zeros(self.N, dtype=torch.int64, device=dev)
        # log_alpha | exp_avg | exp_avg_sq | alpha | alpha_loss: --no-autotune leaves args.alpha in the alpha slot and never launches the step
        self.alpha_state = torch.tensor([0.0, 0.0, 0.0, 1.0 if self.autotune else float(args.alpha), 0.0], dtype=torch.float32, device=dev)
        self.log_alpha_t, self._am, self._av, self.alpha_t, self._alsc = (self.alpha_state[i:i + 1] for i in range(5))
        self._te = float(self.target_entropy) if self.autotune else 0.0
        self._trunks = Trunks()

    def _host_buffer(self, act_dtype):
        return HostFrameBuffer2(self.args.buffer_size, self.device, n_envs=self.N)

    def _check_sizes(self):
        if not ops.sacd_limits_ok(self.n, int(self.args.batch_size)):
            raise ValueError(f"MI355PPO_OFFPOLICY=fused: the fused discrete-SAC heads take 2 <= n_actions <= {ops.DQN_MAX_ACT} and batch_size <= "
                             f"{ops.DQN_HEAD_MAX_ROWS}, not {self.n} / {self.args.batch_size}; use MI355PPO_OFFPOLICY=torch")

    # ------------------------------------------------------------------ views of the flat buffers
    def _seg(self, flat, which):
        """``actor``: the first network's floats; ``critics``: ``qf1 | qf2`` with the padding between them."""
        return flat[:self.P] if which == "actor" else flat[self.stride:2 * self.stride + self.P]

    def _head(self, flat, i):
        """(w (n, 512), b (n,)) of network ``i`` inside ``flat`` (``online`` / ``grads``: actor, qf1, qf2; ``target``: qf1_t, qf2_t)."""
        n, Hd = self.n, ops.DQN_HEAD_HIDDEN
        end = i * self.stride + self.P
        return flat[end - n * Hd - n:end - n].view(n, Hd), flat[end - n:end]

    # ------------------------------------------------------------------ the networks below the heads
    def _hidden(self, net, frames_hwc):
        """``fc1``'s ReLU output on (rows, 84, 84, 4) u8 rows: this library's trunk and FC on a GPU, torch's on the CPU."""
        if self.device.type != "cuda":
            return F.relu(net.fc1(F.relu(net.conv(frames_hwc.permute(0, 3, 1, 2).float() / 255.0))))
        from . import cnn

        trunk = self._trunks.of(id(net))
        feats = trunk(frames_hwc, None, net.conv[0], net.conv[2], net.conv[4])
        return cnn.LinearReLUHwcFn.apply(feats, net.fc1.weight, net.fc1.bias, trunk.bufs)

    # ------------------------------------------------------------------ rollout
    def act(self, obs, global_step: int):
        """The step's actions (N,) int64."""
        if global_step < self.args.learning_starts:
            return np.array([self.space.sample() for _ in range(self.N)])
        with torch.no_grad():
            if not self.fused:
                actions, _, _ = self.actor.get_action(torch.Tensor(obs).to(self.device))
                return actions.detach().cpu().numpy()
            rows = self._stage_frames(obs)
            noise = torch.empty((self.N, self.n), dtype=torch.float32, device=self.device).exponential_()
            w, b = self._head(self.online, 0)
            self.g.sacd_head_act(self._hidden(self.actor, rows).contiguous(), w, b, noise, self._sampled)
            return self._copy_out(self._sampled)

    # ------------------------------------------------------------------ training
    def train_step(self, indices=None):
        """One ``if global_step % args.update_frequency == 0:`` block.  ``indices`` replaces the draws (teacher forcing)."""
        M = int(self.args.batch_size)
        bi, ei = self.sample_indices(M) if indices is None else indices
        if not self.fused:
            return self._train_torch(np.asarray(bi), np.asarray(ei))
        idx = self._stage_indices(bi, ei)
        self.update_kernels(idx[0], idx[1])
        self.last = "fused"
        return self

    def update_kernels(self, bi, ei, adam: bool = True, aux=None):
        """The update on device-resident indices: gather, the five trunks, the critic head kernels, the backward below the heads, Adam,
        the two critics' trunks again, the actor's, the actor head kernels, backward, Adam, the temperature step.  ``adam=False``
        leaves every weight and ``log_alpha`` alone: the flat gradient then holds both segments' gradients at the same weights.
        ``aux``: an optional pair of (M,) tensors for ``V`` and ``y`` (tests)."""
        a, g = self.args, self.g
        M = bi.numel()
        frames, actions, rewards, dones = self._batch
        g.replay_gather2_u8(self.ring, bi, ei, frames, actions, rewards, dones)
        obs, next_obs = frames[:M], frames[M:]
        qf1, qf2 = self.qfs
        with torch.no_grad():
            h_pi_next = self._hidden(self.actor, next_obs).contiguous()
            h_q1t = self._hidden(self.qf_targets[0], next_obs).contiguous()
            h_q2t = self._hidden(self.qf_targets[1], next_obs).contiguous()
        h1, h2 = self._hidden(qf1, obs), self._hidden(qf2, obs)
        heads = [self._head(self.online, i) for i in range(3)]
        gheads = [self._head(self.grads, i) for i in range(3)]
        self._seg(self.grads, "critics").zero_()
        v_out, y_out = aux or (None, None)
        g.sacd_critic_fwd_bwd((h1.detach().contiguous(), h2.detach().contiguous(), h_pi_next, h_q1t, h_q2t),
                              (heads[1], heads[2], heads[0], self._head(self.target, 0), self._head(self.target, 1)), actions, rewards, dones,
                              self.alpha_t, a.gamma, self._dh[:2], (gheads[1], gheads[2]), self._qsc, v_out, y_out)
        h1.backward(self._dh[0])
        h2.backward(self._dh[1])
        if adam:
            self.q_step += 1
            self._adam([self._seg(f, "critics") for f in self._flats], self.q_step, a.q_lr, ADAM_EPS)
            self._trunks.bump()
        with torch.no_grad():                                                  # the reference evaluates both critics again, after their step
            h1n = self._hidden(qf1, obs).contiguous()
            h2n = self._hidden(qf2, obs).contiguous()
        hp = self._hidden(self.actor, obs)
        self._seg(self.grads, "actor").zero_()
        g.sacd_actor_fwd_bwd((hp.detach().contiguous(), h1n, h2n), (heads[0], heads[1], heads[2]), self.alpha_t, self._te, self._dh[2], *gheads[0],
                             self._er, self._asc)
        hp.backward(self._dh[2])
        if adam:
            self.actor_step += 1
            self._adam([self._seg(f, "actor") for f in self._flats], self.actor_step, a.policy_lr, ADAM_EPS)
            self._trunks.bump()
            if self.autotune:
                self.alpha_step += 1
                g.sac_alpha_(self._er, 0.0, self.log_alpha_t, self._am, self._av, self.alpha_step, a.q_lr, self.alpha_t, self._alsc, eps=ADAM_EPS)

    def sync_target(self):
        """The two ``tau`` loops: a flat copy at ``tau == 1`` (it keeps ``-0.0`` and does not read the old target), Polyak otherwise."""
        tau = self.args.tau
        if self.fused:
            src = self._seg(self.online, "critics")
            dst = self.target[:src.numel()]
            if tau == 1.0:
                dst.copy_(src)
            else:
                self.g.polyak_(src, dst, tau)
            self._trunks.bump()
            return
        for net, tgt in zip(self.qfs, self.qf_targets):
            for param, target_param in zip(net.parameters(), tgt.parameters()):
                target_param.data.copy_(tau * param.data + (1 - tau) * target_param.data)

    def _train_torch(self, bi, ei):
        """The update in the reference's ops."""
        a, alpha = self.args, self.alpha
        actor, (qf1, qf2), (qf1_target, qf2_target) = self.actor, self.qfs, self.qf_targets
        observations, actions, next_observations, dones, rewards = self.rb.gather(bi, ei)
        with torch.no_grad():
            _, next_state_log_pi, next_state_action_probs = actor.get_action(next_observations)
            qf1_next_target = qf1_target(next_observations)
            qf2_next_target = qf2_target(next_observations)
            min_qf_next_target = next_state_action_probs * (torch.min(qf1_next_target, qf2_next_target) - alpha * next_state_log_pi)
            min_qf_next_target = min_qf_next_target.sum(dim=1)
            next_q_value = rewards.flatten() + (1 - dones.flatten()) * a.gamma * (min_qf_next_target)
        qf1_values = qf1(observations)
        qf2_values = qf2(observations)
        qf1_a_values = qf1_values.gather(1, actions.long()).view(-1)
        qf2_a_values = qf2_values.gather(1, actions.long()).view(-1)
        qf1_loss = F.mse_loss(qf1_a_values, next_q_value)
        qf2_loss = F.mse_loss(qf2_a_values, next_q_value)
        qf_loss = qf1_loss + qf2_loss
        self.q_optimizer.zero_grad()
        qf_loss.backward()
        self.q_optimizer.step()
        self.q_step += 1
        _, log_pi, action_probs = actor.get_action(observations)
        with torch.no_grad():
            qf1_values = qf1(observations)
            qf2_values = qf2(observations)
            min_qf_values = torch.min(qf1_values, qf2_values)
        actor_loss = (action_probs * ((alpha * log_pi) - min_qf_values)).mean()
        self.actor_optimizer.zero_grad()
        actor_loss.backward()
        self.actor_optimizer.step()
        self.actor_step += 1
        if self.autotune:
            alpha_loss = (action_probs.detach() * (-self.log_alpha.exp() * (log_pi + self.target_entropy).detach())).mean()
            self.a_optimizer.zero_grad()
            alpha_loss.backward()
            self.a_optimizer.step()
            self.alpha_step += 1
            self.alpha = self.log_alpha.exp().item()
            self._alpha_loss = alpha_loss.detach()
        self.last = ("torch", (qf1_a_values.detach(), qf2_a_values.detach()), (qf1_loss.detach(), qf2_loss.detach()), qf_loss.detach(),
                     actor_loss.detach())
        self.next_q_value = next_q_value
        return self

    def metrics(self) -> dict:
        """The last update's scalars as Python floats (the script's ``losses/*``; ``qf_loss`` is the sum, the script halves it).  On
        ``fused`` this is where ``alpha`` reaches the host."""
        out = {}
        if self.last != "fused":
            _, q_values, q_losses, qf_loss, actor_loss = self.last
            for i in range(2):
                out[f"qf{i + 1}_values"] = q_values[i].mean().item()
                out[f"qf{i + 1}_loss"] = q_losses[i].item()
            out["qf_loss"] = qf_loss.item()
            out["actor_loss"] = actor_loss.item()
            out["alpha"] = self.alpha
            if self.alpha_step:
                out["alpha_loss"] = self._alpha_loss.item()
            return out
        sc = self._qsc.tolist()
        out["qf1_loss"], out["qf2_loss"], out["qf1_values"], out["qf2_values"] = sc
        out["qf_loss"] = float(np.float32(sc[0]) + np.float32(sc[1]))
        out["actor_loss"] = self._asc.item()
        st = self.alpha_state.tolist()
        out["alpha"] = st[3]
        if self.alpha_step:
            out["alpha_loss"] = st[4]
        return out

    def log_alpha_value(self) -> float:
        return (self.log_alpha_t if self.fused else self.log_alpha.detach()).item() if self.autotune else math.log(self.args.alpha)

    def flat_params(self):
        """(actor, qf1 | qf2, qf1_target | qf2_target) flat parameters, detached copies (tests)."""
        return self._flat([self.actor]), self._flat(self.qfs), self._flat(self.qf_targets)
