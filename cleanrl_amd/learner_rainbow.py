"""The learner of ``rainbow_atari.py``: noisy dueling distributional double-Q learning on a prioritized n-step replay buffer.

==========================================  =====================================================================================
reference (cleanrl/rainbow_atari.py)        here
==========================================  =====================================================================================
``argmax(sum(q_network(obs) * support))``    ``act``: the noisy online network in training mode; ``fused``: trunk, ``Linear(3136, 1024)``
                                             on the composed weights, ``mi355ppo_rainbow_head_act_f32``
``rb.add(obs, actions, rewards, ...)``       ``store``: the n-step window on the host, then ``HostPrioritizedReplay`` / the device buffer
``rb.beta = ...``                            ``beta`` (settable; the device buffer keeps it in device memory)
the update up to ``optimizer.step``          ``train_step``: ``reset_noise`` of both networks, the sample, the loss, the priority update,
                                             Adam.  ``fused``: ``rainbow_per_sample`` / ``per_gather_u8``, two no-grad trunk passes and one
                                             with autograd, ``rainbow_head_fwd_bwd`` (3 launches), ``h.backward(dh)``,
                                             ``rainbow_noisy_grad``, ``rainbow_per_update``, ``clip_adam_``, ``rainbow_noisy_compose``
the ``tau`` loop                             ``sync_target`` (``polyak_`` on the flat parameters, then the target's compose)
==========================================  =====================================================================================

``MI355PPO_OFFPOLICY`` selects the backend, default ``torch`` (the reference's ops around ``rainbow_replay.HostPrioritizedReplay``).  Both
consume ``random``, ``np.random`` and torch's generators in the reference's order: two ``reset_noise`` (online, then target: eight
``normal_()`` each) and then ``batch_size`` uniform draws per update.  On ``fused`` nothing between the sample and Adam reads the device
back.  The flat buffers, the target update and the logged scalars are ``learner_dqn.QLearner``'s, the projection
is ``learner_dqn.project``, the frame check and the trunk cache ``learner_dqn_atari``'s.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .learner_dqn import QLearner, project
from .learner_dqn_atari import FRAME, Trunks, check_frames
from .rainbow_replay import DevicePrioritizedReplay, HostPrioritizedReplay

ADAM_EPS = 1.5e-4
FC_OUT, FC_IN = ops.RAINBOW_HEAD_IN, 3136


class RainbowLearner(QLearner):
    def __init__(self, q_network, target_network, args, envs, device, backend=None):
        self.n, self.n_atoms = int(envs.single_action_space.n), int(args.n_atoms)
        check_frames(envs)
        self._beta = float(args.prioritized_replay_beta)
        self.gamma_n = args.gamma**args.n_step
        super().__init__(q_network, target_network, args, envs, device, backend, ADAM_EPS)
        if not self.fused:
            return
        dev, n, na = self.device, self.n, self.n_atoms
        self.E, self.P = ops.rainbow_noisy_counts(n, na)
        self.head_off = self.online.numel() - self.P
        for p, off in self._param_offsets(q_network):                       # the trunk's autograd accumulates into the flat gradient
            if off < self.head_off:
                p.grad = self.grads[off:off + p.numel()].view(p.shape)
        self.eps_online, self.eps_target = self._adopt_noise(q_network), self._adopt_noise(target_network)
        self.eff_online, self.eff_target, self.eff_grad = (torch.zeros(self.E, dtype=torch.float32, device=dev) for _ in range(3))
        self._fc = {}
        for key, eff in (("online", self.eff_online), ("target", self.eff_target)):
            W, b = eff[:FC_OUT * FC_IN].view(FC_OUT, FC_IN), eff[FC_OUT * FC_IN:FC_OUT * FC_IN + FC_OUT]
            self._fc[key] = (W, b)
        W, b = (t.requires_grad_() for t in self._fc["online"])
        W.grad, b.grad = self.eff_grad[:FC_OUT * FC_IN].view(FC_OUT, FC_IN), self.eff_grad[FC_OUT * FC_IN:FC_OUT * FC_IN + FC_OUT]
        self.support = q_network.support.detach().to(dev).contiguous()
        M, J = int(args.batch_size), (n + 1) * na
        z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        self._dh, self.loss_per_sample = z((M, FC_OUT)), z(M)
        self._J = J
        self._trunks = Trunks()
        self.compose(True, True)

    def _adopt_noise(self, net):
        """The network's noise buffers become views of one flat buffer, in ``reset_noise()``'s order."""
        flat, off = torch.zeros(self.E, dtype=torch.float32, device=self.device), 0
        for layer in net.noisy_layers():
            for name in ("weight_epsilon", "bias_epsilon"):
                buf = layer._buffers[name]
                flat[off:off + buf.numel()].copy_(buf.reshape(-1))
                layer._buffers[name] = flat[off:off + buf.numel()].view(buf.shape)
                off += buf.numel()
        return flat

    # ------------------------------------------------------------------ what DeviceRing asks of a family
    def _host_buffer(self, act_dtype):
        a = self.args
        return HostPrioritizedReplay(int(a.buffer_size), FRAME, a.n_step, a.gamma, a.prioritized_replay_alpha, self._beta, a.prioritized_replay_eps)

    def _check_sizes(self):
        if not ops.rainbow_head_limits_ok(self.n, self.n_atoms, int(self.args.batch_size)):
            raise ValueError(f"MI355PPO_OFFPOLICY=fused: the fused dueling head takes 2 <= n_actions <= {ops.DQN_MAX_ACT}, 2 <= n_atoms <= "
                             f"{ops.DQN_MAX_ATOMS}, (n_actions + 1) * n_atoms <= {ops.DQN_HEAD_MAX_OUT} and batch_size <= {ops.DQN_HEAD_MAX_ROWS}, "
                             f"not {self.n} / {self.n_atoms} / {self.args.batch_size}; use MI355PPO_OFFPOLICY=torch")

    def _alloc_ring(self, M: int):
        a = self.args
        self.rb = DevicePrioritizedReplay(int(a.buffer_size), self.device, a.n_step, a.gamma, a.prioritized_replay_alpha, self._beta,
                                          a.prioritized_replay_eps)
        self._norm = torch.zeros(1, dtype=torch.float32, device=self.device)      # clip_adam_'s total norm (unused: no clipping here)

    beta = property(lambda self: self.rb.beta, lambda self, v: setattr(self.rb, "beta", v))

    # ------------------------------------------------------------------ the networks below the head (fused)
    def compose(self, online: bool, target: bool):
        """``mu + sigma * eps`` of a network's four noisy layers into its effective buffer: after every ``reset_noise``, after Adam
        (online) and after ``sync_target`` (target)."""
        if online:
            self.g.rainbow_noisy_compose(self.online[self.head_off:], self.eps_online, self.eff_online, self.n, self.n_atoms)
        if target:
            self.g.rainbow_noisy_compose(self.target[self.head_off:], self.eps_target, self.eff_target, self.n, self.n_atoms)
        self._trunks.bump()

    _weights_changed = compose

    def _out(self, eff):
        a = FC_OUT * FC_IN + FC_OUT
        return eff[a:a + self._J * ops.DQN_HEAD_HIDDEN].view(self._J, ops.DQN_HEAD_HIDDEN), eff[a + self._J * ops.DQN_HEAD_HIDDEN:]

    def _hidden(self, net, key, frames_hwc):
        """Both streams' hidden layers as ONE ``Linear(3136, 1024)`` + ReLU on (rows, 84, 84, 4) u8 rows."""
        seq, (W, b) = net.network, self._fc[key]
        if self.device.type != "cuda":
            return torch.relu(torch.nn.functional.linear(seq(frames_hwc.permute(0, 3, 1, 2).float() / 255.0), W, b))
        from . import cnn

        trunk = self._trunks.of(key)
        return cnn.LinearReLUHwcFn.apply(trunk(frames_hwc, None, seq[0], seq[2], seq[4]), W, b, trunk.bufs)

    # ------------------------------------------------------------------ rollout
    def act(self, obs):
        """The step's actions (N,) int64: the argmax of the noisy online network's expectations (no epsilon-greedy here)."""
        with torch.no_grad():
            if not self.fused:
                q_dist = self.q_network(torch.Tensor(obs).to(self.device))
                return torch.argmax(torch.sum(q_dist * self.q_network.support, dim=2), dim=1).cpu().numpy()
            rows = torch.from_numpy(np.ascontiguousarray(obs, np.uint8)).reshape((self.N,) + FRAME).to(self.device).permute(0, 2, 3, 1).contiguous()
            w, b = self._out(self.eff_online)
            self.g.rainbow_head_act(self._hidden(self.q_network, "online", rows).contiguous(), w, b, self.support, self.n, self._greedy)
            return self._copy_out(self._greedy)

    def store(self, obs, actions, rewards, real_next_obs, terminations):
        """``rb.add(obs, actions, rewards, real_next_obs, terminations)``."""
        self.rb.add(obs, actions, rewards, real_next_obs, terminations)

    # ------------------------------------------------------------------ training
    def reset_noise(self, noise=None):
        """The reference's two ``reset_noise()`` calls, online first; ``noise``: a pair of flat (E,) tensors instead of the draws."""
        if noise is None:
            self.q_network.reset_noise()
            self.target_network.reset_noise()
        else:
            for net, flat in zip((self.q_network, self.target_network), noise):
                off = 0
                for layer in net.noisy_layers():
                    for buf in (layer.weight_epsilon, layer.bias_epsilon):
                        buf.copy_(flat[off:off + buf.numel()].view(buf.shape))
                        off += buf.numel()
        if self.fused:
            self.compose(True, True)

    def train_step(self, indices=None, noise=None):
        """One ``# ALGO LOGIC: training.`` block up to the optimizer step.  ``indices``: the batch's draws ``u`` (batch_size,) float64
        instead of ``np.random`` (teacher forcing); ``noise``: see ``reset_noise``."""
        self.reset_noise(noise)
        M = int(self.args.batch_size)
        if not self.fused:
            return self._train_torch(M, indices)
        self.update_kernels(self.rb.sample(M, u=indices))
        self.last = ("fused",)
        return self

    def update_kernels(self, batch, adam: bool = True, aux=None):
        """The update on a device-resident batch (``DevicePrioritizedReplay.sample``'s dict).  ``aux``: optional (best_actions,
        next_pmfs, target_pmfs) outputs (tests)."""
        a, g, M = self.args, self.g, batch["indices"].numel()
        frames = batch["frames"]
        with torch.no_grad():
            h_next_target = self._hidden(self.target_network, "target", frames[M:]).contiguous()
            h_next = self._hidden(self.q_network, "online", frames[M:]).contiguous().clone()
        h = self._hidden(self.q_network, "online", frames[:M])
        (w, b), (wt, bt), (dw, db) = self._out(self.eff_online), self._out(self.eff_target), self._out(self.eff_grad)
        self.grads[:self.head_off].zero_()
        self.eff_grad[:FC_OUT * FC_IN + FC_OUT].zero_()
        g.rainbow_head_fwd_bwd(h.detach().contiguous(), h_next, h_next_target, w, b, wt, bt, self.support, batch["actions"], batch["rewards"],
                               batch["dones"], batch["weights"], self.n, self.gamma_n, a.v_min, a.v_max, self._dh, dw, db, self._sc,
                               self.loss_per_sample, *(aux or (None, None, None)))
        self.rb.update_priorities(batch["indices"], self.loss_per_sample)
        h.backward(self._dh)
        g.rainbow_noisy_grad(self.eff_grad, self.eps_online, self.grads[self.head_off:], self.n, self.n_atoms)
        if adam:
            self.step += 1
            self._adam(self._flats, self.step, a.learning_rate, ADAM_EPS)
            self._weights_changed(True, False)

    def _train_torch(self, M, u):
        a, q_network, target_network, dev = self.args, self.q_network, self.target_network, self.device
        data = self.rb.sample(M, u=u)
        t = lambda x: torch.from_numpy(x).to(dev)  # noqa: E731
        observations, next_observations = t(data["observations"]), t(data["next_observations"])
        actions, rewards, dones, weights = t(data["actions"]).unsqueeze(1), t(data["rewards"]).unsqueeze(1), t(data["dones"]).unsqueeze(1), t(
            data["weights"]).unsqueeze(1)
        with torch.no_grad():
            next_dist = target_network(next_observations)
            support = target_network.support
            next_dist_online = q_network(next_observations)
            next_q_online = torch.sum(next_dist_online * support, dim=2)
            best_actions = torch.argmax(next_q_online, dim=1)
            next_pmfs = next_dist[torch.arange(M), best_actions]
            target_pmfs = project(next_pmfs, rewards, dones, support, q_network.delta_z, self.gamma_n, q_network.v_min, q_network.v_max, a.n_atoms,
                                  True)
        dist = q_network(observations)
        pred_dist = dist.gather(1, actions.unsqueeze(-1).expand(-1, -1, a.n_atoms)).squeeze(1)
        log_pred = torch.log(pred_dist.clamp(min=1e-5, max=1 - 1e-5))
        loss_per_sample = -(target_pmfs * log_pred).sum(dim=1)
        loss = (loss_per_sample * weights.squeeze()).mean()
        self.rb.update_priorities(data["indices"], loss_per_sample.detach().cpu().numpy())
        q_values = (pred_dist * q_network.support).sum(dim=1)
        self.optimizer.zero_grad()
        loss.backward()
        self.optimizer.step()
        self.step += 1
        self.loss_per_sample = loss_per_sample.detach()
        self.last = ("torch", loss.detach(), q_values.detach(), data["indices"], data["weights"])
        return self
