"""The rollout, Q(lambda) targets and recurrent Q-network update of ``pqn_atari_envpool_lstm.py`` (reference:
cleanrl/pqn_atari_envpool_lstm.py, the main loop after ``QNetwork``) on ``PQNLearner``'s storage, random stream and optimiser.

====================================================  ==============================================================
reference                                              here
====================================================  ==============================================================
``next_lstm_state`` zeros                              ``LSTMPQNLearner.__init__`` (``next_lstm_state``)
``initial_lstm_state`` clone per iteration             ``act(0)``: the first step of an iteration snapshots the state
action logic with the recurrent state                  ``act``: ``torch`` -- the reference's ops; ``fused`` -- trunk + the gx GEMM
                                                       (torch), then ONE launch, ``mi355ppo_pqn_lstm_act_f32``: done reset, LSTM
                                                       cell, ``q_func``, e-greedy, the ``actions`` / ``values`` / ``dones`` rows
                                                       and the new state (in place)
``# Compute Q(lambda) targets`` with the state         ``finish_rollout``: the same entry point in its bootstrap form (q only),
                                                       then ``mi355ppo_pqn_qlambda_f32``
ENV-WISE minibatches: ``np.random.shuffle(envinds)``,  ``update``: ``mb_inds = flatinds[:, mbenvinds].ravel()``, state and dones
``flatinds[:, mbenvinds].ravel()``, the initial        gathered per minibatch; ``fused`` -- trunk + gx (torch), ``ops.lstm_seq``
state per env, ``mse_loss``, ``backward``,             (one scan forward, one backward), ``mi355ppo_pqn_lstm_td_fwd_bwd_f32``
``clip_grad_norm_``, ``RAdam.step``                    (q_func + gather + TD loss, forward and backward; q_func's gradient goes
                                                       straight into its ``FlatParams`` views), ``h.backward(dh)``, then
                                                       ``mi355ppo_clip_radam_f32``
``losses/td_loss``, ``losses/q_values``                the dict ``update`` returns (last minibatch)
====================================================  ==============================================================

Backend: ``MI355PPO_PQN=torch|fused`` alone, as for the other PQN scripts (``fused`` on a CUDA device by default, ``torch`` on the
CPU, where ``fused`` runs the host twins); ``MI355PPO_LSTM`` is not read here.  Both backends draw the reference's random stream:
``torch.randint`` then ``torch.rand`` on the CPU generator every step, ``np.random.shuffle(envinds)`` every epoch.

Trunk: ``MI355PPO_PQN_TRUNK=torch|fused`` (or the ``trunk`` keyword), default ``torch``, read as ``PQNLearner`` reads it.  ``fused`` -- only
with ``MI355PPO_PQN=fused``, a HIP device and ``(1, 84, 84)`` uint8 observations -- keeps the rollout frames as ``(T, N, 84, 84)`` uint8 (a
quarter of the f32 storage's bytes; ``reset`` / ``observe`` copy the incoming bytes, no conversion) and runs ``network`` on the LayerNorm
NatureCNN node of ``cleanrl_amd/ln_cnn.py`` with the one-frame conv1 kernels (csrc/conv1q1.hip, csrc/conv1p1.hip) in ``act``,
``finish_rollout`` and ``update``: gx = ``AtariLSTMQNetwork.gates_fused``, the time-major ``mb_inds`` gather rides in conv1's loader.  The LSTM
scan, the act kernel, the TD kernel, clip + RAdam and the random streams are the same calls.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .learner_pqn import PQNLearner


class LSTMPQNLearner(PQNLearner):
    TRUNK_FRAME = (1, 84, 84)
    TRUNK_ROWS = (84, 84)            # (N, 1, 84, 84) and (N, 84, 84, 1) are the same bytes: no transposition

    def __init__(self, q_network: nn.Module, args, obs_shape, n_actions: int, num_envs: int, device, backend=None, trunk=None, obs_space=None):
        super().__init__(q_network, args, obs_shape, n_actions, num_envs, device, mlp=False, backend=backend, trunk=trunk, obs_space=obs_space)
        assert self.N % int(args.num_minibatches) == 0
        if self.fused and not (q_network.lstm.hidden_size == 128 and 1 <= self.A <= ops.PQN_MAX_ACTIONS):
            raise ValueError(f"MI355PPO_PQN=fused: the recurrent Q head takes LSTM(512, 128) and <= {ops.PQN_MAX_ACTIONS} actions, not "
                             f"{q_network.lstm.hidden_size} / {self.A}; use MI355PPO_PQN=torch")
        self.next_lstm_state = q_network.initial_state(self.N, self.device)
        self.initial_lstm_state = (self.next_lstm_state[0].clone(), self.next_lstm_state[1].clone())
        if self.fused:
            self._next_q = torch.zeros((self.N, self.A), dtype=torch.float32, device=self.device)

    # ------------------------------------------------------------------ rollout
    def _rows(self, frames):
        """Incoming (N, 1, 84, 84) uint8 frames -> (N, 84, 84) uint8 rows on the device: the same bytes, copied."""
        f = torch.as_tensor(np.asarray(frames) if not isinstance(frames, torch.Tensor) else frames)
        if f.dtype != torch.uint8 or tuple(f.shape) != (self.N,) + self.TRUNK_FRAME:
            raise ValueError(f"MI355PPO_PQN_TRUNK=fused takes ({self.N}, 1, 84, 84) uint8 frames, got {tuple(f.shape)} {f.dtype}")
        return f.to(self.device).contiguous().view(self.N, 84, 84)

    def _gates(self, obs, inds=None):
        """gx of ``obs`` (of ``obs[inds]``): the fused trunk on the uint8 rows, or the torch trunk on the f32 frames."""
        if self.fused_trunk:
            return self.net.gates_fused(self._ln, obs, inds)
        return self.net.gates(obs if inds is None else obs[inds])

    def act(self, step: int, force_action=None):
        """One step's action logic with the recurrent state; see ``PQNLearner.act`` for ``force_action``."""
        if step == 0:
            self.initial_lstm_state = (self.next_lstm_state[0].clone(), self.next_lstm_state[1].clone())
        self.global_step += self.N
        self.epsilon = epsilon = self._epsilon()
        if not self.fused:
            self.obs[step] = self.next_obs
            self.dones[step] = self.next_done
            random_actions = torch.randint(0, self.A, (self.N,)).to(self.device)
            with torch.no_grad():
                q_values, self.next_lstm_state = self.net(self.next_obs, self.next_lstm_state, self.next_done)
                max_actions = torch.argmax(q_values, dim=1)
                self.values[step] = q_values[torch.arange(self.N), max_actions].flatten()
            explore = torch.rand((self.N,)).to(self.device) < epsilon
            action = torch.where(explore, random_actions, max_actions)
            if force_action is not None:
                action = force_action.to(self.device, torch.int64)
            self.actions[step] = action
            return action
        self._rnd_host.copy_(torch.randint(0, self.A, (self.N,)))     # the reference's draws, in its order
        self._u_host.copy_(torch.rand((self.N,)))
        rnd, u = self._rnd_host, self._u_host
        if self.device.type == "cuda":
            self._rnd.copy_(self._rnd_host, non_blocking=True)
            self._u.copy_(self._u_host, non_blocking=True)
            rnd, u = self._rnd, self._u
        self.obs[step] = self.next_obs
        net = self.net
        with torch.no_grad():
            gx = self._gates(self.next_obs)
        h, c = self.next_lstm_state[0][0], self.next_lstm_state[1][0]         # (N, H) views: the state is advanced in place
        self.g.pqn_lstm_act(gx, net.lstm.weight_hh_l0.detach(), h, c, self.next_done, net.q_func.weight.detach(), net.q_func.bias.detach(),
                            rnd, u, epsilon, h_out=h, c_out=c, actions_out=self.actions[step], values_out=self.values[step],
                            action_i64_out=self._act, done_row_out=self.dones[step])
        if force_action is not None:
            self._act.copy_(force_action.to(torch.int64))
            self.actions[step] = self._act
        return self._act

    @torch.no_grad()
    def finish_rollout(self):
        """``# Compute Q(lambda) targets``: the bootstrap runs the network one more step and discards its state."""
        a, net = self.args, self.net
        if self.fused:
            h, c = self.next_lstm_state[0][0], self.next_lstm_state[1][0]
            self.g.pqn_lstm_act(self._gates(self.next_obs), net.lstm.weight_hh_l0, h, c, self.next_done, net.q_func.weight, net.q_func.bias,
                                q_out=self._next_q)
            self.returns = self.g.pqn_qlambda(self.rewards, self.dones, self.values, self.next_done, self._next_q, a.gamma, a.q_lambda)
            return self.returns
        returns = torch.zeros_like(self.rewards).to(self.device)
        for t in reversed(range(self.T)):
            if t == self.T - 1:
                next_value, _ = torch.max(net(self.next_obs, self.next_lstm_state, self.next_done)[0], dim=-1)
                nextnonterminal = 1.0 - self.next_done
                returns[t] = self.rewards[t] + a.gamma * next_value * nextnonterminal
            else:
                nextnonterminal = 1.0 - self.dones[t + 1]
                next_value = self.values[t + 1]
                returns[t] = self.rewards[t] + a.gamma * (a.q_lambda * returns[t + 1] + (1 - a.q_lambda) * next_value) * nextnonterminal
        self.returns = returns
        return returns

    # ------------------------------------------------------------------ update
    def update(self):
        a, net = self.args, self.net
        batch_size = self.T * self.N
        b_obs = self.obs.view(-1, 84, 84) if self.fused_trunk else self.obs.reshape((-1,) + self.obs_shape)
        b_actions = self.actions.reshape(-1)
        b_returns = self.returns.reshape(-1)
        b_dones = self.dones.reshape(-1)
        envsperbatch = self.N // int(a.num_minibatches)
        envinds = np.arange(self.N)
        flatinds = np.arange(batch_size).reshape(self.T, self.N)
        initial = self.initial_lstm_state
        scalars = None
        for epoch in range(a.update_epochs):
            np.random.shuffle(envinds)
            for start in range(0, self.N, envsperbatch):
                end = start + envsperbatch
                mbenvinds = envinds[start:end]
                mb_inds = flatinds[:, mbenvinds].ravel()  # be really careful about the index
                if not self.fused:
                    old_val, _ = net(b_obs[mb_inds], (initial[0][:, mbenvinds], initial[1][:, mbenvinds]), b_dones[mb_inds])
                    old_val = old_val.gather(1, b_actions[mb_inds].unsqueeze(-1).long()).squeeze()
                    loss = F.mse_loss(b_returns[mb_inds], old_val)
                    self.optimizer.zero_grad()
                    loss.backward()
                    nn.utils.clip_grad_norm_(net.parameters(), a.max_grad_norm)
                    self.optimizer.step()
                    continue
                mb = torch.from_numpy(mb_inds).to(self.device)
                env = torch.from_numpy(mbenvinds).to(self.device)
                if self.fused_trunk:
                    h, _ = net.states_from_gates(self._gates(b_obs, mb), (initial[0][:, env], initial[1][:, env]), b_dones[mb])
                else:
                    h, _ = net.states_fused(b_obs[mb], (initial[0][:, env], initial[1][:, env]), b_dones[mb])
                dh, scalars = self.g.pqn_lstm_td_fwd_bwd(h.detach(), mb, b_actions, b_returns, net.q_func.weight.detach(),
                                                         net.q_func.bias.detach(), net.q_func.weight.grad, net.q_func.bias.grad,
                                                         scalars=scalars)
                h.backward(dh)
                self.flat.step += 1
                self.g.clip_radam_(self.flat.params, self.flat.grads, self.flat.exp_avg, self.flat.exp_avg_sq, self.flat.step, self.lr,
                                   a.max_grad_norm)
                if self.fused_trunk:
                    self._ln.bufs.weights_version += 1              # the step wrote the flat buffer through raw pointers: re-derive the packs
        if not self.fused:
            return {"td_loss": loss.item(), "q_values": old_val.mean().item()}
        td_loss, q_values = scalars.tolist()
        return {"td_loss": td_loss, "q_values": q_values}
