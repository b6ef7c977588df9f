"""The rollout, episodic-memory bookkeeping and PPO update of ``ppo_trxl.py`` (reference: cleanrl/ppo_trxl/ppo_trxl.py, the main
loop after ``Agent``).

====================================================  ==============================================================
reference                                              here
====================================================  ==============================================================
storage setup, ``next_memory``, ``memory_mask``,       ``TrXLLearner.__init__``
``memory_indices``
learning-rate / entropy-coefficient annealing          ``start_iteration``
``stored_memories = [next_memory[e] ...]``             ``start_iteration``: the episode pool restarts with the envs'
                                                       current episodes
action logic, ``next_memory`` writes                   ``act``
episode end: clone the finished episode, zero the      ``observe`` -> ``_end_episodes``: the finished episode is
env's memory, index its new episode                    copied into its pool slot; a running one stays in ``next_memory``
bootstrap value (rows ``arange(start, end)``,          ``finish_rollout`` (GAE: K1 on the GPU, its host twin on CPU)
positions ``stored_memory_indices[-1]``) and GAE
flatten, ``actual_max_episode_steps`` trim,            ``update``
minibatch loss, AdamW, ``clip_grad_norm_``,
``target_kl``
====================================================  ==============================================================

The episode memories live in one pool tensor (``self.pool``, (episodes, T_ep, layers, D)) instead of a Python list of views
stacked before the update: the slot of an episode is the reference's ``stored_memory_index``.  With the ``torch`` backend the
minibatch windows are gathered as the reference gathers them; with ``fused`` the kernel reads the rows straight from the pool.
The loss and the optimizer stay torch ops (the loss has one policy term per action branch).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn as nn
import torch.optim as optim

from . import ops
from .agents import MemoryWindow, batched_index_select


class TrXLLearner:
    def __init__(self, agent, args, observation_space, action_space_shape, num_envs: int, max_episode_steps: int, device):
        self.agent, self.args, self.device = agent, args, torch.device(device)
        self.N, self.T, self.T_ep = int(num_envs), int(args.num_steps), int(max_episode_steps)
        self.action_space_shape = tuple(action_space_shape)
        self.optimizer = optim.AdamW(agent.parameters(), lr=args.init_lr)
        self.bce_loss = nn.BCELoss()
        dev, N, T, L = self.device, self.N, self.T, int(args.trxl_memory_length)
        self.L = L
        self.rewards = torch.zeros((T, N), device=dev)
        self.actions = torch.zeros((T, N, len(self.action_space_shape)), dtype=torch.long, device=dev)
        self.dones = torch.zeros((T, N), device=dev)
        self.obs = torch.zeros((T, N) + tuple(observation_space.shape), device=dev)
        self.log_probs = torch.zeros((T, N, len(self.action_space_shape)), device=dev)
        self.values = torch.zeros((T, N), device=dev)
        self.stored_memory_masks = torch.zeros((T, N, L), dtype=torch.bool, device=dev)
        self.stored_memory_index = torch.zeros((T, N), dtype=torch.long, device=dev)
        self.stored_memory_indices = torch.zeros((T, N, L), dtype=torch.long, device=dev)
        self.env_ids = torch.arange(N, device=dev)
        self.env_current_episode_step = torch.zeros((N,), dtype=torch.long, device=dev)
        self._episode_step = np.zeros(N, np.int64)                       # host copy: the done loop reads it without a sync
        layers, D = int(args.trxl_num_layers), int(args.trxl_dim)
        self.next_memory = torch.zeros((N, self.T_ep, layers, D), dtype=torch.float32, device=dev)
        self.memory_mask = torch.tril(torch.ones((L, L), device=dev), diagonal=-1)
        repetitions = torch.repeat_interleave(torch.arange(0, L, device=dev).unsqueeze(0), L - 1, dim=0).long()
        memory_indices = torch.stack([torch.arange(i, i + L, device=dev) for i in range(self.T_ep - L + 1)]).long()
        self.memory_indices = torch.cat((repetitions, memory_indices))
        # the episode pool: slot k holds episode k of the iteration once it has ended; a running episode lives in next_memory
        self._pool = torch.zeros((2 * N, self.T_ep, layers, D), dtype=torch.float32, device=dev)
        self._live = []                                                   # slot -> env whose next_memory holds it, or -1
        self._slot_of_env = np.arange(N)
        self.global_step = 0
        self.next_obs = None
        self.next_done = None

    # ------------------------------------------------------------------ episodes
    def reset(self, obs):
        self.next_obs = torch.Tensor(obs).to(self.device)
        self.next_done = torch.zeros(self.N, device=self.device)

    def start_iteration(self):
        """Annealing of the learning rate and entropy coefficient by global step; the pool restarts with the running episodes."""
        a = self.args
        do_anneal = a.anneal_steps > 0 and self.global_step < a.anneal_steps
        frac = 1 - self.global_step / a.anneal_steps if do_anneal else 0
        self.lr = (a.init_lr - a.final_lr) * frac + a.final_lr
        for param_group in self.optimizer.param_groups:
            param_group["lr"] = self.lr
        self.ent_coef = (a.init_ent_coef - a.final_ent_coef) * frac + a.final_ent_coef
        self._live = list(range(self.N))
        self._slot_of_env = np.arange(self.N)
        self.stored_memory_index.copy_(self.env_ids.unsqueeze(0).expand(self.T, self.N))

    def _new_slot(self):
        k = len(self._live)
        if k == self._pool.shape[0]:                                      # grow: rollout-time allocation only
            self._pool = torch.cat((self._pool, torch.zeros_like(self._pool)))
        self._live.append(-1)
        return k

    def _end_episodes(self, step, done_np):
        for id in np.flatnonzero(done_np):
            self._episode_step[id] = 0
            k = self._slot_of_env[id]
            self._pool[k].copy_(self.next_memory[id])                    # keep the finished episode
            self._live[k] = -1
            self.next_memory[id].zero_()
            if step < self.T - 1:
                k = self._new_slot()
                self._live[k] = int(id)
                self._slot_of_env[id] = k
                self.stored_memory_index[step + 1:, id] = k
        self._episode_step[~done_np] += 1
        self.env_current_episode_step.copy_(torch.from_numpy(self._episode_step))

    @property
    def pool(self):
        """(episodes, T_ep, layers, D): every episode of the iteration, running ones copied in (the reference's stacked list)."""
        for k, e in enumerate(self._live):
            if e >= 0:
                self._pool[k].copy_(self.next_memory[e])
                self._live[k] = -1
        return self._pool[:len(self._live)]

    # ------------------------------------------------------------------ rollout
    def _window(self, memory, rows):
        if self.agent.trxl_backend == "fused":
            return MemoryWindow(memory, self.env_ids, rows)
        return batched_index_select(memory, 1, rows)

    @torch.no_grad()
    def act(self, step: int, action=None):
        """The action logic of one step; ``action`` (N, branches) replaces the sample (teacher forcing)."""
        self.obs[step] = self.next_obs
        self.dones[step] = self.next_done
        self.stored_memory_masks[step] = self.memory_mask[torch.clip(self.env_current_episode_step, 0, self.L - 1)]
        self.stored_memory_indices[step] = self.memory_indices[self.env_current_episode_step]
        memory_window = self._window(self.next_memory, self.stored_memory_indices[step])
        action, logprob, _, value, new_memory = self.agent.get_action_and_value(
            self.next_obs, memory_window, self.stored_memory_masks[step], self.stored_memory_indices[step], action)
        self.next_memory[self.env_ids, self.env_current_episode_step] = new_memory
        self.actions[step], self.log_probs[step], self.values[step] = action, logprob, value
        return action

    def observe(self, step: int, next_obs, reward, terminations, truncations):
        self.global_step += self.N
        next_done = np.logical_or(terminations, truncations)
        self.rewards[step] = torch.tensor(reward).to(self.device).view(-1)
        self.next_obs, self.next_done = torch.Tensor(next_obs).to(self.device), torch.Tensor(next_done).to(self.device)
        self._end_episodes(step, np.asarray(next_done, dtype=bool))

    @torch.no_grad()
    def finish_rollout(self):
        """Bootstrap value (window rows ``arange(start, end)``, positions of the last stored step) and GAE."""
        a, L = self.args, self.L
        start = torch.clip(self.env_current_episode_step - L, 0)
        end = torch.clip(self.env_current_episode_step, L)
        indices = torch.stack([torch.arange(start[b], end[b], device=self.device) for b in range(self.N)]).long()
        next_value = self.agent.get_value(self.next_obs, self._window(self.next_memory, indices),
                                          self.memory_mask[torch.clip(self.env_current_episode_step, 0, L - 1)],
                                          self.stored_memory_indices[-1])
        self.advantages, self.returns = ops.twins(self.device).gae(self.rewards, self.dones, self.values, self.next_done, next_value, a.gamma, a.gae_lambda)

    # ------------------------------------------------------------------ update
    def update(self):
        a = self.args
        batch_size, minibatch_size = self.T * self.N, (self.T * self.N) // int(a.num_minibatches)
        b_obs = self.obs.reshape(-1, *self.obs.shape[2:])
        b_logprobs = self.log_probs.reshape(-1, *self.log_probs.shape[2:])
        b_actions = self.actions.reshape(-1, *self.actions.shape[2:])
        b_advantages = self.advantages.reshape(-1)
        b_returns = self.returns.reshape(-1)
        b_values = self.values.reshape(-1)
        b_memory_index = self.stored_memory_index.reshape(-1)
        b_memory_indices = self.stored_memory_indices.reshape(-1, *self.stored_memory_indices.shape[2:])
        b_memory_mask = self.stored_memory_masks.reshape(-1, *self.stored_memory_masks.shape[2:])
        stored_memories = self.pool
        fused = self.agent.trxl_backend == "fused"

        actual_max_episode_steps = (self.stored_memory_indices * self.stored_memory_masks).max().item() + 1
        self.trimmed = actual_max_episode_steps < self.L
        if self.trimmed:
            b_memory_indices = b_memory_indices[:, :actual_max_episode_steps]
            b_memory_mask = b_memory_mask[:, :actual_max_episode_steps]
            if not fused:                                                 # the kernel reads the untrimmed pool in place
                stored_memories = stored_memories[:, :actual_max_episode_steps]

        clipfracs = []
        for epoch in range(a.update_epochs):
            b_inds = torch.randperm(batch_size).to(self.device)             # the host generator on every device
            for start in range(0, batch_size, minibatch_size):
                end = start + minibatch_size
                mb_inds = b_inds[start:end]
                if fused:
                    mb_memory_windows = MemoryWindow(stored_memories, b_memory_index[mb_inds], b_memory_indices[mb_inds])
                else:
                    mb_memories = stored_memories[b_memory_index[mb_inds]]
                    mb_memory_windows = batched_index_select(mb_memories, 1, b_memory_indices[mb_inds])

                _, newlogprob, entropy, newvalue, _ = self.agent.get_action_and_value(
                    b_obs[mb_inds], mb_memory_windows, b_memory_mask[mb_inds], b_memory_indices[mb_inds], b_actions[mb_inds])

                mb_advantages = b_advantages[mb_inds]
                if a.norm_adv:
                    mb_advantages = (mb_advantages - mb_advantages.mean()) / (mb_advantages.std() + 1e-8)
                mb_advantages = mb_advantages.unsqueeze(1).repeat(1, len(self.action_space_shape))
                logratio = newlogprob - b_logprobs[mb_inds]
                ratio = torch.exp(logratio)
                pgloss1 = -mb_advantages * ratio
                pgloss2 = -mb_advantages * torch.clamp(ratio, 1.0 - a.clip_coef, 1.0 + a.clip_coef)
                pg_loss = torch.max(pgloss1, pgloss2).mean()

                v_loss_unclipped = (newvalue - b_returns[mb_inds]) ** 2
                if a.clip_vloss:
                    v_loss_clipped = b_values[mb_inds] + (newvalue - b_values[mb_inds]).clamp(min=-a.clip_coef, max=a.clip_coef)
                    v_loss = torch.max(v_loss_unclipped, (v_loss_clipped - b_returns[mb_inds]) ** 2).mean()
                else:
                    v_loss = v_loss_unclipped.mean()

                entropy_loss = entropy.mean()
                loss = pg_loss - self.ent_coef * entropy_loss + v_loss * a.vf_coef

                r_loss = torch.tensor(0.0, device=self.device)
                if a.reconstruction_coef > 0.0:
                    r_loss = self.bce_loss(self.agent.reconstruct_observation(), b_obs[mb_inds] / 255.0)
                    loss += a.reconstruction_coef * r_loss

                self.optimizer.zero_grad()
                loss.backward()
                torch.nn.utils.clip_grad_norm_(self.agent.parameters(), max_norm=a.max_grad_norm)
                self.optimizer.step()

                with torch.no_grad():
                    old_approx_kl = (-logratio).mean()
                    approx_kl = ((ratio - 1) - logratio).mean()
                    clipfracs += [((ratio - 1.0).abs() > a.clip_coef).float().mean().item()]

            if a.target_kl is not None and approx_kl > a.target_kl:
                break

        y_pred, y_true = b_values.cpu().numpy(), b_returns.cpu().numpy()
        var_y = np.var(y_true)
        explained_var = np.nan if var_y == 0 else 1 - np.var(y_true - y_pred) / var_y
        return {
            "policy_loss": pg_loss.item(), "value_loss": v_loss.item(), "loss": loss.item(), "entropy": entropy_loss.item(),
            "reconstruction_loss": r_loss.item(), "old_approx_kl": old_approx_kl.item(), "approx_kl": approx_kl.item(),
            "clipfrac": float(np.mean(clipfracs)), "explained_variance": float(explained_var),
            "value_mean": torch.mean(self.values).item(), "advantage_mean": torch.mean(self.advantages).item(),
            "learning_rate": self.lr, "entropy_coefficient": self.ent_coef, "actual_max_episode_steps": actual_max_episode_steps,
        }
