"""The replay buffer, action logic and training step of ``ddpg_continuous_action.py`` and ``td3_continuous_action.py`` (reference:
cleanrl/ddpg_continuous_action.py, cleanrl/td3_continuous_action.py and ``ReplayBuffer`` of cleanrl_utils/buffers.py).

====================================================  ==============================================================
reference                                              here
====================================================  ==============================================================
``optim.Adam`` x 2, ``ReplayBuffer(...,                ``OffPolicyLearner.__init__``: ``torch`` -- ``HostReplayBuffer`` + torch optimizers;
handle_timeout_termination=False)``                    ``fused`` -- the ring in device memory, flat parameter / gradient / Adam buffers
``single_action_space.sample()`` before                ``act``: ``fused`` -- one launch (``mi355ppo_ddpg_act_f32``) on the staged obs and
``learning_starts``, else ``actor(obs)`` +             the ``torch.normal`` row
``torch.normal(0, action_scale * exploration_noise)``,
numpy ``clip(low, high)``
``real_next_obs`` / ``rb.add(...)``                    ``store``: ``fused`` -- one staged copy + ``mi355ppo_replay_add_f32``
``rb.sample`` (``np.random.randint`` twice)            ``sample_indices`` (``upper_bound = buffer_size if full else pos``)
``with torch.no_grad():`` target block                 ``train_step``: ``mi355ppo_td3_target_f32`` (``torch.randn_like`` drawn here)
``qf*_a_values``, ``mse_loss``, ``backward``,          ``mi355ppo_td3_critic_fwd_bwd_f32`` (2 launches) + ``mi355ppo_clip_adam_f32``
``q_optimizer.step``                                   (grad_scale 1, max_grad_norm inf, eps 1e-8: 2 launches)
``actor_loss``, ``backward``,                          ``mi355ppo_td3_actor_fwd_bwd_f32`` (2 launches) + ``mi355ppo_clip_adam_f32``
``actor_optimizer.step``
the three Polyak loops                                 ``mi355ppo_polyak_f32`` over the flat buffers (1 launch)
``losses/*``                                           ``metrics`` (one device -> host copy when the script logs)
====================================================  ==============================================================

Backend: ``MI355PPO_OFFPOLICY=torch|fused``.  The default is ``torch`` on the CPU (``fused`` runs the host twins there) and on a GPU
(see DESIGN.md section 3.13 for why).  Both backends draw the reference's random streams in its order, so a fused run follows the
reference's trajectory for a seed up to rounding.  A TD3 step with the delayed update is 12 library launches on ``fused``.
``DeviceRing`` is the base class this learner shares with ``learner_sac.SACLearner`` and ``learner_dqn.DQNLearner``.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch
import torch.nn.functional as F
import torch.optim as optim

from . import ops
from .staging import Staging

BACKENDS = ("torch", "fused")


def offpolicy_backend(device) -> str:
    b = os.environ.get("MI355PPO_OFFPOLICY", "").strip().lower()
    if not b:
        return "torch"
    if b not in BACKENDS:
        raise ValueError(f"MI355PPO_OFFPOLICY={b!r}: expected one of {BACKENDS}")
    return b


class HostReplayBuffer:
    """``ReplayBuffer(buffer_size, ..., n_envs, handle_timeout_termination=False)``: numpy arrays of ``buffer_size // n_envs`` slots,
    ``pos`` / ``full``; ``sample`` draws ``batch_inds`` and then ``env_indices`` from ``np.random``."""

    def __init__(self, buffer_size: int, obs_dim: int, act_dim: int, device, n_envs: int = 1, act_dtype=np.float32):
        self.slots, self.n_envs, self.device = max(int(buffer_size) // n_envs, 1), n_envs, device
        self.observations = np.zeros((self.slots, n_envs, obs_dim), np.float32)
        self.next_observations = np.zeros((self.slots, n_envs, obs_dim), np.float32)
        self.actions = np.zeros((self.slots, n_envs, act_dim), act_dtype)     # int64 for a Discrete space (dqn.py, c51.py)
        self.rewards = np.zeros((self.slots, n_envs), np.float32)
        self.dones = np.zeros((self.slots, n_envs), np.float32)
        self.pos, self.full = 0, False

    def add(self, obs, next_obs, action, reward, done):
        self.observations[self.pos] = np.array(obs)
        self.next_observations[self.pos] = np.array(next_obs)
        self.actions[self.pos] = np.array(action).reshape(self.n_envs, -1)
        self.rewards[self.pos] = np.array(reward)
        self.dones[self.pos] = np.array(done)
        advance(self)

    def gather(self, bi, ei):
        t = lambda a: torch.tensor(a, device=self.device)  # noqa: E731
        return (t(self.observations[bi, ei, :]), t(self.actions[bi, ei, :]), t(self.next_observations[bi, ei, :]),
                t(self.dones[bi, ei].reshape(-1, 1)), t(self.rewards[bi, ei].reshape(-1, 1)))


def advance(ring):
    ring.pos += 1
    if ring.pos == ring.slots:
        ring.full, ring.pos = True, 0


class DeviceRing:
    """What the learners on the replay ring share.  ``__init__`` resolves the backend (``fused``), reads ``N`` / ``O`` from ``envs`` and
    sets ``space``, ``g`` (``ops.twins``), ``slots`` and ``pos`` / ``full``; then ``torch`` gets ``rb`` (a ``HostReplayBuffer``) and
    ``fused`` the ring: the five device arrays and three ``staging.Staging`` groups (a step's transition, its observations, a batch's
    indices; pinned and guarded on a GPU).  ``act_width``
    is the ring's action width ``A`` and ``act_dtype`` the host buffer's action dtype: ``prod(space.shape)`` / float32 for the
    continuous families, ``1`` / int64 for a Discrete space.  ``store``, ``sample_indices`` and the helpers of the flat parameter
    buffers (``_alloc_flat``, ``_adopt``, ``_adam``, ``_copy_out``, ``_flat``) are here once.  Base of ``OffPolicyLearner``,
    ``learner_sac.SACLearner`` and ``learner_dqn.DQNLearner``."""

    def __init__(self, args, envs, device, backend, act_width: int, act_dtype=np.float32):
        self.args, self.device = args, torch.device(device)
        self.backend = offpolicy_backend(self.device) if backend is None else backend
        if self.backend not in BACKENDS:
            raise ValueError(f"off-policy backend {self.backend!r}: expected one of {BACKENDS}")
        self.fused = self.backend == "fused"
        self.space = envs.single_action_space
        self.N = int(envs.num_envs)
        self.O = int(np.array(envs.single_observation_space.shape).prod())
        self.A = int(act_width)
        self.g = ops.twins(self.device)
        self.pos, self.full = 0, False
        self.slots = max(int(args.buffer_size) // self.N, 1)
        self.last = None
        if not self.fused:
            self.rb = self._host_buffer(act_dtype)
            return
        self._check_sizes()                                      # before anything of the ring's size is allocated
        self._alloc_ring(int(args.batch_size))

    def _host_buffer(self, act_dtype):
        """The ``torch`` backend's buffer (``learner_dqn_atari.AtariDQNLearner`` keeps frames as bytes instead)."""
        return HostReplayBuffer(self.args.buffer_size, self.O, self.A, self.device, n_envs=self.N, act_dtype=act_dtype)

    def _check_sizes(self):
        """The refusal of sizes the fused networks do not take: the continuous families' (``DQNLearner`` has its own limits)."""
        if not (1 <= self.O <= ops.OFFPOLICY_MAX_OBS and 1 <= self.A <= ops.OFFPOLICY_MAX_ACT):
            raise ValueError(f"MI355PPO_OFFPOLICY=fused: the fused networks take obs_dim <= {ops.OFFPOLICY_MAX_OBS} and act_dim <= "
                             f"{ops.OFFPOLICY_MAX_ACT}, not {self.O} / {self.A}; use MI355PPO_OFFPOLICY=torch")

    def _alloc_ring(self, M: int):
        dev, N, O, A = self.device, self.N, self.O, self.A
        self.ring = (torch.zeros((self.slots, N, O), device=dev), torch.zeros((self.slots, N, O), device=dev),
                     torch.zeros((self.slots, N, A), device=dev), torch.zeros((self.slots, N), device=dev),
                     torch.zeros((self.slots, N), device=dev))
        # the step's transition (obs | next_obs | actions | rewards | dones), the rollout's observations and the batch's draws
        self._step_stage = Staging(dev, step=((N * (2 * O + A + 2),), torch.float32))
        self._obs_stage = Staging(dev, obs=((N, O), torch.float32))
        self._idx_stage = Staging(dev, idx=((2, M), torch.int64))
        self._act = torch.zeros((N, A), dtype=torch.float32, device=dev)
        self._norm = torch.zeros(1, dtype=torch.float32, device=dev)

    # ------------------------------------------------------------------ the flat parameter / gradient / Adam buffers
    def _alloc_flat(self, total: int):
        """``online`` | ``grads`` | ``exp_avg`` | ``exp_avg_sq``, ``total`` floats each (``_flats``: the order ``_adam`` takes them in)."""
        self._flats = tuple(torch.zeros(total, dtype=torch.float32, device=self.device) for _ in range(4))
        self.online, self.grads, self.exp_avg, self.exp_avg_sq = self._flats

    @staticmethod
    def _adopt(nets, flat, off: int = 0) -> int:
        """The modules keep working: their parameters become views of ``flat`` from ``off`` on, in ``.parameters()`` order.  Returns
        the offset behind the last one."""
        with torch.no_grad():
            for net in nets:
                for p in net.parameters():
                    n = p.numel()
                    flat[off:off + n].copy_(p.reshape(-1))
                    p.data = flat[off:off + n].view(p.shape)
                    off += n
        return off

    def _adam(self, segs, step, lr, eps=1e-8):
        """One clip + Adam launch pair (grad_scale 1, max_grad_norm inf) over ``segs``, the four flat segments in ``_flats`` order.
        ``step`` is the step number or a device row of a schedule tensor (``clip_adam_sched_``; a device only: the host twins take
        the step as an argument)."""
        if torch.is_tensor(step):
            ops.clip_adam_sched_(*segs, step, math.inf, 1.0, eps=eps, total_norm_out=self._norm)
            return
        kw = {"total_norm_out": self._norm} if self.device.type == "cuda" else {}
        self.g.clip_adam_(*segs, step, lr, math.inf, 1.0, eps=eps, **kw)

    def _copy_out(self, buf):
        """The action kernel's reused output buffer as a numpy array the caller owns."""
        out = buf.cpu().numpy()
        return out if self.device.type == "cuda" else out.copy()          # on the CPU .cpu() aliases the reused buffer

    @staticmethod
    def _flat(nets):
        """The modules' parameters as one flat detached copy (``flat_params``)."""
        return torch.cat([p.detach().reshape(-1) for n in nets for p in n.parameters()]).clone()

    def _stage_obs(self, obs):
        """The rollout's observations (N, O) where the action kernel reads them."""
        self._obs_stage.begin()["obs"].copy_(torch.from_numpy(np.ascontiguousarray(obs, np.float32)).reshape(self.N, self.O))
        return self._obs_stage.push()["obs"]

    def _stage_indices(self, bi, ei):
        """The batch's (batch_inds, env_inds) as two int64 rows on the learner's device."""
        h = self._idx_stage.begin()["idx"]
        h[0].copy_(torch.from_numpy(np.asarray(bi, np.int64)))
        h[1].copy_(torch.from_numpy(np.asarray(ei, np.int64)))
        return self._idx_stage.push()["idx"]

    def store(self, obs, real_next_obs, actions, rewards, terminations):
        """``rb.add(obs, real_next_obs, actions, rewards, terminations, infos)``."""
        if not self.fused:
            self.rb.add(obs, real_next_obs, actions, rewards, terminations)
            self.pos, self.full = self.rb.pos, self.rb.full
            return
        N, O, A = self.N, self.O, self.A
        h = self._step_stage.begin()["step"]
        parts, off = [], 0
        for src, n in ((obs, N * O), (real_next_obs, N * O), (actions, N * A), (rewards, N), (terminations, N)):
            h[off:off + n].copy_(torch.from_numpy(np.ascontiguousarray(np.asarray(src).reshape(-1).astype(np.float32))))
            parts.append((off, n))
            off += n
        buf = self._step_stage.push()["step"]
        v = [buf[o:o + n] for o, n in parts]
        self.g.replay_add(self.ring, self.pos, v[0].view(N, O), v[1].view(N, O), v[2].view(N, A), v[3], v[4])
        advance(self)

    def sample_indices(self, batch_size: int):
        """``ReplayBuffer.sample`` / ``_get_samples``: ``batch_inds`` and then ``env_indices`` from ``np.random``."""
        upper_bound = self.slots if self.full else self.pos
        batch_inds = np.random.randint(0, upper_bound, size=batch_size)
        env_indices = np.random.randint(0, high=self.N, size=(len(batch_inds),))
        return batch_inds, env_indices


class OffPolicyLearner(DeviceRing):
    """``qfs`` / ``qf_targets``: one network (DDPG) or two (TD3).  ``td3``: target policy smoothing and the delayed update."""

    def __init__(self, actor, qfs, target_actor, qf_targets, args, envs, device, td3: bool, backend=None):
        super().__init__(args, envs, device, backend, int(np.prod(envs.single_action_space.shape)))
        self.actor, self.qfs, self.target_actor, self.qf_targets = actor, list(qfs), target_actor, list(qf_targets)
        self.td3 = bool(td3)
        self.ncrit = len(self.qfs)
        self.low = np.asarray(self.space.low, np.float32).reshape(-1)
        self.high = np.asarray(self.space.high, np.float32).reshape(-1)
        self.q_step = self.actor_step = 0
        if not self.fused:
            self.q_optimizer = optim.Adam([p for q in self.qfs for p in q.parameters()], lr=args.learning_rate)
            self.actor_optimizer = optim.Adam(list(actor.parameters()), lr=args.learning_rate)
            return
        dev = self.device
        self.pa, self.pq = ops.offpolicy_counts(self.O, self.A)
        self.q_off = (self.pa + 3) // 4 * 4                      # the critics start 16-byte aligned (the Adam kernel's float4s)
        total = self.q_off + self.ncrit * self.pq
        self._alloc_flat(total)
        self.target = torch.zeros(total, dtype=torch.float32, device=dev)
        for flat, a_net, q_nets in ((self.online, actor, self.qfs), (self.target, target_actor, self.qf_targets)):
            self._adopt([a_net], flat)
            self._adopt(q_nets, flat, self.q_off)
        self.scale = actor.action_scale.detach().reshape(-1).to(dev).contiguous()
        self.bias = actor.action_bias.detach().reshape(-1).to(dev).contiguous()
        self.low_t, self.high_t = torch.from_numpy(self.low.copy()).to(dev), torch.from_numpy(self.high.copy()).to(dev)
        M = int(args.batch_size)
        self._y = torch.zeros(M, dtype=torch.float32, device=dev)
        self._qsc = torch.zeros(2 * self.ncrit, dtype=torch.float32, device=dev)
        self._asc = torch.zeros(1, dtype=torch.float32, device=dev)

    # ------------------------------------------------------------------ views of the flat buffers
    def _seg(self, flat, which):
        if which == "actor":
            return flat[:self.pa]
        if which == "critics":
            return flat[self.q_off:self.q_off + self.ncrit * self.pq]
        return flat[self.q_off:self.q_off + self.pq]              # qf1

    # ------------------------------------------------------------------ rollout
    def act(self, obs, global_step: int):
        """The step's action (N, A) as a float32 numpy array."""
        a = self.args
        if global_step < a.learning_starts:
            return np.array([self.space.sample() for _ in range(self.N)])
        with torch.no_grad():
            if not self.fused:
                actions = self.actor(torch.Tensor(obs).to(self.device))
                actions += torch.normal(0, self.actor.action_scale * a.exploration_noise)
                return actions.cpu().numpy().clip(self.space.low, self.space.high)
            noise = torch.normal(0, self.actor.action_scale * a.exploration_noise).reshape(-1)
            self.g.ddpg_act(self._stage_obs(obs), self._seg(self.online, "actor"), self.scale, self.bias, noise, self.low_t, self.high_t, self._act)
            return self._copy_out(self._act)

    # ------------------------------------------------------------------ training
    def train_step(self, policy_update: bool, indices=None, noise=None):
        """One ``# ALGO LOGIC: training.`` block.  ``indices`` / ``noise`` replace the draws (teacher forcing)."""
        a = self.args
        M = int(a.batch_size)
        bi, ei = self.sample_indices(M) if indices is None else indices
        if not self.fused:
            return self._train_torch(bi, ei, policy_update, noise)
        dev = self.device
        if self.td3 and noise is None:
            noise = torch.randn((M, self.A), dtype=torch.float32, device=dev)     # torch.randn_like(data.actions)
        idx = self._stage_indices(bi, ei)
        self.update_kernels(idx[0], idx[1], noise, policy_update)
        self.last = ("fused", policy_update)
        return self

    def update_kernels(self, bi, ei, noise, policy_update: bool, adam: bool = True, sched=None):
        """The step's library launches on device-resident indices and noise (what a graph capture records).  With ``sched``, a
        (2, 2) float32 device tensor holding ``adam_schedules()``, both Adam steps read their step size and bias correction from
        it (``clip_adam_sched_``) and the caller advances ``q_step`` / ``actor_step``: the whole step then replays as one graph."""
        a, g = self.args, self.g
        lo0, hi0 = float(self.low[0]), float(self.high[0])
        g.td3_target(self.ring, bi, ei, self._seg(self.target, "actor"), self._seg(self.target, "critics"), self.ncrit, self.scale, self.bias,
                     noise if self.td3 else None, getattr(a, "policy_noise", 0.0), getattr(a, "noise_clip", 0.0), lo0, hi0, a.gamma, self._y)
        g.td3_critic_fwd_bwd(self.ring, bi, ei, self._seg(self.online, "critics"), self.ncrit, self._y, self._seg(self.grads, "critics"),
                             self._qsc)
        if adam:
            if sched is None:
                self.q_step += 1
            self._adam_seg("critics", self.q_step if sched is None else sched[0])
        if policy_update:
            g.td3_actor_fwd_bwd(self.ring, bi, ei, self._seg(self.online, "actor"), self._seg(self.online, "qf1"), self.scale, self.bias,
                                self._seg(self.grads, "actor"), self._asc)
            if adam:
                if sched is None:
                    self.actor_step += 1
                self._adam_seg("actor", self.actor_step if sched is None else sched[1])
            g.polyak_(self.online, self.target, a.tau)

    def _adam_seg(self, which, step):
        self._adam([self._seg(f, which) for f in self._flats], step, self.args.learning_rate)

    def adam_schedules(self):
        """(2, 2) host tensor: the library's (step size, bias correction) of the NEXT critic and actor Adam steps."""
        lr = self.args.learning_rate
        return torch.tensor([ops.adam_schedule(lr, self.q_step + 1), ops.adam_schedule(lr, self.actor_step + 1)], dtype=torch.float32)

    def _train_torch(self, bi, ei, policy_update, noise):
        a, dev = self.args, self.device
        obs, actions, next_obs, dones, rewards = self.rb.gather(bi, ei)
        with torch.no_grad():
            if self.td3:
                if noise is None:
                    noise = torch.randn_like(actions, device=dev)
                clipped_noise = (noise * a.policy_noise).clamp(-a.noise_clip, a.noise_clip) * self.target_actor.action_scale
                next_state_actions = (self.target_actor(next_obs) + clipped_noise).clamp(self.space.low[0], self.space.high[0])
            else:
                next_state_actions = self.target_actor(next_obs)
            next_target = self.qf_targets[0](next_obs, next_state_actions)
            if self.ncrit == 2:
                next_target = torch.min(next_target, self.qf_targets[1](next_obs, next_state_actions))
            next_q_value = rewards.flatten() + (1 - dones.flatten()) * a.gamma * (next_target).view(-1)
        q_values = [q(obs, actions).view(-1) for q in self.qfs]
        q_losses = [F.mse_loss(v, next_q_value) for v in q_values]
        qf_loss = q_losses[0] + q_losses[1] if self.ncrit == 2 else q_losses[0]
        self.q_optimizer.zero_grad()
        qf_loss.backward()
        self.q_optimizer.step()
        self.q_step += 1
        if policy_update:
            actor_loss = -self.qfs[0](obs, self.actor(obs)).mean()
            self.actor_optimizer.zero_grad()
            actor_loss.backward()
            self.actor_optimizer.step()
            self.actor_step += 1
            with torch.no_grad():
                for net, tgt in zip([self.actor] + self.qfs, [self.target_actor] + self.qf_targets):
                    for param, target_param in zip(net.parameters(), tgt.parameters()):
                        target_param.data.copy_(a.tau * param.data + (1 - a.tau) * target_param.data)
            self._actor_loss = actor_loss.detach()
        self.last = ("torch", q_values, q_losses, qf_loss)
        self.next_q_value = next_q_value
        return self

    def metrics(self) -> dict:
        """The last step's scalars as Python floats (the script's ``losses/*``); ``actor_loss`` is the last policy update's."""
        out = {}
        if self.last[0] == "torch":
            _, q_values, q_losses, qf_loss = self.last
            for i in range(self.ncrit):
                out[f"qf{i + 1}_values"] = q_values[i].mean().item()
                out[f"qf{i + 1}_loss"] = q_losses[i].item()
            out["qf_loss"] = qf_loss.item()
            if self.actor_step:
                out["actor_loss"] = self._actor_loss.item()
            return out
        sc = self._qsc.tolist()
        for i in range(self.ncrit):
            out[f"qf{i + 1}_values"], out[f"qf{i + 1}_loss"] = sc[2 * i], sc[2 * i + 1]
        out["qf_loss"] = float(np.float32(sc[1]) + np.float32(sc[3])) if self.ncrit == 2 else sc[1]
        if self.actor_step:
            out["actor_loss"] = self._asc.item()
        return out

    def flat_params(self):
        """(actor, critics) flat parameters, detached copies (tests)."""
        return self._flat([self.actor]), self._flat(self.qfs)
