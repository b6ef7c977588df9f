"""The replay buffer, action logic and training step of ``dqn_atari.py`` and ``c51_atari.py`` (reference: cleanrl/dqn_atari.py,
cleanrl/c51_atari.py and ``ReplayBuffer(..., optimize_memory_usage=True, handle_timeout_termination=False)`` of cleanrl_utils/buffers.py).

====================================================  ==============================================================
reference                                              here
====================================================  ==============================================================
``ReplayBuffer(optimize_memory_usage=True)``           ``torch`` -- ``HostFrameBuffer`` (one u8 array, the reference's add / sample rules);
                                                       ``fused`` -- the u8 frame ring in device memory, channels-last, pinned staging
``random.random() < epsilon``, then ``sample()``       ``act``: the same two draws in the same order; greedy on ``fused``: the trunk and
per env or ``argmax(q_network(obs))`` /                ``Linear(3136, 512)`` on this library's kernels, then ``mi355ppo_dqn_head_act_f32``
``get_action(obs)``
``rb.add(obs, real_next_obs, ...)``                    ``store``: one staged copy + ``mi355ppo_replay_add_u8``
``rb.sample`` (skips ``pos`` when full)                ``sample_indices``
the update up to ``optimizer.step``                    ``train_step``: ``mi355ppo_replay_gather_u8``, target trunk + FC under ``no_grad``, online
                                                       trunk + FC under autograd, ``mi355ppo_dqn_head_td_fwd_bwd_f32`` /
                                                       ``mi355ppo_c51_head_fwd_bwd_f32`` (3 launches), ``h.backward(dh)`` into the flat gradient,
                                                       ``mi355ppo_clip_adam_f32`` (eps 1e-8 / ``0.01 / batch_size``)
the ``tau`` loop / ``load_state_dict``                 ``sync_target``: ``mi355ppo_polyak_f32`` / one flat copy
====================================================  ==============================================================

Backend: ``MI355PPO_OFFPOLICY=torch|fused``, default ``torch``.  Both backends draw ``random``, ``np.random`` and
the action space's stream in the reference's order.  On the CPU ``fused`` runs the host twins around torch's convolutions.

The flat buffers, the target update, the torch update and the logged scalars are ``learner_dqn.QLearner``'s.  ``check_frames`` and
``Trunks`` serve ``learner_rainbow.RainbowLearner`` too; ``FrameRing`` (the ring's allocation, its pinned staging through
``staging.Staging``, ``store``) serves ``learner_sac_atari.SACAtariLearner`` and ``learner_qdagger.QDaggerLearner`` too.
"""
from __future__ import annotations

import random

import numpy as np
import torch

from . import ops
from .learner_dqn import QLearner
from .learner_offpolicy import advance
from .staging import Staging

FRAME = (4, 84, 84)


def check_frames(envs):
    if tuple(envs.single_observation_space.shape) != FRAME:
        raise ValueError(f"the Atari learners take {FRAME} uint8 frame stacks, not {tuple(envs.single_observation_space.shape)}")


class Trunks(dict):
    """One ``cnn.NatureTrunk`` per key, made on first use.  A trunk keeps packed copies of its convolutions' weights: ``bump`` after
    every write to them."""

    def of(self, key):
        from . import cnn

        if key not in self:
            self[key] = cnn.NatureTrunk()
        return self[key]

    def bump(self):
        for trunk in self.values():
            trunk.bufs.weights_version += 1


class HostFrameBuffer:
    """The memory-optimised ``ReplayBuffer``: ONE u8 observation array; ``add`` writes obs to ``pos`` and next_obs to
    ``(pos + 1) % slots``; a sample's next_obs is the frame one slot on."""

    def __init__(self, buffer_size: int, device, n_envs: int = 1):
        self.slots, self.n_envs, self.device = max(int(buffer_size) // n_envs, 1), n_envs, device
        self.observations = np.zeros((self.slots, n_envs) + FRAME, np.uint8)
        self.actions = np.zeros((self.slots, n_envs, 1), np.int64)
        self.rewards = np.zeros((self.slots, n_envs), np.float32)
        self.dones = np.zeros((self.slots, n_envs), np.float32)
        self.pos, self.full = 0, False

    def add(self, obs, next_obs, action, reward, done):
        self.observations[self.pos] = np.array(obs)
        self.observations[(self.pos + 1) % self.slots] = np.array(next_obs)
        self.actions[self.pos] = np.array(action).reshape(self.n_envs, 1)
        self.rewards[self.pos] = np.array(reward)
        self.dones[self.pos] = np.array(done)
        advance(self)

    def gather(self, bi, ei):
        t = lambda a: torch.tensor(a, device=self.device)  # noqa: E731
        return (t(self.observations[bi, ei, :]), t(self.actions[bi, ei, :]), t(self.observations[(bi + 1) % self.slots, ei, :]),
                t(self.dones[bi, ei].reshape(-1, 1)), t(self.rewards[bi, ei].reshape(-1, 1)))


class FrameRing:
    """What the learners on u8 frame rings share, mixed in in front of a ``DeviceRing``: the ``fused`` ring with ``FRAME_ARRAYS`` frame
    arrays (1: the memory-optimised ring, next_obs one slot on; 2: ``observations`` and ``next_observations``), its staging groups
    (``staging.Staging``), the batch buffers, ``store`` and the staging of the rollout's frames."""

    FRAME_ARRAYS = 1

    def _alloc_ring(self, M: int):
        dev, N, K = self.device, self.N, self.FRAME_ARRAYS
        H, W, C = ops.ATARI_FRAME
        try:
            frames = tuple(torch.zeros((self.slots, N, H, W, C), dtype=torch.uint8, device=dev) for _ in range(K))
        except (RuntimeError, MemoryError) as e:
            raise ValueError(f"MI355PPO_OFFPOLICY=fused: {'a frame ring' if K == 1 else 'two frame rings'} of {self.slots} slots x {N} envs "
                             f"({K * self.slots * N * H * W * C / 1e9:.1f} GB) cannot be allocated on {dev}; lower --buffer-size or use "
                             f"MI355PPO_OFFPOLICY=torch") from e
        self.ring = frames + (torch.zeros((self.slots, N), dtype=torch.int64, device=dev), torch.zeros((self.slots, N), device=dev),
                              torch.zeros((self.slots, N), device=dev))
        # obs | next_obs as the env gives them, the actions, rewards | dones; the rollout's frames; the batch's draws
        self._step_stage = Staging(dev, frames=((2, N, C, H, W), torch.uint8), act=((N,), torch.int64), rd=((2, N), torch.float32))
        self._obs_stage = Staging(dev, frames=((N, C, H, W), torch.uint8))
        self._idx_stage = Staging(dev, idx=((2, M), torch.int64))
        self._obs_hwc = torch.zeros((N, H, W, C), dtype=torch.uint8, device=dev)
        self._batch = (torch.zeros((2 * M, H, W, C), dtype=torch.uint8, device=dev), torch.zeros(M, dtype=torch.int64, device=dev),
                       torch.zeros(M, device=dev), torch.zeros(M, device=dev))
        self._norm = torch.zeros(1, dtype=torch.float32, device=dev)

    def _stage_frames(self, obs):
        """The rollout's frames as (N, 84, 84, 4) u8 rows where the trunks read them."""
        self._obs_stage.begin()["frames"].copy_(torch.from_numpy(np.ascontiguousarray(obs, np.uint8)).reshape((self.N,) + FRAME))
        frames = self._obs_stage.push()["frames"]
        if self.device.type == "cuda":
            return ops.obs_nchw_to_nhwc_u8(frames, out=self._obs_hwc)
        return frames.permute(0, 2, 3, 1).contiguous()

    def store(self, obs, real_next_obs, actions, rewards, terminations):
        """``rb.add(obs, real_next_obs, actions, rewards, terminations, infos)``."""
        if not self.fused:
            self.rb.add(obs, real_next_obs, actions, rewards, terminations)
            self.pos, self.full = self.rb.pos, self.rb.full
            return
        h = self._step_stage.begin()
        fh, rh = h["frames"], h["rd"]
        fh[0].copy_(torch.from_numpy(np.ascontiguousarray(obs, np.uint8)).reshape(fh[0].shape))
        fh[1].copy_(torch.from_numpy(np.ascontiguousarray(real_next_obs, np.uint8)).reshape(fh[1].shape))
        h["act"].copy_(torch.from_numpy(np.asarray(actions, np.int64).reshape(-1)))
        rh[0].copy_(torch.from_numpy(np.asarray(rewards, np.float32).reshape(-1)))
        rh[1].copy_(torch.from_numpy(np.asarray(terminations, np.float32).reshape(-1)))
        d = self._step_stage.push()
        add = self.g.replay_add_u8 if self.FRAME_ARRAYS == 1 else self.g.replay_add2_u8
        add(self.ring, self.pos, d["frames"][0], d["frames"][1], d["act"], d["rd"][0], d["rd"][1])
        advance(self)


class AtariDQNLearner(FrameRing, QLearner):
    """``c51``: the networks are ``AtariC51Network`` (atoms, ``get_action``) and the update is the categorical one."""

    def __init__(self, q_network, target_network, args, envs, device, c51: bool, backend=None):
        self.c51 = bool(c51)
        self.n = int(envs.single_action_space.n)
        self.n_atoms = int(args.n_atoms) if self.c51 else 1
        check_frames(envs)
        super().__init__(q_network, target_network, args, envs, device, backend, 0.01 / args.batch_size if self.c51 else 1e-8)
        if not self.fused:
            return
        for p, off in self._param_offsets(q_network):                       # autograd accumulates into the flat gradient
            p.grad = self.grads[off:off + p.numel()].view(p.shape)
        J = self.n * self.n_atoms
        self.head_off = self.online.numel() - J * ops.DQN_HEAD_HIDDEN - J
        self.atoms = q_network.atoms.detach().to(self.device).contiguous() if self.c51 else None
        self._dh = torch.zeros((int(args.batch_size), ops.DQN_HEAD_HIDDEN), dtype=torch.float32, device=self.device)
        self._trunks = Trunks()

    def _host_buffer(self, act_dtype):
        return HostFrameBuffer(self.args.buffer_size, self.device, n_envs=self.N)

    def _check_sizes(self):
        if not ops.dqn_head_limits_ok(self.n, self.n_atoms, int(self.args.batch_size)) or (self.c51 and self.n_atoms < 2):
            raise ValueError(f"MI355PPO_OFFPOLICY=fused: the fused Q heads take 2 <= n_actions <= {ops.DQN_MAX_ACT}, n_atoms <= "
                             f"{ops.DQN_MAX_ATOMS} (at least 2 for c51), n_actions * n_atoms <= {ops.DQN_HEAD_MAX_OUT} and batch_size <= "
                             f"{ops.DQN_HEAD_MAX_ROWS}, not {self.n} / {self.n_atoms} / {self.args.batch_size}; use MI355PPO_OFFPOLICY=torch")

    # ------------------------------------------------------------------ the networks below the head
    def _hidden(self, net, frames_hwc):
        """``Linear(3136, 512)``'s ReLU output on (rows, 84, 84, 4) u8 rows: this library's trunk and FC on a GPU, torch's on the CPU."""
        seq = net.network
        if self.device.type != "cuda":
            return seq[:9](frames_hwc.permute(0, 3, 1, 2).float() / 255.0)
        from . import cnn

        trunk = self._trunks.of(id(net))
        feats = trunk(frames_hwc, None, seq[0], seq[2], seq[4])
        return cnn.LinearReLUHwcFn.apply(feats, seq[7].weight, seq[7].bias, trunk.bufs)

    def _head(self, flat):
        J = self.n * self.n_atoms
        w = flat[self.head_off:self.head_off + J * ops.DQN_HEAD_HIDDEN].view(J, ops.DQN_HEAD_HIDDEN)
        return w, flat[self.head_off + J * ops.DQN_HEAD_HIDDEN:]

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
            w, b = self._head(self.online)
            self.g.dqn_head_act(self._hidden(self.q_network, self._stage_frames(obs)).contiguous(), w, b, self.n, self._greedy, atoms=self.atoms)
            return self._copy_out(self._greedy)

    def sample_indices(self, batch_size: int):
        """The memory-optimised ``ReplayBuffer.sample``: never slot ``pos`` once full; then ``env_indices``."""
        if self.full:
            batch_inds = (np.random.randint(1, self.slots, size=batch_size) + self.pos) % self.slots
        else:
            batch_inds = np.random.randint(0, self.pos, size=batch_size)
        env_indices = np.random.randint(0, high=self.N, size=(len(batch_inds),))
        return batch_inds, env_indices

    # ------------------------------------------------------------------ training
    def train_step(self, indices=None):
        """One ``# ALGO LOGIC: training.`` block up to the optimizer step.  ``indices`` replaces the draws (teacher forcing)."""
        M = int(self.args.batch_size)
        bi, ei = self.sample_indices(M) if indices is None else indices
        if not self.fused:
            return self._train_torch(np.asarray(bi), np.asarray(ei))
        idx = self._stage_indices(bi, ei)
        self.update_kernels(idx[0], idx[1])
        self.last = ("fused",)
        return self

    def update_kernels(self, bi, ei, adam: bool = True, aux=None):
        """The update on device-resident indices: gather, both trunks, the head kernels, the backward below the head, Adam.  ``aux``:
        an optional pair of tensors for the target side's outputs (tests)."""
        a, g = self.args, self.g
        M = bi.numel()
        frames, actions, rewards, dones = self._batch
        g.replay_gather_u8(self.ring, bi, ei, frames, actions, rewards, dones)
        with torch.no_grad():
            h_next = self._hidden(self.target_network, frames[M:]).contiguous()
        h = self._hidden(self.q_network, frames[:M])
        hd = h.detach().contiguous()
        (w, b), (wt, bt), (dw, db) = self._head(self.online), self._head(self.target), self._head(self.grads)
        self.grads[:self.head_off].zero_()
        aux = aux or (None, None)
        if self.c51:
            g.c51_head_fwd_bwd(hd, h_next, w, b, wt, bt, self.atoms, actions, rewards, dones, self.n, a.gamma, a.v_min, a.v_max, self._dh, dw, db,
                               self._sc, *aux)
        else:
            g.dqn_head_td_fwd_bwd(hd, h_next, w, b, wt, bt, actions, rewards, dones, self.n, a.gamma, self._dh, dw, db, self._sc, *aux)
        h.backward(self._dh)
        if adam:
            self.step += 1
            self._adam(self._flats, self.step, a.learning_rate, self.eps)
            self._weights_changed(True, False)

    def _weights_changed(self, online: bool, target: bool):
        self._trunks.bump()
