"""rainbow_atari.py's prioritized n-step replay, twice: on the host by the reference's rules, and in device memory on the kernels
of csrc/rainbow.hip.  Both consume ``np.random`` as the reference's buffer does and are driven by the same calls:
``add(obs, action, reward, next_obs, done)``, ``sample(batch_size)``, ``update_priorities(indices, loss_per_sample)`` and a settable
``beta``.

The rules (the reference's ``PrioritizedReplayBuffer``; its min tree is written but never read, so neither buffer keeps one):

* two u8 arrays, ``obs`` and ``next_obs``, no memory-optimised aliasing;
* the n-step window emits nothing until ``n_step`` entries are held; the reward is ``sum gamma**i * r_i`` up to and including the
  first done, ``next_obs`` and ``done`` come from that entry; the window is cleared after a stored transition whose ``done`` is set;
* a new leaf gets ``max_priority ** alpha``; sampling is stratified, one ``np.random.uniform(a, b)`` per sample and the tree walk;
  weights are ``(size * p / p_total) ** -beta / max``; ``update_priorities`` takes ``abs + eps``, the running maximum and ``** alpha``.

``HostPrioritizedReplay`` keeps NumPy's float32 arithmetic, so its tree, indices and weights are the reference's bit for bit.
``DevicePrioritizedReplay`` keeps the rings, the tree, ``max_priority``, ``size`` and ``beta`` in device memory: ``sample`` uploads the
batch's draws and nothing between it and ``update_priorities`` reads the device back, so an update built on it can be captured.  Its
powers are ``pow`` in double rounded once (include/mi355ppo.h): leaves within 1 ulp of the host buffer's.  The n-step window stays
on the host on both: it works on one env step's host data.
"""
from __future__ import annotations

from collections import deque

import numpy as np
import torch

from . import ops
from .staging import Staging

__all__ = ["NStepAccumulator", "SumTree", "HostPrioritizedReplay", "DevicePrioritizedReplay"]


class NStepAccumulator:
    """The n-step window: ``push`` returns the transition to store, or None while fewer than ``n_step`` entries are held; the caller
    reports a stored transition's done through ``stored(done)``, which clears the window."""

    def __init__(self, n_step: int, gamma: float):
        self.n_step, self.gamma = n_step, gamma
        self.window = deque(maxlen=n_step)

    def push(self, obs, action, reward, next_obs, done):
        self.window.append((obs, action, reward, next_obs, done))
        if len(self.window) < self.n_step:
            return None
        ret, nxt, dn = 0.0, self.window[-1][3], self.window[-1][4]
        for i, (_, _, r, o, d) in enumerate(self.window):
            ret += self.gamma**i * r                      # in the dtype the env's reward brings, as the reference's line has it
            if d:
                nxt, dn = o, True
                break
        return self.window[0][0], self.window[0][1], ret, nxt, dn

    def stored(self, done):
        if done:
            self.window.clear()


class SumTree:
    """The reference's heap of ``2 * capacity - 1`` float32 words: leaf ``i`` is word ``capacity - 1 + i``."""

    def __init__(self, capacity: int):
        self.capacity = capacity
        self.tree = np.zeros(2 * capacity - 1, dtype=np.float32)

    def update(self, idx, value):
        node = idx + self.capacity - 1
        self.tree[node] = value
        while node > 0:
            node = (node - 1) // 2
            self.tree[node] = self.tree[2 * node + 1] + self.tree[2 * node + 2]

    def total(self):
        return self.tree[0]

    def retrieve(self, value):
        node = 0
        while 2 * node + 1 < len(self.tree):
            left = 2 * node + 1
            if value <= self.tree[left]:
                node = left
            else:
                value -= self.tree[left]                  # a float32 from here on: NumPy takes the Python float as weak
                node = left + 1
        return node - (self.capacity - 1)


class _Replay:
    def __init__(self, capacity, n_step, gamma, alpha, beta, eps):
        self.capacity, self.alpha, self.eps = capacity, alpha, eps
        self.pos = self.size = 0
        self.nstep = NStepAccumulator(n_step, gamma)
        self._beta = beta

    def add(self, obs, action, reward, next_obs, done):
        out = self.nstep.push(obs, action, reward, next_obs, done)
        if out is None:
            return False
        self._store(*out)
        self.pos = (self.pos + 1) % self.capacity
        self.size = min(self.size + 1, self.capacity)
        self.nstep.stored(out[4])
        return True


class HostPrioritizedReplay(_Replay):
    """The buffer on the host, in NumPy, by the rules of this module's docstring."""

    def __init__(self, capacity, obs_shape, n_step, gamma, alpha=0.6, beta=0.4, eps=1e-6):
        super().__init__(capacity, n_step, gamma, alpha, beta, eps)
        self.obs = np.zeros((capacity,) + tuple(obs_shape), dtype=np.uint8)
        self.next_obs = np.zeros((capacity,) + tuple(obs_shape), dtype=np.uint8)
        self.actions = np.zeros(capacity, dtype=np.int64)
        self.rewards = np.zeros(capacity, dtype=np.float32)
        self.dones = np.zeros(capacity, dtype=np.bool_)
        self.max_priority = 1.0
        self.sum_tree = SumTree(capacity)

    beta = property(lambda self: self._beta, lambda self, v: setattr(self, "_beta", v))

    def _store(self, obs, action, reward, next_obs, done):
        i = self.pos
        first = lambda x: np.asarray(x).reshape(-1)[0]  # noqa: E731
        self.obs[i], self.next_obs[i] = obs, next_obs
        self.actions[i], self.rewards[i], self.dones[i] = first(action), first(reward), first(done)
        self.sum_tree.update(i, self.max_priority**self.alpha)

    def sample(self, batch_size, u=None):
        """``u``: the batch's draws (B,) float64 for teacher forcing, used as ``np.random.uniform`` uses its one ``random_sample()``."""
        total = self.sum_tree.total()
        segment = total / batch_size

        def draw(i):
            lo, hi = segment * i, segment * (i + 1)
            return np.random.uniform(lo, hi) if u is None else float(lo) + (float(hi) - float(lo)) * float(u[i])

        indices = [self.sum_tree.retrieve(draw(i)) for i in range(batch_size)]
        probs = np.array([self.sum_tree.tree[i + self.capacity - 1] for i in indices])
        weights = (self.size * probs / total) ** -self._beta
        weights = weights / weights.max()
        return dict(observations=self.obs[indices], next_observations=self.next_obs[indices], actions=self.actions[indices],
                    rewards=self.rewards[indices], dones=self.dones[indices], indices=indices, weights=weights)

    def update_priorities(self, indices, priorities):
        priorities = np.abs(priorities) + self.eps
        self.max_priority = max(self.max_priority, priorities.max())
        for i, p in zip(indices, priorities):
            self.sum_tree.update(i, p**self.alpha)


class DevicePrioritizedReplay(_Replay):
    """The buffer in ``device`` memory (a CPU device runs the host twins of the same entry points).  Observations are (1, 4, 84, 84)
    u8 stacks of one env; the rings hold them channels-last.  ``sample`` returns tensors on ``device``: ``frames`` (2B, 84, 84, 4) u8,
    the B obs stacks and then the B next_obs stacks, ``actions`` int64, ``rewards`` / ``dones`` / ``weights`` f32 and ``indices``
    int64, all overwritten by the next ``sample``."""

    def __init__(self, capacity, device, n_step, gamma, alpha=0.6, beta=0.4, eps=1e-6):
        super().__init__(capacity, n_step, gamma, alpha, beta, eps)
        self.device = torch.device(device)
        self.g = ops.twins(self.device)
        try:
            self.buf = ops.rainbow_new_buffer(capacity, self.device, beta)
        except (RuntimeError, MemoryError) as e:
            gb = 2 * capacity * 84 * 84 * 4 / 1e9
            raise ValueError(f"buffer_size={capacity}: the two device frame rings need {gb:.1f} GB and could not be allocated ({e}); lower "
                             "--buffer-size or keep MI355PPO_OFFPOLICY=torch") from e
        self._batch = None
        self._stage = Staging(self.device, frames=((2, 1, 4, 84, 84), torch.uint8), act=((1,), torch.int64), rd=((2,), torch.float32))

    @property
    def beta(self):
        return self._beta

    @beta.setter
    def beta(self, v):
        self._beta = v
        self.buf[6][1:2].fill_(float(v))                  # read by the sample kernel from device memory

    def _store(self, obs, action, reward, next_obs, done):
        """One staged transition (``staging.Staging``: on a GPU three asynchronous copies) and one launch."""
        h = self._stage.begin()
        fh, rh = h["frames"], h["rd"]
        fh[0].copy_(torch.from_numpy(np.ascontiguousarray(obs, np.uint8)).reshape(fh[0].shape))
        fh[1].copy_(torch.from_numpy(np.ascontiguousarray(next_obs, np.uint8)).reshape(fh[1].shape))
        h["act"][0] = int(np.asarray(action).reshape(-1)[0])
        rh[0], rh[1] = float(np.float32(np.asarray(reward).reshape(-1)[0])), float(bool(np.asarray(done).reshape(-1)[0]))
        d = self._stage.push()
        self.g.rainbow_per_add_u8(self.buf, self.pos, d["frames"][0], d["frames"][1], d["act"], d["rd"][0:1], d["rd"][1:2], self.alpha)

    def _outputs(self, B):
        if self._batch is None or self._batch["indices"].numel() != B:
            z = lambda shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=self.device)  # noqa: E731
            self._batch = dict(u=z((B,), torch.float64), indices=z((B,), torch.int64), weights=z((B,)), frames=z((2 * B, 84, 84, 4), torch.uint8),
                               actions=z((B,), torch.int64), rewards=z((B,)), dones=z((B,)))
        return self._batch

    def sample(self, batch_size, u=None):
        """``u``: the batch's draws (B,) float64, for teacher forcing; by default ``np.random.random_sample(batch_size)``, which leaves
        ``np.random`` where the reference's ``batch_size`` calls of ``np.random.uniform`` leave it."""
        o = self._outputs(batch_size)
        u = np.random.random_sample(batch_size) if u is None else np.asarray(u, dtype=np.float64)
        o["u"].copy_(torch.from_numpy(u))
        self.g.rainbow_per_sample(self.buf, o["u"], o["indices"], o["weights"])
        self.g.rainbow_per_gather_u8(self.buf, o["indices"], o["frames"], o["actions"], o["rewards"], o["dones"])
        return o

    def update_priorities(self, indices, loss_per_sample):
        self.g.rainbow_per_update(self.buf, indices, loss_per_sample, self.alpha, self.eps)

    tree = property(lambda self: self.buf[5])
    max_priority = property(lambda self: self.buf[6][0].item())
