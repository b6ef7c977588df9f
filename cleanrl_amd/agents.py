"""The reference's three ``Agent`` networks with identical structure, parameter names, initialisation
order (hence identical weights for a given torch seed) and method surface:

* ``AtariAgent``      -- NatureCNN, ppo_atari_multigpu.py:133-159 (== ppo_atari.py, ppo_atari_envpool.py)
* ``MlpAgent``        -- 64-64 tanh actor/critic, ppo.py:100-126
* ``ContinuousAgent`` -- 64-64 tanh + state-independent logstd, ppo_continuous_action.py:112-141

``get_value`` / ``get_action_and_value`` keep the reference signatures.  On a CUDA (HIP) device the
distribution math (sample / log_prob / entropy) runs in the libmi355ppo kernels; on an explicit CPU
device (``--no-cuda``, config A plumbing, gloo tests) it is ``torch.distributions`` exactly as in the
reference.  The learner's update does not go through these methods: it feeds the network outputs to the
fused loss kernel (``heads``/``dist_params`` below are the seam).
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.distributions.categorical import Categorical
from torch.distributions.normal import Normal

from . import ops


def layer_init(layer, std=np.sqrt(2), bias_const=0.0):
    torch.nn.init.orthogonal_(layer.weight, std)
    torch.nn.init.constant_(layer.bias, bias_const)
    return layer


class _SampleCounter:
    """(seed, offset) for the Philox streams of the sampling kernels: one fresh offset per call."""

    def __init__(self):
        self.seed, self.offset = 0, 0

    def next(self):
        self.offset += 1
        return self.seed, self.offset

    def reserve(self, n: int) -> int:
        """Set ``n`` offsets aside and return the first one: the env-group lanes of a rollout (pipeline.py) draw
        ``first + step * groups + group`` so that their streams do not depend on which lane's thread runs first."""
        first = self.offset + 1
        self.offset += int(n)
        return first


def fused_mlp_ptrs(agent):
    """``(actor MlpNetPtrs, critic MlpNetPtrs)`` of an agent whose two networks the fused MLP kernels cover (64-64 tanh,
    obs_dim <= 512, n_out <= 20, f32 on a HIP device), else None.  Rebuilt when the parameters moved (``.to()``, flat buffers)."""
    import os

    if os.environ.get("MI355PPO_MLP", "fused") == "torch":       # A/B: keep the networks on library GEMMs
        return None
    actor, critic = agent.mlp_nets()
    w = actor[0].weight
    if not w.is_cuda or w.dtype != torch.float32:
        return None
    key = tuple(p.data_ptr() for p in list(actor.parameters()) + list(critic.parameters()))
    if agent._fused is None or agent._fused[0] != key:
        try:
            a, c = ops.MlpNetPtrs(actor), ops.MlpNetPtrs(critic)
        except AssertionError:
            agent._fused = (key, None)
            return None
        ok = ops.mlp_supported(a.obs_dim, a.n_out) and c.n_out == 1 and c.obs_dim == a.obs_dim
        agent._fused = (key, (a, c) if ok else None)
    return agent._fused[1]


def _fused_mlp(agent, x):
    """The fused forward applies when no autograd graph is being recorded (rollout, bootstrap value) on a HIP device."""
    if not x.is_cuda or x.dim() != 2 or x.dtype != torch.float32:
        return None
    if torch.is_grad_enabled() and any(p.requires_grad for p in agent.parameters()):
        return None
    return fused_mlp_ptrs(agent)


class _DiscreteMixin:
    discrete = True

    def _dist(self, logits, action):
        if logits.is_cuda:
            if action is None:
                seed, off = self.rng.next()
                a64, _, lp, ent = ops.categorical_sample(logits.contiguous(), seed=seed, offset=off)
                return a64, lp, ent
            if torch.is_grad_enabled() and logits.requires_grad:
                lp, ent = ops.CategoricalLogProbEntropy.apply(logits, action)
            else:
                lp, ent = ops.categorical_logprob_entropy(logits.contiguous(), action.contiguous())
            return action, lp, ent
        probs = Categorical(logits=logits)
        if action is None:
            action = probs.sample()
        return action, probs.log_prob(action), probs.entropy()


class _NatureTrunkMixin:
    """The fast path of the agents whose ``network`` is the NatureCNN (three Conv2d + ReLU, Flatten, Linear(3136, 512) + ReLU): uint8 rollout
    rows straight into the libmi355ppo kernels (cleanrl_amd/cnn.py: gather, /255, bias, ReLU and their backward fused)."""

    _trunk = None                 # cnn.NatureTrunk: made on first use, or by the learner that owns its buffers (PPOLearner._owned_trunk)

    def _nature_trunk(self):
        from . import cnn

        if self._trunk is None:
            self._trunk = cnn.NatureTrunk()
        net = self.network
        if net[7].out_features == 512:      # the all-packs launch is sized for Linear(3136, 512); RNDAgent's 256 rows derive pack by pack
            self._trunk.bufs.pack_params = (net[0].weight, net[2].weight, net[4].weight, net[7].weight)
        return self._trunk

    def _hidden_u8(self, obs_rows, inds=None, ind=None):
        """``network`` on the rows ``obs_rows[inds]`` (``ind``: ``MAAtariAgent.heads_u8``) -> (M, 512)."""
        from . import cnn

        trunk, net = self._nature_trunk(), self.network
        feats = trunk(obs_rows, inds, net[0], net[2], net[4], ind=ind)
        return cnn.LinearReLUHwcFn.apply(feats, net[7].weight, net[7].bias, trunk.bufs)

    def _heads_u8(self, obs_rows, inds=None, ind=None):
        from . import cnn

        hidden = self._hidden_u8(obs_rows, inds, ind)
        if cnn.heads_supported(self.actor, self.critic):
            return cnn.HeadsFn.apply(hidden, self.actor.weight, self.actor.bias, self.critic.weight, self.critic.bias, self._trunk.bufs)
        return self.actor(hidden), self.critic(hidden)      # > 18 actions: library GEMMs

    def _act_u8(self, obs_rows, ind, seed, offset, offset_base, action_f32_out, logprob_out, value_out, want_i64):
        """The rollout step on uint8 rows (no autograd graph): trunk, then Linear(3136,512) + heads + Categorical draw in two launches
        (``cnn.fc_heads_act_categorical``).  None when the fused step does not apply (wide action spaces, huge batches)."""
        from . import cnn

        trunk, net = self._nature_trunk(), self.network
        if torch.is_grad_enabled() or not cnn.heads_supported(self.actor, self.critic) or not cnn.fc_heads_act_supported_rows(obs_rows.shape[0]):
            return None                                   # (decided before the trunk runs: the caller's fallback computes it)
        feats = trunk(obs_rows, None, net[0], net[2], net[4], ind=ind)
        if not cnn.fc_heads_act_supported(feats):
            return None
        bufs = trunk.bufs
        return cnn.fc_heads_act_categorical(feats, bufs.fc_pack_fwd(net[7].weight), net[7].bias.detach().contiguous(),
                                            self.actor.weight.detach(), self.actor.bias.detach(), self.critic.weight.detach(),
                                            self.critic.bias.detach(), seed, offset, offset_base, action_f32_out, logprob_out, value_out,
                                            want_i64=want_i64, amax=bufs.rec_of(cnn.REC_A3, feats) if bufs.f16(feats) else None)


class AtariAgent(_NatureTrunkMixin, _DiscreteMixin, nn.Module):
    obs_is_image = True

    def __init__(self, envs):
        super().__init__()
        self.network = nn.Sequential(
            layer_init(nn.Conv2d(4, 32, 8, stride=4)),
            nn.ReLU(),
            layer_init(nn.Conv2d(32, 64, 4, stride=2)),
            nn.ReLU(),
            layer_init(nn.Conv2d(64, 64, 3, stride=1)),
            nn.ReLU(),
            nn.Flatten(),
            layer_init(nn.Linear(64 * 7 * 7, 512)),
            nn.ReLU(),
        )
        self.actor = layer_init(nn.Linear(512, envs.single_action_space.n), std=0.01)
        self.critic = layer_init(nn.Linear(512, 1), std=1)
        self.n_actions = envs.single_action_space.n
        self.rng = _SampleCounter()

    def _normalise(self, x):
        if x.dtype == torch.uint8:
            return ops.obs_u8_to_f32(x.contiguous()) if x.is_cuda else x.float() / 255.0
        return x / 255.0

    def heads(self, xn):
        """xn: already-normalised f32 observations -> (logits (B,A), value (B,1))."""
        hidden = self.network(xn)
        return self.actor(hidden), self.critic(hidden)

    def heads_u8(self, obs_rows, inds=None):
        """The learner's fast path: ``obs_rows`` is the uint8 rollout buffer in its pixel-interleaved layout
        (rows, 84, 84, 4) and ``inds`` optionally gathers rows (``b_obs[mb_inds]``).  Same function as
        ``heads(obs / 255.0)`` with the three convolutions on the libmi355ppo f32-MFMA kernels (gather, /255, bias,
        ReLU and the ReLU / bias backward fused; cleanrl_amd/cnn.py); the two Linear layers stay on hipBLASLt."""
        return self._heads_u8(obs_rows, inds)

    def act_u8(self, obs_rows, seed, offset, offset_base=None, action_f32_out=None, logprob_out=None, value_out=None, want_i64=True):
        """The learner's rollout step on uint8 rows (``_act_u8``)."""
        return self._act_u8(obs_rows, None, seed, offset, offset_base, action_f32_out, logprob_out, value_out, want_i64)

    def get_value(self, x):
        return self.critic(self.network(self._normalise(x)))

    def get_action_and_value(self, x, action=None):
        logits, value = self.heads(self._normalise(x))
        action, lp, ent = self._dist(logits, action)
        return action, lp, ent, value


class MlpAgent(_DiscreteMixin, nn.Module):
    obs_is_image = False

    def __init__(self, envs):
        super().__init__()
        obs_dim = int(np.array(envs.single_observation_space.shape).prod())
        self.critic = nn.Sequential(
            layer_init(nn.Linear(obs_dim, 64)),
            nn.Tanh(),
            layer_init(nn.Linear(64, 64)),
            nn.Tanh(),
            layer_init(nn.Linear(64, 1), std=1.0),
        )
        self.actor = nn.Sequential(
            layer_init(nn.Linear(obs_dim, 64)),
            nn.Tanh(),
            layer_init(nn.Linear(64, 64)),
            nn.Tanh(),
            layer_init(nn.Linear(64, envs.single_action_space.n), std=0.01),
        )
        self.n_actions = envs.single_action_space.n
        self.rng = _SampleCounter()
        self._fused = None

    def mlp_nets(self):
        """(actor, critic) ``nn.Sequential`` pair: the seam of the fused MLP kernels (csrc/mlp.hip)."""
        return self.actor, self.critic

    def heads(self, x):
        f = _fused_mlp(self, x)
        if f is not None:                      # no autograd graph wanted: both networks in one launch
            logits, value = ops.mlp_forward(x.contiguous(), *f)
            return logits, value.unsqueeze(1)
        return self.actor(x), self.critic(x)

    def get_value(self, x):
        f = _fused_mlp(self, x)
        if f is not None:
            return ops.mlp_forward(x.contiguous(), *f)[1].unsqueeze(1)
        return self.critic(x)

    def get_action_and_value(self, x, action=None):
        f = _fused_mlp(self, x) if action is None else None
        if f is not None:                      # rollout step: forwards + sample + log_prob + entropy in one launch
            seed, off = self.rng.next()
            a64, _, lp, ent, value, _ = ops.mlp_act_categorical(x.contiguous(), *f, seed=seed, offset=off, want_entropy=True)
            return a64, lp, ent, value.unsqueeze(1)
        logits, value = self.heads(x)
        action, lp, ent = self._dist(logits, action)
        return action, lp, ent, value


class ContinuousAgent(nn.Module):
    obs_is_image = False
    discrete = False

    def __init__(self, envs, rpo_alpha=None):
        super().__init__()
        self.rpo_alpha = rpo_alpha      # rpo_continuous_action.py:109-111: perturb the mean when re-evaluating actions
        obs_dim = int(np.array(envs.single_observation_space.shape).prod())
        act_dim = int(np.prod(envs.single_action_space.shape))
        self.critic = nn.Sequential(
            layer_init(nn.Linear(obs_dim, 64)),
            nn.Tanh(),
            layer_init(nn.Linear(64, 64)),
            nn.Tanh(),
            layer_init(nn.Linear(64, 1), std=1.0),
        )
        self.actor_mean = nn.Sequential(
            layer_init(nn.Linear(obs_dim, 64)),
            nn.Tanh(),
            layer_init(nn.Linear(64, 64)),
            nn.Tanh(),
            layer_init(nn.Linear(64, act_dim), std=0.01),
        )
        self.actor_logstd = nn.Parameter(torch.zeros(1, act_dim))
        self.act_dim = act_dim
        self.rng = _SampleCounter()
        self._fused = None

    def mlp_nets(self):
        """(actor_mean, critic) ``nn.Sequential`` pair: the seam of the fused MLP kernels (csrc/mlp.hip)."""
        return self.actor_mean, self.critic

    def heads(self, x):
        f = _fused_mlp(self, x)
        if f is not None:
            mean, value = ops.mlp_forward(x.contiguous(), *f)
            return mean, value.unsqueeze(1)
        return self.actor_mean(x), self.critic(x)

    def get_value(self, x):
        f = _fused_mlp(self, x)
        if f is not None:
            return ops.mlp_forward(x.contiguous(), *f)[1].unsqueeze(1)
        return self.critic(x)

    def perturb_mean(self, mean):
        """rpo_continuous_action.py:138-142: ``action_mean + U(-alpha, alpha)`` (only when actions are re-evaluated)."""
        if self.rpo_alpha is None:
            return mean
        return mean + torch.empty_like(mean).uniform_(-self.rpo_alpha, self.rpo_alpha)

    def get_action_and_value(self, x, action=None):
        f = _fused_mlp(self, x) if action is None else None
        if f is not None:                      # rollout step: forwards + sample + log_prob + entropy in one launch
            seed, off = self.rng.next()
            act, lp, ent, value, _ = ops.mlp_act_normal(x.contiguous(), *f, self.actor_logstd.detach(), seed=seed, offset=off,
                                                        want_entropy=True)
            return act, lp, ent, value.unsqueeze(1)
        mean, value = self.heads(x)
        if action is not None:
            mean = self.perturb_mean(mean)
        if mean.is_cuda:
            if action is None:
                seed, off = self.rng.next()
                action, lp, ent = ops.normal_sample(mean.contiguous(), self.actor_logstd, seed=seed, offset=off)
            elif torch.is_grad_enabled() and (mean.requires_grad or self.actor_logstd.requires_grad):
                lp, ent = ops.NormalLogProbEntropy.apply(mean, self.actor_logstd, action)
            else:
                lp, ent = ops.normal_logprob_entropy(mean.contiguous(), self.actor_logstd, action.contiguous())
            return action, lp, ent, value
        action_logstd = self.actor_logstd.expand_as(mean)
        probs = Normal(mean, torch.exp(action_logstd))
        if action is None:
            action = probs.sample()
        return action, probs.log_prob(action).sum(1), probs.entropy().sum(1), value


LSTM_BACKENDS = ("torch", "fused")


def lstm_backend_from_env() -> str:
    """``MI355PPO_LSTM``: ``torch`` (default: the reference's per-step ``nn.LSTM`` loop) or ``fused`` (the sequence scans of
    csrc/lstm.hip, ``ops.lstm_seq``)."""
    v = os.environ.get("MI355PPO_LSTM", "torch")
    if v not in LSTM_BACKENDS:
        raise ValueError(f"MI355PPO_LSTM={v!r}: expected torch or fused")
    return v


LSTM_TRUNKS = ("torch", "fused")


def lstm_trunk_backend_from_env() -> str:
    """``MI355PPO_LSTM_TRUNK``: ``torch`` (default: ``AtariLSTMAgent.network`` on torch's Conv2d / Linear behind the K5 gather + convert
    kernel) or ``fused`` (HIP learner only: the one-frame NatureCNN kernels of ``cnn.NatureTrunkFn`` on the uint8 rollout rows)."""
    v = os.environ.get("MI355PPO_LSTM_TRUNK", "torch")
    if v not in LSTM_TRUNKS:
        raise ValueError(f"MI355PPO_LSTM_TRUNK={v!r}: expected torch or fused")
    return v


class AtariLSTMAgent(_NatureTrunkMixin, _DiscreteMixin, nn.Module):
    """ppo_atari_lstm.py:117-165: NatureCNN on ONE 84x84 frame -> Linear(3136,512) -> LSTM(512,128) -> actor / critic.
    Same construction order as the reference (network layers, ``nn.LSTM`` default init, then bias := 0 and orthogonal
    weights in ``named_parameters`` order, then actor, critic), hence the same weights for the same torch seed.
    The recurrent state is reset where ``done`` is 1, one time step at a time, exactly as ``get_states`` (:138-156).
    ``lstm_backend`` (from ``MI355PPO_LSTM`` at construction; tests may set the attribute): ``torch`` runs that loop, ``fused``
    runs all T steps as one scan (``ops.lstm_seq``: HIP kernels on the GPU, their host twins on CPU)."""

    obs_is_image = True
    recurrent = True

    def __init__(self, envs):
        super().__init__()
        self.network = nn.Sequential(
            layer_init(nn.Conv2d(1, 32, 8, stride=4)),
            nn.ReLU(),
            layer_init(nn.Conv2d(32, 64, 4, stride=2)),
            nn.ReLU(),
            layer_init(nn.Conv2d(64, 64, 3, stride=1)),
            nn.ReLU(),
            nn.Flatten(),
            layer_init(nn.Linear(64 * 7 * 7, 512)),
            nn.ReLU(),
        )
        self.lstm = nn.LSTM(512, 128)
        for name, param in self.lstm.named_parameters():
            if "bias" in name:
                nn.init.constant_(param, 0)
            elif "weight" in name:
                nn.init.orthogonal_(param, 1.0)
        self.actor = layer_init(nn.Linear(128, envs.single_action_space.n), std=0.01)
        self.critic = layer_init(nn.Linear(128, 1), std=1)
        self.n_actions = envs.single_action_space.n
        self.rng = _SampleCounter()
        self.lstm_backend = lstm_backend_from_env()

    def _normalise(self, x):
        if x.dtype == torch.uint8:
            return ops.obs_u8_to_f32(x.contiguous()) if x.is_cuda else x.float() / 255.0
        return x / 255.0

    def heads_seq_u8(self, obs_rows, inds, lstm_state, done):
        """``heads_seq`` on the uint8 rollout rows (rows, 84, 84, 1), ``inds`` optionally gathering them time-major (``b_obs[mb_inds]``):
        the three convolutions and Linear(3136,512) on the libmi355ppo kernels (gather, /255, bias, ReLU and their backward fused;
        conv1 on kernels Q1 / P1, cleanrl_amd/cnn.py), then the same LSTM seam (either ``lstm_backend``) and the torch heads."""
        hidden, lstm_state = self.states_from_features(self._hidden_u8(obs_rows, inds), lstm_state, done)
        return self.actor(hidden), self.critic(hidden), lstm_state

    def initial_state(self, num_envs: int, device):
        """(:225-228) zero hidden and cell state, (num_layers, N, hidden)."""
        shape = (self.lstm.num_layers, num_envs, self.lstm.hidden_size)
        return torch.zeros(shape, device=device), torch.zeros(shape, device=device)

    def states_from_features(self, hidden, lstm_state, done):
        """The LSTM logic of ``get_states`` (:141-156) on the (T*B, 512) features of T time-major steps of B envs."""
        batch_size = lstm_state[0].shape[1]
        if self.lstm_backend == "fused":
            return self._states_fused(hidden, lstm_state, done, batch_size)
        hidden = hidden.reshape((-1, batch_size, self.lstm.input_size))
        done = done.reshape((-1, batch_size))
        new_hidden = []
        for h, d in zip(hidden, done):
            keep = (1.0 - d).view(1, -1, 1)
            h, lstm_state = self.lstm(h.unsqueeze(0), (keep * lstm_state[0], keep * lstm_state[1]))
            new_hidden += [h]
        return torch.flatten(torch.cat(new_hidden), 0, 1), lstm_state

    def _states_fused(self, hidden, lstm_state, done, batch_size):
        """The same recurrence as one scan: gx = x W_ih^T + (b_ih + b_hh) for all T steps, then ``ops.lstm_seq``."""
        lstm, H = self.lstm, self.lstm.hidden_size
        gx = nn.functional.linear(hidden, lstm.weight_ih_l0, lstm.bias_ih_l0 + lstm.bias_hh_l0).reshape(-1, batch_size, 4 * H)
        h, hT, cT = ops.lstm_seq(gx, lstm.weight_hh_l0, lstm_state[0][0], lstm_state[1][0], done.reshape(-1, batch_size))
        return h.reshape(-1, H), (hT.unsqueeze(0), cT.unsqueeze(0))

    def heads_seq(self, xn, lstm_state, done):
        """xn: already-normalised f32 frames, time-major (T*B, 1, 84, 84) -> (logits, value, new state): the seam the
        learner's update uses (the fused loss kernel consumes logits / value; autograd runs through this function)."""
        hidden, lstm_state = self.states_from_features(self.network(xn), lstm_state, done)
        return self.actor(hidden), self.critic(hidden), lstm_state

    def get_states(self, x, lstm_state, done):
        return self.states_from_features(self.network(self._normalise(x)), lstm_state, done)

    def get_value(self, x, lstm_state, done):
        hidden, _ = self.get_states(x, lstm_state, done)
        return self.critic(hidden)

    def get_action_and_value(self, x, lstm_state, done, action=None):
        hidden, lstm_state = self.get_states(x, lstm_state, done)
        logits = self.actor(hidden)
        action, lp, ent = self._dist(logits, action)
        return action, lp, ent, self.critic(hidden), lstm_state


IMPALA_BACKENDS = ("torch", "fused")


def impala_backend_from_env() -> str:
    """``MI355PPO_IMPALA``: ``torch`` (default: the reference's ConvSequence modules) or ``fused`` (the trunk kernels of
    csrc/impala.hip, ``ops.impala_trunk``)."""
    v = os.environ.get("MI355PPO_IMPALA", "torch")
    if v not in IMPALA_BACKENDS:
        raise ValueError(f"MI355PPO_IMPALA={v!r}: expected torch or fused")
    return v


def _impala_features(agent, xn):
    """The IMPALA network (conv sequences, then Flatten -> ReLU -> Linear -> ReLU) on normalised (B, C, H, W) frames.  With the
    ``fused`` backend the three conv sequences run as ``ops.impala_trunk`` on the channels-last frames (``xn`` is a permuted
    view of them, so the permute back is free) and the tail runs on the NCHW view of the trunk's output, so ``Flatten`` sees
    the reference's (C, H, W) order."""
    if agent.impala_backend != "fused":
        return agent.network(xn)
    net = agent.network
    params = [p for i in range(3) for p in net[i].parameters()]
    y = ops.impala_trunk(xn.permute(0, 2, 3, 1), params)
    return net[3:](y.permute(0, 3, 1, 2))


class ResidualBlock(nn.Module):
    """ppo_procgen.py:86-98 (IMPALA-CNN residual block): x + conv1(relu(conv0(relu(x))))."""

    def __init__(self, channels):
        super().__init__()
        self.conv0 = nn.Conv2d(in_channels=channels, out_channels=channels, kernel_size=3, padding=1)
        self.conv1 = nn.Conv2d(in_channels=channels, out_channels=channels, kernel_size=3, padding=1)

    def forward(self, x):
        inputs = x
        x = nn.functional.relu(x)
        x = self.conv0(x)
        x = nn.functional.relu(x)
        x = self.conv1(x)
        return x + inputs


class ConvSequence(nn.Module):
    """ppo_procgen.py:101-124: conv3x3 -> max_pool(3, stride 2, pad 1) -> two residual blocks."""

    def __init__(self, input_shape, out_channels):
        super().__init__()
        self._input_shape = input_shape
        self._out_channels = out_channels
        self.conv = nn.Conv2d(in_channels=self._input_shape[0], out_channels=self._out_channels, kernel_size=3, padding=1)
        self.res_block0 = ResidualBlock(self._out_channels)
        self.res_block1 = ResidualBlock(self._out_channels)

    def forward(self, x):
        x = self.conv(x)
        x = nn.functional.max_pool2d(x, kernel_size=3, stride=2, padding=1)
        x = self.res_block0(x)
        x = self.res_block1(x)
        assert x.shape[1:] == self.get_output_shape()
        return x

    def get_output_shape(self):
        _c, h, w = self._input_shape
        return (self._out_channels, (h + 1) // 2, (w + 1) // 2)


class AtariImpalaQNetwork(nn.Module):
    """qdagger_dqn_atari_impalacnn.py:164-184 (the QDagger student's ``QNetwork``): IMPALA-CNN [16, 32, 32] on (4, 84, 84) frame
    stacks, then Flatten -> ReLU -> Linear(3872, 256) -> ReLU -> Linear(256, n).  Same ``state_dict`` keys and default
    initialisation as the reference.  ``forward`` takes the reference's (B, 4, 84, 84) stacks; ``forward_hwc`` takes the
    channels-last (B, 84, 84, 4) uint8 rows of the frame ring, which with ``impala_backend == "fused"`` (MI355PPO_IMPALA) go
    to ``ops.impala84_trunk`` as bytes (csrc/impala.hip) while the tail runs on the NCHW view of its output."""

    def __init__(self, env, obs_shape=(4, 84, 84)):
        super().__init__()
        n_actions = env if isinstance(env, int) else env.single_action_space.n        # the reference takes ``envs``
        self.n = int(n_actions)
        shape = tuple(obs_shape) if isinstance(env, int) else tuple(env.single_observation_space.shape)
        conv_seqs = []
        for out_channels in [16, 32, 32]:
            conv_seq = ConvSequence(shape, out_channels)
            shape = conv_seq.get_output_shape()
            conv_seqs.append(conv_seq)
        conv_seqs += [
            nn.Flatten(),
            nn.ReLU(),
            nn.Linear(in_features=shape[0] * shape[1] * shape[2], out_features=256),
            nn.ReLU(),
            nn.Linear(in_features=256, out_features=int(n_actions)),
        ]
        self.network = nn.Sequential(*conv_seqs)
        self.impala_backend = impala_backend_from_env()

    def hidden_hwc(self, x_hwc):
        """(B, 84, 84, 4) uint8 channels-last rows -> the 256-wide hidden layer (the input of the Q head)."""
        if self.impala_backend != "fused":
            return self.network[:-1](x_hwc.permute(0, 3, 1, 2) / 255.0)
        y = ops.impala84_trunk(x_hwc, ops.impala84_params(self))
        return self.network[3:-1](y.permute(0, 3, 1, 2))

    def forward_hwc(self, x_hwc):
        return self.network[-1](self.hidden_hwc(x_hwc))

    def forward(self, x):
        if self.impala_backend == "fused" and x.dtype == torch.uint8:      # the fused trunk reads bytes; float stacks take the reference's ops
            return self.forward_hwc(x.permute(0, 2, 3, 1).contiguous())
        return self.network(x / 255.0)


class ProcgenAgent(_DiscreteMixin, nn.Module):
    """ppo_procgen.py:127-158: IMPALA-CNN [16, 32, 32] on (64, 64, 3) frames that arrive pixel-interleaved ("bhwc") --
    which is how the rollout buffer stores images anyway, so no relayout kernel runs for this script.  The conv layers
    keep torch's default initialisation, as in the reference (only actor / critic use ``layer_init``)."""

    obs_is_image = True
    obs_layout = "hwc"

    def __init__(self, envs):
        super().__init__()
        h, w, c = envs.single_observation_space.shape
        shape = (c, h, w)
        conv_seqs = []
        for out_channels in [16, 32, 32]:
            conv_seq = ConvSequence(shape, out_channels)
            shape = conv_seq.get_output_shape()
            conv_seqs.append(conv_seq)
        conv_seqs += [
            nn.Flatten(),
            nn.ReLU(),
            nn.Linear(in_features=shape[0] * shape[1] * shape[2], out_features=256),
            nn.ReLU(),
        ]
        self.network = nn.Sequential(*conv_seqs)
        self.actor = layer_init(nn.Linear(256, envs.single_action_space.n), std=0.01)
        self.critic = layer_init(nn.Linear(256, 1), std=1)
        self.n_actions = envs.single_action_space.n
        self.rng = _SampleCounter()
        self.impala_backend = impala_backend_from_env()

    def _normalise(self, x):
        """(B, H, W, C) frames -> normalised (B, C, H, W) view ("bhwc" -> "bchw", :147,150)."""
        if x.dtype == torch.uint8:
            x = ops.obs_u8_to_f32(x.contiguous()) if x.is_cuda else x.float() / 255.0
        else:
            x = x / 255.0
        return x.permute((0, 3, 1, 2))

    def heads(self, xn):
        """xn: normalised f32 frames as (B, C, H, W) (any strides) -> (logits, value)."""
        hidden = _impala_features(self, xn)
        return self.actor(hidden), self.critic(hidden)

    def get_value(self, x):
        return self.critic(_impala_features(self, self._normalise(x)))

    def get_action_and_value(self, x, action=None):
        logits, value = self.heads(self._normalise(x))
        action, lp, ent = self._dist(logits, action)
        return action, lp, ent, value


class RNDAgent(_NatureTrunkMixin, _DiscreteMixin, nn.Module):
    """ppo_rnd_envpool.py:139-185: NatureCNN -> Linear(3136,256) -> Linear(256,448), a 448-448 "extra" layer feeding two
    value heads (extrinsic / intrinsic) through a residual sum, and a two-layer actor.  Same construction order as the
    reference."""

    obs_is_image = True
    two_value_heads = True

    def __init__(self, envs):
        super().__init__()
        self.network = nn.Sequential(
            layer_init(nn.Conv2d(4, 32, 8, stride=4)),
            nn.ReLU(),
            layer_init(nn.Conv2d(32, 64, 4, stride=2)),
            nn.ReLU(),
            layer_init(nn.Conv2d(64, 64, 3, stride=1)),
            nn.ReLU(),
            nn.Flatten(),
            layer_init(nn.Linear(64 * 7 * 7, 256)),
            nn.ReLU(),
            layer_init(nn.Linear(256, 448)),
            nn.ReLU(),
        )
        self.extra_layer = nn.Sequential(layer_init(nn.Linear(448, 448), std=0.1), nn.ReLU())
        self.actor = nn.Sequential(
            layer_init(nn.Linear(448, 448), std=0.01),
            nn.ReLU(),
            layer_init(nn.Linear(448, envs.single_action_space.n), std=0.01),
        )
        self.critic_ext = layer_init(nn.Linear(448, 1), std=0.01)
        self.critic_int = layer_init(nn.Linear(448, 1), std=0.01)
        self.n_actions = envs.single_action_space.n
        self.rng = _SampleCounter()

    def _normalise(self, x):
        if x.dtype == torch.uint8:
            return ops.obs_u8_to_f32(x.contiguous()) if x.is_cuda else x.float() / 255.0
        return x / 255.0

    def heads3(self, xn):
        """xn: normalised f32 observations (B,4,84,84) -> (logits, extrinsic value, intrinsic value)."""
        return self._heads3(self.network(xn))

    def _heads3(self, hidden):
        logits = self.actor(hidden)
        features = self.extra_layer(hidden)
        return logits, self.critic_ext(features + hidden), self.critic_int(features + hidden)

    def heads3_u8(self, obs_rows, inds=None):
        """``heads3(obs_rows[inds] / 255.0)`` on the uint8 (rows, 84, 84, 4) rollout rows (MI355PPO_RND_TRUNK=fused): ``network[0:9]`` --
        the three convolutions and Linear(3136, 256) + ReLU -- on the trunk kernels (``_hidden_u8``: gather and /255 inside conv1);
        ``network[9:]``, the extra layer, the actor and the two critics stay torch modules."""
        net = self.network
        return self._heads3(net[10](net[9](self._hidden_u8(obs_rows, inds))))

    def get_action_and_value(self, x, action=None):
        logits, v_ext, v_int = self.heads3(self._normalise(x))
        action, lp, ent = self._dist(logits, action)
        return action, lp, ent, v_ext, v_int

    def get_value(self, x):
        _, v_ext, v_int = self.heads3(self._normalise(x))
        return v_ext, v_int


class RNDModel(nn.Module):
    """ppo_rnd_envpool.py:188-233: predictor and frozen random target network on ONE normalised 84x84 frame."""

    def __init__(self, input_size, output_size):
        super().__init__()
        self.input_size = input_size
        self.output_size = output_size
        feature_output = 7 * 7 * 64
        self.predictor = nn.Sequential(
            layer_init(nn.Conv2d(in_channels=1, out_channels=32, kernel_size=8, stride=4)),
            nn.LeakyReLU(),
            layer_init(nn.Conv2d(in_channels=32, out_channels=64, kernel_size=4, stride=2)),
            nn.LeakyReLU(),
            layer_init(nn.Conv2d(in_channels=64, out_channels=64, kernel_size=3, stride=1)),
            nn.LeakyReLU(),
            nn.Flatten(),
            layer_init(nn.Linear(feature_output, 512)),
            nn.ReLU(),
            layer_init(nn.Linear(512, 512)),
            nn.ReLU(),
            layer_init(nn.Linear(512, 512)),
        )
        self.target = nn.Sequential(
            layer_init(nn.Conv2d(in_channels=1, out_channels=32, kernel_size=8, stride=4)),
            nn.LeakyReLU(),
            layer_init(nn.Conv2d(in_channels=32, out_channels=64, kernel_size=4, stride=2)),
            nn.LeakyReLU(),
            layer_init(nn.Conv2d(in_channels=64, out_channels=64, kernel_size=3, stride=1)),
            nn.LeakyReLU(),
            nn.Flatten(),
            layer_init(nn.Linear(feature_output, 512)),
        )
        for param in self.target.parameters():          # target network is not trainable
            param.requires_grad = False

    def forward(self, next_obs):
        target_feature = self.target(next_obs)
        predict_feature = self.predictor(next_obs)
        return predict_feature, target_feature


def layer_init_normed(layer, norm_dim, scale=1.0):
    """ppg_procgen.py:100-104: rescale every output unit's weight vector to norm ``scale``; zero bias."""
    with torch.no_grad():
        layer.weight.data *= scale / layer.weight.norm(dim=norm_dim, p=2, keepdim=True)
        layer.bias *= 0
    return layer


class ResidualBlockNormed(nn.Module):
    """ppg_procgen.py:123-139."""

    def __init__(self, channels, scale):
        super().__init__()
        scale = np.sqrt(scale)
        conv0 = nn.Conv2d(in_channels=channels, out_channels=channels, kernel_size=3, padding=1)
        self.conv0 = layer_init_normed(conv0, norm_dim=(1, 2, 3), scale=scale)
        conv1 = nn.Conv2d(in_channels=channels, out_channels=channels, kernel_size=3, padding=1)
        self.conv1 = layer_init_normed(conv1, norm_dim=(1, 2, 3), scale=scale)

    def forward(self, x):
        inputs = x
        x = nn.functional.relu(x)
        x = self.conv0(x)
        x = nn.functional.relu(x)
        x = self.conv1(x)
        return x + inputs


class ConvSequenceNormed(nn.Module):
    """ppg_procgen.py:142-165."""

    def __init__(self, input_shape, out_channels, scale):
        super().__init__()
        self._input_shape = input_shape
        self._out_channels = out_channels
        conv = nn.Conv2d(in_channels=self._input_shape[0], out_channels=self._out_channels, kernel_size=3, padding=1)
        self.conv = layer_init_normed(conv, norm_dim=(1, 2, 3), scale=1.0)
        nblocks = 2
        scale = scale / np.sqrt(nblocks)
        self.res_block0 = ResidualBlockNormed(self._out_channels, scale=scale)
        self.res_block1 = ResidualBlockNormed(self._out_channels, scale=scale)

    def forward(self, x):
        x = self.conv(x)
        x = nn.functional.max_pool2d(x, kernel_size=3, stride=2, padding=1)
        x = self.res_block0(x)
        x = self.res_block1(x)
        assert x.shape[1:] == self.get_output_shape()
        return x

    def get_output_shape(self):
        _c, h, w = self._input_shape
        return (self._out_channels, (h + 1) // 2, (w + 1) // 2)


class PPGAgent(_DiscreteMixin, nn.Module):
    """ppg_procgen.py:168-211: IMPALA-CNN with norm-scaled initialisation, a policy head, a value head on the DETACHED
    features (the policy phase's value loss does not shape the encoder) and an auxiliary value head on the live features
    (the auxiliary phase's does)."""

    obs_is_image = True
    obs_layout = "hwc"

    def __init__(self, envs):
        super().__init__()
        h, w, c = envs.single_observation_space.shape
        shape = (c, h, w)
        conv_seqs = []
        chans = [16, 32, 32]
        scale = 1 / np.sqrt(len(chans))
        for out_channels in chans:
            conv_seq = ConvSequenceNormed(shape, out_channels, scale=scale)
            shape = conv_seq.get_output_shape()
            conv_seqs.append(conv_seq)
        encodertop = nn.Linear(in_features=shape[0] * shape[1] * shape[2], out_features=256)
        encodertop = layer_init_normed(encodertop, norm_dim=1, scale=1.4)
        conv_seqs += [
            nn.Flatten(),
            nn.ReLU(),
            encodertop,
            nn.ReLU(),
        ]
        self.network = nn.Sequential(*conv_seqs)
        self.actor = layer_init_normed(nn.Linear(256, envs.single_action_space.n), norm_dim=1, scale=0.1)
        self.critic = layer_init_normed(nn.Linear(256, 1), norm_dim=1, scale=0.1)
        self.aux_critic = layer_init_normed(nn.Linear(256, 1), norm_dim=1, scale=0.1)
        self.n_actions = envs.single_action_space.n
        self.rng = _SampleCounter()
        self.impala_backend = impala_backend_from_env()

    def _normalise(self, x):
        """(B, H, W, C) frames -> normalised (B, C, H, W) view ("bhwc" -> "bchw")."""
        if x.dtype == torch.uint8:
            x = ops.obs_u8_to_f32(x.contiguous()) if x.is_cuda else x.float() / 255.0
        else:
            x = x / 255.0
        return x.permute((0, 3, 1, 2))

    def heads(self, xn):
        """xn: normalised (B, C, H, W) frames -> (logits, value on the detached features): the policy-phase seam."""
        hidden = _impala_features(self, xn)
        return self.actor(hidden), self.critic(hidden.detach())

    def heads_aux(self, xn):
        """-> (logits, value on detached features, auxiliary value on live features): the auxiliary-phase seam."""
        hidden = _impala_features(self, xn)
        return self.actor(hidden), self.critic(hidden.detach()), self.aux_critic(hidden)

    def get_action_and_value(self, x, action=None):
        logits, value = self.heads(self._normalise(x))
        action, lp, ent = self._dist(logits, action)
        return action, lp, ent, value

    def get_value(self, x):
        return self.critic(_impala_features(self, self._normalise(x)))

    def get_pi_value_and_aux_value(self, x):
        logits, value, aux = self.heads_aux(self._normalise(x))
        return Categorical(logits=logits), value, aux

    def get_pi(self, x):
        return Categorical(logits=self.actor(_impala_features(self, self._normalise(x))))


MA_ATARI_BACKENDS = ("torch", "fused")


def ma_atari_backend() -> str:
    """``MI355PPO_MA_ATARI``: ``torch`` (the default: K5 + MIOpen convolutions + library GEMMs on the six-channel rows) or ``fused`` (the
    NatureCNN trunk kernels on four-channel rows with the indicator planes as a per-row bias; HIP learner only); read when a learner is
    built."""
    v = os.environ.get("MI355PPO_MA_ATARI", "torch").strip().lower() or "torch"
    if v not in MA_ATARI_BACKENDS:
        raise ValueError(f"MI355PPO_MA_ATARI={v!r}: expected 'torch' or 'fused'")
    return v


class MAAtariAgent(_NatureTrunkMixin, _DiscreteMixin, nn.Module):
    """ppo_pettingzoo_ma_atari.py:86-118: NatureCNN on (84, 84, 6) pixel-interleaved observations -- four stacked frames plus
    two agent-indicator planes.  Only the four frame channels are divided by 255 (:104,109)."""

    obs_is_image = True
    obs_layout = "hwc"
    frame_channels = 4            # channels [0, 4) are pixels; the rest pass through unscaled
    indicator_planes = 2          # channels [4, 6): constant over an observation (supersuit's agent_indicator_v0)

    def __init__(self, envs):
        super().__init__()
        self.network = nn.Sequential(
            layer_init(nn.Conv2d(6, 32, 8, stride=4)),
            nn.ReLU(),
            layer_init(nn.Conv2d(32, 64, 4, stride=2)),
            nn.ReLU(),
            layer_init(nn.Conv2d(64, 64, 3, stride=1)),
            nn.ReLU(),
            nn.Flatten(),
            layer_init(nn.Linear(64 * 7 * 7, 512)),
            nn.ReLU(),
        )
        self.actor = layer_init(nn.Linear(512, envs.single_action_space.n), std=0.01)
        self.critic = layer_init(nn.Linear(512, 1), std=1)
        self.n_actions = envs.single_action_space.n
        self.rng = _SampleCounter()

    def scale_frames_(self, x):
        """In place on a (B, H, W, C) f32 tensor holding raw 0..255 values: ``x[:, :, :, [0,1,2,3]] /= 255.0``."""
        x[..., : self.frame_channels] /= 255.0
        return x

    def _normalise(self, x):
        if x.dtype == torch.uint8:
            x = ops.obs_u8_to_f32(x.contiguous(), scale_255=False) if x.is_cuda else x.float()
        else:
            x = x.clone()
        return self.scale_frames_(x).permute((0, 3, 1, 2))

    def heads(self, xn):
        """xn: normalised (B, 6, 84, 84) -> (logits, value)."""
        hidden = self.network(xn)
        return self.actor(hidden), self.critic(hidden)

    def heads_u8(self, obs_rows, inds=None, ind=None):
        """``MI355PPO_MA_ATARI=fused``: ``obs_rows`` are the (rows, 84, 84, 4) u8 frame channels, ``ind`` (rows, 2) the two indicator bytes of
        each row, ``inds`` optionally gathers rows.  Same function as ``heads`` on the six-channel observation whose planes 4 / 5 hold
        ``ind`` everywhere: conv1 on kernel Q with the planes' contribution as a per-row bias, the rest as ``AtariAgent.heads_u8``."""
        return self._heads_u8(obs_rows, inds, ind)

    def act_u8(self, obs_rows, ind, seed, offset, offset_base=None, action_f32_out=None, logprob_out=None, value_out=None, want_i64=True):
        """The fused rollout step on the four-channel rows and their indicator bytes (``_act_u8``); None when it does not apply."""
        return self._act_u8(obs_rows, ind, seed, offset, offset_base, action_f32_out, logprob_out, value_out, want_i64)

    def get_value(self, x):
        return self.critic(self.network(self._normalise(x)))

    def get_action_and_value(self, x, action=None):
        logits, value = self.heads(self._normalise(x))
        action, lp, ent = self._dist(logits, action)
        return action, lp, ent, value


# ------------------------------------------------------------------------------------------- TrXL (ppo_trxl.py)
TRXL_BACKENDS = ("torch", "fused")


def trxl_backend_from_env() -> str:
    """``MI355PPO_TRXL``: ``torch`` (default: the reference's window gather and attention ops) or ``fused`` (the episodic-memory
    attention of csrc/trxl_attn.hip, ``ops.TrXLMemoryAttention``)."""
    v = os.environ.get("MI355PPO_TRXL", "torch")
    if v not in TRXL_BACKENDS:
        raise ValueError(f"MI355PPO_TRXL={v!r}: expected torch or fused")
    return v


def _trxl_init(layer, std=np.sqrt(2)):
    """ppo_trxl.py's ``layer_init``: orthogonal weight only -- the bias keeps nn.Linear's default init."""
    torch.nn.init.orthogonal_(layer.weight, std)
    return layer


def batched_index_select(input, dim, index):
    """ppo_trxl.py's gather of per-sample rows along ``dim``."""
    for ii in range(1, len(input.shape)):
        if ii != dim:
            index = index.unsqueeze(ii)
    expanse = list(input.shape)
    expanse[0] = -1
    expanse[dim] = -1
    index = index.expand(expanse)
    return torch.gather(input, dim, index)


class MemoryWindow:
    """A memory window given as indices into an episode pool instead of a gathered tensor: sample b's rows are
    ``pool[ep[b], rows[b, :]]``.  ``pool`` is (E, T_ep, layers, D); the ``fused`` backend streams the rows from it, the ``torch``
    backend gathers them as the reference does (``batched_index_select(pool[ep], 1, rows)``)."""

    def __init__(self, pool, ep, rows):
        self.pool, self.ep, self.rows = pool, ep, rows

    def gather(self):
        return batched_index_select(self.pool[self.ep], 1, self.rows)


class TrXLPositionalEncoding(nn.Module):
    """ppo_trxl.py ``PositionalEncoding``: sinusoids of reversed positions, (seq_len, dim)."""

    def __init__(self, dim, min_timescale=2.0, max_timescale=1e4):
        super().__init__()
        freqs = torch.arange(0, dim, min_timescale)
        inv_freqs = max_timescale ** (-freqs / dim)
        self.register_buffer("inv_freqs", inv_freqs)

    def forward(self, seq_len):
        seq = torch.arange(seq_len - 1, -1, -1.0, device=self.inv_freqs.device)
        sinusoidal_inp = seq.reshape(-1, 1) * self.inv_freqs.reshape(1, -1)
        return torch.cat((sinusoidal_inp.sin(), sinusoidal_inp.cos()), dim=-1)


class TrXLMultiHeadAttention(nn.Module):
    """ppo_trxl.py ``MultiHeadAttention`` (no dropout): per-head (d, d) values / keys / queries, ``fc_out``."""

    def __init__(self, embed_dim, num_heads):
        super().__init__()
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.head_size = embed_dim // num_heads
        assert self.head_size * num_heads == embed_dim, "Embedding dimension needs to be divisible by the number of heads"
        self.values = nn.Linear(self.head_size, self.head_size, bias=False)
        self.keys = nn.Linear(self.head_size, self.head_size, bias=False)
        self.queries = nn.Linear(self.head_size, self.head_size, bias=False)
        self.fc_out = nn.Linear(self.num_heads * self.head_size, embed_dim)

    def forward(self, values, keys, query, mask):
        N = query.shape[0]
        value_len, key_len, query_len = values.shape[1], keys.shape[1], query.shape[1]
        values = self.values(values.reshape(N, value_len, self.num_heads, self.head_size))
        keys = self.keys(keys.reshape(N, key_len, self.num_heads, self.head_size))
        queries = self.queries(query.reshape(N, query_len, self.num_heads, self.head_size))
        energy = torch.einsum("nqhd,nkhd->nhqk", [queries, keys])
        if mask is not None:
            energy = energy.masked_fill(mask.unsqueeze(1).unsqueeze(1) == 0, float("-1e20"))
        attention = torch.softmax(energy / (self.embed_dim ** (1 / 2)), dim=3)
        out = torch.einsum("nhql,nlhd->nqhd", [attention, values]).reshape(N, query_len, self.num_heads * self.head_size)
        return self.fc_out(out), attention


class TrXLTransformerLayer(nn.Module):
    """ppo_trxl.py ``TransformerLayer``: pre-LN attention over the memory window (K = V), skip, pre-LN ReLU projection, skip."""

    def __init__(self, dim, num_heads):
        super().__init__()
        self.attention = TrXLMultiHeadAttention(dim, num_heads)
        self.layer_norm_q = nn.LayerNorm(dim)
        self.norm_kv = nn.LayerNorm(dim)
        self.layer_norm_attn = nn.LayerNorm(dim)
        self.fc_projection = nn.Sequential(nn.Linear(dim, dim), nn.ReLU())

    def forward(self, value, key, query, mask):
        query_ = self.layer_norm_q(query)
        value = self.norm_kv(value)
        key = value
        attention, attention_weights = self.attention(value, key, query_, mask)
        x = attention + query
        x_ = self.layer_norm_attn(x)
        forward = self.fc_projection(x_)
        return forward + x, attention_weights

    def forward_fused(self, x, window, layer, pos, mask, pe):
        """The same layer with the window path (gather, pe, norm_kv, keys, softmax, weighted sum) in one kernel:
        q~ = queries(LN_q(x)) @ keys.weight, u = sum_j att_j norm_kv(row_j), then ``values`` and ``fc_out`` on u."""
        att = self.attention
        B = x.shape[0]
        q = att.queries(self.layer_norm_q(x).reshape(B, att.num_heads, att.head_size))
        u = ops.trxl_memory_attention(q @ att.keys.weight, self.norm_kv.weight, self.norm_kv.bias, window.pool, layer, window.ep,
                                      window.rows, pos, mask, pe)
        x = att.fc_out(att.values(u).reshape(B, att.embed_dim)) + x
        return self.fc_projection(self.layer_norm_attn(x)) + x


class TrXLTransformer(nn.Module):
    """ppo_trxl.py ``Transformer``: positional encoding (``absolute``, ``learned`` or none) added to the memory window, then the
    layers; returns the output and the per-layer inputs (detached: the next episodic-memory row)."""

    def __init__(self, num_layers, dim, num_heads, max_episode_steps, positional_encoding, backend="torch"):
        super().__init__()
        self.max_episode_steps = max_episode_steps
        self.positional_encoding = positional_encoding
        if positional_encoding == "absolute":
            self.pos_embedding = TrXLPositionalEncoding(dim)
        elif positional_encoding == "learned":
            self.pos_embedding = nn.Parameter(torch.randn(max_episode_steps, dim))
        self.transformer_layers = nn.ModuleList([TrXLTransformerLayer(dim, num_heads) for _ in range(num_layers)])
        self.backend = backend

    def forward(self, x, memories, mask, memory_indices):
        if self.backend == "fused":
            return self._forward_fused(x, memories, mask, memory_indices)
        if isinstance(memories, MemoryWindow):
            memories = memories.gather()
        if self.positional_encoding == "absolute":
            pos_embedding = self.pos_embedding(self.max_episode_steps)[memory_indices]
            memories = memories + pos_embedding.unsqueeze(2)
        elif self.positional_encoding == "learned":
            memories = memories + self.pos_embedding[memory_indices].unsqueeze(2)
        out_memories = []
        for i, layer in enumerate(self.transformer_layers):
            out_memories.append(x.detach())
            x, attention_weights = layer(memories[:, :, i], memories[:, :, i], x.unsqueeze(1), mask)
            x = x.squeeze()
            if len(x.shape) == 1:
                x = x.unsqueeze(0)
        return x, torch.stack(out_memories, dim=1)

    def _forward_fused(self, x, memories, mask, memory_indices):
        if not isinstance(memories, MemoryWindow):              # an already gathered (B, L, layers, D) window
            B, L = memories.shape[:2]
            memories = MemoryWindow(memories, torch.arange(B, device=memories.device),
                                    torch.arange(L, device=memories.device).expand(B, L))
        pe = self.pos_embedding(self.max_episode_steps) if self.positional_encoding == "absolute" else None
        out_memories = []
        for i, layer in enumerate(self.transformer_layers):
            out_memories.append(x.detach())
            x = layer.forward_fused(x, memories, i, memory_indices, mask, pe)
        return x, torch.stack(out_memories, dim=1)


class TrXLAgent(nn.Module):
    """ppo_trxl.py ``Agent``: encoder (Linear for vector observations, NatureCNN on (84, 84, 3) images / 255), Transformer-XL over
    the episodic memory window, ``hidden_post_trxl``, one Categorical branch per MultiDiscrete component, the critic, and the
    optional transposed-CNN observation reconstruction.  Same modules, parameter order and initialisation as the reference, so a
    seeded construction gives the reference's weights.

    ``trxl_backend`` (from ``MI355PPO_TRXL`` at construction): ``torch`` runs the reference's ops; ``fused`` routes each layer's
    window path through ``ops.TrXLMemoryAttention`` (HIP kernels on the GPU, their host twins on CPU).  ``fused`` refuses a
    ``learned`` positional encoding, whose gradient would be a scatter-add into the table.  The ``memory`` argument of the methods
    is a gathered window (B, L, layers, D), as in the reference, or a ``MemoryWindow`` into an episode pool."""

    def __init__(self, args, observation_space, action_space_shape, max_episode_steps):
        super().__init__()
        self.obs_shape = observation_space.shape
        self.max_episode_steps = max_episode_steps
        self.trxl_backend = trxl_backend_from_env()
        if self.trxl_backend == "fused" and args.trxl_positional_encoding == "learned":
            raise ValueError("MI355PPO_TRXL=fused does not support --trxl-positional-encoding learned (use torch)")

        if len(self.obs_shape) > 1:
            self.encoder = nn.Sequential(
                _trxl_init(nn.Conv2d(3, 32, 8, stride=4)),
                nn.ReLU(),
                _trxl_init(nn.Conv2d(32, 64, 4, stride=2)),
                nn.ReLU(),
                _trxl_init(nn.Conv2d(64, 64, 3, stride=1)),
                nn.ReLU(),
                nn.Flatten(),
                _trxl_init(nn.Linear(64 * 7 * 7, args.trxl_dim)),
                nn.ReLU(),
            )
        else:
            self.encoder = _trxl_init(nn.Linear(observation_space.shape[0], args.trxl_dim))

        self.transformer = TrXLTransformer(args.trxl_num_layers, args.trxl_dim, args.trxl_num_heads, self.max_episode_steps,
                                           args.trxl_positional_encoding, backend=self.trxl_backend)
        self.hidden_post_trxl = nn.Sequential(_trxl_init(nn.Linear(args.trxl_dim, args.trxl_dim)), nn.ReLU())
        self.actor_branches = nn.ModuleList(
            [_trxl_init(nn.Linear(args.trxl_dim, out_features=num_actions), np.sqrt(0.01)) for num_actions in action_space_shape])
        self.critic = _trxl_init(nn.Linear(args.trxl_dim, 1), 1)

        if args.reconstruction_coef > 0.0:
            self.transposed_cnn = nn.Sequential(
                _trxl_init(nn.Linear(args.trxl_dim, 64 * 7 * 7)),
                nn.ReLU(),
                nn.Unflatten(1, (64, 7, 7)),
                _trxl_init(nn.ConvTranspose2d(64, 64, 3, stride=1)),
                nn.ReLU(),
                _trxl_init(nn.ConvTranspose2d(64, 32, 4, stride=2)),
                nn.ReLU(),
                _trxl_init(nn.ConvTranspose2d(32, 3, 8, stride=4)),
                nn.Sigmoid(),
            )

    @property
    def trxl_backend(self):
        return self._trxl_backend

    @trxl_backend.setter
    def trxl_backend(self, v):
        if v not in TRXL_BACKENDS:
            raise ValueError(f"trxl_backend={v!r}: expected torch or fused")
        self._trxl_backend = v
        if "transformer" in self._modules:
            self.transformer.backend = v

    def _encode(self, x):
        if len(self.obs_shape) > 1:
            return self.encoder(x.permute((0, 3, 1, 2)) / 255.0)
        return self.encoder(x)

    def get_value(self, x, memory, memory_mask, memory_indices):
        x, _ = self.transformer(self._encode(x), memory, memory_mask, memory_indices)
        x = self.hidden_post_trxl(x)
        return self.critic(x).flatten()

    def get_action_and_value(self, x, memory, memory_mask, memory_indices, action=None):
        x, memory = self.transformer(self._encode(x), memory, memory_mask, memory_indices)
        x = self.hidden_post_trxl(x)
        self.x = x
        probs = [Categorical(logits=branch(x)) for branch in self.actor_branches]
        if action is None:
            action = torch.stack([dist.sample() for dist in probs], dim=1)
        log_probs = []
        for i, dist in enumerate(probs):
            log_probs.append(dist.log_prob(action[:, i]))
        entropies = torch.stack([dist.entropy() for dist in probs], dim=1).sum(1).reshape(-1)
        return action, torch.stack(log_probs, dim=1), entropies, self.critic(x).flatten(), memory

    def reconstruct_observation(self):
        x = self.transposed_cnn(self.x)
        return x.permute((0, 2, 3, 1))


# ------------------------------------------------------------------------------------------- PQN (pqn.py, pqn_atari_envpool.py)
class QNetwork(nn.Module):
    """pqn.py's ``QNetwork``: Linear -> LayerNorm(120) -> ReLU -> Linear -> LayerNorm(84) -> ReLU -> Linear, built in the reference's
    order (``layer_init``: orthogonal std sqrt(2), bias 0), so a seed gives the reference's weights and ``parameters()`` order.  The
    learner runs it through the fused kernels on the flat parameters (``MI355PPO_PQN=fused``) or as this module (``torch``)."""

    def __init__(self, env):
        super().__init__()
        self.network = nn.Sequential(
            layer_init(nn.Linear(np.array(env.single_observation_space.shape).prod(), 120)),
            nn.LayerNorm(120),
            nn.ReLU(),
            layer_init(nn.Linear(120, 84)),
            nn.LayerNorm(84),
            nn.ReLU(),
            layer_init(nn.Linear(84, env.single_action_space.n)),
        )

    def forward(self, x):
        return self.network(x)


class AtariQNetwork(nn.Module):
    """pqn_atari_envpool.py's ``QNetwork``: the NatureCNN with LayerNorm after every layer, on ``x / 255.0``, built in the
    reference's order.  It stays torch on every backend (MIOpen convolutions, ATen LayerNorm); the fused backend takes its ``q``."""

    def __init__(self, env):
        super().__init__()
        self.network = nn.Sequential(
            layer_init(nn.Conv2d(4, 32, 8, stride=4)),
            nn.LayerNorm([32, 20, 20]),
            nn.ReLU(),
            layer_init(nn.Conv2d(32, 64, 4, stride=2)),
            nn.LayerNorm([64, 9, 9]),
            nn.ReLU(),
            layer_init(nn.Conv2d(64, 64, 3, stride=1)),
            nn.LayerNorm([64, 7, 7]),
            nn.ReLU(),
            nn.Flatten(),
            layer_init(nn.Linear(3136, 512)),
            nn.LayerNorm(512),
            nn.ReLU(),
            layer_init(nn.Linear(512, env.single_action_space.n)),
        )

    def forward(self, x):
        return self.network(x / 255.0)


class AtariLSTMQNetwork(nn.Module):
    """pqn_atari_envpool_lstm.py's ``QNetwork``: the LayerNorm NatureCNN on ONE frame -> ``nn.LSTM(512, 128)`` (zero biases,
    orthogonal weights) with the done reset of ``get_states`` -> ``q_func = Linear(128, A)``, built in the reference's order, so a
    torch seed gives the reference's weights.  ``forward`` / ``get_states`` are the reference's per-step loop (the ``torch``
    backend).  The fused backend of ``LSTMPQNLearner`` uses the seams below: ``gates`` (trunk + the gx GEMM, both torch) and
    ``states_fused`` (``ops.lstm_seq``: all T steps in one scan, HIP kernels on the GPU and their host twins on the CPU); the cell of
    a rollout step, ``q_func``, e-greedy and the TD loss run in csrc/pqn_lstm.hip on this module's parameters.  With
    ``MI355PPO_PQN_TRUNK=fused`` the learner takes ``gates_fused`` / ``states_from_gates`` instead: the same two with ``network`` on the
    kernels of ``ln_cnn`` (uint8 frames, the one-frame conv1 of csrc/conv1q1.hip / conv1p1.hip)."""

    def __init__(self, env):
        super().__init__()
        self.network = nn.Sequential(
            layer_init(nn.Conv2d(1, 32, 8, stride=4)),
            nn.LayerNorm([32, 20, 20]),
            nn.ReLU(),
            layer_init(nn.Conv2d(32, 64, 4, stride=2)),
            nn.LayerNorm([64, 9, 9]),
            nn.ReLU(),
            layer_init(nn.Conv2d(64, 64, 3, stride=1)),
            nn.LayerNorm([64, 7, 7]),
            nn.ReLU(),
            nn.Flatten(),
            layer_init(nn.Linear(3136, 512)),
            nn.LayerNorm(512),
            nn.ReLU(),
        )
        self.lstm = nn.LSTM(512, 128)
        for name, param in self.lstm.named_parameters():
            if "bias" in name:
                nn.init.constant_(param, 0)
            elif "weight" in name:
                nn.init.orthogonal_(param, 1.0)
        self.q_func = layer_init(nn.Linear(128, env.single_action_space.n))

    def initial_state(self, num_envs: int, device):
        shape = (self.lstm.num_layers, num_envs, self.lstm.hidden_size)
        return torch.zeros(shape).to(device), torch.zeros(shape).to(device)

    def get_states(self, x, lstm_state, done):
        hidden = self.network(x / 255.0)

        # LSTM logic
        batch_size = lstm_state[0].shape[1]
        hidden = hidden.reshape((-1, batch_size, self.lstm.input_size))
        done = done.reshape((-1, batch_size))
        new_hidden = []
        for h, d in zip(hidden, done):
            h, lstm_state = self.lstm(
                h.unsqueeze(0),
                (
                    (1.0 - d).view(1, -1, 1) * lstm_state[0],
                    (1.0 - d).view(1, -1, 1) * lstm_state[1],
                ),
            )
            new_hidden += [h]
        new_hidden = torch.flatten(torch.cat(new_hidden), 0, 1)
        return new_hidden, lstm_state

    def forward(self, x, lstm_state, done):
        hidden, lstm_state = self.get_states(x, lstm_state, done)
        return self.q_func(hidden), lstm_state

    # ---- the fused seams
    def gates(self, x):
        """gx (rows, 4H) = trunk(x / 255) W_ih^T + (b_ih + b_hh): the input half of every gate pre-activation, as the scan and the
        act kernel take it."""
        lstm = self.lstm
        return nn.functional.linear(self.network(x / 255.0), lstm.weight_ih_l0, lstm.bias_ih_l0 + lstm.bias_hh_l0)

    def gates_fused(self, trunk, rows_u8, inds=None):
        """``gates`` with ``network`` on the LayerNorm NatureCNN node (``ln_cnn.LnNatureTrunk``): ``rows_u8`` (R, 84, 84) uint8 frames,
        ``inds`` an optional int64 row gather that rides in conv1's loader; the ``/ 255`` is the kernel's."""
        lstm = self.lstm
        return nn.functional.linear(trunk(rows_u8, inds, self.network), lstm.weight_ih_l0, lstm.bias_ih_l0 + lstm.bias_hh_l0)

    def states_from_gates(self, gx, lstm_state, done):
        """``states_fused`` behind the gx GEMM: ``gx`` (T*B, 4H) time-major."""
        batch_size, H = lstm_state[0].shape[1], self.lstm.hidden_size
        h, hT, cT = ops.lstm_seq(gx.reshape(-1, batch_size, 4 * H), self.lstm.weight_hh_l0, lstm_state[0][0], lstm_state[1][0],
                                 done.reshape(-1, batch_size))
        return h.reshape(-1, H), (hT.unsqueeze(0), cT.unsqueeze(0))

    def states_fused(self, x, lstm_state, done):
        """``get_states`` as one scan over the T time-major steps of the B envs of ``lstm_state`` -> (h (T*B, H), new state)."""
        batch_size, H = lstm_state[0].shape[1], self.lstm.hidden_size
        gx = self.gates(x).reshape(-1, batch_size, 4 * H)
        h, hT, cT = ops.lstm_seq(gx, self.lstm.weight_hh_l0, lstm_state[0][0], lstm_state[1][0], done.reshape(-1, batch_size))
        return h.reshape(-1, H), (hT.unsqueeze(0), cT.unsqueeze(0))


# ------------------------------------------------------------------------------------------- DDPG / TD3 (ddpg_continuous_action.py, td3_continuous_action.py)
class ActionValueNetwork(nn.Module):
    """The two scripts' ``QNetwork`` (named apart from the PQN ``QNetwork`` above): Linear(obs + act, 256) -> ReLU -> Linear(256, 256)
    -> ReLU -> Linear(256, 1) on ``cat([x, a], 1)``, torch's default initialisation in the reference's construction order, so a seed
    gives the reference's weights."""

    def __init__(self, env):
        super().__init__()
        self.fc1 = nn.Linear(np.array(env.single_observation_space.shape).prod() + np.prod(env.single_action_space.shape), 256)
        self.fc2 = nn.Linear(256, 256)
        self.fc3 = nn.Linear(256, 1)

    def forward(self, x, a):
        x = torch.cat([x, a], 1)
        x = torch.relu(self.fc1(x))
        x = torch.relu(self.fc2(x))
        return self.fc3(x)


class Actor(nn.Module):
    """The two scripts' ``Actor``: Linear(obs, 256) -> ReLU -> Linear(256, 256) -> ReLU -> Linear(256, act) -> tanh, rescaled by the
    ``action_scale`` / ``action_bias`` buffers.  ``batched_space``: ddpg_continuous_action.py forms the buffers from the vector
    env's batched ``action_space`` (shape (1, act)), td3_continuous_action.py from ``single_action_space`` (shape (act,))."""

    def __init__(self, env, batched_space: bool = False):
        super().__init__()
        self.fc1 = nn.Linear(np.array(env.single_observation_space.shape).prod(), 256)
        self.fc2 = nn.Linear(256, 256)
        self.fc_mu = nn.Linear(256, np.prod(env.single_action_space.shape))
        space = env.action_space if batched_space else env.single_action_space
        self.register_buffer("action_scale", torch.tensor((space.high - space.low) / 2.0, dtype=torch.float32))
        self.register_buffer("action_bias", torch.tensor((space.high + space.low) / 2.0, dtype=torch.float32))

    def forward(self, x):
        x = torch.relu(self.fc1(x))
        x = torch.relu(self.fc2(x))
        x = torch.tanh(self.fc_mu(x))
        return x * self.action_scale + self.action_bias


# ------------------------------------------------------------------------------------------- SAC (sac_continuous_action.py)
SoftQNetwork = ActionValueNetwork           # the script's critic is the same network under another name
LOG_STD_MAX = 2
LOG_STD_MIN = -5


class SoftActor(nn.Module):
    """sac_continuous_action.py's ``Actor``: Linear(obs, 256) -> ReLU -> Linear(256, 256) -> ReLU, then ``fc_mean`` and ``fc_logstd``
    (Linear(256, act) each, in that construction order, so a seed gives the reference's weights); ``log_std`` is squashed into
    [LOG_STD_MIN, LOG_STD_MAX] through tanh.  ``get_action`` draws ``Normal.rsample`` (one standard normal of the mean's shape from
    the global stream) unless ``eps`` is given."""

    def __init__(self, env):
        super().__init__()
        self.fc1 = nn.Linear(np.array(env.single_observation_space.shape).prod(), 256)
        self.fc2 = nn.Linear(256, 256)
        self.fc_mean = nn.Linear(256, np.prod(env.single_action_space.shape))
        self.fc_logstd = nn.Linear(256, np.prod(env.single_action_space.shape))
        space = env.single_action_space
        self.register_buffer("action_scale", torch.tensor((space.high - space.low) / 2.0, dtype=torch.float32))
        self.register_buffer("action_bias", torch.tensor((space.high + space.low) / 2.0, dtype=torch.float32))

    def forward(self, x):
        x = torch.relu(self.fc1(x))
        x = torch.relu(self.fc2(x))
        mean = self.fc_mean(x)
        log_std = self.fc_logstd(x)
        log_std = torch.tanh(log_std)
        log_std = LOG_STD_MIN + 0.5 * (LOG_STD_MAX - LOG_STD_MIN) * (log_std + 1)
        return mean, log_std

    def get_action(self, x, eps=None):
        mean, log_std = self(x)
        std = log_std.exp()
        normal = torch.distributions.Normal(mean, std)
        x_t = normal.rsample() if eps is None else mean + eps * std
        y_t = torch.tanh(x_t)
        action = y_t * self.action_scale + self.action_bias
        log_prob = normal.log_prob(x_t)
        log_prob -= torch.log(self.action_scale * (1 - y_t.pow(2)) + 1e-6)
        log_prob = log_prob.sum(1, keepdim=True)
        mean = torch.tanh(mean) * self.action_scale + self.action_bias
        return action, log_prob, mean


# ------------------------------------------------------------------------------------------- DQN / C51 (dqn.py, c51.py)
class DQNNetwork(nn.Module):
    """dqn.py's ``QNetwork`` (named apart from the PQN ``QNetwork`` above): Linear(obs, 120) -> ReLU -> Linear(120, 84) -> ReLU ->
    Linear(84, n), torch's default initialisation in the reference's construction order, so a seed gives the reference's weights."""

    def __init__(self, env):
        super().__init__()
        self.network = nn.Sequential(
            nn.Linear(np.array(env.single_observation_space.shape).prod(), 120),
            nn.ReLU(),
            nn.Linear(120, 84),
            nn.ReLU(),
            nn.Linear(84, env.single_action_space.n),
        )

    def forward(self, x):
        return self.network(x)


class C51Network(nn.Module):
    """c51.py's ``QNetwork``: the same trunk with ``n * n_atoms`` outputs, the ``atoms`` buffer and ``get_action``."""

    def __init__(self, env, n_atoms=101, v_min=-100, v_max=100):
        super().__init__()
        self.env = env
        self.n_atoms = n_atoms
        self.register_buffer("atoms", torch.linspace(v_min, v_max, steps=n_atoms))
        self.n = env.single_action_space.n
        self.network = nn.Sequential(
            nn.Linear(np.array(env.single_observation_space.shape).prod(), 120),
            nn.ReLU(),
            nn.Linear(120, 84),
            nn.ReLU(),
            nn.Linear(84, self.n * n_atoms),
        )

    def get_action(self, x, action=None):
        logits = self.network(x)
        pmfs = torch.softmax(logits.view(len(x), self.n, self.n_atoms), dim=2)
        q_values = (pmfs * self.atoms).sum(2)
        if action is None:
            action = torch.argmax(q_values, 1)
        return action, pmfs[torch.arange(len(x)), action]


def _nature_q(outputs):
    """The NatureCNN trunk, ``Linear(3136, 512)`` and the head of dqn_atari.py / c51_atari.py: torch's default initialisation (these
    scripts have no ``layer_init``) in the reference's construction order."""
    return nn.Sequential(
        nn.Conv2d(4, 32, 8, stride=4),
        nn.ReLU(),
        nn.Conv2d(32, 64, 4, stride=2),
        nn.ReLU(),
        nn.Conv2d(64, 64, 3, stride=1),
        nn.ReLU(),
        nn.Flatten(),
        nn.Linear(3136, 512),
        nn.ReLU(),
        nn.Linear(512, outputs),
    )


class AtariDQNNetwork(nn.Module):
    """dqn_atari.py's ``QNetwork``; ``x / 255.0`` is part of the network."""

    def __init__(self, env):
        super().__init__()
        self.n = env.single_action_space.n
        self.network = _nature_q(self.n)

    def forward(self, x):
        return self.network(x / 255.0)


class AtariC51Network(nn.Module):
    """c51_atari.py's ``QNetwork``: ``n * n_atoms`` outputs, the ``atoms`` buffer and ``get_action``."""

    def __init__(self, env, n_atoms=51, v_min=-10, v_max=10):
        super().__init__()
        self.env = env
        self.n_atoms = n_atoms
        self.register_buffer("atoms", torch.linspace(v_min, v_max, steps=n_atoms))
        self.n = env.single_action_space.n
        self.network = _nature_q(self.n * n_atoms)

    def get_action(self, x, action=None):
        logits = self.network(x / 255.0)
        pmfs = torch.softmax(logits.view(len(x), self.n, self.n_atoms), dim=2)
        q_values = (pmfs * self.atoms).sum(2)
        if action is None:
            action = torch.argmax(q_values, 1)
        return action, pmfs[torch.arange(len(x)), action]


class NoisyLinear(nn.Module):
    """rainbow_atari.py's ``NoisyLinear``: ``W = weight_mu + weight_sigma * weight_epsilon`` in training mode, independent Gaussian noise
    per weight.  Names, registration order and the construction's draws (``uniform_`` on weight_mu, ``uniform_`` on bias_mu, then the
    two ``normal_()``) are the reference's, so a seeded construction gives its tensors."""

    def __init__(self, in_features, out_features, std_init=0.5):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.std_init = std_init
        self.weight_mu = nn.Parameter(torch.empty(out_features, in_features))
        self.weight_sigma = nn.Parameter(torch.empty(out_features, in_features))
        self.register_buffer("weight_epsilon", torch.empty(out_features, in_features))
        self.bias_mu = nn.Parameter(torch.empty(out_features))
        self.bias_sigma = nn.Parameter(torch.empty(out_features))
        self.register_buffer("bias_epsilon", torch.empty(out_features))
        self.reset_parameters()
        self.reset_noise()

    def reset_parameters(self):
        mu_range = 1 / math.sqrt(self.in_features)
        self.weight_mu.data.uniform_(-mu_range, mu_range)
        self.weight_sigma.data.fill_(self.std_init / math.sqrt(self.in_features))
        self.bias_mu.data.uniform_(-mu_range, mu_range)
        self.bias_sigma.data.fill_(self.std_init / math.sqrt(self.out_features))

    def reset_noise(self):
        self.weight_epsilon.normal_()
        self.bias_epsilon.normal_()

    def forward(self, input):
        if self.training:
            return F.linear(input, self.weight_mu + self.weight_sigma * self.weight_epsilon, self.bias_mu + self.bias_sigma * self.bias_epsilon)
        return F.linear(input, self.weight_mu, self.bias_mu)


class NoisyDuelingDistributionalNetwork(nn.Module):
    """rainbow_atari.py's network: the NatureCNN trunk, then a value and an advantage stream of two ``NoisyLinear`` layers each, the
    dueling combine per atom and a softmax over the atoms -> (B, n_actions, n_atoms).  ``x / 255.0`` is part of the network."""

    def __init__(self, env, n_atoms, v_min, v_max):
        super().__init__()
        self.n_atoms = n_atoms
        self.v_min = v_min
        self.v_max = v_max
        self.delta_z = (v_max - v_min) / (n_atoms - 1)
        self.n_actions = env.single_action_space.n
        self.register_buffer("support", torch.linspace(v_min, v_max, n_atoms))
        self.network = nn.Sequential(
            nn.Conv2d(4, 32, 8, stride=4),
            nn.ReLU(),
            nn.Conv2d(32, 64, 4, stride=2),
            nn.ReLU(),
            nn.Conv2d(64, 64, 3, stride=1),
            nn.ReLU(),
            nn.Flatten(),
        )
        self.value_head = nn.Sequential(NoisyLinear(3136, 512), nn.ReLU(), NoisyLinear(512, n_atoms))
        self.advantage_head = nn.Sequential(NoisyLinear(3136, 512), nn.ReLU(), NoisyLinear(512, n_atoms * self.n_actions))

    def forward(self, x):
        h = self.network(x / 255.0)
        value = self.value_head(h).view(-1, 1, self.n_atoms)
        advantage = self.advantage_head(h).view(-1, self.n_actions, self.n_atoms)
        q_atoms = value + advantage - advantage.mean(dim=1, keepdim=True)
        return F.softmax(q_atoms, dim=2)

    def noisy_layers(self):
        """The four NoisyLinear layers in ``reset_noise``'s order: value_head.0, value_head.2, advantage_head.0, advantage_head.2."""
        return [m for head in (self.value_head, self.advantage_head) for m in head if isinstance(m, NoisyLinear)]

    def reset_noise(self):
        for layer in self.noisy_layers():
            layer.reset_noise()


def _kaiming_init(layer, bias_const=0.0):
    """sac_atari.py's ``layer_init``: ``kaiming_normal_`` weights, constant biases."""
    nn.init.kaiming_normal_(layer.weight)
    torch.nn.init.constant_(layer.bias, bias_const)
    return layer


def _sac_atari_conv(channels):
    """The convolutions of sac_atari.py's two network classes: the third ReLU is a functional call after ``Flatten``, not a module."""
    return nn.Sequential(
        _kaiming_init(nn.Conv2d(channels, 32, kernel_size=8, stride=4)),
        nn.ReLU(),
        _kaiming_init(nn.Conv2d(32, 64, kernel_size=4, stride=2)),
        nn.ReLU(),
        _kaiming_init(nn.Conv2d(64, 64, kernel_size=3, stride=1)),
        nn.Flatten(),
    )


class AtariSoftQNetwork(nn.Module):
    """sac_atari.py's ``SoftQNetwork``: ``conv`` / ``fc1`` / ``fc_q``; ``x / 255.0`` is part of the network."""

    def __init__(self, envs):
        super().__init__()
        obs_shape = envs.single_observation_space.shape
        self.conv = _sac_atari_conv(obs_shape[0])
        with torch.inference_mode():
            output_dim = self.conv(torch.zeros(1, *obs_shape)).shape[1]
        self.fc1 = _kaiming_init(nn.Linear(output_dim, 512))
        self.fc_q = _kaiming_init(nn.Linear(512, envs.single_action_space.n))

    def forward(self, x):
        x = F.relu(self.conv(x / 255.0))
        x = F.relu(self.fc1(x))
        return self.fc_q(x)


class AtariSACActor(nn.Module):
    """sac_atari.py's ``Actor``: ``conv`` / ``fc1`` / ``fc_logits``; ``get_action`` divides by 255, ``forward`` does not."""

    def __init__(self, envs):
        super().__init__()
        obs_shape = envs.single_observation_space.shape
        self.conv = _sac_atari_conv(obs_shape[0])
        with torch.inference_mode():
            output_dim = self.conv(torch.zeros(1, *obs_shape)).shape[1]
        self.fc1 = _kaiming_init(nn.Linear(output_dim, 512))
        self.fc_logits = _kaiming_init(nn.Linear(512, envs.single_action_space.n))

    def forward(self, x):
        x = F.relu(self.conv(x))
        x = F.relu(self.fc1(x))
        return self.fc_logits(x)

    def get_action(self, x):
        logits = self(x / 255.0)
        policy_dist = Categorical(logits=logits)
        action = policy_dist.sample()
        action_probs = policy_dist.probs
        log_prob = F.log_softmax(logits, dim=1)
        return action, log_prob, action_probs
